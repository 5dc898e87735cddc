#!/usr/bin/env python3
"""Milliseconds and allocator peak of `clip.evaluate_labels(pred, gt, C, band=d)` end to end (csrc/label_agreement.hip: one zeroing
launch, one counting launch, the counts copied to the host) against the same arithmetic written in torch ops on the device:
the confusion as `bincount` of gt (C + 1) + pred over the valid pixels, the band of each map as "max_pool2d of the map and of
its negation differ from the map" over the (2d + 1)^2 window (run as a row pool and a column pool, which is the same maximum
and the cheaper form; the padding is -inf, so the image border is set by hand), the band counts as three more bincounts.
Maps: nearest-upsampled random cells of 32 x 32 pixels with C classes; pred is gt moved by (5, 9) pixels with 3 % "none".
Cases: 1920 x 1080 and 4032 x 3024, C = 9 and 128, band = 0, 4 and 32.

The method of tools/dense_stitch_time.py: device events around every call after `--warmup` calls, the median of `--reps`
alternating calls in one process.  The allocator peak is torch.cuda.max_memory_allocated() above what is allocated with only
the two maps live.  Asserts that the two give EQUAL counts.  Prints one JSON line per case and a markdown table.

    python tools/agreement_time.py [--reps 5] [--warmup 1] [--sizes 1920x1080 4032x3024] [--classes 9 128] [--bands 0 4 32]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dense_time import _event_ms  # noqa: E402


def make_maps(H: int, W: int, C: int):
    rng = np.random.RandomState(0)
    cells = rng.randint(0, C, size=((H + 31) // 32, (W + 31) // 32)).astype(np.uint8)
    gt = torch.from_numpy(np.ascontiguousarray(np.kron(cells, np.ones((32, 32), dtype=np.uint8))[:H, :W])).cuda()
    yy = (torch.arange(H, device="cuda") - 5).clamp_(0, H - 1)
    xx = (torch.arange(W, device="cuda") - 9).clamp_(0, W - 1)
    pred = gt[yy][:, xx].contiguous()
    pred[torch.rand(H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.03] = 255
    return pred, gt


def _band(m: torch.Tensor, d: int) -> torch.Tensor:
    f = m.float()[None, None]

    def pool(x):
        return F.max_pool2d(F.max_pool2d(x, (1, 2 * d + 1), stride=1, padding=(0, d)), (2 * d + 1, 1), stride=1, padding=(d, 0))
    inb = ((pool(f) != f) | (pool(-f) != -f))[0, 0]
    inb[:d] = True
    inb[-d:] = True
    inb[:, :d] = True
    inb[:, -d:] = True
    return inb


def torch_counts(pred: torch.Tensor, gt: torch.Tensor, C: int, d: int):
    """(confusion [C, C + 1], bands [C, 3] or None) of maps without labels in [C, 254]"""
    g, p = gt.long(), pred.long()
    valid = g < C
    col = torch.where(p == 255, torch.full_like(p, C), p)
    confusion = torch.bincount((g * (C + 1) + col)[valid], minlength=C * (C + 1)).view(C, C + 1)
    if d == 0:
        return confusion, None
    ing, inp = _band(gt, d), _band(pred, d)
    G = torch.bincount(g[valid & ing], minlength=C)
    P = torch.bincount(p[valid & inp & (p < C)], minlength=C)
    both = torch.bincount(g[valid & ing & inp & (p == g)], minlength=C)
    return confusion, torch.stack([G, P, both], dim=1)


def _peak(fn) -> float:
    """MiB the allocator holds at most during fn() above what is live before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "4032x3024"])
    ap.add_argument("--classes", type=int, nargs="+", default=[9, 128])
    ap.add_argument("--bands", type=int, nargs="+", default=[0, 4, 32])
    args = ap.parse_args(argv)
    import clip
    rows = []
    for size in args.sizes:
        W, H = (int(v) for v in size.split("x"))
        for C in args.classes:
            pred, gt = make_maps(H, W, C)
            for d in args.bands:
                hip = lambda: clip.evaluate_labels(pred, gt, C, band=d)                     # noqa: E731
                ref = lambda: tuple(None if t is None else t.cpu() for t in torch_counts(pred, gt, C, d))   # noqa: E731
                s, (conf, bands) = hip(), ref()
                assert torch.equal(s.confusion, conf), f"{size} C {C} band {d}: confusion differs"
                assert (bands is None and s.bands is None) or torch.equal(s.bands, bands), f"{size} C {C} band {d}: bands differ"
                for _ in range(args.warmup):
                    hip(), ref()
                hip_ms, ref_ms = [], []
                for _ in range(args.reps):
                    hip_ms.append(_event_ms(hip))
                    ref_ms.append(_event_ms(ref))
                line = dict(width=W, height=H, classes=C, band=d, reps=args.reps, hip_ms=round(statistics.median(hip_ms), 3),
                            torch_ms=round(statistics.median(ref_ms), 3), hip_peak_mib=round(_peak(hip), 2), torch_peak_mib=round(_peak(ref), 1),
                            miou=round(s.miou, 6), mean_boundary_iou=None if s.bands is None else round(s.mean_boundary_iou, 6))
                print(json.dumps(line), flush=True)
                rows.append(line)
            del pred, gt
            torch.cuda.empty_cache()
    print("| map | C | band | evaluate_labels (ms) | torch ops (ms) | evaluate_labels peak (MiB) | torch peak (MiB) |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']}x{r['height']} | {r['classes']} | {r['band']} | {r['hip_ms']} | {r['torch_ms']} | {r['hip_peak_mib']} | {r['torch_peak_mib']} |")


if __name__ == "__main__":
    main()
