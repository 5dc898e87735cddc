#!/usr/bin/env python3
"""Milliseconds and peak device memory of the image-guided refinement (clip.refine_maps, csrc/dense_refine.hip: one prepare
launch and T step launches) against the same arithmetic as torch ops on the device: the guide and, per iteration, the maps
replicate-padded by the largest dilation, 8 D shifted slices each, an unbiased std over the 9 D taps, a softmax over the
neighbours and 8 D multiply-adds of [C, H, W] tensors.  Photos of 1920 x 1080 and 4032 x 3024, C = 9 and 128, the default dilations
(1, 2, 4, 8, 12, 24), T = 10.  The method of tools/dense_stitch_time.py: device events around every call after `--warmup` calls,
the median of `--reps`, the two alternating in one process; peak = torch's allocator peak over one call above what was live
before it (the inputs).  Also reports the largest difference between the two results.  Prints one JSON line per shape as soon
as it is measured, then a markdown table.

    python tools/refine_time.py [--reps 30] [--warmup 2] [--shapes 1920x1080x9 ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dense_time import _event_ms, _peak_mb  # noqa: E402

DILATIONS = (1, 2, 4, 8, 12, 24)
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _shifted(x, p):
    """x [K, H, W] -> the 48 shifted views of its replicate-padded copy, in neighbour order"""
    H, W = x.shape[-2:]
    xp = F.pad(x[None], (p, p, p, p), mode="replicate")[0]
    return [xp[:, p + d * oy:p + d * oy + H, p + d * ox:p + d * ox + W] for d in DILATIONS for oy, ox in OFFSETS]


def torch_refine(maps, guide, iterations):
    p = max(DILATIONS)
    x = guide.permute(2, 0, 1).float() / 255.0
    nb = torch.stack(_shifted(x, p), dim=1)                                   # [3, N, H, W]
    taps = torch.cat([nb, x[:, None].expand(-1, len(DILATIONS), -1, -1)], dim=1)
    f = 1.0 / (1e-8 + 0.1 * taps.std(dim=1, unbiased=True))
    w = torch.softmax(-((x[:, None] - nb).abs() * f[:, None]).sum(dim=0) / 3.0, dim=0)      # [N, H, W]
    del nb, taps
    m = maps
    for _ in range(iterations):
        out = None
        for n, s in enumerate(_shifted(m, p)):
            out = w[n] * s if out is None else out.addcmul_(w[n], s)
        m = out
    return m


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--shapes", nargs="+", default=["1920x1080x9", "1920x1080x128", "4032x3024x9", "4032x3024x128"], metavar="WxHxC")
    args = ap.parse_args(argv)
    import clip
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for shape in args.shapes:
        W, H, C = (int(v) for v in shape.split("x"))
        guide = torch.randint(0, 256, (H, W, 3), device="cuda", dtype=torch.uint8, generator=gen)
        maps = (3.0 * torch.randn(C, H, W, device="cuda", generator=gen)).softmax(dim=0).contiguous()
        fns = dict(hip=lambda: clip.refine_maps(maps, guide, dilations=DILATIONS, iterations=args.iterations),
                   torch=lambda: torch_refine(maps, guide, args.iterations))
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        diff = float((fns["hip"]() - fns["torch"]()).abs().max())
        times = dict(hip=[], torch=[])
        for _ in range(args.reps):
            for k, fn in fns.items():
                times[k].append(_event_ms(fn))
        line = dict(width=W, height=H, C=C, dilations=list(DILATIONS), iterations=args.iterations, reps=args.reps, max_abs_diff=diff,
                    ms={k: round(statistics.median(v), 3) for k, v in times.items()},
                    peak_mb={k: round(_peak_mb(fn), 1) for k, fn in fns.items()})
        print(json.dumps(line), flush=True)
        rows.append(line)
        del maps, guide
        torch.cuda.empty_cache()
    print("| photo | C | T | HIP (ms) | torch ops (ms) | HIP peak (MB) | torch peak (MB) | max abs diff |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']}x{r['height']} | {r['C']} | {r['iterations']} | {r['ms']['hip']} | {r['ms']['torch']} | {r['peak_mb']['hip']} | "
              f"{r['peak_mb']['torch']} | {r['max_abs_diff']:.2e} |")


if __name__ == "__main__":
    main()
