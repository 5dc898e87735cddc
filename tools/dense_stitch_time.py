#!/usr/bin/env python3
"""Milliseconds and peak device memory of the window stitch (ops.dense_stitch, csrc/dense_stitch.hip: labels, conf and picture of
one photo from the class maps of K sliding windows, one launch) against the same arithmetic as torch ops on the device: one
F.interpolate(bilinear) per window added into a [C, H, W] fp32 accumulator and a count map, a division, max / argmax, the threshold
and the palette gather.  Photos of 1920 x 1080 and 4032 x 3024, windows of 224 and 448 at half-window stride (`clip.plan_windows`),
grid 7, C = 9 and 128.  The method of tools/dense_time.py: device events around every call after `--warmup` calls, the median of
`--reps`, the two alternating in one process; peak = torch's allocator peak over one call above what was live before it.  Also
checks that the two label maps agree on at least 99.9 % of the pixels.  Prints one JSON line per shape and a markdown table.

    python tools/dense_stitch_time.py [--reps 30] [--warmup 3]
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


def hip_stitch(probs, boxes_dev, boxes, H, W, pal):
    from cclip_hip import ops
    labels = torch.empty(H, W, device=probs.device, dtype=torch.uint8)
    conf = torch.empty(H, W, device=probs.device)
    out = torch.empty(H, W, 3, device=probs.device, dtype=torch.uint8)
    ops.dense_stitch(probs, boxes_dev, H, W, labels, conf, min_conf=0.2, overlay=out, palette=pal)
    return labels, out


def torch_stitch(probs, boxes_dev, boxes, H, W, pal):
    C = probs.shape[1]
    acc = torch.zeros(C, H, W, device=probs.device)
    cnt = torch.zeros(H, W, device=probs.device)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        acc[:, y0:y1, x0:x1] += F.interpolate(probs[k:k + 1], size=(y1 - y0, x1 - x0), mode="bilinear", align_corners=False)[0]
        cnt[y0:y1, x0:x1] += 1
    conf, arg = (acc / cnt).max(dim=0)
    labels = torch.where(conf < 0.2, torch.full_like(arg, 255), arg).to(torch.uint8)
    return labels, pal[labels.long()]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    import clip
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, g = [], 7
    for W, H in ((1920, 1080), (4032, 3024)):
        for window in (224, 448):
            for C in (9, 128):
                boxes_np = clip.plan_windows(W, H, window, window // 2)
                boxes = boxes_np.tolist()
                K = len(boxes)
                boxes_dev = torch.from_numpy(boxes_np).int().cuda()
                probs = (3.0 * torch.randn(K, C, g, g, device="cuda", generator=gen)).softmax(dim=1).contiguous()
                pal = clip.default_palette(C).cuda()
                fns = dict(hip=lambda: hip_stitch(probs, boxes_dev, boxes, H, W, pal), torch=lambda: torch_stitch(probs, boxes_dev, boxes, H, W, pal))
                for _ in range(args.warmup):
                    for fn in fns.values():
                        fn()
                torch.cuda.synchronize()
                same = float((fns["hip"]()[0] == fns["torch"]()[0]).float().mean())
                assert same >= 0.999, f"kernel and torch restatement agree on only {same:.5f} of the labels"
                times = dict(hip=[], torch=[])
                for _ in range(args.reps):
                    for k, fn in fns.items():
                        times[k].append(_event_ms(fn))
                line = dict(width=W, height=H, window=window, stride=window // 2, K=K, C=C, grid=g, reps=args.reps, labels_equal=round(same, 6),
                            ms={k: round(statistics.median(v), 4) for k, v in times.items()},
                            peak_mb={k: round(_peak_mb(fn), 2) for k, fn in fns.items()})
                print(json.dumps(line), flush=True)
                rows.append(line)
                del probs
                torch.cuda.empty_cache()
    print("| photo | window | K | C | HIP (ms) | torch ops (ms) | HIP peak (MB) | torch peak (MB) |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']}x{r['height']} | {r['window']} | {r['K']} | {r['C']} | {r['ms']['hip']} | {r['ms']['torch']} | "
              f"{r['peak_mb']['hip']} | {r['peak_mb']['torch']} |")


if __name__ == "__main__":
    main()
