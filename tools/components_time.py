#!/usr/bin/env python3
"""Milliseconds of `clip.label_components(labels, conf)` end to end (csrc/label_components.hip: six labelling launches, the read of
the count, two statistics launches, the statistics copied to the host) against what it replaces: `labels.cpu()` and
`clip.label_boxes` for every class present (host, numpy + Python; boxes only).  Maps of 1920 x 1080 and 4032 x 3024, four kinds:
  blocky   nearest-upsampled random cells of 32 x 32 pixels (7 x 7 per 224), 9 classes: what a real stitch gives
  uniform  one class everywhere: the atomic-contention worst case of the statistics
  random   a per-pixel random map with 2 classes: the component-count worst case
  spiral   a one-pixel-wide spiral: the chain-length worst case
The method of tools/dense_stitch_time.py: device events around every call after `--warmup` calls, the median of `--reps`
alternating calls in one process.  The host side takes seconds and more, so it runs `--host-reps` times (default 1, wall clock,
the median), and `label_boxes` compares every run of a row with every run of the row above, which no one can wait for on the
random and spiral maps: there it is timed on the first `--host-rows` rows only (default 16) and the figure is printed as measured,
with the row count, NOT scaled up.  Also checks that the device boxes of the timed rows equal the host's.  Prints one JSON line
per map and a markdown table.

    python tools/components_time.py [--reps 20] [--warmup 3] [--host-reps 1] [--host-rows 16] [--sizes 1920x1080 4032x3024]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dense_time import _event_ms  # noqa: E402

KINDS = ("blocky", "uniform", "random", "spiral")


def make_map(kind: str, H: int, W: int) -> np.ndarray:
    rng = np.random.RandomState(0)
    if kind == "blocky":
        cells = rng.randint(0, 9, size=((H + 31) // 32, (W + 31) // 32)).astype(np.uint8)
        return np.ascontiguousarray(np.kron(cells, np.ones((32, 32), dtype=np.uint8))[:H, :W])
    if kind == "uniform":
        return np.full((H, W), 3, dtype=np.uint8)
    if kind == "random":
        return rng.randint(0, 2, size=(H, W)).astype(np.uint8)
    from label_components_ref import spiral
    return spiral(H, W)


def host_boxes(labels_dev, rows):
    import clip
    lab = labels_dev.cpu()[:rows]
    return {int(c): clip.label_boxes(lab, int(c)) for c in np.unique(lab.numpy()) if c != 255}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=16)
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "4032x3024"])
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=KINDS)
    args = ap.parse_args(argv)
    import clip
    rows = []
    for size in args.sizes:
        W, H = (int(v) for v in size.split("x"))
        for kind in args.kinds:
            m = make_map(kind, H, W)
            labels = torch.from_numpy(m).cuda()
            conf = torch.rand(H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            host_rows = H if kind in ("blocky", "uniform") else min(H, args.host_rows)
            for _ in range(args.warmup):
                clip.label_components(labels, conf)
            torch.cuda.synchronize()
            dev_ms = [_event_ms(lambda: clip.label_components(labels, conf)) for _ in range(args.reps)]
            host_ms, boxes = [], None
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                boxes = host_boxes(labels, host_rows)
                host_ms.append(1e3 * (time.perf_counter() - t0))
            part = clip.label_components(labels[:host_rows].contiguous())
            for c, b in boxes.items():
                assert part.boxes_of(c) == b, f"{kind} {size}: class {c} differs from label_boxes"
            res = clip.label_components(labels, conf)
            line = dict(width=W, height=H, kind=kind, components=res.n, reps=args.reps, device_ms=round(statistics.median(dev_ms), 3),
                        host_reps=args.host_reps, host_rows=host_rows, host_ms=round(statistics.median(host_ms), 1))
            print(json.dumps(line), flush=True)
            rows.append(line)
            del labels, conf, res, part
            torch.cuda.empty_cache()
    print("| map | kind | components | device, whole map (ms) | host (ms) | host rows timed |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['width']}x{r['height']} | {r['kind']} | {r['components']} | {r['device_ms']} | {r['host_ms']} | {r['host_rows']} of {r['height']} |")


if __name__ == "__main__":
    main()
