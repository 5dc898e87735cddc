#!/usr/bin/env python3
"""Microseconds per batch of N relevance overlays (grid 7, image and picture 224 x 224: ViT-B/32) at N in {1, 8, 64}:
  kernel  clip.relevance_overlay - one launch (csrc/relevance_overlay.hip), 3 * 224 * 224 bytes per picture left on the device;
  torch   the same arithmetic as torch ops on the device: clip.image_relevance_map, min-max of the image, the table look-up,
          the sum, its maximum, the scaling, .to(torch.uint8);
  host    the path of scripts/explain_clip.py::overlay per picture: clip.image_relevance_map on the device, the fp32 map and the
          fp32 image copied to the host, numpy / PIL there (a host clock around it; its copies wait for the device).
kernel and torch: device events around every call after `--warmup` calls, the median of `--reps` calls; the two alternate.
Also checks that the torch restatement and the kernel agree to one level on at least 99 % of the bytes.  Prints one JSON line
and a markdown table.

    python tools/overlay_time.py [--reps 50] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def torch_overlay(rel, images, lut, size):
    import clip
    m = clip.image_relevance_map(rel, size)
    lo = images.amin(dim=(1, 2, 3), keepdim=True)
    rng = images.amax(dim=(1, 2, 3), keepdim=True) - lo
    xn = ((images - lo) / rng).permute(0, 2, 3, 1)
    k = (255 * m).floor().long().clamp(max=255)
    cam = lut[k] + xn
    return (255 * (cam / cam.amax(dim=(1, 2, 3), keepdim=True))).floor().to(torch.uint8)


def host_overlay(rel, images, size):
    import clip
    import explain_clip
    maps = clip.image_relevance_map(rel, size).cpu().numpy()
    return [explain_clip.overlay(images[i], maps[i]) for i in range(rel.shape[0])]


def _event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1000 * e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    import clip
    gen = torch.Generator(device="cuda").manual_seed(0)
    lut = clip.jet_table().cuda()
    size, grid = 224, 7
    out = dict(grid=grid, size=size, reps=args.reps, us={})
    for n in (1, 8, 64):
        rel = torch.rand(n, grid * grid, device="cuda", generator=gen)
        images = torch.randn(n, 3, size, size, device="cuda", generator=gen)
        fns = dict(kernel=lambda: clip.relevance_overlay(rel, images, size=size, lut=lut), torch=lambda: torch_overlay(rel, images, lut, size))
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
            host_overlay(rel, images, size)
        torch.cuda.synchronize()
        a, b = fns["kernel"]().int(), fns["torch"]().int()
        close = float(((a - b).abs() <= 1).float().mean())
        assert close >= 0.99, f"kernel and torch restatement agree on only {close:.4f} of the bytes"
        times = dict(kernel=[], torch=[], host=[])
        for _ in range(args.reps):
            for name, fn in fns.items():
                times[name].append(_event_us(fn))
        for _ in range(max(3, args.reps // 10)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_overlay(rel, images, size)
            times["host"].append(1e6 * (time.perf_counter() - t0))
        out["us"][f"n{n}"] = {k: round(statistics.median(v), 1) for k, v in times.items()}
        out["us"][f"n{n}"]["agree_within_1"] = round(close, 5)
    print(json.dumps(out))
    print("| N | kernel (us) | torch ops (us) | host path (us) |\n|---|---|---|---|")
    for n in (1, 8, 64):
        r = out["us"][f"n{n}"]
        print(f"| {n} | {r['kernel']} | {r['torch']} | {r['host']} |")


if __name__ == "__main__":
    main()
