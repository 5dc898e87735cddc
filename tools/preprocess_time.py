#!/usr/bin/env python3
"""Milliseconds on one MI355X of the region preprocess against the per-box loop it replaces.

Boxes of one photo: a seeded 1920 x 1080 photo and K = 8, 64, 256 seeded random boxes (32 .. 600 pixels a side), n = 224:
  (a) regions     `pre.regions(image, boxes)`: one upload, tables built on the device, three launches;
  (b) loop_cold   `torch.stack([pre(image.crop(b)) for b in boxes])` with a cold plan cache - a fresh DevicePreprocess and
                  `resample_coeffs.cache_clear()` before every sample: what a list of detector boxes costs today, since every
                  box has its own (w, h) and so misses the cache;
  (c) loop_warm   the same loop with every table already cached on the device (the same boxes again).
Whole photos: 64 seeded photos of mixed sizes (200 .. 1200 pixels a side): `pre.many(images)` against `pre.batch(images)`,
cold and warm in the same sense.

A sample is one call, host and device together: a host clock from before the call to after a device synchronise (`wall`), and a
pair of device events around the same call (`device`: from the first to the last device operation the call enqueues; for the
loops it contains the host work between their launches).  The legs of a case alternate sample by sample in one process; the
first `--warmup` samples of each leg are discarded; median and quartiles [q1, q3] of the rest.  The outputs of the legs are
compared for equality before anything is timed.  One JSON line per case; `--out FILE` also writes the lines there.

    python tools/preprocess_time.py [--reps 15] [--cold-reps 7] [--warmup 2] [--out profiles/preprocess_time.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_PX = 224
KS = (8, 64, 256)
PHOTOS = 64


def _photo(rng, w, h):
    from PIL import Image
    return Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB")


def _boxes(rng, k, width, height):
    w, h = rng.integers(32, 601, k), rng.integers(32, 601, k)
    x0, y0 = rng.integers(0, width - w + 1), rng.integers(0, height - h + 1)
    return np.stack([x0, y0, x0 + w, y0 + h], axis=1).astype(np.int64)


def _sample(fn):
    """(wall ms, device ms) of one call"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def _stat(v):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), 3), q1=round(q[0], 3), q3=round(q[2], 3), samples=len(v))


def _alternate(legs, reps, warmup):
    """legs: name -> (callable, samples wanted).  Round r runs every leg that still wants a sample, in order."""
    got = {name: [] for name in legs}
    for r in range(warmup + max(n for _, n in legs.values())):
        for name, (fn, n) in legs.items():
            if r < warmup + n:
                s = _sample(fn)
                if r >= warmup:
                    got[name].append(s)
    return {name: dict(wall_ms=_stat([s[0] for s in v]), device_ms=_stat([s[1] for s in v])) for name, v in got.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15, help="timed samples of the warm legs and of the new path")
    ap.add_argument("--cold-reps", type=int, default=7, help="timed samples of the cold legs (each rebuilds every table on the host)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, action="append", default=None, help="time this K only (repeatable)")
    ap.add_argument("--photos", type=int, default=PHOTOS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.reps < 5 or args.cold_reps < 5 or args.warmup < 1:
        ap.error("at least 5 timed samples after 1 discarded")
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_time: no GPU; there is nothing to time without one")
    import clip
    from clip.preprocess_device import resample_coeffs
    rng = np.random.default_rng(567)
    image = _photo(rng, 1920, 1080)
    lines = []

    def emit(rec, t):
        a = t[rec["new"]]["wall_ms"]["median"]
        for name, v in t.items():
            rec[name] = v
            if name != rec["new"]:
                rec[f"wall_ratio_{name}_over_{rec['new']}"] = round(v["wall_ms"]["median"] / a, 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for K in (args.k or KS):
        boxes = _boxes(rng, K, 1920, 1080)
        crops = [tuple(int(v) for v in b) for b in boxes]
        warm = clip.DevicePreprocess(N_PX)

        def regions():
            return warm.regions(image, boxes)

        def loop_warm():
            return torch.stack([warm(image.crop(b)) for b in crops])

        def loop_cold():
            resample_coeffs.cache_clear()
            pre = clip.DevicePreprocess(N_PX)
            return torch.stack([pre(image.crop(b)) for b in crops])

        assert torch.equal(regions(), loop_warm()), "the two paths disagree"
        t = _alternate(dict(regions=(regions, args.reps), loop_warm=(loop_warm, args.reps), loop_cold=(loop_cold, args.cold_reps)),
                       args.reps, args.warmup)
        emit(dict(case="boxes_of_one_photo", photo="1920x1080", K=K, n=N_PX, new="regions"), t)

    sizes = [(int(w), int(h)) for w, h in zip(rng.integers(200, 1201, args.photos), rng.integers(200, 1201, args.photos))]
    photos = [_photo(rng, w, h) for w, h in sizes]
    warm = clip.DevicePreprocess(N_PX)

    def many():
        return warm.many(photos)

    def batch_warm():
        return warm.batch(photos)

    def batch_cold():
        resample_coeffs.cache_clear()
        return clip.DevicePreprocess(N_PX).batch(photos)

    assert torch.equal(many(), batch_warm()), "the two paths disagree"
    t = _alternate(dict(many=(many, args.reps), batch_warm=(batch_warm, args.reps), batch_cold=(batch_cold, args.cold_reps)),
                   args.reps, args.warmup)
    emit(dict(case="whole_photos_of_mixed_sizes", photos=args.photos, sides="200..1200", n=N_PX, new="many"), t)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
