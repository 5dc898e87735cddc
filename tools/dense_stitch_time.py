#!/usr/bin/env python3
"""Milliseconds and peak device memory of the window stitch (ops.dense_stitch, csrc/dense_stitch.hip: labels, conf and picture of
one photo from the class maps of K sliding windows, one launch) against the same arithmetic as torch ops on the device: one
F.interpolate(bilinear) per window added into a [C, H, W] fp32 accumulator and a count map, a division, max / argmax, the threshold
and the palette gather.  Photos of 1920 x 1080 and 4032 x 3024, windows of 224 and 448 at half-window stride (`clip.plan_windows`),
grid 7, C = 9 and 128 (`--maps`: ops.dense_stitch_maps, the averaged maps themselves, against the same accumulator without the
max).  The method of tools/dense_time.py: device events around every call after `--warmup` calls, the median of
`--reps`, the two alternating in one process; peak = torch's allocator peak over one call above what was live before it.  Also
checks that the two label maps agree on at least 99.9 % of the pixels.  Prints one JSON line per shape and a markdown table.

    python tools/dense_stitch_time.py [--reps 30] [--warmup 3] [--maps]

`--ab OTHER_LIB` instead compares this tree's library with another build of it (the commit before a refactor) in ONE process:
cclip_dense_stitch and cclip_dense_stitch_maps of both through ctypes on the same buffers, at 1024 x 768 (54 windows of 224, C = 9)
and 1920 x 1080 with C = 128, `--windows` alternating windows of about `--window-s` seconds per build (parent, new | new, parent |
..), each between two device events; ms per call, the median over the windows and their range.  An entry passes when the new
median is no more than the other build's own window range (max - min) above its median.

    python tools/dense_stitch_time.py --ab /path/to/parent/libcclip_hip.so [--windows 15] [--window-s 0.3]
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


def hip_maps(probs, boxes_dev, boxes, H, W, pal):
    from cclip_hip import ops
    maps = torch.empty(probs.shape[1], H, W, device=probs.device)
    ops.dense_stitch_maps(probs, boxes_dev, H, W, maps)
    return maps


def torch_maps(probs, boxes_dev, boxes, H, W, pal):
    acc = torch.zeros(probs.shape[1], H, W, device=probs.device)
    cnt = torch.zeros(H, W, device=probs.device)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        acc[:, y0:y1, x0:x1] += F.interpolate(probs[k:k + 1], size=(y1 - y0, x1 - x0), mode="bilinear", align_corners=False)[0]
        cnt[y0:y1, x0:x1] += 1
    return acc / cnt


def _window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def ab(args):
    import ctypes
    from ctypes import c_float, c_int, c_void_p
    import clip
    from cclip_hip import load_library
    libs = dict(parent=ctypes.CDLL(args.ab), new=load_library())
    gen = torch.Generator(device="cuda").manual_seed(0)
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    for W, H, window, C, g in ((1024, 768, 224, 9, 7), (1920, 1080, 224, 128, 7)):
        boxes = torch.from_numpy(clip.plan_windows(W, H, window, window // 2)).int().cuda()
        K = boxes.shape[0]
        probs = (3.0 * torch.randn(K, C, g, g, device="cuda", generator=gen)).softmax(dim=1).contiguous()
        pal = clip.default_palette(C).cuda()
        labels, conf = torch.empty(H, W, device="cuda", dtype=torch.uint8), torch.empty(H, W, device="cuda")
        out, maps = torch.empty(H, W, 3, device="cuda", dtype=torch.uint8), torch.empty(C, H, W, device="cuda")
        head = (ptr(probs), c_int(K), c_int(C), c_int(g), ptr(boxes), c_int(H), c_int(W))
        entries = dict(
            dense_stitch=lambda lib: lib.cclip_dense_stitch(*head, c_float(0.2), ptr(labels), ptr(conf), c_void_p(0), ptr(pal), c_void_p(0),
                                                            c_int(256), ptr(out), stream),
            dense_stitch_maps=lambda lib: lib.cclip_dense_stitch_maps(*head, ptr(maps), c_void_p(0), stream))
        for entry, call in entries.items():
            results = {}
            for tag, lib in libs.items():                                        # equal bytes at the timed size, and a warm-up
                assert call(lib) == 0
                results[tag] = [t.clone() for t in ((labels, conf, out) if entry == "dense_stitch" else (maps,))]
            assert all(torch.equal(a, b) for a, b in zip(results["parent"], results["new"])), f"{entry}: the two builds differ"
            calls = max(1, int(args.window_s * 1e3 / _window_ms(lambda: call(libs["new"]), 20)))
            ms = dict(parent=[], new=[])
            for w in range(args.windows):
                for tag in (("parent", "new") if w % 2 == 0 else ("new", "parent")):
                    ms[tag].append(_window_ms(lambda: call(libs[tag]), calls))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rng = max(ms["parent"]) - min(ms["parent"])
            print(json.dumps(dict(entry=entry, width=W, height=H, K=K, C=C, grid=g, calls_per_window=calls, windows=args.windows,
                                  parent_ms=round(med["parent"], 5), new_ms=round(med["new"], 5), ratio=round(med["new"] / med["parent"], 4),
                                  parent_min_max=[round(min(ms["parent"]), 5), round(max(ms["parent"]), 5)], parent_range=round(rng, 5),
                                  new_min_max=[round(min(ms["new"]), 5), round(max(ms["new"]), 5)],
                                  verdict="pass" if med["new"] <= med["parent"] + rng else "slower")), flush=True)
        del probs, maps
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", action="store_true", help="time ops.dense_stitch_maps instead of ops.dense_stitch")
    ap.add_argument("--ab", metavar="OTHER_LIB", help="compare this tree's library with another build of it, both entries")
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--window-s", type=float, default=0.3)
    args = ap.parse_args(argv)
    if args.ab:
        return ab(args)
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
                hip, ref = (hip_maps, torch_maps) if args.maps else (hip_stitch, torch_stitch)
                fns = dict(hip=lambda: hip(probs, boxes_dev, boxes, H, W, pal), torch=lambda: ref(probs, boxes_dev, boxes, H, W, pal))
                for _ in range(args.warmup):
                    for fn in fns.values():
                        fn()
                torch.cuda.synchronize()
                if args.maps:
                    same = float(((fns["hip"]() - fns["torch"]()).abs() <= 1e-5).float().mean())
                else:
                    same = float((fns["hip"]()[0] == fns["torch"]()[0]).float().mean())
                assert same >= 0.999, f"kernel and torch restatement agree on only {same:.5f} of the {'values' if args.maps else 'labels'}"
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
