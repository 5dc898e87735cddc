#!/usr/bin/env python3
"""Milliseconds and peak device memory of near-duplicate detection on one MI355X, E = 512: `EmbeddingIndex.duplicate_pairs`
(count launch, scan, one host read, emit launch of csrc/embed_range.hip in self-join mode) against the torch composition it
replaces (`s @ s.T`, `triu(1)`, `>= threshold`, `nonzero`, which writes the N x N matrix), at N = 20 000 and 200 000.  The
rows are unit vectors with one in ten re-emitted as a noisy copy, so that there are pairs to find.  The legs alternate call
by call in one process; each call sits between two device events and ends in a synchronise; the first `--warmup` calls of
every leg are discarded; median [min max] of the rest.  A composition that does not fit the device is reported as
"out of memory", not timed.  One JSON line per N.

    python tools/range_time.py [--reps 7] [--warmup 2] [--dtype bf16] [--sizes 20000,200000] [--threshold 0.9]
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

E = 512


def _timed(fn):
    """(ms, peak bytes above the level before the call, result) of one call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - before, out


def _stat(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4), n=len(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--sizes", default="20000,200000")
    ap.add_argument("--threshold", type=float, default=0.9)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    import clip
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    gen = torch.Generator(device="cuda").manual_seed(567)
    for N in (int(v) for v in args.sizes.split(",")):
        base = torch.randn(N - N // 10, E, device="cuda", generator=gen)
        base = base / base.norm(dim=1, keepdim=True)
        copies = base[:N // 10] + 0.15 / E ** 0.5 * torch.randn(N // 10, E, device="cuda", generator=gen)
        feats = torch.cat([base, copies])[torch.randperm(N, device="cuda", generator=gen)]
        index = clip.EmbeddingIndex(feats, dtype=dtype)
        del base, copies, feats
        rows = index.features

        def fused():
            return index.duplicate_pairs(args.threshold)

        def composed():
            s = rows @ rows.t()                                        # the N x N matrix, in the 16-bit type
            return (s.triu_(1) >= args.threshold).nonzero()

        legs = dict(duplicate_pairs=fused, composition=composed)
        times, peaks, found, failed = {n: [] for n in legs}, {n: 0 for n in legs}, {}, {}
        for r in range(args.reps + args.warmup):
            for name, fn in legs.items():
                if name in failed:
                    continue
                try:
                    ms, peak, out = _timed(fn)
                except torch.OutOfMemoryError as e:
                    failed[name] = "out of memory: " + str(e).splitlines()[0][:120]
                    torch.cuda.empty_cache()
                    continue
                found[name] = int((out[0] if isinstance(out, tuple) else out).shape[0])
                peaks[name] = max(peaks[name], peak)
                del out
                if r >= args.warmup:
                    times[name].append(ms)
        out = dict(N=N, E=E, dtype=args.dtype, threshold=args.threshold, matrix_bytes_16bit=2 * N * N)
        for name in legs:
            out[name] = failed[name] if name in failed else dict(ms=_stat(times[name]), peak_bytes=peaks[name], pairs=found[name])
        if not failed:
            out["speedup_median"] = round(statistics.median(times["composition"]) / statistics.median(times["duplicate_pairs"]), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
