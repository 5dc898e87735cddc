#!/usr/bin/env python3
"""Milliseconds and peak device memory of one Lloyd iteration of spherical k-means on one MI355X, D = 512: `ops.kmeans_assign` +
`ops.kmeans_update` (csrc/embed_kmeans.hip; the update includes its stable sort) against the torch composition it replaces
(`argmax(x @ c.T)`, `index_add_` in fp32, normalise, round - which writes the N x K matrix and sums with float atomics), at
N in {20 000, 10^6} and K in {64, 1024}, both 16-bit types.  The rows are unit vectors around K directions.  The legs alternate
call by call in one process; each call sits between two device events and ends in a synchronise; the first `--warmup` calls
of every leg are discarded; median [min max] of the rest.  A composition that does not fit the device is reported as "out of
memory", not timed.  One JSON line per (N, K, dtype).

    python tools/kmeans_time.py [--reps 7] [--warmup 2] [--sizes 20000,1000000] [--ks 64,1024] [--dtypes bf16,fp16]
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

D = 512


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
    ap.add_argument("--sizes", default="20000,1000000")
    ap.add_argument("--ks", default="64,1024")
    ap.add_argument("--dtypes", default="bf16,fp16")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    for N in (int(v) for v in args.sizes.split(",")):
        for K in (int(v) for v in args.ks.split(",")):
            for name in args.dtypes.split(","):
                dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[name]
                dirs = torch.nn.functional.normalize(torch.randn(K, D, device="cuda", generator=gen), dim=1)
                member = torch.randint(0, K, (N,), device="cuda", generator=gen)
                x = dirs[member] + 0.5 / D ** 0.5 * torch.randn(N, D, device="cuda", generator=gen)
                x = torch.nn.functional.normalize(x, dim=1).to(dtype)
                c = x[torch.randperm(N, device="cuda", generator=gen)[:K]].clone()
                del dirs, member

                def fused():
                    assign, best, _ = ops.kmeans_assign(x, c)
                    return ops.kmeans_update(x, assign, K, c, check_range=False)[0]

                def composed():
                    assign = (x @ c.t()).argmax(dim=1)                     # the N x K matrix, in the 16-bit type
                    s = torch.zeros(K, D, device="cuda").index_add_(0, assign, x.float())
                    return torch.nn.functional.normalize(s, dim=1).to(dtype)

                legs = dict(kmeans_hip=fused, composition=composed)
                times, peaks, failed = {n: [] for n in legs}, {n: 0 for n in legs}, {}
                for r in range(args.reps + args.warmup):
                    for leg, fn in legs.items():
                        if leg in failed:
                            continue
                        try:
                            ms, peak, out = _timed(fn)
                        except torch.OutOfMemoryError as e:
                            failed[leg] = "out of memory: " + str(e).splitlines()[0][:120]
                            torch.cuda.empty_cache()
                            continue
                        peaks[leg] = max(peaks[leg], peak)
                        del out
                        if r >= args.warmup:
                            times[leg].append(ms)
                line = dict(N=N, K=K, D=D, dtype=name, matrix_bytes_16bit=2 * N * K)
                for leg in legs:
                    line[leg] = failed[leg] if leg in failed else dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
                if not failed:
                    line["speedup_median"] = round(statistics.median(times["composition"]) / statistics.median(times["kmeans_hip"]), 3)
                print(json.dumps(line), flush=True)
                del x, c


if __name__ == "__main__":
    main()
