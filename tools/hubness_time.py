#!/usr/bin/env python3
"""Milliseconds and peak device memory of hubness-corrected retrieval on one MI355X: `clip.fit_querybank` +
`EmbeddingIndex.search(querybank=)` (csrc/embed_hub.hip, the biased top-k of csrc/embed_topk.hip) against the torch composition
it replaces - `q @ g.T`, `bank @ g.T`, `logsumexp`, `topk`, which writes the Q x N and the B x N matrix - at one shape
(N stored rows, Q queries, B bank rows, D = 512, k = 10, the inverted softmax at beta = 20), both 16-bit types.  The rows are
unit vectors around a common direction, the regime in which hubs appear.  The legs alternate call by call in one process; each
call sits between two device events and ends in a synchronise; the first `--warmup` calls of every leg are discarded; median
[min max] of the rest.  Two compositions: `composition` works in fp32 on the 16-bit rows (an fp32 copy of the gallery, fp32
matmuls, 4-byte matrices: the arithmetic the kernels match), `composition_16bit` multiplies in the 16-bit type (scores rounded
to 16 bits, 2-byte matrices and their fp32 copies) and does the rest in fp32.  One JSON line per dtype.  Not measured: other
shapes, "dis" and "csls", the search alone with a bank fitted once.

    python tools/hubness_time.py [--reps 7] [--warmup 2] [--n 200000] [--q 1024] [--bank 4096] [--dtypes bf16,fp16]
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

D, K, BETA = 512, 10, 20.0


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


def _cone(n, gen, axis):
    x = torch.nn.functional.normalize(torch.randn(n, D, device="cuda", generator=gen), dim=1) + 0.9 * axis
    return torch.nn.functional.normalize(x, dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--bank", type=int, default=4096)
    ap.add_argument("--dtypes", default="bf16,fp16")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    import clip
    gen = torch.Generator(device="cuda").manual_seed(567)
    N, Q, B = args.n, args.q, args.bank
    for name in args.dtypes.split(","):
        dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[name]
        axis = torch.nn.functional.normalize(torch.randn(1, D, device="cuda", generator=gen), dim=1)
        index = clip.EmbeddingIndex(_cone(N, gen, axis), dtype=dtype)
        queries, bank = _cone(Q, gen, axis), _cone(B, gen, axis)
        q16, b16, g16 = queries.to(dtype), bank.to(dtype), index.features

        def fused():
            return index.search(queries, K, querybank=index.querybank(bank, method="is", beta=BETA))

        def composed():
            g = g16.float()
            lse = torch.logsumexp(BETA * (b16.float() @ g.t()), dim=0)               # the B x N matrix
            return torch.topk(BETA * (q16.float() @ g.t()) - lse[None, :], K, dim=1)  # the Q x N matrix

        def composed16():                                                            # 16-bit matmuls, the rest in fp32
            lse = torch.logsumexp(BETA * (b16 @ g16.t()).float(), dim=0)
            return torch.topk(BETA * (q16 @ g16.t()).float() - lse[None, :], K, dim=1)

        legs = dict(hubness_hip=fused, composition=composed, composition_16bit=composed16)
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
        line = dict(N=N, Q=Q, B=B, D=D, k=K, beta=BETA, method="is", dtype=name, matrix_bytes_fp32=4 * N * (Q + B))
        for leg in legs:
            line[leg] = failed[leg] if leg in failed else dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
        if not failed:
            for leg in ("composition", "composition_16bit"):
                line["speedup_median_vs_" + leg] = round(statistics.median(times[leg]) / statistics.median(times["hubness_hip"]), 3)
        print(json.dumps(line), flush=True)
        del index, queries, bank, q16, b16, g16


if __name__ == "__main__":
    main()
