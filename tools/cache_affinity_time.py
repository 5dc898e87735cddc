#!/usr/bin/env python3
"""Milliseconds per class-affinity call on one MI355X: the fused launch pair `ops.cache_affinity` (csrc/embed_cache.hip) against
the same arithmetic as torch ops on the device - matmul of the rows into a Q x N fp32 matrix (in fp32, and as the 16-bit matmul whose scores are rounded to 16 bits), `exp(beta * (s - 1))` in
place, a matmul with the fp32 one-hot [N, C] label matrix.  Shapes (Q, N, C, D): (1024, 100 000, 9, 512) and the reference
data's own size (64, 306, 9, 512).  The legs alternate call by call in one process; each call sits between two device
events; the first `--warmup` calls of every leg are discarded; median [min max] of the rest.  One JSON line per shape, with
the largest relative difference of the two legs' results.  No speed ratio is promised: the small shape is launch-bound.

    python tools/cache_affinity_time.py [--reps 7] [--warmup 2] [--dtype bf16]
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

SHAPES = [(1024, 100_000, 9, 512), (64, 306, 9, 512)]
BETA = 5.5
PEAK_PFLOPS = 2.5


def _alternate(legs, reps, warmup):
    """legs: {name: fn}.  reps + warmup rounds, one call of every leg per round; ms per call of the kept rounds."""
    times = {n: [] for n in legs}
    for r in range(reps + warmup):
        for n, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[n].append(e0.elapsed_time(e1))
    return times


def _stat(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4), n=len(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--shapes", default=None, help="Q,N,C,D;Q,N,C,D;... instead of the built-in list")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    import clip
    from cclip_hip import ops
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    gen = torch.Generator(device="cuda").manual_seed(567)
    for Q, N, C, D in shapes:
        labels = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(N))
        g16 = clip.retrieval.normalize_rows(torch.randn(N, D, device="cuda", generator=gen), dtype)
        q16 = clip.retrieval.normalize_rows(torch.randn(Q, D, device="cuda", generator=gen), dtype)
        gather, off, ln = ops.cache_layout(labels, C)
        laid = torch.zeros(gather.numel(), D, device="cuda", dtype=dtype)
        keep = (gather >= 0).cuda()
        laid[keep] = g16[gather.cuda()[keep]]
        onehot = torch.nn.functional.one_hot(labels, C).float().cuda()
        out = torch.empty(Q, C, device="cuda")

        def fused():
            return ops.cache_affinity(q16, laid, off, ln, BETA, out=out)

        g32, q32 = g16.float(), q16.float()

        def composed():                                        # fp32 throughout: the kernel's arithmetic
            s = torch.matmul(q32, g32.t())
            s.sub_(1.0).mul_(BETA).exp_()
            return s @ onehot

        def composed16():                                      # the 16-bit matmul: its Q x N scores are rounded to 16 bits
            s = torch.matmul(q16, g16.t()).float()
            s.sub_(1.0).mul_(BETA).exp_()
            return s @ onehot

        t = _alternate(dict(kernel=fused, composition=composed, composition16=composed16), args.reps, args.warmup)
        a, b = fused().double(), composed().double()
        km = statistics.median(t["kernel"]) * 1e-3
        res = dict(Q=Q, N=N, C=C, D=D, Np=gather.numel(), beta=BETA, dtype=args.dtype, kernel_pair_ms=_stat(t["kernel"]),
                   torch_composition_ms=_stat(t["composition"]), torch_composition_16bit_scores_ms=_stat(t["composition16"]),
                   composition_over_kernel=round(statistics.median(t["composition"]) / statistics.median(t["kernel"]), 3),
                   TFLOPs=round(2.0 * Q * gather.numel() * D / km / 1e12, 2),
                   flop_share_of_peak=round(2.0 * Q * gather.numel() * D / km / (PEAK_PFLOPS * 1e15), 4),
                   matrix_bytes=4 * Q * N, workspace_bytes=ops.cache_affinity_workspace(Q, gather.numel(), C),
                   max_rel_diff=float(((a - b).abs() / b.abs().clamp(min=1e-30)).max()))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
