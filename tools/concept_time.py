#!/usr/bin/env python3
"""Milliseconds and peak device memory of one full concept decomposition on one MI355X: `ops.concept_codes`
(csrc/concept_codes.hip: every FISTA iteration inside one launch, the dictionary re-streamed per sweep) against the same
recurrence written in torch as two dense matmuls per iteration - y = w + beta (w - w_prev), r = x - y c, g = r c^T,
w = relu(y + eta (g - l1)) - on the same device and the same unit 16-bit rows, once with fp32 operands (the arithmetic the
kernel's hi + lo pairs stand for) and once with the products in bf16 (what a plain 16-bit formulation gives).  Default shape:
N = 16384, V = 8192, D = 512, iters = 100.  A timed call is one whole decomposition between two device events, ending in a
synchronise; buffers are allocated before the clock starts, so peak_bytes is what a call allocates on top of its inputs and
state (state_bytes: w and w_prev, fp32 [N, V] each, for every leg).  The legs alternate call by call in one process; the first
`--warmup` calls of every leg are discarded; median [min max] of the rest.  Before timing, every leg's w is compared with the
kernel's on the first 64 rows (max |difference|): the bf16 leg is there for its time, not for its digits.  useful_flops counts
the two products once (4 N V D per iteration); the kernel issues each twice (hi and lo).  One JSON line per shape.

    python tools/concept_time.py [--reps 7] [--warmup 2] [--n 16384] [--v 8192] [--d 512] [--iters 100] [--l1 0.1]
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


def _timed(fn):
    """(ms, peak bytes above the level before the call) of one call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - before


def _stat(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3), n=len(ts))


def torch_fista(x, c, l1, eta, iters, w, wp, product_dtype):
    """The recurrence of include/cclip_hip.h in torch: x, c in product_dtype, w and wp fp32 [N, V] (zeroed here), two matmuls
    an iteration.  Returns the buffer that holds w_T."""
    w.zero_()
    wp.zero_()
    xf, ct = x.float(), c.t().contiguous()
    for k in range(iters):
        beta = k / (k + 3.0)
        y = torch.add(w, w - wp, alpha=beta) if k else w
        r = xf - torch.mm(y.to(product_dtype), c).float()
        g = torch.mm(r.to(product_dtype), ct).float()
        torch.clamp_min(y + eta * (g - l1), 0.0, out=wp)
        w, wp = wp, w
    return w


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--v", type=int, default=8192)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--l1", type=float, default=0.1)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    from cclip_hip import ops
    import clip
    N, V, D, T = args.n, args.v, args.d, args.iters
    gen = torch.Generator(device="cuda").manual_seed(567)
    x = clip.EmbeddingIndex(torch.randn(N, D, device="cuda", generator=gen)).features
    d = clip.ConceptDictionary(torch.randn(V, D, device="cuda", generator=gen))
    c, eta = d.rows, 1.0 / d.L
    w = torch.empty(N, V, device="cuda", dtype=torch.float32)
    w2 = torch.empty(N, V, device="cuda", dtype=torch.float32)
    c32 = c.float()
    out = {}

    def kernel():
        out["w"] = ops.concept_codes(x, c, args.l1, eta, T, out_w=w, workspace=w2.view(-1))[0]

    def torch_fp32():
        out["w"] = torch_fista(x, c32, args.l1, eta, T, w, w2, torch.float32)

    def torch_bf16():
        out["w"] = torch_fista(x, c, args.l1, eta, T, w, w2, torch.bfloat16)

    legs = dict(concept_codes_hip=kernel, torch_fp32=torch_fp32, torch_bf16=torch_bf16)
    head = {}
    for leg, fn in legs.items():
        fn()
        head[leg] = out["w"][:64].clone()
    nnz = float((head["concept_codes_hip"] > 0).sum(1).float().mean())
    apart = {leg: float((head[leg] - head["concept_codes_hip"]).abs().max()) for leg in legs if leg != "concept_codes_hip"}
    times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
    for r in range(args.reps + args.warmup):
        for leg, fn in legs.items():
            ms, peak = _timed(fn)
            peaks[leg] = max(peaks[leg], peak)
            if r >= args.warmup:
                times[leg].append(ms)
    flops = 4.0 * N * V * D * T
    line = dict(N=N, V=V, D=D, iters=T, l1=args.l1, L=round(d.L, 3), mean_nnz_first_rows=round(nnz, 2), state_bytes=8 * N * V,
                useful_flops=flops, max_abs_w_apart_from_kernel=apart)
    for leg in legs:
        med = statistics.median(times[leg])
        line[leg] = dict(ms=_stat(times[leg]), peak_bytes=peaks[leg], useful_tflops=round(flops / (med * 1e-3) / 1e12, 1))
    for leg in ("torch_fp32", "torch_bf16"):
        line["kernel_over_" + leg] = round(statistics.median(times["concept_codes_hip"]) / statistics.median(times[leg]), 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
