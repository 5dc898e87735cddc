#!/usr/bin/env python3
"""Milliseconds per key-gradient call on one MI355X: the fused launch pair `ops.cache_affinity_backward`
(csrc/embed_cache_bwd.hip) against torch autograd through the composition tools/cache_affinity_time.py times for the forward -
fp32 matmul of the rows into a Q x N matrix, `exp(beta * (s - 1))`, a matmul with the fp32 one-hot [N, C] label matrix.  The
composition's graph is built once outside the timed region (its Q x N matrices stay allocated); what is timed is
`torch.autograd.grad` through it, i.e. its backward alone, as the kernel leg is the backward alone.  Shapes (Q, N, C, D):
(1024, 100 000, 9, 512) and the reference data's own size trained on itself (306, 306, 9, 512).  The legs alternate call by
call in one process; each call sits between two device events; the first `--warmup` calls of every leg are discarded; median
[min max] of the rest.  One JSON line per shape, with the largest difference of the two legs' results relative to the largest
gradient entry.  No speed ratio is promised: the small shape is launch-bound and fills 6 work-groups.

    python tools/cache_affinity_bwd_time.py [--reps 7] [--warmup 2] [--dtype bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from cache_affinity_time import _alternate, _stat  # noqa: E402

SHAPES = [(1024, 100_000, 9, 512), (306, 306, 9, 512)]
BETA = 5.5


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
    gen = torch.Generator(device="cuda").manual_seed(568)
    for Q, N, C, D in shapes:
        labels = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(N))
        g16 = clip.retrieval.normalize_rows(torch.randn(N, D, device="cuda", generator=gen), dtype)
        q16 = clip.retrieval.normalize_rows(torch.randn(Q, D, device="cuda", generator=gen), dtype)
        dA = torch.randn(Q, C, device="cuda", generator=gen) / Q
        gather, off, ln = ops.cache_layout(labels, C)
        keep = (gather >= 0).cuda()
        laid = torch.zeros(gather.numel(), D, device="cuda", dtype=dtype)
        laid[keep] = g16[gather.cuda()[keep]]
        onehot = torch.nn.functional.one_hot(labels, C).float().cuda()
        out = torch.empty(gather.numel(), D, device="cuda")

        def fused():
            return ops.cache_affinity_backward(q16, laid, off, ln, BETA, dA, out=out)

        g32, q32 = g16.float().requires_grad_(True), q16.float()
        A = torch.exp((torch.matmul(q32, g32.t()) - 1.0) * BETA) @ onehot      # fp32 throughout: the kernel's arithmetic

        def composed():
            return torch.autograd.grad(A, g32, dA, retain_graph=True)[0]

        t = _alternate(dict(kernel=fused, composition=composed), args.reps, args.warmup)
        a, b = fused()[keep].double(), composed()[gather.cuda()[keep]].double()
        km = statistics.median(t["kernel"]) * 1e-3
        res = dict(Q=Q, N=N, C=C, D=D, Np=gather.numel(), beta=BETA, dtype=args.dtype, kernel_pair_ms=_stat(t["kernel"]),
                   torch_autograd_backward_ms=_stat(t["composition"]),
                   composition_over_kernel=round(statistics.median(t["composition"]) / statistics.median(t["kernel"]), 3),
                   TFLOPs=round(6.0 * Q * gather.numel() * D / km / 1e12, 2),       # scores, and hi + lo of the second product
                   matrix_bytes=4 * Q * N, max_diff_over_max=float((a - b).abs().max() / b.abs().max()))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
