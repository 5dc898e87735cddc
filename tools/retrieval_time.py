#!/usr/bin/env python3
"""Milliseconds per retrieval call on one MI355X, E = 512: `EmbeddingIndex.search` (normalise + round the queries, then the
fused similarity top-k launch pair) against the composition it replaces (`clip.model.normalized_logits` on the fp32
features, then `torch.topk` on the Q x N matrix), and the kernel pair alone (`ops.similarity_topk`) with its gallery GB/s and
TFLOP/s.  The legs alternate call by call in one process; each call sits between two device events; the first `--warmup`
calls of every leg are discarded; median [min max] of the rest.  One JSON line per shape.

    python tools/retrieval_time.py [--reps 7] [--warmup 2] [--dtype bf16]
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

SHAPES = [(1, 10 ** 5, 10), (16, 10 ** 5, 10), (1024, 10 ** 5, 10), (1, 10 ** 6, 10), (16, 10 ** 6, 10), (1024, 10 ** 6, 10),
          (1024, 10 ** 6, 64)]
E = 512
PEAK_TBS, PEAK_PFLOPS = 8.0, 2.5


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
    ap.add_argument("--shapes", default=None, help="Q,N,k;Q,N,k;... instead of the built-in list")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    import clip
    from cclip_hip import ops
    from clip.model import normalized_logits
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    gen = torch.Generator(device="cuda").manual_seed(567)
    zero = torch.zeros(1, device="cuda")                      # logit_scale = 0: exp(0) = 1, plain cosine
    galleries = {}
    for Q, N, k in shapes:
        if N not in galleries:
            galleries.clear()                                  # one gallery at a time on the device
            g32 = torch.randn(N, E, device="cuda", generator=gen)
            galleries[N] = (g32, clip.EmbeddingIndex(g32, dtype=dtype))
        g32, index = galleries[N]
        q32 = torch.randn(Q, E, device="cuda", generator=gen)
        q16 = clip.retrieval.normalize_rows(q32, dtype)

        def fused():
            return index.search(q32, k)

        def kernel():
            return ops.similarity_topk(q16, index.features, k)

        def composed():
            logits = normalized_logits(q32, g32, zero)[0]
            return torch.topk(logits, k, dim=1)

        t = _alternate(dict(search=fused, composition=composed, kernel=kernel), args.reps, args.warmup)
        # same answer (up to 16-bit operand rounding): share of the fused hits found in the composition's top k
        idx_f, idx_c = fused()[1], composed()[1]
        agree = (idx_f[:, :, None] == idx_c[:, None, :]).any(dim=2).float().mean().item()
        km = statistics.median(t["kernel"]) * 1e-3
        out = dict(Q=Q, N=N, E=E, k=k, dtype=args.dtype, search_ms=_stat(t["search"]), composition_ms=_stat(t["composition"]),
                   kernel_ms=_stat(t["kernel"]),
                   speedup_median=round(statistics.median(t["composition"]) / statistics.median(t["search"]), 3),
                   gallery_GBps=round(N * E * 2 / km / 1e9, 1), gallery_share_of_peak=round(N * E * 2 / km / (PEAK_TBS * 1e12), 4),
                   TFLOPs=round(2.0 * Q * N * E / km / 1e12, 2), flop_share_of_peak=round(2.0 * Q * N * E / km / (PEAK_PFLOPS * 1e15), 4),
                   matrix_bytes=4 * Q * N, workspace_bytes=ops.similarity_topk_workspace(Q, N, k),
                   topk_overlap=round(agree, 4))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
