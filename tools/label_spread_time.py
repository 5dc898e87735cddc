#!/usr/bin/env python3
"""Milliseconds and peak device memory of one label-spreading iteration on one MI355X: `ops.label_spread_step`
(csrc/label_spread.hip, one launch) against the torch composition `alpha * (S_sparse_csr @ F) + (1 - alpha) * Y` on the same
device and the same normalised graph, at N in {20 000, 1 000 000}, C in {2, 9, 64}, k = 15 random neighbours per row
symmetrised (about 30 entries per row) and 1 % of the rows labelled.  A timed call is `--inner` iterations between two
buffers, between two device events and ending in a synchronise; ms are per iteration.  The legs alternate call by call in
one process; the first `--warmup` calls of every leg are discarded; median [min max] of the rest.  step_bytes is what the
iteration must move at least - F read once and written once, cols, vals, offsets and labels read once - and
share_of_hbm_peak = step_bytes / 8.0 TB/s (the spec peak; 6.29 TB/s is the measured copy rate) over the step's median;
gathered_bytes = nnz * 4 C is what the lanes actually request from the caches.  Last, one whole `clip.spread_labels` call (N =
20 000, D = 64, C = 9, k = 15, 50 iterations) by the host clock around a synchronise, run twice: the two results must be
bitwise equal, or the tool fails.  One JSON line per shape and one for the whole call.

    python tools/label_spread_time.py [--reps 7] [--warmup 2] [--inner 20] [--sizes 20000,1000000] [--classes 2,9,64] [--whole 20000]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

K_NEIGHBOURS = 15
ALPHA = 0.9
HBM_PEAK = 8.0e12


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
    return dict(median=round(statistics.median(ts), 5), min=round(min(ts), 5), max=round(max(ts), 5), n=len(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20, help="iterations per timed call")
    ap.add_argument("--sizes", default="20000,1000000")
    ap.add_argument("--classes", default="2,9,64")
    ap.add_argument("--whole", type=int, default=20000, help="N of the whole clip.spread_labels call (0 = skip)")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.inner < 1:
        ap.error("at least 7 timed calls after 2 discarded, --inner >= 1")
    from cclip_hip import ops
    P = importlib.import_module("clip.propagate")
    gen = torch.Generator(device="cuda").manual_seed(567)
    for N in (int(v) for v in args.sizes.split(",")):
        # 15 distinct other rows per row: row + d mod N with distinct d in 1 .. N - 1 from a random start
        start = torch.randint(0, N - 1, (N, 1), device="cuda", generator=gen)
        d = 1 + (start + 97 * torch.arange(K_NEIGHBOURS, device="cuda")[None, :]) % (N - 1)
        index = ((torch.arange(N, device="cuda")[:, None] + d) % N).to(torch.int32)
        scores = 0.5 + 0.5 * torch.rand(N, K_NEIGHBOURS, device="cuda", generator=gen)
        offsets, cols, vals = P.affinity_csr(scores, index, 5.5)
        ops.label_graph_normalize(offsets, cols, vals, out_vals=vals)
        nnz = int(cols.numel())
        S = torch.sparse_csr_tensor(offsets, cols.long(), vals, (N, N))
        del start, d, index, scores
        for C in (int(v) for v in args.classes.split(",")):
            labels = torch.where(torch.rand(N, device="cuda", generator=gen) < 0.01,
                                 torch.randint(0, C, (N,), device="cuda", generator=gen), torch.full((N,), -1, device="cuda"))
            lab32 = labels.to(torch.int32)
            cw = P.class_weights(labels, C)
            Y = torch.zeros(N, C, device="cuda")
            given = labels >= 0
            Y[given, labels[given]] = cw[labels[given]]
            bufs = [(1.0 - ALPHA) * Y, torch.empty(N, C, device="cuda")]

            def fused():
                for it in range(args.inner):
                    ops.label_spread_step(bufs[it % 2], lab32, offsets, cols, vals, ALPHA, cw, out_F=bufs[1 - it % 2], delta=False)

            def composed():
                F = bufs[0]
                for it in range(args.inner):
                    F = ALPHA * (S @ F) + (1.0 - ALPHA) * Y
                return F

            legs = dict(label_spread_hip=fused, composition=composed)
            times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
            for r in range(args.reps + args.warmup):
                for leg, fn in legs.items():
                    ms, peak = _timed(fn)
                    peaks[leg] = max(peaks[leg], peak)
                    if r >= args.warmup:
                        times[leg].append(ms / args.inner)
            # the two legs compute the same thing: one step from the same F
            one = ops.label_spread_step(bufs[0], lab32, offsets, cols, vals, ALPHA, cw)[0]
            ref = ALPHA * (S @ bufs[0]) + (1.0 - ALPHA) * Y
            agree = ((one - ref).abs() <= 64 * 2.0 ** -24 * ref.abs() + 1e-30).all().item()
            step_bytes = 2 * 4 * N * C + 8 * nnz + 8 * (N + 1) + 4 * N
            med = statistics.median(times["label_spread_hip"])
            line = dict(N=N, C=C, k=K_NEIGHBOURS, nnz=nnz, groups=ops.label_spread_groups(C), inner=args.inner, step_bytes=step_bytes,
                        gathered_bytes=4 * C * nnz, legs_agree=bool(agree))
            for leg in legs:
                line[leg] = dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
            line["share_of_hbm_peak"] = round(step_bytes / HBM_PEAK / (med * 1e-3), 4)
            line["speedup_median"] = round(statistics.median(times["composition"]) / med, 3)
            print(json.dumps(line), flush=True)
            del labels, lab32, cw, Y, bufs, one, ref
        del S, offsets, cols, vals
        torch.cuda.empty_cache()

    if args.whole:
        import clip
        N = args.whole
        dirs = torch.nn.functional.normalize(torch.randn(9, 64, device="cuda", generator=gen), dim=1)
        truth = torch.randint(0, 9, (N,), device="cuda", generator=gen)
        x = dirs[truth] + 1.0 / 8.0 * torch.randn(N, 64, device="cuda", generator=gen)
        x = clip.EmbeddingIndex(x).features
        labels = torch.where(torch.rand(N, device="cuda", generator=gen) < 0.01, truth, torch.full_like(truth, -1))
        clip.spread_labels(x, labels, n_classes=9, n_iter=2)                     # warm-up: code objects, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        res = clip.spread_labels(x, labels, n_classes=9, k=K_NEIGHBOURS, n_iter=50)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated() - before
        again = clip.spread_labels(x, labels, n_classes=9, k=K_NEIGHBOURS, n_iter=50)
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in
                   ((res.distributions, again.distributions), (res.confidence, again.confidence), (res.certainty, again.certainty)))
        same = same and torch.equal(res.pred, again.pred)
        un = labels < 0
        print(json.dumps(dict(whole_call=dict(N=N, D=64, C=9, k=K_NEIGHBOURS, n_iter=50, seconds=round(sec, 4), peak_bytes=peak,
                                              unlabelled_accuracy=round((res.pred[un] == truth[un]).float().mean().item(), 4),
                                              unreachable=int(res.unreachable.numel()), two_calls_bitwise_equal=bool(same)))), flush=True)
        if not same:
            raise SystemExit("label_spread_time: two fresh spread_labels calls differ")


if __name__ == "__main__":
    main()
