#!/usr/bin/env python3
"""Milliseconds and peak device memory of one t-SNE iteration on one MI355X: `ops.tsne_repulsion` + `ops.tsne_step`
(csrc/tsne.hip) against the torch composition of the same arithmetic on the same device (`cdist`^2 -> w -> row sums, the
repulsion as a dense product, the attraction through a sparse CSR product, gains and momentum elementwise - which forms
several dense N x N fp32 matrices), at N in {5 000, 20 000, 200 000} on a random map of scale 10 and a symmetrised random
30-neighbour graph.  The legs alternate call by call in one process; each call sits between two device events and ends in a
synchronise; the first `--warmup` calls of every leg are discarded; median [min max] of the rest.  A composition whose three
dense matrices exceed the device's memory is reported as "does not fit" and not run.  The repulsion call is also timed alone:
pairs_per_s = N (N - 1) / its median.  Last, one whole `clip.tsne` call (N = 20 000, D = 64, perplexity 10, 1000 iterations)
by the host clock around a synchronise.  One JSON line per size and one for the whole call.

    python tools/tsne_time.py [--reps 7] [--warmup 2] [--sizes 5000,20000,200000] [--whole 20000]
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

K_NEIGHBOURS = 30


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
    ap.add_argument("--sizes", default="5000,20000,200000")
    ap.add_argument("--whole", type=int, default=20000, help="N of the whole clip.tsne call (0 = skip)")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    from cclip_hip import ops
    T = importlib.import_module("clip.tsne")
    gen = torch.Generator(device="cuda").manual_seed(567)
    ex, mom, lr, mg = 12.0, 0.5, 200.0, 0.01
    for N in (int(v) for v in args.sizes.split(",")):
        y = 10.0 * torch.randn(N, 2, device="cuda", generator=gen)
        # 30 distinct other rows per row: row + d mod N with distinct d in 1 .. N - 1 from a random start
        start = torch.randint(0, N - 1, (N, 1), device="cuda", generator=gen)
        d = 1 + (start + 97 * torch.arange(K_NEIGHBOURS, device="cuda")[None, :]) % (N - 1)
        index = ((torch.arange(N, device="cuda")[:, None] + d) % N).to(torch.int32)
        P = torch.full((N, K_NEIGHBOURS), 1.0 / K_NEIGHBOURS, device="cuda")
        offsets, cols, vals = T.joint_csr(P, index)
        rows = torch.repeat_interleave(torch.arange(N, device="cuda"), offsets.diff())
        cols64 = cols.long()
        vel, gains = 0.1 * torch.randn(N, 2, device="cuda", generator=gen), torch.ones(N, 2, device="cuda")
        y2, zrow, rep = torch.empty_like(y), torch.empty(N, device="cuda"), torch.empty_like(y)
        z, kl = torch.empty(1, device="cuda"), torch.empty(N, device="cuda")
        ws = torch.empty(ops.tsne_repulsion_workspace(N) // 4, device="cuda")

        def repulsion():
            return ops.tsne_repulsion(y, out_zrow=zrow, out_rep=rep, out_z=z, workspace=ws)

        def fused():
            repulsion()
            return ops.tsne_step(y, vel.clone(), gains.clone(), offsets, cols, vals, rep, z, exaggeration=ex, momentum=mom,
                                 learning_rate=lr, min_gain=mg, out_y=y2, out_kl=kl)

        def composed():
            w = torch.cdist(y, y).square_().add_(1.0).reciprocal_()             # dense N x N
            w.fill_diagonal_(0.0)
            zr = w.sum(dim=1)
            Z = zr.sum()
            pw = ex * vals * w[rows, cols64]
            w2 = w * w                                                          # dense N x N
            r = w2.sum(dim=1, keepdim=True) * y - w2 @ y
            A = torch.sparse_csr_tensor(offsets, cols64, pw, (N, N))
            row_pw = torch.zeros(N, device="cuda").index_add_(0, rows, pw)
            att = row_pw[:, None] * y - A @ y
            grad = 4.0 * (att - r / Z)
            g = torch.where((vel > 0) != (grad > 0), gains + 0.2, gains * 0.8).clamp_(min=mg)
            v = mom * vel - lr * g * grad
            return y + v, g, v

        legs = dict(tsne_hip=fused, composition=composed, repulsion_alone=repulsion)
        total = torch.cuda.mem_get_info()[1]
        failed = {}
        if 3 * 4 * N * N > total:
            failed["composition"] = f"does not fit: three dense N x N fp32 matrices are {3 * 4 * N * N / 2 ** 30:.0f} GiB, the device has {total / 2 ** 30:.0f} GiB"
        times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
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
        line = dict(N=N, nnz=int(cols.numel()), splits=ops.tsne_repulsion_splits(N), dense_matrix_bytes=4 * N * N,
                    state_bytes=int(ws.numel() * 4 + 9 * N * 4 + cols.numel() * 8 + (N + 1) * 8))
        for leg in legs:
            line[leg] = failed[leg] if leg in failed else dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
        if "repulsion_alone" not in failed:
            line["pairs_per_s"] = float(f"{N * (N - 1) / (statistics.median(times['repulsion_alone']) * 1e-3):.4g}")
        if not failed:
            line["speedup_median"] = round(statistics.median(times["composition"]) / statistics.median(times["tsne_hip"]), 3)
        print(json.dumps(line), flush=True)
        del y, index, P, offsets, cols, vals, rows, cols64, vel, gains, ws, start, d
        torch.cuda.empty_cache()

    if args.whole:
        import clip
        N = args.whole
        dirs = torch.nn.functional.normalize(torch.randn(20, 64, device="cuda", generator=gen), dim=1)
        x = dirs[torch.randint(0, 20, (N,), device="cuda", generator=gen)] + 0.5 / 8.0 * torch.randn(N, 64, device="cuda", generator=gen)
        x = clip.EmbeddingIndex(x).features
        clip.tsne(x, perplexity=10, n_iter=5)                                    # warm-up: code objects, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        res = clip.tsne(x, perplexity=10, n_iter=1000)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        print(json.dumps(dict(whole_call=dict(N=N, D=64, perplexity=10, n_iter=1000, seconds=round(sec, 3),
                                              ms_per_iteration=round(1e3 * sec / 1000, 4), kl_divergence=round(res.kl_divergence, 4),
                                              peak_bytes=torch.cuda.max_memory_allocated() - before))), flush=True)


if __name__ == "__main__":
    main()
