#!/usr/bin/env python3
"""Milliseconds and peak device memory of the two Gaussian-model kernels on one MI355X against their torch compositions on the
same device and the same 16-bit rows:
  * `ops.class_moments` (csrc/embed_moments.hip) against x.float().T @ x.float() plus an index_add_ of the fp32 rows;
  * `ops.gauss_scores` (csrc/gauss_scores.hip) against x.float() @ T.T, torch.cdist(...) ** 2, min / argmin / logsumexp.
Default shapes: the stored set N = 262144, C = 9, D = 512; queries Q = 65536 with R = D.  A timed call sits between two device
events and ends in a synchronise; peak_bytes is what a call allocates above its inputs.  The legs alternate call by call in one
process; the first `--warmup` calls of every leg are discarded; median [min max] of the rest.  One JSON line per kernel.
Each kernel's comparison is one GPU step and runs under its own time limit: without --only this process never opens the GPU,
it starts one fresh child per step under `--timeout` seconds and stops at the first that fails or runs out of time.

    python tools/gaussian_time.py [--timeout 300] [--reps 7] [--warmup 2] [--n 262144] [--c 9] [--d 512] [--q 65536]
    timeout -k 10 300 python tools/gaussian_time.py --only moments
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def _timed(fn):
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


def _race(legs, reps, warmup):
    times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
    for r in range(reps + warmup):
        for leg, fn in legs.items():
            ms, peak = _timed(fn)
            peaks[leg] = max(peaks[leg], peak)
            if r >= warmup:
                times[leg].append(ms)
    return {leg: dict(ms=_stat(times[leg]), peak_bytes=peaks[leg]) for leg in legs}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--c", type=int, default=9)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--q", type=int, default=65536)
    ap.add_argument("--only", choices=("moments", "scores"), default=None, help="run this one step in this process")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each step may take when started from here")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    if args.only is None:
        for step in ("moments", "scores"):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", step, "--reps", str(args.reps), "--warmup", str(args.warmup),
                   "--n", str(args.n), "--c", str(args.c), "--d", str(args.d), "--q", str(args.q)]
            try:
                rc = subprocess.run(cmd, timeout=args.timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:                                    # nothing more is started on the GPU after a step that failed or hung
                print(f"gaussian_time: step {step!r} ended with status {rc}", file=sys.stderr)
                return rc
        return 0
    from cclip_hip import ops
    N, C, D, Q = args.n, args.c, args.d, args.q
    gen = torch.Generator(device="cuda").manual_seed(567)
    if args.only == "moments":
        x = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=gen), dim=1).bfloat16()
        y = torch.randint(0, C, (N,), device="cuda", generator=gen, dtype=torch.int32)
        yl = y.long()
        ws = torch.empty(ops.moments_workspace(N, C, D) // 4, device="cuda")
        out = (torch.empty(C, device="cuda", dtype=torch.int32), torch.empty(C, D, device="cuda"), torch.empty(D, D, device="cuda"))

        def kernel():
            ops.class_moments(x, y, C, out=out, workspace=ws)

        def composed():
            xf = x.float()
            g = xf.T @ xf
            s = torch.zeros(C, D, device="cuda").index_add_(0, yl, xf)
            return g, s, torch.bincount(yl, minlength=C)

        g, s, _ = composed()
        kernel()
        apart = dict(gram=float((out[2] - g).abs().max()), sum=float((out[1] - s).abs().max()))
        line = dict(what="class_moments", N=N, C=C, D=D, parts=ops.moments_parts(N, C, D), workspace_bytes=ws.numel() * 4,
                    max_abs_apart=apart, **_race(dict(class_moments_hip=kernel, torch_fp32=composed), args.reps, args.warmup))
        line["kernel_over_torch"] = round(line["class_moments_hip"]["ms"]["median"] / line["torch_fp32"]["ms"]["median"], 3)
        print(json.dumps(line), flush=True)
        del x, y, yl, ws, out, g, s
    if args.only == "scores":
        x = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=gen), dim=1).bfloat16()
        T = torch.randn(D, D, device="cuda", generator=gen)
        t0 = torch.randn(D, device="cuda", generator=gen)
        m = torch.randn(C, D, device="cuda", generator=gen)
        off = torch.randn(C, device="cuda", generator=gen)
        res = {}

        def kernel():
            res["k"] = ops.gauss_scores(x, T, t0=t0, centres=m, offset=off)

        def composed():
            z = x.float() @ T.T - t0
            d2 = torch.cdist(z, m) ** 2
            score = -0.5 * d2 + off
            dmin, nearest = d2.min(1)
            res["t"] = (score.argmax(1), torch.logsumexp(score, 1), nearest, dmin)

        kernel()
        composed()
        apart = dict(dmin_relative=float(((res["k"][3] - res["t"][3]).abs() / res["t"][3]).max()),
                     pred_differs=int((res["k"][0].long() != res["t"][0]).sum()))
        line = dict(what="gauss_scores", Q=Q, C=C, D=D, R=D, workspace_bytes=ops.gauss_scores_workspace(D, D), apart=apart,
                    **_race(dict(gauss_scores_hip=kernel, torch_fp32=composed), args.reps, args.warmup))
        line["kernel_over_torch"] = round(line["gauss_scores_hip"]["ms"]["median"] / line["torch_fp32"]["ms"]["median"], 3)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
