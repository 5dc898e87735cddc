#!/usr/bin/env python3
"""Milliseconds and peak device memory of one objective evaluation of the linear probe on one MI355X, D = 512:
`ops.probe_forward` + `ops.probe_backward` (csrc/embed_probe.hip: forward, partial gradients, merge, objective) against the
torch composition it replaces (`x32 @ W.T + b`, `cross_entropy`, autograd, the l2 term), once on a fp32 copy of x converted
beforehand (`composition_fp32_copy`: it keeps a second, fp32 copy of the store, which is not counted in its peak) and once with
the conversion inside the call (`composition_convert`), at N in {20 000, 10^6} and C in {16, 256}, both 16-bit types.  The legs
alternate call by call in one process; each call sits between two device events and ends in a synchronise; the first
`--warmup` calls of every leg are discarded; median [min max] of the rest.  A composition that does not fit the device is
reported as "out of memory", not timed.  One JSON line per (N, C, dtype).

    python tools/probe_time.py [--reps 7] [--warmup 2] [--sizes 20000,1000000] [--cs 16,256] [--dtypes bf16,fp16]
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
    ap.add_argument("--cs", default="16,256")
    ap.add_argument("--dtypes", default="bf16,fp16")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    l2 = 1e-3
    for N in (int(v) for v in args.sizes.split(",")):
        for C in (int(v) for v in args.cs.split(",")):
            for name in args.dtypes.split(","):
                dtype = dict(bf16=torch.bfloat16, fp16=torch.float16)[name]
                x = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=gen), dim=1).to(dtype)
                y = torch.randint(0, C, (N,), device="cuda", generator=gen)
                y32 = y.to(torch.int32)
                W = torch.randn(C, D, device="cuda", generator=gen)
                b = torch.zeros(C, device="cuda")
                x32 = x.float()

                def fused():
                    lse, loss, _, _ = ops.probe_forward(x, W, b, y32)
                    return ops.probe_backward(x, W, b, y32, lse, 1.0 / N, l2, loss=loss)

                def composed(rows):
                    Wp, bp = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
                    f = torch.nn.functional.cross_entropy(rows @ Wp.t() + bp, y) + 0.5 * l2 * (Wp * Wp).sum()
                    f.backward()
                    return Wp.grad, bp.grad, f.detach()

                legs = dict(probe_hip=fused, composition_fp32_copy=lambda: composed(x32), composition_convert=lambda: composed(x.float()))
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
                line = dict(N=N, C=C, D=D, dtype=name, logits_bytes_fp32=4 * N * C, fp32_copy_bytes=4 * N * D,
                            workspace_bytes=ops.probe_workspace(N, C, D))
                for leg in legs:
                    line[leg] = failed[leg] if leg in failed else dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
                for leg in ("composition_fp32_copy", "composition_convert"):
                    if leg not in failed and "probe_hip" not in failed:
                        line["speedup_vs_" + leg] = round(statistics.median(times[leg]) / statistics.median(times["probe_hip"]), 3)
                print(json.dumps(line), flush=True)
                del x, x32, y, y32, W, b


if __name__ == "__main__":
    main()
