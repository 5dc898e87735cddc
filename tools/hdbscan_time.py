#!/usr/bin/env python3
"""Milliseconds and peak device memory of the spanning-tree hot path of HDBSCAN on one MI355X (csrc/mst.hip): one Boruvka
round's N^2 search, `ops.mreach_nearest` - per row the closest row outside its component under mutual-reachability similarity -
against the torch composition that also reads nothing back: x @ x.T in the stored dtype, `minimum` with the two cores, the
mask on `comp`, `max(dim=1)`; and a whole tree, `ops.mst_boruvka` (every round enqueued by one native call).  Same device, same
unit bf16 rows - `--centres` planted directions plus noise - at N in {20 000, 100 000}, D in {64, 512}, min_samples 5, the
components of the round being the singletons of round 0.  A timed call sits between two device events and ends in a
synchronise; the legs alternate call by call in one process; the first `--warmup` calls of every leg are discarded; median
[min max] of the rest.  round_flops = 2 N^2 D.  `live_rounds` is the number of Boruvka rounds that found more than one
component (read from the round flags after the timing).  Before timing, the two ways are checked against each other: the
composition's maximum, rounded to the stored dtype as it is, must lie within that rounding of the kernel's fp32 value.  One
JSON line per shape.

    python tools/hdbscan_time.py [--reps 7] [--warmup 2] [--sizes 20000,100000] [--dims 64,512]
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
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - before


def _stat(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4), n=len(ts))


def composition(x, core16, comp):
    """the torch way, nothing read back: (best m in the stored dtype [N], its row [N])"""
    s = x @ x.t()
    s = torch.minimum(torch.minimum(s, core16[:, None]), core16[None, :])
    s.masked_fill_(comp[:, None] == comp[None, :], float("-inf"))
    return s.max(dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--dims", default="64,512")
    ap.add_argument("--centres", type=int, default=50)
    ap.add_argument("--min-samples", type=int, default=5)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2:
        ap.error("at least 7 timed calls after 2 discarded")
    from cclip_hip import ops
    import clip
    gen = torch.Generator(device="cuda").manual_seed(567)
    for N in (int(v) for v in args.sizes.split(",")):
        for D in (int(v) for v in args.dims.split(",")):
            dirs = torch.randn(args.centres, D, device="cuda", generator=gen)
            dirs = dirs / dirs.norm(dim=1, keepdim=True)
            which = torch.randint(0, args.centres, (N,), device="cuda", generator=gen)
            feats = dirs[which] + 0.5 / D ** 0.5 * torch.randn(N, D, device="cuda", generator=gen)
            x = clip.EmbeddingIndex(feats).features
            del feats
            core = ops.similarity_topk(x, x, args.min_samples)[0][:, args.min_samples - 1].contiguous()
            core16 = core.to(x.dtype)
            comp = torch.arange(N, dtype=torch.int32, device="cuda")
            keys = torch.empty(N, dtype=torch.int64, device="cuda")
            ws = torch.empty((ops.mst_workspace(N) + 7) // 8, dtype=torch.int64, device="cuda")

            got = ops.mreach_nearest(x, core, comp, out=keys)
            hi = (got >> 32) & 0xFFFFFFFF
            bits = torch.where(hi >= 0x80000000, hi ^ 0x80000000, ~hi & 0xFFFFFFFF)            # the key back to fp32 bits
            mine = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
            theirs = composition(x, core16, comp)[0].float()
            agree = bool(((mine - theirs).abs() <= 2.0 ** -7 * mine.abs().clamp(min=2.0 ** -7)).all().item())
            del got, hi, bits, mine, theirs

            legs = dict(mreach_nearest_hip=lambda: ops.mreach_nearest(x, core, comp, out=keys),
                        composition=lambda: composition(x, core16, comp),
                        mst_boruvka_hip=lambda: ops.mst_boruvka(x, core, workspace=ws))
            times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
            for r in range(args.reps + args.warmup):
                for leg, fn in legs.items():
                    ms, peak = _timed(fn)
                    peaks[leg] = max(peaks[leg], peak)
                    if r >= args.warmup:
                        times[leg].append(ms)
            flags = ws.view(torch.int32)[8 * N: 8 * N + 64]
            live = int(flags.sum().item())
            flops = 2.0 * N * N * D
            med = statistics.median(times["mreach_nearest_hip"])
            line = dict(N=N, D=D, min_samples=args.min_samples, splits=ops.mreach_nearest_splits(N), round_flops=flops,
                        rounds_enqueued=max(0, (N - 1).bit_length()), live_rounds=live, values_agree=agree)
            for leg in legs:
                line[leg] = dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
            line["round_tflops"] = round(flops / (med * 1e-3) / 1e12, 1)
            line["composition_over_hip"] = round(statistics.median(times["composition"]) / med, 3)
            line["tree_over_round"] = round(statistics.median(times["mst_boruvka_hip"]) / med, 2)
            print(json.dumps(line), flush=True)
            del x, core, core16, comp, keys, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
