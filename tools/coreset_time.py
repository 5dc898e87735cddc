#!/usr/bin/env python3
"""Milliseconds and peak device memory of one k-centre greedy pick on one MI355X: `ops.coreset_step` from the partial keys
(csrc/coreset.hip, one launch) and the same launch enqueued by `ops.coreset_greedy`'s native loop, against the torch
composition that also reads nothing back - c = argmax(w * mind), index_select, x @ x_c, minimum, where - on the same device and
the same unit bf16 rows, at N in {20 000, 1 000 000}, D in {64, 512}, with random weights.  A timed call is `--inner` picks
between two device events, ending in a synchronise; ms are per pick.  The legs alternate call by call in one process, each on
its own state; the first `--warmup` calls of every leg are discarded; median [min max] of the rest.  step_bytes = 2 N D is what a
pick must move at least (every row read once; the state is 8 N more) and share_of_hbm_peak = step_bytes / 8.0 TB/s (the spec
peak) over the step's median.  Before timing, the two ways are checked against each other: from equal states the kernel's
pick must carry the composition's largest key within the bf16 rounding of the composition's distances.  One JSON line per shape.

    python tools/coreset_time.py [--reps 7] [--warmup 2] [--inner 50] [--sizes 20000,1000000] [--dims 64,512]
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


class Composition:
    """the torch way, state on the device, no read: a chosen row has distance 0 and so the smallest key"""

    def __init__(self, x, w, first):
        N = x.shape[0]
        self.x, self.w = x, w
        self.mind = torch.full((N,), float("inf"), device=x.device)
        self.owner = torch.full((N,), -1, dtype=torch.int64, device=x.device)
        self.update(torch.tensor(first, device=x.device))

    def update(self, c):
        d = 1.0 - torch.mv(self.x, self.x.index_select(0, c.reshape(1))[0])
        self.owner = torch.where(d < self.mind, c, self.owner)
        self.mind = torch.minimum(self.mind, d)
        self.mind[c] = 0.0

    def pick(self):
        c = torch.argmax(self.w * self.mind)
        d = 1.0 - torch.mv(self.x, self.x.index_select(0, c.reshape(1))[0])
        self.owner = torch.where(d < self.mind, c, self.owner)
        self.mind = torch.minimum(self.mind, d)
        return c


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=50, help="picks per timed call")
    ap.add_argument("--sizes", default="20000,1000000")
    ap.add_argument("--dims", default="64,512")
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.inner < 1:
        ap.error("at least 7 timed calls after 2 discarded, --inner >= 1")
    from cclip_hip import ops
    import clip
    gen = torch.Generator(device="cuda").manual_seed(567)
    for N in (int(v) for v in args.sizes.split(",")):
        for D in (int(v) for v in args.dims.split(",")):
            x = clip.EmbeddingIndex(torch.randn(N, D, device="cuda", generator=gen)).features
            w = 0.25 + 0.75 * torch.rand(N, device="cuda", generator=gen)
            P = ops.coreset_blocks(N)

            def state():
                mind = torch.full((N,), float("inf"), device="cuda")
                owner = torch.full((N,), -1, dtype=torch.int32, device="cuda")
                ws = torch.zeros(2, P, dtype=torch.int64, device="cuda")
                ops.coreset_greedy(x, mind, owner, 1, first=0, workspace=ws, weight=w)      # keys of the state now in ws[1]
                return [mind, owner, ws, 1]

            st_step, st_loop, comp = state(), state(), Composition(x, w, 0)
            # the two ways pick alike from equal states: the kernel's row carries the composition's largest key, within the
            # rounding of the composition's bf16 distances (2^-8 relative on values up to 2)
            chk = state()
            pick, _ = ops.coreset_step(x, chk[0], chk[1], chk[2][0], partial_in=chk[2][1], weight=w)
            c_ref = Composition(x, w, 0).pick()
            key0 = w * (1.0 - torch.mv(x, x[0]).float())
            key0[0] = 0.0
            agree = bool((key0[pick.long()] >= key0[c_ref] - 2.0 ** -6).all().item())
            del chk, key0
            ws_loop = st_loop[2].flip(0).contiguous()          # the native loop reads workspace[0] first

            def step_leg():
                mind, owner, ws, cur = st_step
                for _ in range(args.inner):
                    ops.coreset_step(x, mind, owner, ws[1 - cur], partial_in=ws[cur], weight=w)
                    cur = 1 - cur
                st_step[3] = cur

            def loop_leg():
                ops.coreset_greedy(x, st_loop[0], st_loop[1], args.inner, workspace=ws_loop, weight=w)
                if args.inner % 2:
                    ws_loop.copy_(ws_loop.flip(0))

            def composed():
                for _ in range(args.inner):
                    comp.pick()

            legs = dict(coreset_step_hip=step_leg, coreset_greedy_hip=loop_leg, composition=composed)
            times, peaks = {n: [] for n in legs}, {n: 0 for n in legs}
            for r in range(args.reps + args.warmup):
                for leg, fn in legs.items():
                    ms, peak = _timed(fn)
                    peaks[leg] = max(peaks[leg], peak)
                    if r >= args.warmup:
                        times[leg].append(ms / args.inner)
            step_bytes = 2 * N * D
            med = statistics.median(times["coreset_step_hip"])
            med_loop = statistics.median(times["coreset_greedy_hip"])
            line = dict(N=N, D=D, blocks=P, inner=args.inner, step_bytes=step_bytes, state_bytes=8 * N, first_picks_agree=agree)
            for leg in legs:
                line[leg] = dict(ms=_stat(times[leg]), peak_bytes=peaks[leg])
            line["share_of_hbm_peak"] = round(step_bytes / HBM_PEAK / (min(med, med_loop) * 1e-3), 4)
            line["speedup_median_step"] = round(statistics.median(times["composition"]) / med, 3)
            line["speedup_median_greedy"] = round(statistics.median(times["composition"]) / med_loop, 3)
            print(json.dumps(line), flush=True)
            del x, w, st_step, st_loop, comp, ws_loop
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
