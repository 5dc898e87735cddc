#!/usr/bin/env python3
"""Microseconds per launch on one MI355X of the class-aware row kernel (`ops.xent_rows_classes`) against its pairwise sibling
(`ops.xent_rows`), both with every output on (loss rows, arg-max, fp32 gradient, rowdot; the class-aware one also `hit`), at
the contrastive head's shapes [1024, 1024] and [1024, 8192].  The class-aware kernel moves the same logits bytes (two reads,
one write) plus one int32 per column, so the expectation is parity.

Both legs run in this one process and alternate sample by sample.  A sample is `--launches` back-to-back launches between two
device events (one launch is a few microseconds: below what a pair of events resolves); the first `--warmup` samples of each
leg are discarded; median [min max] of the rest.  The gradient goes to a buffer of its own, so every launch reads the same
logits.  One JSON line per shape; `--out FILE` also writes the lines there.

Where a kernel is shorter than the host's time per call (measured: [1024, 1024], 7.6 us of kernel under a 12.5 us window), the
window is the launch rate, not kernel time: take kernel times from `rocprofv3 --kernel-trace --stats -- python tools/loss_time.py`
in a run of its own.

    python tools/loss_time.py [--reps 30] [--warmup 5] [--launches 50] [--out profiles/class_loss_time.txt]
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

SHAPES = [(1024, 1024), (1024, 8192)]
CLASSES = 9


def _alternate(legs, reps, warmup, launches):
    """legs: {name: fn}.  reps + warmup rounds, one sample of every leg per round; microseconds per launch of the kept rounds."""
    times = {n: [] for n in legs}
    for r in range(reps + warmup):
        for n, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[n].append(e0.elapsed_time(e1) * 1e3 / launches)
    return times


def _stat(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3), n=len(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.launches < 1:
        ap.error("at least 7 timed samples after 2 discarded")
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    lines = []
    for R, C in SHAPES:
        lg = torch.randn(R, C, device="cuda", generator=gen)
        d = torch.empty_like(lg)
        loss_row, rowdot, hit = (torch.empty(R, device="cuda") for _ in range(3))
        pred = torch.empty(R, device="cuda", dtype=torch.int32)
        labels = torch.randint(0, C, (R,), device="cuda", generator=gen, dtype=torch.int32)
        row_class = torch.randint(0, CLASSES, (R,), device="cuda", generator=gen, dtype=torch.int32)
        col_class = torch.randint(0, CLASSES, (C,), device="cuda", generator=gen, dtype=torch.int32)
        gs = 1.0 / (2 * R)

        def pairwise():
            ops.xent_rows(lg, labels, loss_row=loss_row, pred=pred, dlogits=d, grad_scale=gs, rowdot=rowdot)

        def classes():
            ops.xent_rows_classes(lg, row_class, col_class, loss_row=loss_row, pred=pred, hit=hit, dlogits=d, grad_scale=gs,
                                  rowdot=rowdot)

        t = _alternate(dict(xent_rows=pairwise, xent_rows_classes=classes), args.reps, args.warmup, args.launches)
        m0, m1 = statistics.median(t["xent_rows"]), statistics.median(t["xent_rows_classes"])
        moved = 3 * 4 * R * C                                   # logits read twice, gradient written once
        out = dict(R=R, C=C, launches_per_sample=args.launches, xent_rows_us=_stat(t["xent_rows"]),
                   xent_rows_classes_us=_stat(t["xent_rows_classes"]), ratio_classes_over_pairwise=round(m1 / m0, 3),
                   xent_rows_GBps=round(moved / m0 / 1e3, 1), xent_rows_classes_GBps=round((moved + 4 * C) / m1 / 1e3, 1))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
