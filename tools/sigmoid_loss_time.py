#!/usr/bin/env python3
"""Microseconds on one MI355X of the sigmoid (SigLIP) loss against the softmax loss it sits next to, at the contrastive head's
shapes [1024, 1024] and [1024, 8192] (rows x columns of the logits; E = 512 features):

  * one `ops.sigmoid_rows` launch against one `ops.xent_rows_classes` launch, both with every output on (loss rows, arg-max,
    hit, fp32 gradient, rowdot; the sigmoid kernel also rowsum).  The sigmoid kernel reads each logit once and writes it once;
    the softmax kernel reads it twice (the second time from L2 at these sizes) and writes it once.  Per element the sigmoid
    kernel spends exp, log and rcp against one exp per pass.
  * the full `clip.sigmoid_loss` forward + backward against the full `clip.contrastive_loss` forward + backward on the same
    features and classes (square [1024, 1024]: labels alone; [1024, 8192]: 1024 images against 8192 texts, text_labels).
    The sigmoid loss runs one logits GEMM, one row-kernel launch and two gradient GEMMs, the softmax loss two, two and four.

All legs of a shape run in this one process and alternate sample by sample.  A sample is `--launches` back-to-back calls between
two device events; the first `--warmup` samples of each leg are discarded; median [min max] of the rest.  The kernel legs write
the gradient to a buffer of their own, so every launch reads the same logits.  One JSON line per shape; `--out FILE` also writes
the lines there.

Where a kernel is shorter than the host's time per call ([1024, 1024]: see profiles/class_loss_time.txt) the window is the
launch rate, not kernel time: take kernel times from a `rocprofv3 --kernel-trace --stats` run of its own (second line below).
The loss legs time whole Python calls (a dozen launches plus autograd each): host and device time together.

    python tools/sigmoid_loss_time.py [--reps 30] [--warmup 5] [--launches 50] [--out profiles/sigmoid_loss_time.txt]
    rocprofv3 --kernel-trace --stats -- python tools/sigmoid_loss_time.py --shape 1024x8192 --kernels-only     # kernel times
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from loss_time import _alternate, _stat  # noqa: E402

SHAPES = [(1024, 1024), (1024, 8192)]
CLASSES = 9
E = 512


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--loss-calls", type=int, default=5, help="forward + backward passes per sample of the loss legs")
    ap.add_argument("--shape", action="append", default=None, metavar="RxC", help="time this shape only (repeatable)")
    ap.add_argument("--kernels-only", action="store_true", help="skip the loss legs (for a kernel trace of one shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.launches < 1 or args.loss_calls < 1:
        ap.error("at least 7 timed samples after 2 discarded")
    import clip
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    lines = []
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shape] if args.shape else SHAPES
    for R, C in shapes:
        lg = torch.randn(R, C, device="cuda", generator=gen) * 3
        d = torch.empty_like(lg)
        loss_row, rowdot, rowsum, hit = (torch.empty(R, device="cuda") for _ in range(4))
        pred = torch.empty(R, device="cuda", dtype=torch.int32)
        row_class = torch.randint(0, CLASSES, (R,), device="cuda", generator=gen, dtype=torch.int32)
        col_class = torch.randint(0, CLASSES, (C,), device="cuda", generator=gen, dtype=torch.int32)
        bias = torch.tensor([-10.0], device="cuda")
        gs = 1.0 / R

        def sigmoid():
            ops.sigmoid_rows(lg, row_class, col_class, bias, loss_row=loss_row, pred=pred, hit=hit, dlogits=d, grad_scale=gs,
                             rowdot=rowdot, rowsum=rowsum)

        def classes():
            ops.xent_rows_classes(lg, row_class, col_class, loss_row=loss_row, pred=pred, hit=hit, dlogits=d, grad_scale=gs,
                                  rowdot=rowdot)

        t = _alternate(dict(sigmoid_rows=sigmoid, xent_rows_classes=classes), args.reps, args.warmup, args.launches)
        k0, k1 = statistics.median(t["xent_rows_classes"]), statistics.median(t["sigmoid_rows"])
        out = dict(R=R, C=C, E=E, launches_per_sample=args.launches, loss_calls_per_sample=args.loss_calls,
                   sigmoid_rows_us=_stat(t["sigmoid_rows"]), xent_rows_classes_us=_stat(t["xent_rows_classes"]),
                   ratio_sigmoid_over_classes=round(k1 / k0, 3),
                   sigmoid_rows_GBps=round((2 * 4 * R * C + 4 * C) / k1 / 1e3, 1))      # logits read once, gradient written once
        if args.kernels_only:
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            continue

        fi = torch.randn(R, E, device="cuda", generator=gen, requires_grad=True)
        ft = torch.randn(C, E, device="cuda", generator=gen, requires_grad=True)
        ls = torch.tensor(2.6593, device="cuda", requires_grad=True)
        lb = torch.tensor(-10.0, device="cuda", requires_grad=True)
        kw = dict(labels=row_class) if R == C else dict(labels=row_class, text_labels=col_class)

        def sigmoid_loss():
            clip.sigmoid_loss(fi, ft, ls, lb, **kw)[0].backward()

        def contrastive_loss():
            clip.contrastive_loss(fi, ft, ls, **kw)[0].backward()

        u = _alternate(dict(sigmoid_loss=sigmoid_loss, contrastive_loss=contrastive_loss), args.reps, args.warmup, args.loss_calls)
        l0, l1 = statistics.median(u["contrastive_loss"]), statistics.median(u["sigmoid_loss"])
        out.update(sigmoid_loss_fwd_bwd_us=_stat(u["sigmoid_loss"]), contrastive_loss_fwd_bwd_us=_stat(u["contrastive_loss"]),
                   ratio_sigmoid_loss_over_contrastive=round(l1 / l0, 3))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
