#!/usr/bin/env python3
"""Time and memory on one MI355X of the distillation row kernel against what it replaces, at square logits N = M = 1024 and
4096 (E = 512 features):

  * one `ops.kl_rows` launch, every output on (loss rows, arg-max, agree, fp32 gradient, rowdot), against the torch
    composition of the same quantities: `log_softmax` of both rows, `kl_div(..., log_target=True)` summed per row, and autograd
    for the gradient.  The kernel reads both [N, M] operands twice and writes one; the composition holds both log-softmaxes,
    the pointwise KL and the autograd temporaries, several [N, M] tensors at once.
  * the full `clip.distill_loss` forward + backward against the full `clip.contrastive_loss` forward + backward on the same
    student features: what one more objective costs a training step.  The distillation loss runs four logits GEMMs (two of
    them the teacher's) where the softmax loss runs two; the gradient GEMMs are the same four.

All legs of a shape run in this one process and alternate sample by sample.  A sample is `--launches` back-to-back calls between
two device events; the first `--warmup` samples of each leg are discarded; median [min max] of the rest, in milliseconds per
call.  Peak bytes are `torch.cuda.max_memory_allocated` over one more call of the leg, above what was allocated before it (the
inputs and the kernel leg's preallocated outputs are not counted; what a leg allocates while it runs is).  One JSON line per
shape; `--out FILE` also writes the lines there.

    python tools/distill_loss_time.py [--reps 7] [--warmup 2] [--launches 20] [--out profiles/distill_loss_time.txt]
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

from loss_time import _alternate  # noqa: E402

SIZES = [1024, 4096]
E = 512
LS, TS = 2.6593, 100.0


def _ms(ts):
    return dict(median=round(statistics.median(ts) / 1e3, 4), min=round(min(ts) / 1e3, 4), max=round(max(ts) / 1e3, 4), n=len(ts))


def _peak(fn):
    """bytes the call holds at its peak above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--loss-calls", type=int, default=5, help="forward + backward passes per sample of the loss legs")
    ap.add_argument("--size", action="append", type=int, default=None, metavar="N", help="time N = M = this only (repeatable)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.launches < 1 or args.loss_calls < 1:
        ap.error("at least 7 timed samples after 2 discarded")
    import clip
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    kl_div = torch.nn.functional.kl_div
    lines = []
    for N in args.size or SIZES:
        lg = torch.randn(N, N, device="cuda", generator=gen) * 3
        te = torch.randn(N, N, device="cuda", generator=gen) * 3
        d = torch.empty_like(lg)
        loss_row, rowdot, agree = (torch.empty(N, device="cuda") for _ in range(3))
        pred = torch.empty(N, device="cuda", dtype=torch.int32)
        gs = 1.0 / (2 * N)
        lg_leaf = lg.clone().requires_grad_(True)

        def kernel():
            ops.kl_rows(lg, te, loss_row=loss_row, pred=pred, agree=agree, dlogits=d, grad_scale=gs, rowdot=rowdot)

        def torch_composition():
            rows = kl_div(torch.log_softmax(lg_leaf, 1), torch.log_softmax(te, 1), reduction="none", log_target=True).sum(1)
            g, = torch.autograd.grad(rows.sum() * gs, lg_leaf)
            return rows, g, (g * lg).sum(1), lg.argmax(1), lg.argmax(1) == te.argmax(1)

        kernel()
        rows, g = torch_composition()[:2]
        apart = dict(loss_row=(loss_row - rows.detach()).abs().max().item(), dlogits=(d - g).abs().max().item())
        t = _alternate(dict(kl_rows=kernel, torch_composition=torch_composition), args.reps, args.warmup, args.launches)
        k0, k1 = statistics.median(t["torch_composition"]), statistics.median(t["kl_rows"])
        out = dict(N=N, M=N, E=E, launches_per_sample=args.launches, loss_calls_per_sample=args.loss_calls,
                   kl_rows_ms=_ms(t["kl_rows"]), torch_composition_ms=_ms(t["torch_composition"]),
                   ratio_kl_rows_over_torch=round(k1 / k0, 3),
                   kl_rows_GBps=round(5 * 4 * N * N / k1 / 1e3, 1),            # two operands read twice, the gradient written once
                   kl_rows_peak_bytes=_peak(kernel), torch_composition_peak_bytes=_peak(torch_composition),
                   max_abs_apart=apart)

        fi = torch.randn(N, E, device="cuda", generator=gen, requires_grad=True)
        ft = torch.randn(N, E, device="cuda", generator=gen, requires_grad=True)
        ti = torch.randn(N, E, device="cuda", generator=gen)
        tt = torch.randn(N, E, device="cuda", generator=gen)
        ls = torch.tensor(LS, device="cuda", requires_grad=True)

        def distill_loss():
            clip.distill_loss(fi, ft, ls, ti, tt, TS)[0].backward()

        def contrastive_loss():
            clip.contrastive_loss(fi, ft, ls)[0].backward()

        u = _alternate(dict(distill_loss=distill_loss, contrastive_loss=contrastive_loss), args.reps, args.warmup, args.loss_calls)
        l0, l1 = statistics.median(u["contrastive_loss"]), statistics.median(u["distill_loss"])
        out.update(distill_loss_fwd_bwd_ms=_ms(u["distill_loss"]), contrastive_loss_fwd_bwd_ms=_ms(u["contrastive_loss"]),
                   ratio_distill_over_contrastive=round(l1 / l0, 3),
                   distill_loss_peak_bytes=_peak(distill_loss), contrastive_loss_peak_bytes=_peak(contrastive_loss))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
