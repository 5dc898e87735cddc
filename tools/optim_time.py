"""Time the grouped AdamW step against the plain one at the ViT-B/32 arena size, on the device.

Four legs over the same flat buffers (N fp32 elements + a 16-bit shadow), in ONE process, alternating leg by leg in every round
so that drift and neighbours on the host hit all of them alike:
  plain         ops.adamw_step                                                    (the step without the new keywords)
  plain+torch   ops.adamw_step + torch.linalg.vector_norm + mul_ + lerp_          (clip and EMA composed from torch ops)
  groups        ops.adamw_step_groups, 28 groups, no scalar, no EMA
  groups+all    ops.sumsq + ops.adamw_step_groups with the clip scalar and the EMA
Each sample is `--calls` back-to-back calls between two device events; reported: median [min max] per call over `--rounds`
samples after `--warmup` rounds.  Bytes per parameter are arithmetic (30 plain, 38 with the EMA, + 4 for the norm's read), the
rates derive from them.

    python tools/optim_time.py [--out profiles/optim_groups_time.txt]
"""
from __future__ import annotations

import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "construction-clip_amd"))

N_VIT_B32 = 151_277_313                      # parameters of CLIP ViT-B/32


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=(N_VIT_B32 + 65535) // 65536 * 65536)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--dtype", choices=("bfloat16", "float16"), default="bfloat16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_groups_time.txt"))
    args = ap.parse_args(argv)
    import torch
    from cclip_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("optim_time: no GPU; this tool measures on the device only")
    dev, n = "cuda", args.n
    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=g) * 0.02
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    sh = torch.zeros(n, device=dev, dtype=getattr(torch, args.dtype))
    G = 28
    table = (torch.arange(n // 64, device=dev) // max(1, n // 64 // G)).clamp_(max=G - 1).to(torch.uint8)
    lrs, wds = [1e-5 * 0.75 ** (k // 2) for k in range(G)], [0.1 * (k % 2) for k in range(G)]
    ss, ws = torch.zeros(1, device=dev), torch.empty(ops.sumsq_workspace(n) // 4, device=dev)
    hyp = dict(beta1=0.9, beta2=0.999, eps=1e-6, step=10, grad_scale=1.0, mode=0, bf16_shadow=sh)

    def plain():
        ops.adamw_step(p, gr, m, v, lr=1e-5, weight_decay=0.1, **hyp)

    def plain_torch():
        coef = (1.0 / (torch.linalg.vector_norm(gr) + 1e-6)).clamp_(max=1.0)
        gr.mul_(coef)
        ops.adamw_step(p, gr, m, v, lr=1e-5, weight_decay=0.1, **hyp)
        ema.lerp_(p, 1e-4)

    def groups():
        ops.adamw_step_groups(p, gr, m, v, table, lrs=lrs, weight_decays=wds, **hyp)

    def groups_all():
        ops.sumsq(gr, out=ss, workspace=ws)
        ops.adamw_step_groups(p, gr, m, v, table, lrs=lrs, weight_decays=wds, sumsq_dev=ss, max_norm=1.0, ema=ema, ema_decay=0.9999, **hyp)

    legs = [("plain", plain, 30), ("plain+torch", plain_torch, 30 + 4 + 8 + 12), ("groups", groups, 30), ("groups+all", groups_all, 38 + 4)]
    times = {name: [] for name, _, _ in legs}
    for r in range(args.warmup + args.rounds):
        for name, fn, _ in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b) / args.calls)
    lines = [f"# tools/optim_time.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  n = {n} fp32 elements, "
             f"{args.dtype} shadow, {G} groups; per call, median [min max] over {args.rounds} samples of {args.calls} calls, legs alternating",
             "# bytes/param are arithmetic (reads + writes of the leg), GB/s = n * bytes / median"]
    for name, _, nbytes in legs:
        t = times[name]
        med = statistics.median(t)
        lines.append(f"{name:12s} {med:8.3f} ms [{min(t):.3f} {max(t):.3f}]   {nbytes:3d} B/param   {n * nbytes / med / 1e6:8.0f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
