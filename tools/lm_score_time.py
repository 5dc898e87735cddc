#!/usr/bin/env python3
"""What `ClipCaptionModel.score` costs next to the two ways of getting the same numbers it replaces, on one build:

  score         model.score(...)                               the fused lm_head scoring kernel, no logits
  caption_loss  model.caption_loss(...) under no_grad          fp32 logits of the target rows + xent_rows (one scalar)
  forward       forward() + log_softmax + gather               fp32 logits of every position

at the real geometry (GPT-2 small, V = 21128, P = A = 20) with --batch captions of --caption-len tokens.  Each call is timed
with device events (recorded before the call and after it, then synchronised) after --warmup discarded calls; the three are
interleaved call by call, and the whole interleaved series is repeated --rounds times so that the spread between rounds shows
next to the medians.  Peak memory is torch.cuda.max_memory_allocated over one call of each, above what is allocated before it.
The stand-alone kernel (ops.lm_head_score on R = batch * caption-len rows) is timed too, with its arithmetic rate.
Weights and inputs are seeded; nothing is read from disk.

    python tools/lm_score_time.py                 # B = 256, Lc = 40, bf16
    python tools/lm_score_time.py --half          # IEEE fp16 operands
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd")]

import torch  # noqa: E402


def one(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak_mb(fn) -> float:
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="ckiplab/gpt2-base-chinese")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--caption-len", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--half", action="store_true", help="IEEE fp16 operands (default bf16)")
    ap.add_argument("--label", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lm_score_time: no GPU - this tool only measures on the device")

    from cclip_hip import ops
    from clip_caption import ClipCaptionModel, GPT2_MODELS, init_caption_state_dict, synthetic_caption_batch
    geo = GPT2_MODELS[args.geometry]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 77))
    model = model.cuda().eval()
    if args.half:
        model.half()
    B, Lc = args.batch, args.caption_len
    tokens, mask, prefix, attribute = [t.cuda() for t in synthetic_caption_batch(B, geo, Lc, 78)]
    P, A = geo.prefix_length, geo.attribute_length

    def f_score():
        return model.score(tokens, prefix, attribute, mask)

    def f_loss():
        with torch.no_grad():
            return model.caption_loss(tokens, prefix, attribute, mask)

    def f_forward():
        with torch.no_grad():
            sl = model(tokens, prefix, attribute, mask).logits[:, P + A - 1:-1]
            return torch.log_softmax(sl, -1).gather(2, tokens[:, :, None])

    calls = (("score", f_score), ("caption_loss", f_loss), ("forward", f_forward))
    out = {"label": args.label, "geometry": args.geometry, "operands": "fp16" if args.half else "bf16", "batch": B, "caption_len": Lc,
           "sequence": P + A + Lc, "vocab": geo.vocab_size, "scored_targets": int((tokens != 0).sum()), "reps": args.reps,
           "warmup": args.warmup, "rounds": args.rounds, "unit": "ms per call, device events: [median, min, max] per round"}
    agree = abs(f_score().loss.item() - f_loss().item())
    out["abs_loss_difference_score_vs_caption_loss"] = agree
    for name, fn in calls:
        out[f"{name}_ms"] = []
    for _ in range(args.rounds):
        ms = {name: [] for name, _ in calls}
        for i in range(args.warmup + args.reps):
            for name, fn in calls:                                   # interleaved: a drift of the machine hits all three alike
                t = one(fn)
                if i >= args.warmup:
                    ms[name].append(t)
        for name, _ in calls:
            out[f"{name}_ms"].append([round(statistics.median(ms[name]), 4), round(min(ms[name]), 4), round(max(ms[name]), 4)])
    for name, _ in calls:
        meds = [r[0] for r in out[f"{name}_ms"]]
        out[f"{name}_median_of_round_medians_ms"] = round(statistics.median(meds), 4)
        out[f"{name}_round_median_spread_ms"] = round(max(meds) - min(meds), 4)
    for name, fn in calls:
        out[f"{name}_peak_MiB_above_resident"] = round(peak_mb(fn), 1)

    # the kernel alone: R rows of ln_f output against the tied wte
    R, D, V = B * Lc, geo.n_embd, geo.vocab_size
    g = torch.Generator().manual_seed(79)
    x = torch.randn(R, D, generator=g).to(model.compute_dtype).cuda()
    w = model.arena.b["model.transformer.wte.weight"]
    labels = torch.randint(1, V, (R,), generator=g).to(torch.int32).cuda()
    bufs = [torch.empty(R, device="cuda", dtype=dt) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]

    def f_kernel():
        ops.lm_head_score(x, w, labels, ignore_index=0, logp=bufs[0], lse=bufs[1], pred=bufs[2], pred_logit=bufs[3])

    def f_logits_xent():
        logits = torch.empty(R, (V + 7) // 8 * 8, device="cuda", dtype=torch.float32)[:, :V]
        ops.gemm_bf16(x, w, out_f32=logits)
        ops.xent_rows(logits, labels, loss_row=bufs[0], ignore_index=0)

    kern = (("lm_head_score_kernel_pair", f_kernel), ("gemm_plus_xent_rows", f_logits_xent))
    for name, _ in kern:
        out[f"{name}_ms"] = []
    for _ in range(args.rounds):
        ms = {name: [] for name, _ in kern}
        for i in range(args.warmup + args.reps):
            for name, fn in kern:
                t = one(fn)
                if i >= args.warmup:
                    ms[name].append(t)
        for name, _ in kern:
            out[f"{name}_ms"].append([round(statistics.median(ms[name]), 4), round(min(ms[name]), 4), round(max(ms[name]), 4)])
    flop = 2.0 * R * D * V
    med = statistics.median(r[0] for r in out["lm_head_score_kernel_pair_ms"])
    out["lm_head_score_rows"] = R
    out["lm_head_score_gflop"] = round(flop / 1e9, 1)
    out["lm_head_score_tflops_at_median"] = round(flop / (med * 1e-3) / 1e12, 1)
    out["lm_head_score_workspace_MiB"] = round(ops.lm_head_score_workspace(R, V) / 2 ** 20, 2)
    out["fp32_logits_of_those_rows_MiB"] = round(R * V * 4 / 2 ** 20, 1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
