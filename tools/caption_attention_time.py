#!/usr/bin/env python3
"""What `return_attention=True` costs: generate_beam (one caption) and generate_beam_batch (--captions captions) at a GPT-2
geometry, with and without the flag, plus the probability kernel alone.

Each call is timed with device events (recorded before the call and after it, then synchronised), after --warmup discarded
calls; the figure is the median of --reps calls, with the smallest and the largest next to it.  The search runs without a
stop token, so every call decodes exactly --entry-length tokens per beam and replays sequences of prefix + attribute +
entry_length - 1 positions: the same work in every repetition.  Weights are seeded; nothing is read from disk.

    python tools/caption_attention_time.py                    # GPT-2 small, 3 beams, 100 tokens, 21 captions
    python tools/caption_attention_time.py --no-attention     # only the calls without the flag (also runs on a tree without it)
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


class _Tok:
    def encode(self, s):
        return [int(x) for x in s.split()]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def timed(fn, reps: int, warmup: int):
    """milliseconds between device events around fn(): (median, min, max) of `reps` calls after `warmup` discarded ones"""
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="ckiplab/gpt2-base-chinese")
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--entry-length", type=int, default=100)
    ap.add_argument("--captions", type=int, default=21)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bf16", action="store_true", help="bf16 operands (default IEEE fp16)")
    ap.add_argument("--no-attention", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args(argv)
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("caption_attention_time: no GPU - this tool only measures on the device")

    from clip_caption import (ClipCaptionModel, GPT2_MODELS, generate_beam, generate_beam_batch, init_caption_state_dict,
                              synthetic_caption_batch)
    geo = GPT2_MODELS[args.geometry]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 77))
    model = model.cuda().eval()
    model.bfloat16() if args.bf16 else model.half()
    N = args.captions
    _, _, prefix, attribute = synthetic_caption_batch(N, geo, 6, 78)
    with torch.no_grad():
        pre = model.clip_project(prefix.cuda()).view(N, geo.prefix_length, geo.n_embd)
        emb = torch.cat((pre, model.gpt.transformer.wte(attribute.cuda())), dim=1)
    tok = _Tok()
    kw = dict(beam_size=args.beam, entry_length=args.entry_length, stop_token=-1)
    out = {"label": args.label, "geometry": args.geometry, "operands": "bf16" if args.bf16 else "fp16", "beams": args.beam,
           "entry_length": args.entry_length, "captions": N, "prefix_positions": emb.shape[1], "reps": args.reps,
           "warmup": args.warmup, "unit": "ms (median, min, max)"}
    flags = (False,) if args.no_attention else (False, True, False, True)       # alternating: the spread shows in the repeats
    for i, flag in enumerate(flags):
        extra = {"return_attention": True} if flag else {}
        tag = ("with" if flag else "without") + f"_attention_{i // 2}"
        out[f"generate_beam_{tag}"] = timed(lambda: generate_beam(model, tok, embed=emb[:1], **kw, **extra), args.reps, args.warmup)
        out[f"generate_beam_batch_{tag}"] = timed(lambda: generate_beam_batch(model, tok, emb, **kw, **extra), args.reps, args.warmup)
    if not args.no_attention:
        from cclip_hip import ops
        H, T, B = geo.n_head, emb.shape[1] + args.entry_length, 3                # B*H = 36, T = 140 at the defaults
        D = H * 64
        qkv = torch.randn(B * T, 3 * D, device="cuda").to(model.compute_dtype)
        rows = torch.arange(emb.shape[1] - 1, emb.shape[1] - 1 + args.entry_length, device="cuda", dtype=torch.int32)
        for name, r in (("all_rows", None), ("entry_length_rows", rows)):
            P = torch.empty(B, H, T if r is None else r.numel(), T, device="cuda")
            launches = 200

            def burst():
                for _ in range(launches):
                    ops.attention_probs(qkv[:, :D], qkv[:, D:2 * D], P, B=B, T=T, H=H, causal=True, q_rows=r)
            med, lo, hi = timed(burst, args.reps, args.warmup)
            out[f"probs_kernel_BH{B * H}_T{T}_{name}_us_per_launch_of_{launches}_back_to_back"] = (
                1e3 * med / launches, 1e3 * lo / launches, 1e3 * hi / launches)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
