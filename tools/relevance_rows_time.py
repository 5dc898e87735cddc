#!/usr/bin/env python3
"""Milliseconds per clip.interpret_rows (bf16): next to clip.interpret on ViT-B/32 at N in {1, 8, 1024} pairs, start layers -1
and 0; alone on ViT-B/16 (197 image tokens) and ViT-L/14@336px (577) at N in {1, 8}, where clip.interpret does not run; and the
row relevance kernel's own time per launch at (T, heads) = (50, 12), (197, 12), (577, 16), from a dense r (every query tile
runs) and from a one-hot r (one query tile per sequence: the default start_layer = -1).
Device events around `reps` calls after `warmup` calls; prints one JSON line.

    python tools/relevance_rows_time.py [--reps 5] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    import clip
    from cclip_hip import ops
    from clip.weights import MODELS, init_state_dict, synthetic_text
    g = torch.Generator(device="cuda").manual_seed(0)
    out = dict(dtype="bf16", interpret_rows_ms={}, interpret_ms={}, kernel_us={})
    for name, ns, full in (("ViT-B/32", (1, 8, 1024), True), ("ViT-B/16", (1, 8), False), ("ViT-L/14@336px", (1, 8), False)):
        geo = MODELS[name]
        model = clip.build_model(init_state_dict(geo, 567)).cuda()
        res = geo.image_resolution
        for n in ns:
            img = torch.randn(1, 3, res, res, device="cuda", generator=g)
            txt = synthetic_text(n, geo, 1).cuda()
            for s in (-1, 0):
                ms = _time(lambda: clip.interpret_rows(img, txt, model, start_layer=s, start_layer_text=s), args.reps, args.warmup)
                out["interpret_rows_ms"][f"{name}_n{n}_start{s}"] = round(ms, 3)
                if full:
                    ms = _time(lambda: clip.interpret(img, txt, model, start_layer=s, start_layer_text=s), args.reps, args.warmup)
                    out["interpret_ms"][f"{name}_n{n}_start{s}"] = round(ms, 3)
        del model
        torch.cuda.empty_cache()
    for T, H, B in ((50, 12, 1024), (197, 12, 256), (577, 16, 64)):
        D = 64 * H
        qkv = torch.randn(B * T, 3 * D, device="cuda", generator=g).to(torch.bfloat16)
        da = (torch.randn(B * T, D, device="cuda", generator=g) * 1e-2).to(torch.bfloat16)
        lse = torch.full((B, H, T), 4.0, device="cuda")
        dense = torch.randn(B, T, device="cuda", generator=g)
        one_hot = torch.zeros(B, T, device="cuda")
        one_hot[:, 0] = 1
        r_out = torch.empty(B, T, device="cuda")
        for tag, r_in in (("dense", dense), ("one_hot", one_hot)):
            def k():
                ops.attention_relevance_row(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], lse, da, r_in, r_out, B=B, T=T, H=H)
            out["kernel_us"][f"T{T}_H{H}_B{B}_{tag}"] = round(1000 * _time(k, 20, 3), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
