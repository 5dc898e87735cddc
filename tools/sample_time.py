#!/usr/bin/env python3
"""Microseconds on one MI355X of the row-sampling kernel against the torch composition it replaces, and of generate_sample
against generate2:

  * one `ops.sample_rows` launch (csrc/sample_rows.hip: temperature, top-k, nucleus and the draw) against softmax -> sort ->
    cumsum -> mask (the reference's filter, test.py:492-500) -> renormalise -> `torch.multinomial` -> gather of the
    log-probability, on seeded N(0, 3^2) logits [n, V] for n in {1, 8, 64} and V in {21128, 50257}, at top_p = 0.8 and at
    top_p = 1 (no filter: every token is kept and takes part in the draw);
  * `generate_sample` with K in {1, 8} samples against `generate2` (the persistent greedy kernel) on the GPT-2-small caption
    geometry (V = 21128, 12 layers, prefix 20 + attribute 20), `--entry-length` positions, a stop token that is never drawn, so
    every call decodes the same number of positions.  These legs time whole Python calls: host and device time together.

All legs of a shape run in this one process and alternate sample by sample.  A sample is `--launches` back-to-back calls between
two device events; the first `--warmup` samples of each leg are discarded; median [min max] of the rest.  One JSON line per
shape; `--out FILE` also writes the lines there.

    python tools/sample_time.py [--reps 20] [--warmup 3] [--launches 20] [--out profiles/sample_time.txt]
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

ROWS = [1, 8, 64]
VOCABS = [21128, 50257]


def torch_sample(logits, top_p, gen):
    """the host-side sampler, launch by launch: (token, log-probability)"""
    p = logits.softmax(-1)
    sp, si = p.sort(descending=True)
    remove = sp.cumsum(-1) > top_p
    remove[:, 1:] = remove[:, :-1].clone()
    remove[:, 0] = False
    kept = sp.masked_fill(remove, 0.0)
    pick = torch.multinomial(kept / kept.sum(-1, keepdim=True), 1, generator=gen)
    return si.gather(1, pick), sp.gather(1, pick).log()


class _Tok:
    def encode(self, s):
        return [int(x) for x in s.split()]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--entry-length", type=int, default=32)
    ap.add_argument("--generate-calls", type=int, default=2, help="calls per sample of the generate legs")
    ap.add_argument("--kernels-only", action="store_true", help="skip the generate legs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.reps < 7 or args.warmup < 2 or args.launches < 1 or args.generate_calls < 1:
        ap.error("at least 7 timed samples after 2 discarded")
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(567)
    lines = []
    for V in VOCABS:
        for n in ROWS:
            lg = torch.randn(n, V, device="cuda", generator=gen) * 3
            u = torch.rand(n, device="cuda", generator=gen)
            done = torch.zeros(n, device="cuda", dtype=torch.int32)
            outs = dict(token=torch.empty(n, device="cuda", dtype=torch.int32), logprob=torch.empty(n, device="cuda"),
                        n_kept=torch.empty(n, device="cuda", dtype=torch.int32), kept_mass=torch.empty(n, device="cuda"))
            legs = {}
            for top_p in (0.8, 1.0):
                legs[f"sample_rows_p{top_p}"] = lambda top_p=top_p: ops.sample_rows(lg, u, done, top_p=top_p, **outs)
                legs[f"torch_p{top_p}"] = lambda top_p=top_p: torch_sample(lg, top_p, gen)
            t = _alternate(legs, args.reps, args.warmup, args.launches)
            out = dict(n=n, V=V, launches_per_sample=args.launches, **{k + "_us": _stat(v) for k, v in t.items()})
            for top_p in (0.8, 1.0):
                out[f"ratio_torch_over_kernel_p{top_p}"] = round(statistics.median(t[f"torch_p{top_p}"]) /
                                                                 statistics.median(t[f"sample_rows_p{top_p}"]), 2)
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
    if not args.kernels_only:
        from clip_caption import (ClipCaptionModel, GPT2_MODELS, generate2, generate_sample, init_caption_state_dict,
                                  synthetic_caption_batch)
        geo = GPT2_MODELS["ckiplab/gpt2-base-chinese"]
        model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
        model.load_state_dict(init_caption_state_dict(geo, 567))
        model = model.cuda().eval()
        _, _, prefix, attribute = synthetic_caption_batch(1, geo, 6, 568)
        with torch.no_grad():
            emb = torch.cat((model.clip_project(prefix.cuda()).view(1, geo.prefix_length, geo.n_embd),
                             model.gpt.transformer.wte(attribute.cuda())), dim=1)
        E, tok = args.entry_length, _Tok()
        legs = dict(generate2=lambda: generate2(model, tok, embed=emb, entry_length=E, stop_token=-1))
        for K in (1, 8):
            legs[f"generate_sample_K{K}"] = lambda K=K: generate_sample(model, tok, embed=emb, num_samples=K, entry_length=E,
                                                                        stop_token=-1, generator=gen)
        t = _alternate(legs, args.reps, args.warmup, args.generate_calls)
        out = dict(geometry="ckiplab/gpt2-base-chinese", entry_length=E, calls_per_sample=args.generate_calls,
                   **{k + "_us": _stat(v) for k, v in t.items()})
        for K in (1, 8):
            out[f"us_per_position_K{K}"] = round(statistics.median(t[f"generate_sample_K{K}"]) / E, 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
