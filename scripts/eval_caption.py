#!/usr/bin/env python3
"""Held-out evaluation of a caption model: embedding pickle + checkpoint -> one JSON line with the teacher-forced loss,
perplexity, token accuracy and exact-caption rate (clip_caption.evaluate_captions).  The loss is train.py:354-357's
cross-entropy (ignore_index 0) over the whole set; no logits are materialised.

    python scripts/eval_caption.py --data ./data/val_embedding.pkl --checkpoint checkpoints/caption-009.pt --bs 64
    python scripts/eval_caption.py --synthetic --bs 8          # offline: seeded state dict, toy tokenizer"""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C
import torch
from torch.utils.data import DataLoader


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="./data/embedding.pkl")
    ap.add_argument("--checkpoint", default=None, help="ClipCaptionModel state dict (default: CCLIP_GPT2_CHECKPOINT, else seeded)")
    ap.add_argument("--prefix_length", type=int, default=None)
    ap.add_argument("--attribute_length", type=int, default=None)
    ap.add_argument("--normalize_prefix", action="store_true")
    ap.add_argument("--tokenizer", default="ckiplab/gpt2-base-chinese")
    ap.add_argument("--gpt2", default=None, help="geometry name in clip_caption.GPT2_MODELS (default: the tokenizer's)")
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--half", action="store_true", help="IEEE fp16 operands (default bf16)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--gpt2_synthetic", default="test-tiny", help="--synthetic: geometry")
    args = ap.parse_args(argv)

    from clip_caption import ClipCaptionModel, GPT2_MODELS, evaluate_captions, init_caption_state_dict
    from clip_caption.data import ClipCocoDataset
    device = torch.device("cuda:0")
    tmp, tokenizer = None, None
    if args.synthetic:
        from train_caption import make_synthetic_pickle
        geo = GPT2_MODELS[args.gpt2_synthetic]
        tmp = tempfile.TemporaryDirectory()
        args.data = os.path.join(tmp.name, "embedding.pkl")
        make_synthetic_pickle(args.data, geo)
        tokenizer = C.ByteCaptionTokenizer(geo.vocab_size)
    else:
        geo = GPT2_MODELS[args.gpt2 or args.tokenizer]
    P = args.prefix_length or geo.prefix_length
    A = args.attribute_length or geo.attribute_length
    dataset = ClipCocoDataset(args.data, P, A, gpt2_type=args.tokenizer, normalize_prefix=args.normalize_prefix, tokenizer=tokenizer)
    model = ClipCaptionModel(P, prefix_size=geo.prefix_size, gpt2_type=geo)
    ckpt = args.checkpoint or (None if args.synthetic else os.environ.get("CCLIP_GPT2_CHECKPOINT"))
    if ckpt:
        model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True))
    else:
        model.load_state_dict(init_caption_state_dict(geo, 567))
    model = model.to(device).eval()
    if args.half:
        model.half()
    res = evaluate_captions(model, DataLoader(dataset, batch_size=args.bs, shuffle=False, drop_last=False))
    C.log_line(**res)
    if tmp is not None:
        tmp.cleanup()
    return res


if __name__ == "__main__":
    main()
