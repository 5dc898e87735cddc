#!/usr/bin/env python3
"""CLIP embeddings + zero-shot attributes of an annotated image set - /root/reference/CLIP_prefix_caption/parse_coco.py on the
MI355X packages: per annotation `encode_image`, the 2-way caption-type and 9-way violation-type heads,
`attribute = f'{caption_type} {violation_type} '`, `clip_embedding = i`; written as the pickle
{"clip_embedding": [N, E], "captions": [annotations]} that scripts/train_caption.py and scripts/predict_caption.py read.
Batched (`--bs` images per encode; the heads and the attribute ids are one kernel launch per batch, Captioner.embed).

    python scripts/extract_embeddings.py --json ../fengyu/fengyu_report.json --image-path .. --clip-checkpoint clip_latest.pt
    python scripts/extract_embeddings.py --synthetic --out /tmp/embedding.pkl       # offline: seeded weights, generated images"""
from __future__ import annotations

import argparse
import json
import os
import tempfile

import _common as C
import torch


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip_model_type", default="ViT-B/32")
    ap.add_argument("--clip-checkpoint", default=None, help="fine-tuned CLIP state dict (parse_coco.py:21-23)")
    ap.add_argument("--json", default="../fengyu/fengyu_report.json")
    ap.add_argument("--image-path", default="../")
    ap.add_argument("--out", default=None, help="default: ./embedding/<model>_report_embedding.pkl")
    ap.add_argument("--tokenizer", default="ckiplab/gpt2-base-chinese", help="caption tokenizer (sizes the attribute id table)")
    ap.add_argument("--attribute_length", type=int, default=20)
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=18, help="--synthetic: annotations to embed")
    ap.add_argument("--clip_synthetic", default="test-tiny", help="--synthetic: CLIP geometry")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
    from PIL import Image
    from clip_caption import Captioner
    from clip_caption.data import save_embeddings
    device = torch.device("cuda:0")
    tmp, labels = None, {}
    if args.synthetic:
        from describe_images import SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS
        tmp = tempfile.TemporaryDirectory()
        args.json = C.make_synthetic_annotations(tmp.name, per_class=1 + (args.n_images - 1) // len(C.CLASSES))
        args.image_path = tmp.name
        args.clip_model_type = args.clip_synthetic
        tokenizer = C.ByteCaptionTokenizer(300)
        labels = dict(caption_types=SYNTHETIC_TYPES, violation_types=SYNTHETIC_VIOLATIONS)
    else:
        from transformers import AutoTokenizer                   # a local copy: no network here
        tokenizer = AutoTokenizer.from_pretrained(args.tokenizer)
    out_path = args.out or f"./embedding/{args.clip_model_type.replace('/', '_')}_report_embedding.pkl"
    model, _ = clip.load(args.clip_model_type, device=device, jit=False)                      # parse_coco.py:20
    if args.clip_checkpoint:
        model.load_state_dict(torch.load(args.clip_checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    cap = Captioner(model, None, tokenizer, clip_tokenize=C.get_tokenize(model), attribute_length=args.attribute_length, **labels)
    annotations = json.load(open(args.json))["annotations"]
    if args.synthetic:
        annotations = annotations[:args.n_images]
    print("%0d captions loaded from json " % len(annotations))
    feats, captions = [], []
    n_vio = len(cap.violation_labels)
    for s in range(0, len(annotations), args.bs):
        chunk = annotations[s:s + args.bs]
        images = [Image.open(os.path.join(args.image_path, a["file_name"])) for a in chunk]
        f, index, _ = cap.embed(images, batch_size=args.bs)
        feats.append(f.cpu())
        for j, (a, (c, v)) in enumerate(zip(chunk, index.tolist())):
            a = dict(a)
            a["clip_embedding"] = s + j                                                    # parse_coco.py:55-56
            a["attribute"] = cap.attributes[c * n_vio + v]
            captions.append(a)
        C.log_line(done=len(captions), of=len(annotations))
    if tmp is not None:
        tmp.cleanup()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    save_embeddings(out_path, torch.cat(feats, dim=0), captions)
    C.log_line(saved=out_path, embeddings=len(captions))
    return out_path


if __name__ == "__main__":
    main()
