#!/usr/bin/env python3
"""Explained captions straight from image files - the loop of the reference's root predict.py:57-86 on the MI355X packages,
through `clip_caption.Captioner.explain`: per image the two zero-shot heads, the generated caption, the relevance of every image
patch and caption token for (image, own caption), and the relevance overlay (`clip.relevance_overlay`).  One JSON line per image
(file, caption_type, violation_type, prediction, top_patch, png) and one overlay PNG per image in --out-dir; --html also writes
explained.html with every caption's token heat (`clip.text_heat_html`) under its overlay.  The matplotlib figure and its title
fonts are not carried over.

    python scripts/explain_images.py photos/ --clip-checkpoint clip.pt --checkpoint model.pt --relevance-checkpoint clip_rel.pt
    python scripts/explain_images.py --synthetic --out-dir /tmp/explained --html        # offline: seeded models, generated images"""
from __future__ import annotations

import argparse
import html
import os
import tempfile

import _common as C
import torch

from describe_images import SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".webp")
_BPE = None


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="*", help="image files and / or directories of them")
    ap.add_argument("--clip-model", default="ViT-B/32")
    ap.add_argument("--clip-checkpoint", default=None, help="fine-tuned CLIP state dict for the heads and the prefix (predict.py:45)")
    ap.add_argument("--relevance-checkpoint", default=None,
                    help="CLIP state dict of a second model that computes the relevance (predict.py:46); default: the first model")
    ap.add_argument("--checkpoint", default=None, help="ClipCaptionModel state dict (default: CCLIP_GPT2_CHECKPOINT, else seeded)")
    ap.add_argument("--tokenizer", default="ckiplab/gpt2-base-chinese")
    ap.add_argument("--gpt2", default=None, help="geometry name in clip_caption.GPT2_MODELS (default: the tokenizer's)")
    ap.add_argument("--out-dir", default="explained")
    ap.add_argument("--size", type=int, default=224, help="side of the overlay pictures")
    ap.add_argument("--bs", type=int, default=16, help="images per Captioner.explain call")
    ap.add_argument("--beam_size", type=int, default=3)
    ap.add_argument("--entry_length", type=int, default=100)
    ap.add_argument("--start-layer", type=int, default=-1)
    ap.add_argument("--start-layer-text", type=int, default=-1)
    ap.add_argument("--html", action="store_true", help="also write explained.html (overlay + token heat per image)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=3, help="--synthetic: images to explain")
    return ap


def list_images(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(IMAGE_SUFFIXES)]
        else:
            files.append(p)
    return files


def setup(args):
    """(captioner, relevance model or None, image files, temporary directory or None) for the parsed arguments"""
    import clip
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        C.make_synthetic_annotations(tmp.name, per_class=1 + (args.n_images - 1) // len(C.CLASSES))
        d = os.path.join(tmp.name, "images")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d))][:args.n_images]
        geo = GPT2_MODELS["test-tiny"]
        tokenizer = C.ByteCaptionTokenizer(geo.vocab_size)
        labels = dict(caption_types=SYNTHETIC_TYPES, violation_types=SYNTHETIC_VIOLATIONS)
        args.clip_model = "test-tiny"
    else:
        files = list_images(args.images)
        geo = GPT2_MODELS[args.gpt2 or args.tokenizer]
        from transformers import AutoTokenizer                   # the reference's tokenizer (a local copy: no network here)
        tokenizer = AutoTokenizer.from_pretrained(args.tokenizer)
        labels = {}

    def load_clip(checkpoint):
        model, _ = clip.load(args.clip_model, device=device, jit=False)
        if checkpoint:
            model.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True))
        return model.eval()

    clip_model = load_clip(args.clip_checkpoint)                                              # predict.py:49
    relevance_model = load_clip(args.relevance_checkpoint) if args.relevance_checkpoint else None   # predict.py:50
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    ckpt = args.checkpoint or (None if args.synthetic else os.environ.get("CCLIP_GPT2_CHECKPOINT"))
    model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True) if ckpt else init_caption_state_dict(geo, 567))
    model = model.to(device).eval()
    cap = Captioner(clip_model, model, tokenizer, clip_tokenize=C.get_tokenize(clip_model), prefix_length=geo.prefix_length,
                    attribute_length=geo.attribute_length, **labels)
    return cap, relevance_model, files, tmp


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
    from PIL import Image
    cap, relevance_model, files, tmp = setup(args)
    if not files:
        raise SystemExit("no images given (or --synthetic)")
    os.makedirs(args.out_dir, exist_ok=True)
    out, page = [], []
    for i in range(0, len(files), args.bs):
        chunk = files[i:i + args.bs]
        records = cap.explain([Image.open(f) for f in chunk], size=args.size, relevance_model=relevance_model,
                              start_layer=args.start_layer, start_layer_text=args.start_layer_text, beam_size=args.beam_size,
                              entry_length=args.entry_length)
        for j, (f, r) in enumerate(zip(chunk, records)):
            png = os.path.join(args.out_dir, f"{i + j:05d}_{os.path.splitext(os.path.basename(f))[0]}.png")
            Image.fromarray(r["overlay"]).save(png)
            line = dict(file=f, caption_type=r["caption_type"], violation_type=r["violation_type"], prediction=r["prediction"],
                        top_patch=int(r["image_relevance"].argmax()), png=png)
            C.log_line(**line)
            out.append(line)
            if args.html:
                # one score per CLIP token of the caption; the pieces shown are those tokens' texts where a vocabulary is
                # loaded (clip.tokenize), the caption's UTF-8 bytes under the stand-in tokenizer
                scores = r["token_scores"].cpu()
                page.append(f'<h3>{html.escape(r["caption_type"])} {html.escape(r["violation_type"])}</h3>'
                            f'<img src="{html.escape(os.path.basename(png))}" alt="overlay">'
                            + clip.text_heat_html(token_pieces(r, scores.shape[0]), scores))
    if args.html:
        path = os.path.join(args.out_dir, "explained.html")
        with open(path, "w", encoding="utf-8") as fh:
            fh.write('<!doctype html><html><head><meta charset="utf-8"><title>explained captions</title></head><body>'
                     + "".join(page) + "</body></html>")
        C.log_line(saved=path)
    if tmp is not None:
        tmp.cleanup()
    return out


def token_pieces(record, n: int):
    """the text of caption tokens 1 .. EOT-1, one string per score"""
    ids = [int(t) for t in record["clip_tokens"][1:1 + n]]
    if os.environ.get("CCLIP_BPE_PATH"):
        global _BPE
        if _BPE is None:
            from clip.simple_tokenizer import SimpleTokenizer
            _BPE = SimpleTokenizer()
        return [_BPE.decode([t]) for t in ids]
    raw = record["prediction"].encode("utf-8")[:n]                 # _common.byte_tokenize: one id per byte
    return [bytes([b]).decode("latin-1") for b in raw] + [""] * (n - len(raw))


if __name__ == "__main__":
    main()
