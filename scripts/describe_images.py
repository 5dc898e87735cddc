#!/usr/bin/env python3
"""Captions straight from image files - the loop of /root/reference/CLIP_prefix_caption/test.py:556-639 and the root
predict.py:57-86 on the MI355X packages, through `clip_caption.Captioner`: per image the CLIP encode, the two zero-shot heads
(caption type, violation type), the attribute prompt and the beam search, `--bs` images per call.  The records go to
output_<suffix>.json with the fields of test.py:626-633.  Plotting (export_plot) is not carried over.  `--best-of K` draws K
captions per image and keeps the one CLIP says matches the photo (Captioner.describe(best_of=K)).

    python scripts/describe_images.py --json ../test.json --image-path .. --clip-checkpoint clip.pt --checkpoint model.pt
    python scripts/describe_images.py --synthetic                # offline: seeded state dicts, toy tokenizers, generated images"""
from __future__ import annotations

import argparse
import json
import os
import tempfile

import _common as C
import torch

SYNTHETIC_TYPES = {"status": "a", "violation": "b"}                 # test-tiny has room for 4 attribute ids: one-byte labels
SYNTHETIC_VIOLATIONS = ["c", "d", "e", "f", "g", "h", "i", "j", "k"]


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="../test.json", help="annotation file ({'annotations': [{file_name, caption, ...}]})")
    ap.add_argument("--image-path", default="..", help="directory the annotations' file_name is relative to")
    ap.add_argument("--clip-model", default="ViT-B/32")
    ap.add_argument("--clip-checkpoint", default=None, help="fine-tuned CLIP state dict (test.py:602-604)")
    ap.add_argument("--checkpoint", default=None, help="ClipCaptionModel state dict (default: CCLIP_GPT2_CHECKPOINT, else seeded)")
    ap.add_argument("--tokenizer", default="ckiplab/gpt2-base-chinese")
    ap.add_argument("--gpt2", default=None, help="geometry name in clip_caption.GPT2_MODELS (default: the tokenizer's)")
    ap.add_argument("--prefix_length", type=int, default=None)
    ap.add_argument("--attribute_length", type=int, default=None)
    ap.add_argument("--out_dir", default=".")
    ap.add_argument("--suffix", default="ct")
    ap.add_argument("--bs", type=int, default=16, help="images per Captioner.describe call")
    ap.add_argument("--beam_size", type=int, default=3)
    ap.add_argument("--entry_length", type=int, default=None, help="default: 100 (beam), 67 (--greedy), as the reference")
    ap.add_argument("--greedy", action="store_true", help="generate2 (nucleus-filtered greedy) instead of generate_beam")
    ap.add_argument("--half", action="store_true", help="IEEE fp16 operands for the caption model (default bf16)")
    ap.add_argument("--attention-out", default=None, metavar="FILE.npz",
                    help="also store, per image i, attention_<i> [H, n, S0+n-1] (the best beam's last-layer rows) and map_<i> "
                         "(clip_caption.caption_attention_map of them: the reference's attention_map, test.py:342-349)")
    ap.add_argument("--sample", type=int, default=0, metavar="K",
                    help="also draw K captions per image from the model's distribution (clip_caption.generate_sample_batch); "
                         "each record gets \"samples\", best first by mean token log-probability")
    ap.add_argument("--top-p", type=float, default=0.8, help="--sample: nucleus mass (1 = off)")
    ap.add_argument("--top-k", type=int, default=0, help="--sample: keep the k most probable tokens (0 = off)")
    ap.add_argument("--temperature", type=float, default=1.0, help="--sample: softmax temperature")
    ap.add_argument("--seed", type=int, default=0, help="--sample / --best-of: seed of the draws (one seed, one set of captions)")
    ap.add_argument("--best-of", type=int, default=0, metavar="K",
                    help="draw K captions per image (with --top-p / --top-k / --temperature) and keep the one CLIP scores highest "
                         "against the photo instead of the beam caption; each record gets \"clip_score\" and \"candidates\"")
    ap.add_argument("--lm-weight", type=float, default=0.0, metavar="A",
                    help="--best-of: rank by cos(image, caption) + A * (mean token log-probability)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=9, help="--synthetic: images to describe")
    ap.add_argument("--clip_synthetic", default="test-tiny", help="--synthetic: CLIP geometry")
    ap.add_argument("--gpt2_synthetic", default="test-tiny", help="--synthetic: caption geometry")
    return ap


def setup(args):
    """(captioner, annotations, image directory, temporary directory or None) for the parsed arguments"""
    import clip
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        args.json = C.make_synthetic_annotations(tmp.name, per_class=1 + (args.n_images - 1) // len(C.CLASSES))
        args.image_path = tmp.name
        geo = GPT2_MODELS[args.gpt2_synthetic]
        tokenizer = C.ByteCaptionTokenizer(geo.vocab_size)
        labels = dict(caption_types=SYNTHETIC_TYPES, violation_types=SYNTHETIC_VIOLATIONS)
        args.clip_model = args.clip_synthetic
    else:
        geo = GPT2_MODELS[args.gpt2 or args.tokenizer]
        from transformers import AutoTokenizer                   # the reference's tokenizer (a local copy: no network here)
        tokenizer = AutoTokenizer.from_pretrained(args.tokenizer)
        labels = {}
    clip_model, _ = clip.load(args.clip_model, device=device, jit=False)                       # test.py:601
    if args.clip_checkpoint:
        clip_model.load_state_dict(torch.load(args.clip_checkpoint, map_location="cpu", weights_only=True))
    clip_model.eval()
    P = args.prefix_length or geo.prefix_length
    A = args.attribute_length or geo.attribute_length
    model = ClipCaptionModel(P, prefix_size=geo.prefix_size, gpt2_type=geo)
    ckpt = args.checkpoint or (None if args.synthetic else os.environ.get("CCLIP_GPT2_CHECKPOINT"))
    model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True) if ckpt else init_caption_state_dict(geo, 567))
    model = model.to(device).eval()
    if args.half:
        model.half()
    cap = Captioner(clip_model, model, tokenizer, clip_tokenize=C.get_tokenize(clip_model), prefix_length=P, attribute_length=A,
                    **labels)
    annotations = json.load(open(args.json))["annotations"]
    if args.synthetic:
        annotations = annotations[:args.n_images]
    return cap, annotations, args.image_path, tmp


@torch.no_grad()
def sample_captions(cap, images, args, generator):
    """--sample: K drawn captions per image, on the prefix Captioner.submit decodes from (projected features + attribute ids)"""
    from clip_caption import generate_sample_batch
    feat, _, ids = cap.embed(images)
    model = cap.caption_model
    proj = model.clip_project(feat).view(feat.shape[0], cap.prefix_length, -1)
    emb = torch.cat((proj, model.gpt.transformer.wte(ids.long())), dim=1)
    return generate_sample_batch(model, cap.tokenizer, emb, num_samples=args.sample, entry_length=args.entry_length or 67,
                                 top_p=args.top_p, top_k=args.top_k, temperature=args.temperature, generator=generator)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.sample < 0:
        raise SystemExit("--sample must be >= 0")
    if args.best_of < 0:
        raise SystemExit("--best-of must be >= 0")
    from PIL import Image
    cap, annotations, image_path, tmp = setup(args)
    log = {"caption": []}
    arrays = {}
    entry_length = args.entry_length or (67 if args.greedy else 100)
    generator = torch.Generator(device=cap.device).manual_seed(args.seed) if args.sample else None
    best_of = {}
    if args.best_of:                                                   # (its own generator: --sample's draws stay what they were)
        entry_length = args.entry_length or 67
        best_of = dict(best_of=args.best_of, lm_weight=args.lm_weight, top_p=args.top_p, top_k=args.top_k, temperature=args.temperature,
                       generator=torch.Generator(device=cap.device).manual_seed(args.seed))
    for i in range(0, len(annotations), args.bs):
        chunk = annotations[i:i + args.bs]
        images = [Image.open(os.path.join(image_path, a["file_name"])) for a in chunk]
        records = cap.describe(images, beam_size=args.beam_size, entry_length=entry_length, greedy=args.greedy,
                               return_attention=args.attention_out is not None, **best_of)
        samples = sample_captions(cap, images, args, generator) if args.sample else None
        for j, (a, r) in enumerate(zip(chunk, records)):
            if args.attention_out is not None:
                from clip_caption import caption_attention_map
                arrays[f"attention_{i + j}"] = r["attention"].cpu().numpy()
                arrays[f"map_{i + j}"] = caption_attention_map(r["attention"]).cpu().numpy()
            log["caption"].append({                                                        # test.py:626-633
                "caption_type": r["caption_type"],
                "violation_type": r["violation_type"],
                "prediction": r["prediction"],
                "caption": a.get("caption", "") or a.get("violation_list", ""),           # test.py:622-623
                "file_name": a.get("file_name", ""),
            })
            if samples is not None:
                log["caption"][-1]["samples"] = samples[j]
            if args.best_of:
                log["caption"][-1].update(clip_score=r["clip_score"], candidates=r["candidates"])
        C.log_line(done=min(i + args.bs, len(annotations)), of=len(annotations))
    if tmp is not None:
        tmp.cleanup()
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"output_{args.suffix}.json")
    with open(path, "w") as f:
        json.dump(log, f, indent=2, ensure_ascii=False)
    C.log_line(saved=path)
    if args.attention_out is not None:
        import numpy as np
        np.savez(args.attention_out, **arrays)
        C.log_line(saved=args.attention_out)
    return path


if __name__ == "__main__":
    main()
