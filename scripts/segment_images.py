#!/usr/bin/env python3
"""Dense zero-shot maps straight from image files: where in each photo is which class (`clip.segment`: training-free dense CLIP on
the image tower's per-patch features; csrc/dense_classes.hip).  The classes are --prompts, or with --types the caption / violation
type lists of the reference (the keys of CLIP_prefix_caption/parse_coco.py's caption_type and violation_type, as predict_clip.py's
default prompts and describe_images.py use them).  One JSON line per image: the share of pixels per class ("none" last), the
class with the largest area, the mean confidence; --png DIR also writes the label colours blended over the photo.
With --window (and / or --stride) every photo is segmented at its OWN size by sliding windows (`clip.segment_photo`: overlapping
crops through the tower, probabilities averaged where they overlap, csrc/dense_stitch.hip); several --window sizes make a
multi-scale ensemble.  The JSON line then also carries "windows", "height" and "width", and the PNG has the photo's size.
With --instances the line gains "instances": one record {"class", "name", "box", "area", "score"} per connected component of the
label map (`clip.label_components`, csrc/label_components.hip), filtered by --min-area / --min-score, joined by --connectivity.
With --refine the class maps are first snapped to the photo's edges (`.refine(photo)`: pixel-adaptive mask refinement under the
photo at the map's size, csrc/dense_refine.hip; --refine-iterations, --refine-dilations); areas, top class, mean confidence,
instances and the PNG then come from the refined result and the line carries "refine".

    python scripts/segment_images.py photos/ --checkpoint clip.pt --prompts "a worker without a helmet" scaffold ground --png maps
    python scripts/segment_images.py photos/ --checkpoint clip.pt --window 224 448 --max-side 2048 --png maps
    python scripts/segment_images.py photos/ --checkpoint clip.pt --window 224 --refine --instances --png maps
    python scripts/segment_images.py --synthetic --png /tmp/maps                     # offline: seeded model, generated images"""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C
import torch

from describe_images import SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS
from explain_images import list_images


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="*", help="image files and / or directories of them")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned CLIP state dict")
    ap.add_argument("--prompts", nargs="+", default=None, help="one class per prompt (default: violation status, predict.py:39)")
    ap.add_argument("--types", choices=("caption", "violation"), default=None, help="use the caption / violation type list as the classes")
    ap.add_argument("--mode", choices=("value", "qq", "kk"), default="value", help="the last block's dense tail (clip.segment)")
    ap.add_argument("--size", type=int, default=None, help="side of the label map (default: the model's input resolution)")
    ap.add_argument("--min-conf", type=float, default=0.0, help="pixels whose best probability is lower get no class")
    ap.add_argument("--temperature", type=float, default=None, help="factor on the cosines (default: the model's logit scale)")
    ap.add_argument("--alpha", type=float, default=0.5, help="--png: weight of the label colour over the photo")
    ap.add_argument("--bs", type=int, default=16, help="images per clip.segment call")
    ap.add_argument("--png", default=None, metavar="DIR", help="write one overlay PNG per image here")
    ap.add_argument("--window", type=int, nargs="+", default=None, metavar="N",
                    help="sliding windows of side N over each photo at its own size (several: multi-scale); default with --stride: the model's resolution")
    ap.add_argument("--stride", type=int, default=None, help="step of the window lattice (default: half of each window)")
    ap.add_argument("--max-side", type=int, default=None, metavar="M", help="--window: first shrink a photo whose longer side exceeds M")
    ap.add_argument("--instances", action="store_true", help="add one record per connected component of the label map")
    ap.add_argument("--min-area", type=int, default=1, help="--instances: drop components of fewer pixels")
    ap.add_argument("--min-score", type=float, default=0.0, help="--instances: drop components of a lower mean confidence")
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=4, help="--instances: which neighbours join")
    ap.add_argument("--refine", action="store_true", help="snap the class maps to the photo's edges before labelling (clip.refine_maps)")
    ap.add_argument("--refine-iterations", type=int, default=10, metavar="T", help="--refine: iterations, 1 .. 64")
    ap.add_argument("--refine-dilations", type=int, nargs="+", default=[1, 2, 4, 8, 12, 24], metavar="d",
                    help="--refine: neighbour distances, 1 to 6 values in 1 .. 24")
    ap.add_argument("--prototypes", default=None, metavar="FILE", help="few-shot class prototypes of fit_prototypes.py: the classes are these rows, not the prompts alone")
    ap.add_argument("--text-weight", type=float, default=0.0, help="--prototypes: weight of a class's text embedding in its row, 0 .. 1 (a class without support takes its text row)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=3, help="--synthetic: images to segment")
    return ap


def class_prompts(args):
    if args.prompts:
        return list(args.prompts)
    if args.types == "caption":
        return list(SYNTHETIC_TYPES) if args.synthetic else ["status", "violation"]
    if args.types == "violation":
        return list(SYNTHETIC_VIOLATIONS) if args.synthetic else list(C.CLASSES)
    return ["violation", "status"]


def instance_records(comps, args, prompts, image=None):
    """--instances: a ComponentsResult as JSON-ready records (of one image of a batch when `image` is given)"""
    recs = comps.instances(min_area=args.min_area, min_score=args.min_score, class_names=prompts)
    return [{"class": r["class"], "name": r["name"], "box": list(r["box"]), "area": r["area"], "score": round(r["score"], 6)}
            for r in recs if image is None or r["image"] == image]


def refined(res, photo, args):
    """--refine: (the refined result, what the JSON line says about it)"""
    out = res.refine(photo, dilations=args.refine_dilations, iterations=args.refine_iterations)
    return out, dict(iterations=out.iterations, dilations=list(out.dilations))


def photos(args, model, files, prompts, text):
    """--window / --stride: one clip.segment_photo per photo, at the photo's size"""
    import clip
    import numpy as np
    from PIL import Image
    from clip.preprocess_device import DevicePreprocess
    windows = list(args.window) if args.window else [model.geo.image_resolution]
    window = windows if len(windows) > 1 else windows[0]
    stride = None if args.stride is None else ([args.stride] * len(windows) if len(windows) > 1 else args.stride)
    pre = DevicePreprocess(model.geo.image_resolution, text.device)
    out = []
    for i, f in enumerate(files):
        pic = Image.open(f).convert("RGB")
        if args.max_side and max(pic.size) > args.max_side:
            k = args.max_side / max(pic.size)
            pic = pic.resize((max(1, round(pic.size[0] * k)), max(1, round(pic.size[1] * k))), Image.BICUBIC)
        res = clip.segment_photo(model, pic, text, window=window, stride=stride, mode=args.mode, min_conf=args.min_conf,
                                 temperature=args.temperature, batch=args.bs, preprocess=pre)
        n_windows = int(res.boxes.shape[0])
        photo = torch.from_numpy(np.asarray(pic, dtype=np.uint8).copy()) if args.png or args.refine else None
        note = None
        if args.refine:
            res, note = refined(res, photo, args)
        top = res.top_class()
        line = dict(file=f, classes=prompts, area=[round(v, 6) for v in res.area_fractions().tolist()],
                    top_class=None if top is None else prompts[top], mean_conf=round(float(res.conf.mean()), 5),
                    windows=n_windows, height=int(res.labels.shape[0]), width=int(res.labels.shape[1]))
        if note is not None:
            line["refine"] = note
        if args.instances:
            line["instances"] = instance_records(res.components(args.connectivity), args, prompts)
        if args.png:
            line["png"] = os.path.join(args.png, f"{i:05d}_{os.path.splitext(os.path.basename(f))[0]}.png")
            Image.fromarray(res.overlay(photo=photo, alpha=args.alpha).cpu().numpy()).save(line["png"])
        C.log_line(**line)
        out.append(line)
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
    from PIL import Image
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        C.make_synthetic_annotations(tmp.name, per_class=1 + (args.n_images - 1) // len(C.CLASSES))
        d = os.path.join(tmp.name, "images")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d))][:args.n_images]
        args.model = "test-tiny"
    else:
        files = list_images(args.images)
    if not files:
        raise SystemExit("no images given (or --synthetic)")
    model, preprocess = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    prompts = class_prompts(args)
    with torch.no_grad():
        text = model.encode_text(C.get_tokenize(model)(prompts).to(device)).float()      # once for every image
    if args.prototypes:                                       # few-shot rows: the fitted prototypes, blended with the prompts' embeddings
        from fit_prototypes import load_prototypes
        text = load_prototypes(args.prototypes, len(prompts), model.geo.embed_dim, device).features(text, args.text_weight)
    S = args.size or model.geo.image_resolution
    if args.png:
        os.makedirs(args.png, exist_ok=True)
    if args.window is not None or args.stride is not None:
        out = photos(args, model, files, prompts, text)
        if tmp is not None:
            tmp.cleanup()
        return out
    if args.max_side is not None:
        raise SystemExit("--max-side needs --window")
    out = []
    for i in range(0, len(files), args.bs):
        chunk = files[i:i + args.bs]
        pics = [Image.open(f).convert("RGB") for f in chunk]
        image = torch.stack([preprocess(p) for p in pics]).to(device)
        res = clip.segment(model, image, text, mode=args.mode, size=S, min_conf=args.min_conf, temperature=args.temperature)
        photo, note = None, None
        if args.png or args.refine:
            import numpy as np
            photo = torch.stack([torch.from_numpy(np.asarray(p.resize((S, S), Image.BILINEAR)).copy()) for p in pics])
        if args.refine:
            res, note = refined(res, photo, args)
        fractions, top = res.area_fractions().cpu(), res.top_class()
        mean_conf = res.conf.flatten(1).mean(dim=1).cpu()
        overlay = None
        if args.png:
            overlay = res.overlay(photo=photo, alpha=args.alpha).cpu().numpy()
        comps = res.components(args.connectivity) if args.instances else None
        for j, f in enumerate(chunk):
            line = dict(file=f, classes=prompts, area=[round(v, 6) for v in fractions[j].tolist()],
                        top_class=None if top[j] is None else prompts[top[j]], mean_conf=round(float(mean_conf[j]), 5))
            if note is not None:
                line["refine"] = note
            if comps is not None:
                line["instances"] = instance_records(comps, args, prompts, image=j)
            if overlay is not None:
                line["png"] = os.path.join(args.png, f"{i + j:05d}_{os.path.splitext(os.path.basename(f))[0]}.png")
                Image.fromarray(overlay[j]).save(line["png"])
            C.log_line(**line)
            out.append(line)
    if tmp is not None:
        tmp.cleanup()
    return out


if __name__ == "__main__":
    main()
