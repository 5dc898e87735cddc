#!/usr/bin/env python3
"""Zero-shot labels per detector box - what the reference's application.py could do between its detector step (:51-70;
`/detect`, :248, returns {"boxes", "scores", "labels"}) and its CLIP step, which today only ever sees the whole photo: every box
is cropped, resized and normalised on the device in one `DevicePreprocess.regions` call, encoded, and classified by the two
zero-shot heads of parse_coco.py:24-53 (caption type, violation type).  One JSON line per box.

    python scripts/classify_regions.py --image site.jpg --boxes boxes.json --checkpoint models/clip_latest.pt
    python scripts/classify_regions.py --synthetic                # offline: random photo, random boxes, seeded weights

boxes.json: a bare [[x0, y0, x1, y1], ...] or the `/detect` object {"boxes": [...], "scores": [...], "labels": [...]}."""
from __future__ import annotations

import argparse
import json

import _common as C
import numpy as np
import torch


def parse_boxes(obj):
    """(boxes, scores or None, labels or None) from either boxes.json layout"""
    scores = labels = None
    if isinstance(obj, dict):
        if "boxes" not in obj:
            raise ValueError(f"boxes file: an object needs a \"boxes\" entry, found {sorted(obj)}")
        boxes, scores, labels = obj["boxes"], obj.get("scores"), obj.get("labels")
    else:
        boxes = obj
    if not isinstance(boxes, list) or any(not isinstance(b, (list, tuple)) or len(b) != 4 for b in boxes):
        raise ValueError("boxes file: boxes must be a list of [x0, y0, x1, y1]")
    for name, v in (("scores", scores), ("labels", labels)):
        if v is not None and len(v) != len(boxes):
            raise ValueError(f"boxes file: {len(v)} {name} for {len(boxes)} boxes")
    return [list(b) for b in boxes], scores, labels


def load_boxes(path: str):
    with open(path) as f:
        return parse_boxes(json.load(f))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default=None)
    ap.add_argument("--boxes", default=None, help="boxes.json (see the module docstring)")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned CLIP state dict")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_boxes", type=int, default=8, help="--synthetic: boxes to draw")
    ap.add_argument("--clip_synthetic", default="test-tiny", help="--synthetic: CLIP geometry")
    ap.add_argument("--seed", type=int, default=567, help="--synthetic: seed of the photo and the boxes")
    return ap


def synthetic_inputs(n_boxes: int, seed: int, width: int = 640, height: int = 480):
    """a random photo and a `/detect`-style object of random float boxes, each at least 2 x 2 pixels"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    image = Image.fromarray(rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8), "RGB")
    x0, y0 = rng.uniform(0, width - 40, n_boxes), rng.uniform(0, height - 40, n_boxes)
    x1, y1 = np.minimum(x0 + rng.uniform(2, 300, n_boxes), width), np.minimum(y0 + rng.uniform(2, 300, n_boxes), height)
    det = {"boxes": np.stack([x0, y0, x1, y1], axis=1).round(2).tolist(), "scores": rng.uniform(0.5, 1.0, n_boxes).round(3).tolist(),
           "labels": rng.integers(1, 5, n_boxes).tolist()}
    return image, det


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
    from clip.data import ZeroShotClassifier
    from PIL import Image
    device = torch.device("cuda:0")
    if args.synthetic:
        from describe_images import SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS
        image, det = synthetic_inputs(args.n_boxes, args.seed)
        boxes, scores, labels = parse_boxes(det)
        caption_types, violation_types = SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS
        args.model = args.clip_synthetic
    else:
        if not args.image or not args.boxes:
            raise SystemExit("--image and --boxes are required (or --synthetic)")
        from clip_caption.data import CAPTION_TYPES, VIOLATION_TYPES
        image = Image.open(args.image)
        boxes, scores, labels = load_boxes(args.boxes)
        caption_types, violation_types = CAPTION_TYPES, VIOLATION_TYPES
    model, _ = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    tokenize = C.get_tokenize(model)
    type_head = ZeroShotClassifier(model, tokenize(list(caption_types.keys())), list(caption_types.values()))   # parse_coco.py:24-27
    violation_head = ZeroShotClassifier(model, tokenize(list(violation_types)), list(violation_types))           # parse_coco.py:28
    pre = clip.DevicePreprocess(model.visual.input_resolution, device=device)
    features = clip.encode_regions(model, image, boxes, preprocess=pre)          # the boxes are encoded once for both heads
    t_sim, t_idx, t_lab = type_head(image_features=features)
    v_sim, v_idx, v_lab = violation_head(image_features=features)
    t_p, v_p = t_sim.max(dim=1).values.tolist(), v_sim.max(dim=1).values.tolist()
    out = []
    for k, box in enumerate(boxes):
        rec = dict(box=box)
        if labels is not None:
            rec["label"] = labels[k]
        if scores is not None:
            rec["score"] = scores[k]
        rec.update(caption_type=t_lab[k], caption_type_prob=round(t_p[k], 5), violation_type=v_lab[k], violation_type_prob=round(v_p[k], 5))
        out.append(rec)
        print(json.dumps(rec, ensure_ascii=False), flush=True)
    return out


if __name__ == "__main__":
    main()
