#!/usr/bin/env python3
"""Relevance maps - attention.py:153 (`main`) on the MI355X `clip` package: load the model (+ a fine-tuned
state_dict), preprocess one image, tokenize the captions, `clip.interpret` (`clip.interpret_rows` for a tower of more than 128
image tokens), then the patch map upsampled to 224 x 224 and
min-max normalised (attention.py:88-92) and each caption's per-token scores (attention.py:115-117).  Written to an .npz
(image_map [224, 224], token_scores of the first caption, and per caption token_scores_<i>, text_relevance, image_relevance)
plus an overlay PNG next to it (PIL; the reference's cv2 / matplotlib figure is not reproduced).

    python scripts/explain_clip.py --checkpoint models/clip.pt --image site.jpg --captions "no guard rail" --out rel.npz
    python scripts/explain_clip.py --synthetic --model test-small --out /tmp/rel.npz                # offline smoke run
"""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C
import numpy as np
import torch


def _jet(m: np.ndarray) -> np.ndarray:
    """[H, W] in [0, 1] -> [H, W, 3] in [0, 1], the usual blue-cyan-yellow-red ramp."""
    r = np.clip(1.5 - np.abs(4 * m - 3), 0, 1)
    g = np.clip(1.5 - np.abs(4 * m - 2), 0, 1)
    b = np.clip(1.5 - np.abs(4 * m - 1), 0, 1)
    return np.stack([r, g, b], axis=-1)


def overlay(image: torch.Tensor, heat: np.ndarray) -> np.ndarray:
    """attention.py:67-84 (show_cam_on_image) with PIL: heat map + the min-max normalised input, rescaled to [0, 255]."""
    from PIL import Image
    x = image.detach().float().cpu().permute(1, 2, 0).numpy()
    x = (x - x.min()) / max(float(x.max() - x.min()), 1e-12)
    size = heat.shape[0]
    x = np.asarray(Image.fromarray(np.uint8(255 * x)).resize((size, size), Image.BILINEAR), dtype=np.float32) / 255
    cam = _jet(heat) + x
    return np.uint8(255 * cam / cam.max())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default=None)
    ap.add_argument("--captions", nargs="+", default=["worker near fall zone"])
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--start-layer", type=int, default=-1)
    ap.add_argument("--start-layer-text", type=int, default=-1)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default="relevance.npz")
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    import clip
    from PIL import Image
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        C.make_synthetic_annotations(tmp.name, per_class=1)
        d = os.path.join(tmp.name, "images")
        args.image = os.path.join(d, sorted(os.listdir(d))[0])
    if args.image is None:
        ap.error("--image is required (or --synthetic)")
    model, preprocess = clip.load(args.model, device=device, jit=False)                  # attention.py:154
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    img = preprocess(Image.open(args.image)).unsqueeze(0).to(device)                     # attention.py:161
    text = C.get_tokenize(model)(args.captions).to(device)                                # attention.py:165
    # more than 128 image tokens (ViT-B/16, ViT-L/14): the full T x T matrices are not offered; their rows are (text_relevance is
    # then [N, T], each caption's EOT row)
    long_tower = model.geo.vision_tokens > 128
    r_text, r_image = (clip.interpret_rows if long_tower else clip.interpret)(
        img, text, model, device=device, start_layer=args.start_layer, start_layer_text=args.start_layer_text)
    maps = clip.image_relevance_map(r_image, args.size).cpu().numpy()
    scores = [s.cpu().numpy() for s in (clip.text_row_scores if long_tower else clip.text_token_scores)(r_text, text)]
    out = dict(image_map=maps[0], token_scores=scores[0], text_relevance=r_text.cpu().numpy(),
               image_relevance=r_image.cpu().numpy(), tokens=text.cpu().numpy())
    for i, s in enumerate(scores):
        out[f"token_scores_{i}"] = s
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **out)
    png = os.path.splitext(args.out)[0] + ".png"
    Image.fromarray(overlay(img[0], maps[0])).save(png)
    for i, cap in enumerate(args.captions):
        C.log_line(caption=cap, tokens=int(scores[i].shape[0]), top_token=int(scores[i].argmax()) + 1 if scores[i].size else None,
                   top_patch=int(r_image[i].argmax()), npz=args.out, png=png)
    if tmp is not None:
        tmp.cleanup()
    return out


if __name__ == "__main__":
    main()
