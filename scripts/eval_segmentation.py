#!/usr/bin/env python3
"""How good are the dense zero-shot maps?  Mean IoU and boundary IoU of `clip.segment_photo` against annotated masks
(`clip.evaluate_labels`: integer counts on the device, csrc/label_agreement.hip; Boundary IoU: Cheng et al., CVPR 2021).

--images DIR holds the photos, --masks DIR one 8-bit PNG per photo with the same stem: the pixel value is the class index in
--classes order, 255 = ignore the pixel.  Every photo is segmented at its own size by sliding windows (segment_images.py's
--mode / --window / --stride / --max-side / --min-conf); a mask whose size differs from the processed photo is resized with
PIL NEAREST.  One JSON line per photo, then one summary line made from the SUMMED counts (dataset-level mIoU, the number
MaskCLIP, SCLIP and ClearCLIP report).  With --refine (segment_images.py's --refine-iterations / --refine-dilations) every line
carries the scores of the unrefined and of the refined maps: {"scores": ..., "refined": ...}.  With --prototypes FILE (fit_prototypes.py)
the class rows are the few-shot prototypes, blended with the prompts' embeddings by --text-weight.

    python scripts/eval_segmentation.py --images photos/ --masks masks/ --classes scaffold ground sky --checkpoint clip.pt
    python scripts/eval_segmentation.py --images photos/ --masks masks/ --classes scaffold ground sky --window 224 448 --refine
    python scripts/eval_segmentation.py --synthetic                                   # offline: seeded model, generated photos and masks"""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C
import torch

from explain_images import list_images


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=None, metavar="DIR", help="the photos")
    ap.add_argument("--masks", default=None, metavar="DIR", help="8-bit PNG masks with the photos' stems: class index, 255 = ignore")
    ap.add_argument("--classes", nargs="+", default=None, help="one prompt per class, in the order of the masks' indices")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned CLIP state dict")
    ap.add_argument("--mode", choices=("value", "qq", "kk"), default="value", help="the last block's dense tail (clip.segment)")
    ap.add_argument("--window", type=int, nargs="+", default=None, metavar="N", help="window sides (several: multi-scale); default: the model's resolution")
    ap.add_argument("--stride", type=int, default=None, help="step of the window lattice (default: half of each window)")
    ap.add_argument("--max-side", type=int, default=None, metavar="M", help="first shrink a photo whose longer side exceeds M")
    ap.add_argument("--min-conf", type=float, default=0.0, help="pixels whose best probability is lower get no class (they count against their ground truth)")
    ap.add_argument("--band", type=int, default=None, help="boundary band half-width in pixels, 0 .. 32 (default: 2 %% of the diagonal, capped; 0: no boundary IoU)")
    ap.add_argument("--bs", type=int, default=16, help="windows per tower call")
    ap.add_argument("--refine", action="store_true", help="also score the maps after image-guided refinement (clip.refine_maps)")
    ap.add_argument("--refine-iterations", type=int, default=10, metavar="T", help="--refine: iterations, 1 .. 64")
    ap.add_argument("--refine-dilations", type=int, nargs="+", default=[1, 2, 4, 8, 12, 24], metavar="d", help="--refine: neighbour distances")
    ap.add_argument("--prototypes", default=None, metavar="FILE", help="few-shot class prototypes of fit_prototypes.py: the classes are these rows, not the prompts alone")
    ap.add_argument("--text-weight", type=float, default=0.0, help="--prototypes: weight of a class's text embedding in its row, 0 .. 1 (a class without support takes its text row)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=3, help="--synthetic: photos to score")
    return ap


SYNTHETIC_CLASSES = ["violation", "status", "ground"]


def make_synthetic_masks(files, mask_dir, n_classes):
    """--synthetic: one mask per generated photo - vertical thirds of classes in a per-photo order, a strip of 255 on top"""
    import numpy as np
    from PIL import Image
    os.makedirs(mask_dir, exist_ok=True)
    for i, f in enumerate(files):
        w, h = Image.open(f).size
        m = ((np.arange(w) * 3 // max(w, 1) + i) % n_classes).astype(np.uint8)[None].repeat(h, axis=0)
        m[:max(1, h // 16)] = 255
        Image.fromarray(m, mode="L").save(os.path.join(mask_dir, os.path.splitext(os.path.basename(f))[0] + ".png"))


def load_mask(path, size):
    """the mask as a uint8 [H, W] tensor at `size` = (width, height), resized with NEAREST when it differs"""
    import numpy as np
    from PIL import Image
    m = Image.open(path)
    if m.mode not in ("L", "P"):
        raise SystemExit(f"{path}: a mask must be an 8-bit single-channel PNG, got mode {m.mode}")
    if m.size != size:
        m = m.resize(size, Image.NEAREST)
    return torch.from_numpy(np.asarray(m, dtype=np.uint8).copy())


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
    import numpy as np
    from PIL import Image
    from clip.preprocess_device import DevicePreprocess
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        C.make_synthetic_annotations(tmp.name, per_class=1 + (args.n_images - 1) // len(C.CLASSES))
        d = os.path.join(tmp.name, "images")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d))][:args.n_images]
        args.model, args.masks = "test-tiny", os.path.join(tmp.name, "masks")
        prompts = list(args.classes) if args.classes else list(SYNTHETIC_CLASSES)
        make_synthetic_masks(files, args.masks, len(prompts))
    else:
        if not args.images or not args.masks or not args.classes:
            raise SystemExit("--images DIR --masks DIR --classes ... are required (or --synthetic)")
        files, prompts = list_images([args.images]), list(args.classes)
    if not files:
        raise SystemExit("no images found")
    model, _ = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    with torch.no_grad():
        text = model.encode_text(C.get_tokenize(model)(prompts).to(device)).float()
    if args.prototypes:                                       # few-shot rows: the fitted prototypes, blended with the prompts' embeddings
        from fit_prototypes import load_prototypes
        text = load_prototypes(args.prototypes, len(prompts), model.geo.embed_dim, device).features(text, args.text_weight)
    windows = list(args.window) if args.window else [model.geo.image_resolution]
    window = windows if len(windows) > 1 else windows[0]
    stride = None if args.stride is None else ([args.stride] * len(windows) if len(windows) > 1 else args.stride)
    pre = DevicePreprocess(model.geo.image_resolution, device)
    out, sums = [], {}
    for f in files:
        mask_path = os.path.join(args.masks, os.path.splitext(os.path.basename(f))[0] + ".png")
        if not os.path.exists(mask_path):
            raise SystemExit(f"{f}: no mask {mask_path}")
        pic = Image.open(f).convert("RGB")
        if args.max_side and max(pic.size) > args.max_side:
            k = args.max_side / max(pic.size)
            pic = pic.resize((max(1, round(pic.size[0] * k)), max(1, round(pic.size[1] * k))), Image.BICUBIC)
        gt = load_mask(mask_path, pic.size).to(device)
        res = clip.segment_photo(model, pic, text, window=window, stride=stride, mode=args.mode, min_conf=args.min_conf,
                                 batch=args.bs, preprocess=pre)
        results = {"scores": res}
        if args.refine:
            photo = torch.from_numpy(np.asarray(pic, dtype=np.uint8).copy())
            results["refined"] = res.refine(photo, dilations=args.refine_dilations, iterations=args.refine_iterations)
        line = dict(file=f, height=int(gt.shape[0]), width=int(gt.shape[1]))
        for k, r in results.items():
            s = r.evaluate(gt, band=args.band)
            s.class_names = prompts                           # the classes went in as features: name them here
            line[k] = s.as_dict()
            key = (k, s.band)                                 # bands of different widths (the default follows the photo's size) are not summed
            sums[key] = s if key not in sums else sums[key] + s
        C.log_line(**line)
        out.append(line)
    summary = dict(summary=True, photos=len(files), classes=prompts)
    for k in ("scores", "refined"):
        parts = [s for (kk, _), s in sorted(sums.items(), key=lambda kv: kv[0][1]) if kk == k]
        if not parts:
            continue
        if len(parts) == 1:
            summary[k] = parts[0].as_dict()
        else:                                                 # several default bands: the confusion counts still sum, the band counts per width
            total = clip.SegmentationScores(sum(p.confusion for p in parts), class_names=prompts)
            summary[k] = dict(total.as_dict(), by_band=[p.as_dict() for p in parts])
    C.log_line(**summary)
    out.append(summary)
    if tmp is not None:
        tmp.cleanup()
    return out


if __name__ == "__main__":
    main()
