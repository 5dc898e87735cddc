#!/usr/bin/env python3
"""Few-shot dense maps: fit one prototype per class from annotated photos (`clip.DensePrototypes`: masked average pooling of the
tower's per-patch features under each class's mask; csrc/dense_prototypes.hip).  No training.

--images DIR holds the photos, --masks DIR one 8-bit PNG per photo with the same stem - eval_segmentation.py's format: the pixel
value is the class index in --classes order, 255 = ignore the pixel.  Every photo goes through segment_images.py's sliding
windows (--mode / --window / --stride / --max-side).  The result is a .pt of the accumulators (sums, weight, patches, pixels, bad
and the class names): segment_images.py and eval_segmentation.py take it with --prototypes, and more photos can be added later
with --resume.  One JSON line per photo, then the support per class.

    python scripts/fit_prototypes.py --images photos/ --masks masks/ --classes scaffold ground sky --checkpoint clip.pt --out protos.pt
    python scripts/fit_prototypes.py --synthetic --out /tmp/protos.pt                    # offline: seeded model, generated photos and masks"""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C
import torch

from eval_segmentation import SYNTHETIC_CLASSES, load_mask, make_synthetic_masks
from explain_images import list_images


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=None, metavar="DIR", help="the annotated photos")
    ap.add_argument("--masks", default=None, metavar="DIR", help="8-bit PNG masks with the photos' stems: class index, 255 = ignore")
    ap.add_argument("--classes", nargs="+", default=None, help="one name per class, in the order of the masks' indices")
    ap.add_argument("--out", required=True, metavar="FILE", help="where the prototypes go (.pt)")
    ap.add_argument("--resume", default=None, metavar="FILE", help="add to the prototypes of an earlier run")
    ap.add_argument("--min-share", type=float, default=None, help="a patch cell supports a class that holds at least this share of its pixels (default 0.5; with --resume: the file's)")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned CLIP state dict")
    ap.add_argument("--mode", choices=("value", "qq", "kk"), default="value", help="the last block's dense tail (clip.segment)")
    ap.add_argument("--window", type=int, nargs="+", default=None, metavar="N", help="window sides (several: multi-scale); default: the model's resolution")
    ap.add_argument("--stride", type=int, default=None, help="step of the window lattice (default: half of each window)")
    ap.add_argument("--max-side", type=int, default=None, metavar="M", help="first shrink a photo whose longer side exceeds M")
    ap.add_argument("--bs", type=int, default=16, help="windows per tower call")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--n_images", type=int, default=3, help="--synthetic: photos to fit on")
    return ap


def load_prototypes(path, n_classes, embed_dim, device):
    """the prototypes of a fit_prototypes.py run, checked against the classes and the model in use"""
    import clip
    protos = clip.DensePrototypes.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), device=device)
    if protos.n_classes != n_classes or protos.embed_dim != embed_dim:
        raise SystemExit(f"{path}: prototypes of {protos.n_classes} classes and width {protos.embed_dim}; "
                         f"this run has {n_classes} classes and a model of width {embed_dim}")
    return protos


def main(argv=None):
    args = build_parser().parse_args(argv)
    import clip
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
        names = list(args.classes) if args.classes else list(SYNTHETIC_CLASSES)
        make_synthetic_masks(files, args.masks, len(names))
    else:
        if not args.images or not args.masks or not args.classes:
            raise SystemExit("--images DIR --masks DIR --classes ... are required (or --synthetic)")
        files, names = list_images([args.images]), list(args.classes)
    if not files:
        raise SystemExit("no images found")
    model, _ = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    if args.resume:
        protos = load_prototypes(args.resume, len(names), model.geo.embed_dim, device)
        if args.min_share is not None and int(round(256 * args.min_share)) != protos.min_share8:
            raise SystemExit(f"{args.resume} was fitted with --min-share {protos.min_share} ({protos.min_share8} / 256); it cannot go on with {args.min_share}")
        if protos.class_names is not None and protos.class_names != names:
            raise SystemExit(f"{args.resume} holds the classes {protos.class_names}; this run names {names}")
    else:
        protos = clip.DensePrototypes(len(names), model.geo.embed_dim, class_names=names, min_share=0.5 if args.min_share is None else args.min_share,
                                       device=device)
    windows = list(args.window) if args.window else [model.geo.image_resolution]
    window = windows if len(windows) > 1 else windows[0]
    stride = None if args.stride is None else ([args.stride] * len(windows) if len(windows) > 1 else args.stride)
    pre = DevicePreprocess(model.geo.image_resolution, device)
    out = []
    for f in files:
        mask_path = os.path.join(args.masks, os.path.splitext(os.path.basename(f))[0] + ".png")
        if not os.path.exists(mask_path):
            raise SystemExit(f"{f}: no mask {mask_path}")
        pic = Image.open(f).convert("RGB")
        if args.max_side and max(pic.size) > args.max_side:
            k = args.max_side / max(pic.size)
            pic = pic.resize((max(1, round(pic.size[0] * k)), max(1, round(pic.size[1] * k))), Image.BICUBIC)
        before = protos.patches.clone()
        protos.add_photo(model, pic, load_mask(mask_path, pic.size), window=window, stride=stride, mode=args.mode, batch=args.bs, preprocess=pre)
        line = dict(file=f, height=pic.size[1], width=pic.size[0], patches=(protos.patches - before).tolist())
        C.log_line(**line)
        out.append(line)
    support = protos.support()
    if support["bad"]:
        raise SystemExit(f"{support['bad']} mask pixels under the windows hold a value in [{len(names)}, 254]: not a class of --classes, not 255")
    torch.save(protos.state_dict(), args.out)
    summary = dict(summary=True, photos=len(files), out=args.out, **support)
    C.log_line(**summary)
    out.append(summary)
    if tmp is not None:
        tmp.cleanup()
    return out


if __name__ == "__main__":
    main()
