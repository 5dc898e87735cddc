#!/usr/bin/env python3
"""Lay the photos of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's layout) out in a
plane: load it into a `clip.EmbeddingIndex`, run t-SNE on the stored 16-bit rows (clip/tsne.py: csrc/tsne.hip) and print one
JSON line per photo: its metadata fields `file_name` and `caption` where it has them, `x`, `y`, then one summary line.

`--label-key violation_type` copies that key of every caption record as `label`.  `--clusters K` adds `cluster`, the row's
spherical k-means cluster among K.  `--png OUT.png` draws the scatter with PIL, coloured by label (or by cluster without a
label key); without PIL it is skipped with a message.

    python scripts/map_images.py --index embeddings.pkl --label-key violation_type --clusters 16 --png map.png
    python scripts/map_images.py --synthetic                                                      # offline smoke run
"""
from __future__ import annotations

import argparse

import _common as C
import torch


def synthetic_embeddings(per_class: int = 60, dim: int = 64, seed: int = 567):
    """Seeded stand-in for an embedding pickle: per_class rows around one random direction per class of C.CLASSES, shuffled.
    Returns (features, captions); the captions carry `violation_type`."""
    g = torch.Generator().manual_seed(seed)
    n_cls = len(C.CLASSES)
    dirs = torch.randn(n_cls, dim, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    cls = torch.arange(n_cls).repeat_interleave(per_class)
    feats = dirs[cls] + 0.5 / dim ** 0.5 * torch.randn(cls.numel(), dim, generator=g)
    perm = torch.randperm(cls.numel(), generator=g)
    feats, cls = feats[perm], cls[perm]
    caps = [{"file_name": f"images/{C.CLASSES[int(c)]}_{j:05d}.png", "clip_embedding": j, "caption": f"photo {j}",
             "violation_type": C.CLASSES[int(c)]} for j, c in enumerate(cls)]
    return feats, caps


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--perplexity", type=float, default=20.0)
    ap.add_argument("--n-iter", type=int, default=1000)
    ap.add_argument("--exaggeration", type=float, default=12.0)
    ap.add_argument("--exaggeration-iters", type=int, default=250)
    ap.add_argument("--learning-rate", default="auto", help="'auto' or a positive number")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--label-key", default=None, help="caption key copied to every line as `label`, e.g. violation_type")
    ap.add_argument("--clusters", type=int, default=None, metavar="K", help="add the row's k-means cluster among K")
    ap.add_argument("--png", default=None, metavar="OUT.png", help="draw the scatter (needs PIL)")
    ap.add_argument("--png-size", type=int, default=1024)
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    if args.index is None and not args.synthetic:
        ap.error("--index is required (or --synthetic)")
    if args.learning_rate != "auto":
        try:
            args.learning_rate = float(args.learning_rate)
        except ValueError:
            ap.error("--learning-rate must be 'auto' or a number")
        if not args.learning_rate > 0:
            ap.error("--learning-rate must be positive")
    if args.clusters is not None and args.clusters < 1:
        ap.error("--clusters must be at least 1")
    if args.n_iter < 0 or args.exaggeration_iters < 0 or args.png_size < 16:
        ap.error("--n-iter and --exaggeration-iters must be >= 0, --png-size >= 16")
    if args.synthetic and args.label_key is None:
        args.label_key = "violation_type"
    return args


def palette(n: int):
    """n well-separated RGB colours (evenly spaced hues)"""
    import colorsys
    return [tuple(int(255 * c) for c in colorsys.hsv_to_rgb(i / max(n, 1), 0.75, 0.9)) for i in range(n)]


def draw_png(path: str, xs, ys, groups, size: int) -> bool:
    """Scatter of (xs, ys) coloured by `groups` (any hashable per point; None = grey).  False when PIL is missing."""
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        return False
    names = sorted({g for g in groups if g is not None}, key=str)
    colour = dict(zip(names, palette(len(names))))
    lo_x, hi_x, lo_y, hi_y = min(xs), max(xs), min(ys), max(ys)
    span = max(hi_x - lo_x, hi_y - lo_y) or 1.0
    margin, r = 0.04 * size, max(1, size // 400)
    scale = (size - 2 * margin) / span
    img = Image.new("RGB", (size, size), (255, 255, 255))
    draw = ImageDraw.Draw(img)
    for x, y, g in zip(xs, ys, groups):
        px, py = margin + (x - lo_x) * scale, size - margin - (y - lo_y) * scale
        draw.ellipse([px - r, py - r, px + r, py + r], fill=colour.get(g, (150, 150, 150)))
    img.save(path)
    return True


def main(argv=None):
    args = parse_args(argv)
    import clip
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.synthetic:
        feats, captions = synthetic_embeddings()
        index = clip.EmbeddingIndex(feats, dtype=dtype, metadata=captions)
    else:
        index = clip.EmbeddingIndex.from_pickle(args.index, dtype=dtype)
        captions = index.metadata
    result = index.tsne(perplexity=args.perplexity, n_iter=args.n_iter, exaggeration=args.exaggeration,
                        exaggeration_iters=args.exaggeration_iters, learning_rate=args.learning_rate, seed=args.seed)
    xy = result.embedding.tolist()
    clusters = index.kmeans(args.clusters, seed=args.seed).labels.tolist() if args.clusters else None

    def field(row, key):
        cap = captions[row]
        return cap.get(key) if isinstance(cap, dict) else None

    lines = []
    for r, (x, y) in enumerate(xy):
        line = dict(row=r)
        for key in ("file_name", "caption"):
            if field(r, key) is not None:
                line[key] = field(r, key)
        line.update(x=x, y=y)
        if args.label_key:
            line["label"] = field(r, args.label_key)
        if clusters is not None:
            line["cluster"] = clusters[r]
        lines.append(line)
        C.log_line(**line)
    summary = dict(rows=len(index), perplexity=args.perplexity, n_iter=result.n_iter, kl_divergence=result.kl_divergence)
    if args.png:
        groups = [ln.get("label") or None for ln in lines] if args.label_key else [ln.get("cluster") for ln in lines]
        if draw_png(args.png, [ln["x"] for ln in lines], [ln["y"] for ln in lines], groups, args.png_size):
            summary["png"] = args.png
        else:
            print("map_images: PIL is not installed; --png skipped")
    C.log_line(summary=summary)
    return lines, summary


if __name__ == "__main__":
    main()
