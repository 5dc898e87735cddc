#!/usr/bin/env python3
"""Which photos of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's layout) should be
labelled next?  Load it into a `clip.EmbeddingIndex` and take `--m` k-centre greedy picks over the stored 16-bit rows
(clip/coreset.py: csrc/coreset.hip): each pick is the photo farthest from everything chosen or labelled so far.  One JSON line
per pick: {rank, row, file_name, radius, covers} - radius is the pick's cosine distance to the centres before it, covers the
number of photos it is the nearest centre of - then one summary line.

`--label-key violation_type` reads that key of every caption record (the reference's monthly folders carry ''): the rows with a
value are centres from the start and are never picked.  `--uncertainty` (needs `--label-key`) first spreads those labels over
the kNN graph (clip/propagate.py) and weighs every photo by 1 - certainty: far from what is labelled AND unsure.

    python scripts/select_to_label.py --index embeddings.pkl --m 50 --label-key violation_type --uncertainty
    python scripts/select_to_label.py --synthetic --m 12                                          # offline smoke run
"""
from __future__ import annotations

import argparse

import _common as C
import torch


def synthetic_embeddings(per_class: int = 40, dim: int = 64, labelled_share: float = 0.1, seed: int = 567):
    """Seeded stand-in for an embedding pickle: per_class rows around one random direction per class of C.CLASSES, shuffled;
    about `labelled_share` of the rows of every class but the last carry `violation_type`, the rest ''."""
    g = torch.Generator().manual_seed(seed)
    n_cls = len(C.CLASSES)
    dirs = torch.randn(n_cls, dim, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    cls = torch.arange(n_cls).repeat_interleave(per_class)
    feats = dirs[cls] + 0.5 / dim ** 0.5 * torch.randn(cls.numel(), dim, generator=g)
    perm = torch.randperm(cls.numel(), generator=g)
    feats, cls = feats[perm], cls[perm]
    known = (torch.rand(cls.numel(), generator=g) < labelled_share) & (cls < n_cls - 1)
    caps = [{"file_name": f"images/{C.CLASSES[int(c)]}_{j:05d}.png", "clip_embedding": j, "caption": f"photo {j}",
             "violation_type": C.CLASSES[int(c)] if k else ""} for j, (c, k) in enumerate(zip(cls, known))]
    return feats, caps


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--m", type=int, default=None, help="photos to pick")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--label-key", default=None, help="caption key that holds a label for some rows, e.g. violation_type")
    ap.add_argument("--uncertainty", action="store_true", help="weigh every photo by 1 - certainty of clip.spread_labels")
    ap.add_argument("--k", type=int, default=15, help="neighbours per photo for --uncertainty")
    ap.add_argument("--first", default="mean", help="without labelled rows: 'mean' or a row index")
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    if args.m is None or (args.index is None and not args.synthetic):
        ap.error("--m and --index are required (or --synthetic)")
    if args.m < 0:
        ap.error("--m must be >= 0")
    if args.synthetic and args.label_key is None:
        args.label_key = "violation_type"
    if args.uncertainty and args.label_key is None:
        ap.error("--uncertainty needs --label-key")
    if args.first != "mean":
        try:
            args.first = int(args.first)
        except ValueError:
            ap.error("--first must be 'mean' or a row index")
    return args


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

    def field(row, key):
        cap = captions[row]
        return cap.get(key) if isinstance(cap, dict) else None

    N = len(index)
    names, given = [], None
    if args.label_key:
        values = [field(r, args.label_key) for r in range(N)]
        names = sorted({str(v) for v in values if v})
        where = {n: i for i, n in enumerate(names)}
        given = [where[str(v)] if v else -1 for v in values]
    labelled = sum(1 for g in given if g >= 0) if given else 0
    if args.m > N - labelled:
        raise SystemExit(f"select_to_label: --m {args.m} above the {N - labelled} unlabelled rows")
    weights = None
    if args.uncertainty:
        if not labelled:
            raise SystemExit(f"select_to_label: no row has a value under {args.label_key!r}; --uncertainty has nothing to spread")
        spread = index.spread_labels(given, n_classes=max(2, len(names)), k=min(args.k, N - 1))
        weights = 1.0 - spread.certainty
    result = index.coreset(args.m, labelled=given if labelled else None, weights=weights, first=args.first)
    centres, counts = result.cover_counts()
    covers = dict(zip(centres.tolist(), counts.tolist()))
    lines = []
    for rank, (row, radius) in enumerate(zip(result.picks.tolist(), result.radius.tolist())):
        if row < 0:                                     # nothing eligible was left (every weight 0)
            break
        line = dict(rank=rank, row=row, file_name=field(row, "file_name"), radius=radius if radius == radius and abs(radius) != float("inf") else None,
                    covers=covers[row])
        lines.append(line)
        C.log_line(**line)
    summary = dict(rows=N, labelled=labelled, picked=len(lines), cover_radius=result.cover_radius.item(),
                   weighted=bool(args.uncertainty))
    C.log_line(summary=summary)
    return lines, summary


if __name__ == "__main__":
    main()
