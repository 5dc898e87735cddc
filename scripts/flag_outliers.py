#!/usr/bin/env python3
"""Flag photos that are unlike everything that was labelled: a shared-covariance Gaussian model (`clip.GaussianClassifier`) of a
labelled embedding pickle of scripts/extract_embeddings.py scores every query by its class, the class probability and the squared
Mahalanobis distance to the nearest class.  One JSON line per query: {file_name, class, probability, mahalanobis, outlier}.

    python scripts/flag_outliers.py labelled.pkl new.pkl --key violation_type --held-out val.pkl --quantile 0.95
    python scripts/flag_outliers.py labelled.pkl new.pkl --threshold 900
    python scripts/flag_outliers.py labelled.pkl --suspects 20          # the 20 labelled rows most likely mislabelled
    python scripts/flag_outliers.py --synthetic                         # offline smoke run

The threshold is --threshold, or the --quantile of the distances of the --held-out photos (photos like the labelled ones that
were NOT used to fit: the fitted rows themselves sit closer to their means than any new photo does).  Without either, `outlier`
is null."""
from __future__ import annotations

import argparse


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("labelled", nargs="?", default=None, help="labelled embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("queries", nargs="?", default=None, help="embedding pickle of the photos to score")
    ap.add_argument("--key", default="violation_type", help="annotation field that holds the label")
    ap.add_argument("--held-out", default=None, help="embedding pickle of in-distribution photos not used to fit")
    ap.add_argument("--quantile", type=float, default=0.95)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--shrinkage", default="auto", help="'auto' (Wang et al.) or a float in [0, 1]")
    ap.add_argument("--priors", choices=("empirical", "uniform"), default="empirical")
    ap.add_argument("--suspects", type=int, default=None, metavar="K", help="list the K most suspicious labelled rows instead")
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    if not args.synthetic and args.labelled is None:
        ap.error("give the labelled embedding pickle (or --synthetic)")
    if not args.synthetic and args.suspects is None and args.queries is None:
        ap.error("give the query pickle, or --suspects K")
    if args.shrinkage != "auto":
        args.shrinkage = float(args.shrinkage)
    return args


def synthetic_sets(C: int = 9, D: int = 64, per_class: int = 12, seed: int = 567):
    """(labelled rows, labels, held-out rows, queries, file names): classes around a common direction; the last 3 queries are
    off-topic (another direction altogether) and one label of the labelled set is swapped"""
    import torch
    g = torch.Generator().manual_seed(seed)
    base = torch.ones(D) * 3.0 / D ** 0.5
    mus = torch.randn(C, D, generator=g) * 0.25

    def draw(n):
        y = torch.arange(n) % C
        return base + mus[y] + 0.05 * torch.randn(n, D, generator=g), y

    x, y = draw(C * per_class)
    held, _ = draw(4 * C)
    q, _ = draw(2 * C)
    far = torch.randn(3, D, generator=g)
    y = y.clone()
    y[0] = 1                                           # row 0 belongs to class 0
    names = [f"query_{i:03d}.png" for i in range(len(q))] + [f"offtopic_{i}.png" for i in range(3)]
    return x, y, held, torch.cat([q, far]), names


def main(argv=None):
    args = parse_args(argv)
    import _common as C
    import torch
    import clip
    from clip_caption.data import load_embeddings
    device = torch.device("cuda:0")
    held = queries = names = None
    if args.synthetic:
        x, y, held, queries, names = synthetic_sets()
        gc = clip.GaussianClassifier(x.to(device), y, class_names=C.CLASSES, shrinkage=args.shrinkage, priors=args.priors)
        labelled_rows, labelled_y = x.to(device), y
        labelled_names = [f"labelled_{i:03d}.png" for i in range(len(x))]
        held, queries = held.to(device), queries.to(device)
    else:
        index = clip.EmbeddingIndex.from_pickle(args.labelled)
        gc = clip.GaussianClassifier.from_index(index, args.key, shrinkage=args.shrinkage, priors=args.priors)
        from clip.fewshot import _labels_from_metadata
        labelled_rows, labelled_y = index.features, _labels_from_metadata(index.metadata, args.key, gc.class_names)[0]
        labelled_names = [m.get("file_name") if isinstance(m, dict) else None for m in index.metadata]
        if args.held_out is not None:
            held = load_embeddings(args.held_out)["clip_embedding"].to(device)
        if args.queries is not None:
            data = load_embeddings(args.queries)
            queries = data["clip_embedding"].to(device)
            names = [c.get("file_name") if isinstance(c, dict) else None for c in data["captions"]]
    out = []
    if args.suspects is not None:
        rows, margin = gc.suspects(labelled_rows, labelled_y, top=args.suspects)
        near = gc.mahalanobis(labelled_rows).nearest[rows].tolist()
        for r, m, n in zip(rows.tolist(), margin.tolist(), near):
            row = dict(row=r, file_name=labelled_names[r], label=gc.class_names[int(labelled_y[r])], nearest=gc.class_names[n],
                       margin=round(m, 4))
            C.log_line(**row)
            out.append(row)
        return out
    threshold = args.threshold
    if threshold is None and held is not None:
        threshold = gc.calibrate(held, args.quantile)
    probs, idx, picked = gc(image_features=queries)
    dmin = gc.mahalanobis(queries).dmin.tolist()
    p = probs.gather(1, idx[:, None])[:, 0].tolist()
    for name, label, pr, d in zip(names, picked, p, dmin):
        row = dict(file_name=name, **{"class": label}, probability=round(pr, 6), mahalanobis=round(d, 4),
                   outlier=None if threshold is None else bool(not d <= threshold))
        C.log_line(**row)
        out.append(row)
    return out


if __name__ == "__main__":
    main()
