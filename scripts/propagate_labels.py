#!/usr/bin/env python3
"""Give the unlabelled photos of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's
layout) a label from the few that carry one: load it into a `clip.EmbeddingIndex`, read `--label-key` of every caption record
(the reference's monthly folders carry ''), spread the non-empty values over the kNN graph of the stored 16-bit rows
(clip/propagate.py: csrc/label_spread.hip) and print one JSON line per unlabelled photo: {row, file_name, label, confidence,
certainty}, then one summary line.

`--min-confidence X` leaves the rows whose confidence is below X unlabelled (`label: null`).  `--suspects` also prints the
labelled rows whose propagated label disagrees with the given one, most confident first.  `--write-labels OUT.json` writes
one record per row, as scripts/cluster_images.py does: {row, file_name, label, inherited, confidence, certainty}.

    python scripts/propagate_labels.py --index embeddings.pkl --label-key violation_type --min-confidence 0.6 --suspects
"""
from __future__ import annotations

import argparse
import json

import _common as C
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--label-key", default=None, help="caption key that holds a label for some rows, e.g. violation_type")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--k", type=int, default=15, help="neighbours per photo")
    ap.add_argument("--beta", type=float, default=5.5, help="sharpness of the affinity exp(-beta (1 - similarity))")
    ap.add_argument("--alpha", type=float, default=0.9, help="share of a row's mass taken from its neighbours per step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-class-balance", action="store_true", help="do not weigh a class's rows by 1 / their number")
    ap.add_argument("--min-confidence", type=float, default=0.0, metavar="X")
    ap.add_argument("--suspects", action="store_true")
    ap.add_argument("--write-labels", default=None, metavar="OUT.json")
    args = ap.parse_args(argv)
    if args.index is None or args.label_key is None:
        ap.error("--index and --label-key are required")
    if not 0.0 < args.alpha < 1.0:
        ap.error("--alpha must lie inside (0, 1)")
    if not 0.0 <= args.beta < float("inf"):
        ap.error("--beta must be finite and >= 0")
    if not 1 <= args.k <= 63:
        ap.error("--k must lie in 1 .. 63")
    if args.iters < 0:
        ap.error("--iters must be >= 0")
    if not 0.0 <= args.min_confidence <= 1.0:
        ap.error("--min-confidence must lie in [0, 1]")
    return args


def encode_labels(values):
    """(class names sorted, labels: the name's position, -1 for an empty or missing value)"""
    names = sorted({str(v) for v in values if v})
    where = {n: i for i, n in enumerate(names)}
    return names, [where[str(v)] if v else -1 for v in values]


def main(argv=None):
    args = parse_args(argv)
    import clip
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    index = clip.EmbeddingIndex.from_pickle(args.index, dtype=dtype)
    captions = index.metadata

    def field(row, key):
        cap = captions[row]
        return cap.get(key) if isinstance(cap, dict) else None

    names, given = encode_labels([field(r, args.label_key) for r in range(len(index))])
    if not names:
        raise SystemExit(f"propagate_labels: no row of {args.index} has a value under {args.label_key!r}")
    result = index.spread_labels(given, n_classes=max(2, len(names)), k=args.k, beta=args.beta, alpha=args.alpha, n_iter=args.iters,
                                 class_balance=not args.no_class_balance)
    pred, conf, cert = result.pred.tolist(), result.confidence.tolist(), result.certainty.tolist()

    def name_of(r):
        return names[pred[r]] if pred[r] >= 0 and conf[r] >= args.min_confidence else None

    lines = []
    for r, g in enumerate(given):
        if g >= 0:
            continue
        line = dict(row=r, file_name=field(r, "file_name"), label=name_of(r), confidence=conf[r], certainty=cert[r])
        lines.append(line)
        C.log_line(**line)
    suspects = []
    if args.suspects:
        for r in result.suspects.tolist():
            line = dict(suspect=r, file_name=field(r, "file_name"), given=names[given[r]], propagated=names[pred[r]],
                        confidence=conf[r], certainty=cert[r])
            suspects.append(line)
            C.log_line(**line)
    summary = dict(rows=len(index), classes=names, labelled=sum(1 for g in given if g >= 0),
                   newly_labelled=sum(1 for ln in lines if ln["label"] is not None), unreachable=int(result.unreachable.numel()),
                   suspects=int(result.suspects.numel()), n_iter=result.n_iter)
    if args.write_labels:
        rows = [dict(row=r, file_name=field(r, "file_name"), label=names[g] if g >= 0 else name_of(r),
                     inherited=bool(g < 0 and name_of(r) is not None), confidence=conf[r], certainty=cert[r])
                for r, g in enumerate(given)]
        with open(args.write_labels, "w") as f:
            json.dump(rows, f)
        summary["written"] = args.write_labels
    C.log_line(summary=summary)
    return lines, suspects, summary


if __name__ == "__main__":
    main()
