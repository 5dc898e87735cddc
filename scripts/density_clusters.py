#!/usr/bin/env python3
"""Find the dense themes of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's layout)
without naming a k: load it into a `clip.EmbeddingIndex` and run HDBSCAN on the stored 16-bit rows (clip/hdbscan.py: the
spanning tree on csrc/mst.hip).  One JSON line per cluster: {cluster, size, persistence, central}, the `file_name`s of its
`--show` members with the highest membership probability (equal ones by the lower row), then one line for the noise and one
summary line.

`--label-key violation_type` reads that key of every caption record (the reference's monthly folders carry ''): a cluster
line then adds the majority label among its non-empty values, that label's share of them, and `inherit`, the number of
unlabelled rows of the cluster that would take the label - the conventions of scripts/cluster_images.py.

    python scripts/density_clusters.py --index embeddings.pkl --min-cluster-size 10 --label-key violation_type
    python scripts/density_clusters.py --synthetic                                              # offline smoke run
"""
from __future__ import annotations

import argparse

import _common as C
import torch

from cluster_images import majority_labels
from select_to_label import synthetic_embeddings


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--min-cluster-size", type=int, default=5, help="the fewest photos a cluster holds")
    ap.add_argument("--min-samples", type=int, default=None, help="neighbour that sets a photo's core similarity (default: "
                    "--min-cluster-size, at most 64)")
    ap.add_argument("--selection", default="eom", choices=["eom", "leaf"])
    ap.add_argument("--allow-single-cluster", action="store_true")
    ap.add_argument("--show", type=int, default=3, metavar="R", help="most central photos printed per cluster")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--label-key", default=None, help="caption key that holds a label for some rows, e.g. violation_type")
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    if args.index is None and not args.synthetic:
        ap.error("--index is required (or --synthetic)")
    if args.min_cluster_size < 2 or args.show < 1:
        ap.error("--min-cluster-size must be at least 2 and --show at least 1")
    if args.synthetic and args.label_key is None:
        args.label_key = "violation_type"
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
    result = index.hdbscan(min_cluster_size=args.min_cluster_size, min_samples=args.min_samples,
                           cluster_selection=args.selection, allow_single_cluster=args.allow_single_cluster)
    labels, prob = result.labels.tolist(), result.probabilities.tolist()
    persistence = result.persistence.tolist()
    K = result.n_clusters
    members = [[] for _ in range(K + 1)]                     # the last list holds the noise
    for r, lab in enumerate(labels):
        members[lab].append(r)                              # (-1 indexes the last list)
    major = None
    if args.label_key:
        major = majority_labels([lab if lab >= 0 else K for lab in labels], [field(r, args.label_key) for r in range(N)], K + 1)
    clusters = []
    for c in range(K):
        central = sorted(members[c], key=lambda r: (-prob[r], r))[:args.show]
        line = dict(cluster=c, size=len(members[c]), persistence=persistence[c], central=[field(r, "file_name") for r in central])
        if major is not None:
            line.update(majority_label=major[c][0], majority_share=major[c][1], inherit=major[c][2] if major[c][0] is not None else 0)
        clusters.append(line)
        C.log_line(**line)
    noise = dict(cluster=-1, size=len(members[K]), rows=members[K][:args.show * 4])
    C.log_line(**noise)
    summary = dict(rows=N, clusters=K, noise=len(members[K]), min_cluster_size=args.min_cluster_size,
                   min_samples=args.min_samples if args.min_samples is not None else min(args.min_cluster_size, 64, N),
                   selection=args.selection)
    C.log_line(summary=summary)
    return clusters, noise, summary


if __name__ == "__main__":
    main()
