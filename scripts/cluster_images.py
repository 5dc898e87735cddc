#!/usr/bin/env python3
"""Organise the photos of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's layout) into
`--k` kinds: load it into a `clip.EmbeddingIndex`, run spherical k-means on the stored 16-bit rows (csrc/embed_kmeans.hip) and
print one JSON line per cluster: {cluster, size, concentration, representatives}, the `file_name`s of its `--show` members
nearest to the centroid, then one summary line.

`--label-key violation_type` reads that key of every caption record (the reference's monthly folders carry ''): a cluster
line then adds the majority label among its non-empty values, that label's share of them, and `inherit`, the number of
unlabelled rows of the cluster that would take the label.  `--prompts FILE` (one prompt per line) with `--model` /
`--checkpoint` names every cluster by its nearest prompt.  `--write-labels OUT.json` writes one record per row.

    python scripts/cluster_images.py --index embeddings.pkl --k 32 --show 3 --label-key violation_type --write-labels rows.json
"""
from __future__ import annotations

import argparse
import json

import _common as C
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--k", type=int, default=None, help="number of clusters")
    ap.add_argument("--show", type=int, default=3, metavar="R", help="representatives printed per cluster")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--init", default="kmeans++", choices=["kmeans++", "random"])
    ap.add_argument("--n-init", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--label-key", default=None, help="caption key that holds a label for some rows, e.g. violation_type")
    ap.add_argument("--prompts", default=None, metavar="FILE", help="one text prompt per line: name every cluster by the nearest")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned state_dict (CLIP/train.py's clip.pt) for --prompts")
    ap.add_argument("--write-labels", default=None, metavar="OUT.json")
    args = ap.parse_args(argv)
    if args.index is None or args.k is None:
        ap.error("--index and --k are required")
    if args.k < 1 or args.show < 1:
        ap.error("--k and --show must be at least 1")
    if args.checkpoint is not None and args.prompts is None:
        ap.error("--checkpoint is only used with --prompts")
    return args


def majority_labels(labels, values, k):
    """Per cluster: (majority value among the non-empty ones or None, its share of them, rows with an empty value).  Equal
    counts go to the value that sorts first."""
    table = [{} for _ in range(k)]
    blank = [0] * k
    for lab, v in zip(labels, values):
        if v:
            table[lab][v] = table[lab].get(v, 0) + 1
        else:
            blank[lab] += 1
    out = []
    for t, b in zip(table, blank):
        if not t:
            out.append((None, 0.0, b))
            continue
        top = min(t, key=lambda v: (-t[v], v))
        out.append((top, t[top] / sum(t.values()), b))
    return out


def main(argv=None):
    args = parse_args(argv)
    import clip
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    index = clip.EmbeddingIndex.from_pickle(args.index, dtype=dtype)
    captions = index.metadata
    result = index.kmeans(args.k, max_iter=args.max_iter, tol=args.tol, init=args.init, n_init=args.n_init, seed=args.seed)
    labels = result.labels.tolist()
    reps = result.representatives(args.show).tolist()
    counts, conc = result.counts.tolist(), result.concentration.tolist()

    def field(row, key):
        cap = captions[row]
        return cap.get(key) if isinstance(cap, dict) else None

    major = None
    if args.label_key:
        major = majority_labels(labels, [field(r, args.label_key) for r in range(len(labels))], args.k)
    names = None
    if args.prompts:
        prompts = [ln.strip() for ln in open(args.prompts) if ln.strip()]
        device = torch.device("cuda:0")
        model, _ = clip.load(args.model, device=device, jit=False)
        if args.checkpoint:
            model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
        model.eval()
        with torch.no_grad():
            text = model.encode_text(C.get_tokenize(model)(prompts).to(device))
        which, score = clip.name_clusters(result, text.float())
        names = [(prompts[i], s) for i, s in zip(which.tolist(), score.tolist())]
    clusters = []
    for c in range(args.k):
        line = dict(cluster=c, size=counts[c], concentration=conc[c],
                    representatives=[field(r, "file_name") for r in reps[c] if r >= 0])
        if major is not None:
            line.update(majority_label=major[c][0], majority_share=major[c][1], inherit=major[c][2] if major[c][0] is not None else 0)
        if names is not None:
            line.update(prompt=names[c][0], prompt_score=names[c][1])
        clusters.append(line)
        C.log_line(**line)
    summary = dict(rows=len(index), k=args.k, n_iter=result.n_iter, converged=result.converged, objective=result.objective,
                   empty_clusters=sum(1 for n in counts if n == 0))
    if args.write_labels:
        scores, margin = result.scores.tolist(), result.margin.tolist()
        rows = []
        for r, lab in enumerate(labels):
            rec = dict(row=r, file_name=field(r, "file_name"), cluster=lab, score=scores[r],
                       margin=None if margin[r] != margin[r] else margin[r])
            if major is not None:
                own = field(r, args.label_key)
                rec.update(label=own if own else major[lab][0], inherited=bool(not own and major[lab][0] is not None))
            rows.append(rec)
        with open(args.write_labels, "w") as f:
            json.dump(rows, f)
        summary["written"] = args.write_labels
    C.log_line(summary=summary)
    return clusters, summary


if __name__ == "__main__":
    main()
