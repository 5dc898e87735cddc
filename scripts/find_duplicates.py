#!/usr/bin/env python3
"""Find the near-duplicate photos of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's
layout): load it into a `clip.EmbeddingIndex`, self-join it at `--threshold` (cosine similarity of the normalised 16-bit
rows) and print one JSON line per single-linkage group of more than one row: {rows, file_names, min_score} (min_score: the
weakest pair of the group that reached the threshold), then one summary line.  `--write-deduped OUT.pkl` writes the pickle
again with only the first row of every group, `captions[i]["clip_embedding"]` renumbered to the kept rows.

    python scripts/find_duplicates.py --index embeddings.pkl --threshold 0.95 --write-deduped deduped.pkl
    python scripts/find_duplicates.py --synthetic                                                 # offline smoke run
"""
from __future__ import annotations

import argparse

import _common as C
import torch


def synthetic_embeddings(n: int = 512, dim: int = 512, seed: int = 567):
    """Seeded stand-in for an embedding pickle: n distinct rows, every tenth of them re-emitted once or twice with a little
    noise (the same photo in the next report), all shuffled.  Returns (features, captions)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, dim, generator=g)
    base = base / base.norm(dim=1, keepdim=True)
    rows, origin = [base], list(range(n))
    for i in range(0, n, 10):
        for _ in range(1 + (i // 10) % 2):
            rows.append(base[i:i + 1] + 0.15 / dim ** 0.5 * torch.randn(1, dim, generator=g))
            origin.append(i)
    feats = torch.cat(rows)
    perm = torch.randperm(feats.shape[0], generator=g)
    feats = feats[perm]
    caps = [{"file_name": f"images/{C.CLASSES[origin[int(p)] % len(C.CLASSES)]}_{origin[int(p)]:05d}_{j:05d}.png", "clip_embedding": j,
             "caption": f"photo {origin[int(p)]}"} for j, p in enumerate(perm)]
    return feats, caps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--write-deduped", default=None, metavar="OUT.pkl")
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    import clip
    from clip_caption.data import load_embeddings, save_embeddings
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.synthetic:
        feats, captions = synthetic_embeddings()
    else:
        if args.index is None:
            ap.error("--index is required (or --synthetic)")
        data = load_embeddings(args.index)
        emb, captions = data["clip_embedding"], data["captions"]
        order = [int(c["clip_embedding"]) if isinstance(c, dict) and "clip_embedding" in c else i for i, c in enumerate(captions)]
        feats = emb[torch.tensor(order, dtype=torch.long)]                     # row i belongs to captions[i], as from_pickle
    index = clip.EmbeddingIndex(feats, dtype=dtype, metadata=captions)
    pairs, scores = index.duplicate_pairs(args.threshold)
    labels = clip.connected_components(len(index), pairs).tolist()
    weakest = {}
    for (a, _), s in zip(pairs.tolist(), scores.tolist()):
        weakest[labels[a]] = min(s, weakest.get(labels[a], s))
    members = {}
    for row, lab in enumerate(labels):
        members.setdefault(lab, []).append(row)
    groups = []
    for lab in sorted(weakest):
        rows = members[lab]
        names = [captions[r].get("file_name") if isinstance(captions[r], dict) else None for r in rows]
        groups.append(dict(rows=rows, file_names=names, min_score=weakest[lab]))
        C.log_line(**groups[-1])
    keep = sorted(members)                                                      # the first (lowest) row of every group
    summary = dict(rows=len(index), threshold=args.threshold, pairs=int(pairs.shape[0]), duplicate_groups=len(groups),
                   rows_in_groups=sum(len(gr["rows"]) for gr in groups), rows_kept=len(keep))
    if args.write_deduped:
        kept_caps = []
        for new, row in enumerate(keep):
            cap = dict(captions[row]) if isinstance(captions[row], dict) else captions[row]
            if isinstance(cap, dict):
                cap["clip_embedding"] = new
            kept_caps.append(cap)
        save_embeddings(args.write_deduped, feats[torch.tensor(keep, dtype=torch.long)], kept_caps)
        summary["written"] = args.write_deduped
    C.log_line(summary=summary)
    return groups, summary


if __name__ == "__main__":
    main()
