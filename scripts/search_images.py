#!/usr/bin/env python3
"""Search stored embeddings - the step after scripts/extract_embeddings.py (CLIP_prefix_caption/parse_coco.py's pickle):
load the pickle into a `clip.EmbeddingIndex`, embed one text or one image with the model, print the k best rows as one
JSON line each: {rank, score, index, file_name}.

    python scripts/search_images.py --index embeddings.pkl --weights models/clip.pt --text "worker without helmet" --k 10
    python scripts/search_images.py --index embeddings.pkl --weights models/clip.pt --image site.jpg
    python scripts/search_images.py --synthetic --k 5                                              # offline smoke run

--querybank PICKLE (another embedding pickle: a sample of typical queries, e.g. the captions' text embeddings) ranks by the
hubness-corrected similarity of clip/hubness.py instead: --hub-method dis | is | csls, --beta for the first two.
"""
from __future__ import annotations

import argparse

import _common as C
import torch


def synthetic_index(n: int = 4096, dim: int = 512, seed: int = 567):
    """Seeded stand-in for an embedding pickle: n rows around the 9 class directions, and a query near the first class."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(len(C.CLASSES), dim, generator=g)
    cls = torch.arange(n) % len(C.CLASSES)
    feats = centres[cls] + 0.5 * torch.randn(n, dim, generator=g)
    meta = [{"file_name": f"images/{C.CLASSES[int(c)]}_{i:05d}.png", "clip_embedding": i} for i, c in enumerate(cls)]
    query = centres[:1] + 0.1 * torch.randn(1, dim, generator=g)
    return feats, meta, query


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--text", default=None)
    ap.add_argument("--image", default=None)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--weights", default=None, help="fine-tuned state_dict (CLIP/train.py's clip.pt)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--querybank", default=None, help="embedding pickle of typical queries: hubness-corrected ranking (clip/hubness.py)")
    ap.add_argument("--hub-method", default="dis", choices=("dis", "is", "csls"))
    ap.add_argument("--beta", type=float, default=20.0, help="inverse temperature of --hub-method dis / is")
    args = ap.parse_args(argv)
    import clip
    device = torch.device("cuda:0")
    if args.synthetic:
        feats, meta, query = synthetic_index()
        index = clip.EmbeddingIndex(feats, metadata=meta)
        kw = {}
        if args.querybank:                                                           # stands in for the pickle: the stored rows themselves
            kw["querybank"] = index.querybank(feats[::16], method=args.hub_method, beta=args.beta)
        scores, idx = index.search(query, args.k, **kw)
    else:
        if args.index is None or (args.text is None) == (args.image is None):
            ap.error("--index and exactly one of --text / --image are required (or --synthetic)")
        model, preprocess = clip.load(args.model, device=device, jit=False)
        if args.weights:
            model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
        model.eval()
        index = clip.EmbeddingIndex.from_pickle(args.index, dtype=model.compute_dtype)
        kw = {}
        if args.querybank:
            from clip_caption.data import load_embeddings
            kw["querybank"] = index.querybank(load_embeddings(args.querybank)["clip_embedding"], method=args.hub_method, beta=args.beta)
        if args.text is not None:
            scores, idx = index.search_text(model, C.get_tokenize(model)([args.text]).to(device), args.k, **kw)
        else:
            from PIL import Image
            scores, idx = index.search_image(model, preprocess(Image.open(args.image)).unsqueeze(0).to(device), args.k, **kw)
    hits = []
    for rank, (s, i) in enumerate(zip(scores[0].tolist(), idx[0].tolist()), start=1):
        m = index.metadata[i] if index.metadata is not None else None
        hit = dict(rank=rank, score=s, index=i, file_name=m.get("file_name") if isinstance(m, dict) else None)
        C.log_line(**hit)
        hits.append(hit)
    return hits


if __name__ == "__main__":
    main()
