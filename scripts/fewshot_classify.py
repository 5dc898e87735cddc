#!/usr/bin/env python3
"""Classify photos from a few stored, labelled embeddings with no training - the step after scripts/extract_embeddings.py:
load the support pickle into a `clip.CacheClassifier` (labels from the annotation dicts' `--key`), classify a query pickle
or image files, print one JSON line per query: {file_name, predicted, probabilities}.

    python scripts/fewshot_classify.py --support embeddings.pkl --key violation_type --queries new.pkl --tune
    python scripts/fewshot_classify.py --support embeddings.pkl --key violation_type --weights models/clip.pt --prompts --images a.jpg b.jpg
    python scripts/fewshot_classify.py --synthetic --tune                                       # offline smoke run
    python scripts/fewshot_classify.py --support embeddings.pkl --queries new.pkl --fit 20 --tune --save-cache cache.pt
    python scripts/fewshot_classify.py --load-cache cache.pt --queries new.pkl

--tune picks alpha and beta on the leave-one-out logits of the support set and prints them first; --prompts adds the
zero-shot term of the prompts "a photo of <class>" (needs the model).  --fit EPOCHS trains the stored keys on the support
set's leave-one-out cross-entropy first (Tip-Adapter-F, towers frozen; --tune then tunes on the trained keys); --save-cache
writes the classifier's state_dict with torch.save and --load-cache classifies with a saved one instead of --support."""
from __future__ import annotations

import argparse
import json
import os
import tempfile

import _common as C
import torch

ALPHAS = (0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)
BETAS = (1.0, 2.0, 5.5, 10.0, 20.0)


def _embed_files(model, preprocess, paths, device, bs: int = 64) -> torch.Tensor:
    from PIL import Image
    feats = []
    with torch.no_grad():
        for s in range(0, len(paths), bs):
            batch = torch.stack([preprocess(Image.open(p)) for p in paths[s:s + bs]]).to(device)
            feats.append(model.encode_image(batch).float())
    return torch.cat(feats)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--support", default=None, help="embedding pickle of scripts/extract_embeddings.py: the labelled photos")
    ap.add_argument("--key", default="violation_type", help="annotation field that holds the label")
    ap.add_argument("--queries", default=None, help="embedding pickle of the photos to classify")
    ap.add_argument("--images", nargs="*", default=None, help="image files to classify (needs the model)")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--weights", default=None, help="fine-tuned state_dict (CLIP/train.py's clip.pt)")
    ap.add_argument("--prompts", action="store_true", help="add the zero-shot term of 'a photo of <class>'")
    ap.add_argument("--tune", action="store_true", help="choose alpha, beta on the support set's leave-one-out logits")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=5.5)
    ap.add_argument("--per_class", choices=("sum", "mean"), default="sum")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--fit", type=int, default=0, metavar="EPOCHS", help="train the stored keys for EPOCHS epochs (leave-one-out)")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save-cache", default=None, metavar="PATH", help="write the classifier's state_dict here")
    ap.add_argument("--load-cache", default=None, metavar="PATH", help="classify with a saved state_dict instead of --support")
    args = ap.parse_args(argv)
    import clip
    from clip_caption.data import load_embeddings, save_embeddings
    device = torch.device("cuda:0")
    tmp = None
    model = preprocess = None
    if args.synthetic:
        # generated photos of the nine classes through a seeded small CLIP: the first 9 of every class are the support set
        tmp = tempfile.TemporaryDirectory()
        anns = json.load(open(C.make_synthetic_annotations(tmp.name, per_class=12)))["annotations"]
        args.model = "test-tiny"
        model, preprocess = clip.load(args.model, device=device, jit=False)
        model.eval()
        feats = _embed_files(model, preprocess, [os.path.join(tmp.name, a["file_name"]) for a in anns], device).cpu()
        sup = [i for i in range(len(anns)) if i % 12 < 9]
        qry = [i for i in range(len(anns)) if i % 12 >= 9]
        args.support = os.path.join(tmp.name, "support.pkl")
        save_embeddings(args.support, feats[sup], [dict(anns[i], clip_embedding=j) for j, i in enumerate(sup)])
        query_feats, names = feats[qry], [anns[i]["file_name"] for i in qry]
    else:
        if (args.support is None and args.load_cache is None) or (args.queries is None) == (not args.images):
            ap.error("--support and exactly one of --queries / --images are required (or --synthetic)")
        if args.images or args.prompts:
            model, preprocess = clip.load(args.model, device=device, jit=False)
            if args.weights:
                model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
            model.eval()
        if args.queries is not None:
            data = load_embeddings(args.queries)
            query_feats = data["clip_embedding"]
            names = [c.get("file_name") if isinstance(c, dict) else None for c in data["captions"]]
        else:
            query_feats, names = _embed_files(model, preprocess, args.images, device), list(args.images)

    dtype = model.compute_dtype if model is not None else None
    if args.load_cache is not None:
        if args.prompts:
            ap.error("--load-cache brings its own text features; drop --prompts")
        clf = clip.CacheClassifier.from_state_dict(torch.load(args.load_cache, map_location="cpu", weights_only=True), device)
        C.log_line(loaded=args.load_cache, support=len(clf), classes=clf.class_names, alpha=clf.alpha, beta=clf.beta)
    else:
        clf = clip.CacheClassifier.from_pickle(args.support, args.key, dtype=dtype, alpha=args.alpha, beta=args.beta,
                                               per_class=args.per_class)
    if args.prompts:
        tokens = C.get_tokenize(model)([f"a photo of {n}" for n in clf.class_names]).to(device)
        with torch.no_grad():
            text = model.encode_text(tokens).float()
        clf = clip.CacheClassifier.from_pickle(args.support, args.key, dtype=dtype, alpha=args.alpha, beta=args.beta,
                                               per_class=args.per_class, text_features=text,
                                               logit_scale=float(model.logit_scale.exp()))
    if args.fit > 0:
        losses = clf.fit(epochs=args.fit, lr=args.lr, seed=args.seed)
        C.log_line(fit=True, epochs=args.fit, lr=args.lr, seed=args.seed, first_loss=losses[0], last_loss=losses[-1])
    if args.tune:
        clf.alpha, clf.beta, acc, _ = clf.tune(ALPHAS, BETAS)
        C.log_line(tuned=True, alpha=clf.alpha, beta=clf.beta, leave_one_out_accuracy=acc, support=len(clf),
                   classes=clf.class_names)
    if args.save_cache is not None:
        torch.save(clf.state_dict(), args.save_cache)
    probs, idx, labels = clf(image_features=query_feats)
    rows = []
    for name, label, p in zip(names, labels, probs.tolist()):
        row = dict(file_name=name, predicted=label, probabilities={n: round(v, 6) for n, v in zip(clf.class_names, p)})
        C.log_line(**row)
        rows.append(row)
    if tmp is not None:
        tmp.cleanup()
    return rows


if __name__ == "__main__":
    main()
