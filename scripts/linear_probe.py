#!/usr/bin/env python3
"""Train a linear probe (multinomial logistic regression, `clip.LinearProbe`) on a labelled embedding pickle of
scripts/extract_embeddings.py and classify with it.  One JSON line per l2 of the sweep, one for the chosen model, and with
--queries one per query: {file_name, predicted, probabilities}.

    python scripts/linear_probe.py embeddings.pkl --key violation_type --val-fraction 0.2 --dedup-threshold 0.95
    python scripts/linear_probe.py embeddings.pkl --val val.pkl --l2 1e-4,1e-3,1e-2 --class-weight balanced --save probe.pt
    python scripts/linear_probe.py embeddings.pkl --weights models/clip.pt --prompts --queries new.pkl
    python scripts/linear_probe.py --load probe.pt --queries new.pkl

The validation rows come from --val or are held out with --val-fraction; --dedup-threshold holds out whole near-duplicate
groups (EmbeddingIndex.duplicate_groups + group_split), so that no validation photo has a twin on the training side.  Without
validation data only the first l2 of the sweep is fitted.  --prompts starts from CLIP's zero-shot classifier of the prompts
"a photo of <class>" (needs the model)."""
from __future__ import annotations

import argparse

L2S = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("embeddings", nargs="?", default=None, help="labelled embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--key", default="violation_type", help="annotation field that holds the label")
    ap.add_argument("--val", default=None, help="embedding pickle of the validation photos")
    ap.add_argument("--val-fraction", type=float, default=None, help="hold this fraction of the rows out for validation")
    ap.add_argument("--dedup-threshold", type=float, default=None, help="keep near-duplicates above this similarity on one side")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--l2", type=lambda s: [float(v) for v in s.split(",") if v], default=list(L2S), help="comma-separated sweep")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--class-weight", choices=("none", "balanced"), default="none")
    ap.add_argument("--prompts", action="store_true", help="start from the zero-shot classifier of 'a photo of <class>'")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--weights", default=None, help="fine-tuned state_dict (CLIP/train.py's clip.pt)")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the probe's state_dict here")
    ap.add_argument("--load", default=None, metavar="PATH", help="classify with a saved state_dict instead of training")
    ap.add_argument("--queries", default=None, help="embedding pickle of the photos to classify")
    args = ap.parse_args(argv)
    if args.val is not None and args.val_fraction is not None:
        ap.error("--val and --val-fraction exclude each other")
    if args.dedup_threshold is not None and args.val_fraction is None:
        ap.error("--dedup-threshold needs --val-fraction")
    if (args.embeddings is None) == (args.load is None):
        ap.error("give the labelled embedding pickle, or --load a saved probe")
    if not args.l2:
        ap.error("--l2: empty sweep")
    return args


def main(argv=None):
    args = parse_args(argv)
    import _common as C
    import torch
    import clip
    from clip.fewshot import _labels_from_metadata
    from clip_caption.data import load_embeddings
    device = torch.device("cuda:0")
    if args.load is not None:
        probe = clip.LinearProbe.from_state_dict(torch.load(args.load, map_location="cpu", weights_only=True), device)
        C.log_line(loaded=args.load, classes=probe.class_names, l2=probe.l2)
    else:
        model = None
        if args.prompts:
            model, _ = clip.load(args.model, device=device, jit=False)
            if args.weights:
                model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
            model.eval()
        index = clip.EmbeddingIndex.from_pickle(args.embeddings, dtype=None if model is None else model.compute_dtype)
        labels, names = _labels_from_metadata(index.metadata, args.key, None)
        rows = index.features
        train_idx, val_rows, val_labels = list(range(len(index))), None, None
        if args.val is not None:
            vidx = clip.EmbeddingIndex.from_pickle(args.val, dtype=index.dtype)
            val_rows, val_labels = vidx.features, _labels_from_metadata(vidx.metadata, args.key, names)[0]
        elif args.val_fraction is not None:
            groups = index.duplicate_groups(args.dedup_threshold) if args.dedup_threshold is not None else torch.arange(len(index))
            train_idx, val_idx = clip.group_split(groups, args.val_fraction, args.seed)
            vi = torch.tensor(val_idx, device=rows.device)
            val_rows, val_labels = rows[vi].contiguous(), labels[val_idx]
        ti = torch.tensor(train_idx, device=rows.device)
        train_rows, train_labels = rows[ti].contiguous(), labels[train_idx]
        probe = clip.LinearProbe(index.dim, class_names=names, dtype=index.dtype)
        kw = dict(max_iter=args.max_iter, tol=args.tol, class_weight=None if args.class_weight == "none" else "balanced")
        if args.prompts:
            tokens = C.get_tokenize(model)([f"a photo of {n}" for n in names]).to(device)
            with torch.no_grad():
                text = model.encode_text(tokens).float()
            kw.update(init="zero_shot", text_features=text / text.norm(dim=1, keepdim=True), logit_scale=float(model.logit_scale.exp()))
        if val_rows is not None:
            table = probe.sweep_l2(train_rows, train_labels, val_rows, val_labels, args.l2, **kw)
            for row in table:
                C.log_line(**row)
        else:                                          # nothing to choose by: the first l2 is the model
            C.log_line(**probe.fit(train_rows, train_labels, l2=args.l2[0], **kw).as_dict())
        C.log_line(chosen=True, l2=probe.l2, train_rows=len(train_idx), train_accuracy=probe.score(train_rows, train_labels),
                   val_accuracy=None if val_rows is None else probe.score(val_rows, val_labels), classes=names,
                   **{k: v for k, v in probe.result.as_dict().items() if k != "l2"})
        if args.save is not None:
            torch.save(probe.state_dict(), args.save)
    out = []
    if args.queries is not None:
        data = load_embeddings(args.queries)
        names = [c.get("file_name") if isinstance(c, dict) else None for c in data["captions"]]
        probs, _, picked = probe(image_features=data["clip_embedding"].to(device))
        classes = probe.class_names if probe.class_names is not None else list(range(probe.num_classes))
        for name, label, p in zip(names, picked, probs.tolist()):
            row = dict(file_name=name, predicted=label, probabilities={n: round(v, 6) for n, v in zip(classes, p)})
            C.log_line(**row)
            out.append(row)
    return out


if __name__ == "__main__":
    main()
