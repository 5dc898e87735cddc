#!/usr/bin/env python3
"""Score a prediction log - the step of /root/reference/CLIP_prefix_caption/score.py:main on the `clip_caption` package:
reads the output_<suffix>.json that predict_caption.py writes (test.py:626-633) and prints the mean character-level
sentence BLEU (smoothing method 1) of `prediction` against `caption` on one JSON line.  Host only.  ROUGE is not carried
over: the reference's rouge() is a stub.

`--clip-score` adds the reference-free measure (Hessel et al. 2021) on the device: the mean CLIPScore of every prediction against
its photo's stored embedding (the pickle of scripts/extract_embeddings.py, matched by `file_name`) and the mean RefCLIPScore
with the log's ground-truth `caption` as the one reference (clip.clip_score).

    python scripts/score_captions.py output_caption.json [--per-item]
    python scripts/score_captions.py output_ct.json --clip-score --embeddings embedding.pkl --clip-checkpoint clip.pt
    python scripts/score_captions.py --clip-score --synthetic     # offline: a seeded log and pickle are generated first"""
from __future__ import annotations

import argparse
import json
import os
import tempfile

import _common as C


def clip_scores(log, embeddings_path, clip_model_name, clip_checkpoint, bs=256):
    """{"clip_score", "ref_clip_score", "n_clip", "clip_scores"}: means over the log's items whose file_name is in the pickle"""
    import clip
    import torch
    from clip_caption.data import load_embeddings
    data = load_embeddings(embeddings_path)
    row_of = {c.get("file_name"): int(c.get("clip_embedding", i)) for i, c in enumerate(data["captions"]) if isinstance(c, dict)}
    items = [d for d in log["caption"] if d.get("file_name") in row_of]
    if not items:
        raise SystemExit(f"no item of the log has its file_name among the {len(row_of)} of {embeddings_path}")
    device = torch.device("cuda:0")
    model, _ = clip.load(clip_model_name, device=device, jit=False)
    if clip_checkpoint:
        model.load_state_dict(torch.load(clip_checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    tokenize = C.get_tokenize(model)
    emb = data["clip_embedding"]
    per_item, ref_item = [], []
    for s in range(0, len(items), bs):
        chunk = items[s:s + bs]
        feats = emb[torch.tensor([row_of[d["file_name"]] for d in chunk])].to(device)
        tokens = tokenize([d["prediction"] for d in chunk]).to(device)
        refs = [tokenize([d["caption"]]).to(device) if d.get("caption") else tokens.new_zeros(0, tokens.shape[1]) for d in chunk]
        res = clip.clip_score(model, feats, tokens, references=refs, batch_size=bs)
        per_item += res.clip_score[:, 0].tolist()
        ref_item += res.ref_clip_score[:, 0].tolist()
    n = len(items)
    return dict(clip_score=sum(per_item) / n, ref_clip_score=sum(ref_item) / n, n_clip=n, clip_scores=per_item)


def synthetic_inputs(tmp: str):
    """a seeded log and the embedding pickle of the same generated images, through the two scripts that write them"""
    import describe_images
    import extract_embeddings
    pkl = extract_embeddings.main(["--synthetic", "--n_images", "9", "--attribute_length", "4", "--out", os.path.join(tmp, "embedding.pkl")])
    log = describe_images.main(["--synthetic", "--n_images", "9", "--entry_length", "8", "--out_dir", tmp])
    return log, pkl


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("log", nargs="?", default="output_log.json", help="prediction log (score.py:9 reads output_log.json)")
    ap.add_argument("--per-item", action="store_true", help="also print every item's score")
    ap.add_argument("--clip-score", action="store_true", help="also the mean CLIPScore / RefCLIPScore (needs --embeddings)")
    ap.add_argument("--embeddings", default=None, metavar="PICKLE", help="--clip-score: the embedding pickle of the log's images")
    ap.add_argument("--clip-model", default="ViT-B/32")
    ap.add_argument("--clip-checkpoint", default=None, metavar="PT", help="--clip-score: fine-tuned CLIP state dict")
    ap.add_argument("--synthetic", action="store_true", help="generate a seeded log and pickle first (offline; CLIP geometry test-tiny)")
    args = ap.parse_args(argv)
    from clip_caption.metrics import corpus_bleu_mean
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        args.log, args.embeddings = synthetic_inputs(tmp.name)
        args.clip_model = "test-tiny"
    with open(args.log, encoding="utf-8") as f:
        log = json.load(f)
    res = corpus_bleu_mean(log)
    out = dict(bleu=res["bleu"], n=res["n"])
    if args.per_item:
        out["scores"] = res["scores"]
    if args.clip_score:
        if not args.embeddings:
            raise SystemExit("--clip-score needs --embeddings PICKLE (scripts/extract_embeddings.py writes it)")
        cs = clip_scores(log, args.embeddings, args.clip_model, args.clip_checkpoint)
        res.update(cs)
        out.update(clip_score=cs["clip_score"], ref_clip_score=cs["ref_clip_score"], n_clip=cs["n_clip"])
        if args.per_item:
            out["clip_scores"] = cs["clip_scores"]
    if tmp is not None:
        tmp.cleanup()
    C.log_line(**out)
    return res


if __name__ == "__main__":
    main()
