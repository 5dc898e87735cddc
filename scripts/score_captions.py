#!/usr/bin/env python3
"""Score a prediction log - the step of /root/reference/CLIP_prefix_caption/score.py:main on the `clip_caption` package:
reads the output_<suffix>.json that predict_caption.py writes (test.py:626-633) and prints the mean character-level
sentence BLEU (smoothing method 1) of `prediction` against `caption` on one JSON line.  Host only.  ROUGE is not carried
over: the reference's rouge() is a stub.

    python scripts/score_captions.py output_caption.json [--per-item]"""
from __future__ import annotations

import argparse
import json

import _common as C


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("log", nargs="?", default="output_log.json", help="prediction log (score.py:9 reads output_log.json)")
    ap.add_argument("--per-item", action="store_true", help="also print every item's score")
    args = ap.parse_args(argv)
    from clip_caption.metrics import corpus_bleu_mean
    with open(args.log, encoding="utf-8") as f:
        res = corpus_bleu_mean(json.load(f))
    out = dict(bleu=res["bleu"], n=res["n"])
    if args.per_item:
        out["scores"] = res["scores"]
    C.log_line(**out)
    return res


if __name__ == "__main__":
    main()
