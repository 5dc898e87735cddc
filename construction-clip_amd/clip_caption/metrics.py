"""Text metric of the caption pipeline's last step (CLIP_prefix_caption/score.py:8-25): character-level sentence BLEU with
method-1 smoothing, averaged over a prediction log.  Host only, standard library only.

score.py calls nltk.translate.bleu_score.sentence_bleu(reference, hypothesis, smoothing_function=SmoothingFunction().method1)
on `list(str)` tokens with one reference and the default uniform 4-gram weights.  NLTK is not a dependency of this package,
so what follows restates that formula.  Parity with NLTK itself is NOT pinned by a test here (the package is absent where
the tests run); the formula is pinned by hand-derived cases in tests/test_caption_metrics_cpu.py:

  p_n   = clipped n-gram matches / max(1, len(hyp) - n + 1), n = 1 .. 4; a zero numerator becomes 0.1 (method 1)
  BP    = 1 if len(hyp) > len(ref) else exp(1 - len(ref) / len(hyp))
  BLEU  = BP * exp(mean_n log p_n); 0 when no unigram matches or the hypothesis is empty
"""
from __future__ import annotations

import math
from collections import Counter
from typing import Dict, List

_MAX_N = 4
_EPSILON = 0.1


def _ngrams(tokens: List[str], n: int) -> Counter:
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


def sentence_bleu(reference: str, hypothesis: str) -> float:
    """Character-level BLEU-4 of `hypothesis` against the single `reference`, method-1 smoothing (module docstring)."""
    ref, hyp = list(reference), list(hypothesis)
    if not hyp:
        return 0.0
    log_sum = 0.0
    for n in range(1, _MAX_N + 1):
        have, want = _ngrams(hyp, n), _ngrams(ref, n)
        num = sum(min(c, want[g]) for g, c in have.items())            # clipped by the reference's count
        den = max(1, len(hyp) - n + 1)
        if num == 0:
            if n == 1:
                return 0.0                                              # no shared character at all
            num = _EPSILON
        log_sum += math.log(num / den) / _MAX_N
    bp = 1.0 if len(hyp) > len(ref) else math.exp(1.0 - len(ref) / len(hyp))
    return bp * math.exp(log_sum)


def corpus_bleu_mean(log: Dict) -> Dict:
    """Mean sentence BLEU over a prediction log in the layout predict_caption.py writes (test.py:626-633):
    {"caption": [{"prediction": str, "caption": str, ...}, ...]}.  Returns {"bleu": mean, "n": count, "scores": per item}."""
    scores = [sentence_bleu(d["caption"], d["prediction"]) for d in log["caption"]]
    return dict(bleu=sum(scores) / len(scores) if scores else 0.0, n=len(scores), scores=scores)
