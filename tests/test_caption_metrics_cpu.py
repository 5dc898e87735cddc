"""Host-side text metric (clip_caption/metrics.py): character-level sentence BLEU with method-1 smoothing, as
CLIP_prefix_caption/score.py:14-17 computes it through NLTK.  NLTK is not installed where these tests run, so parity with
the package itself is not pinned; the formula is pinned by the cases below, derived by hand:

  ("abcd", "abcd")    every order matches: 1
  ("abce", "abcd")    precisions 3/4, 2/3, 1/2 and 0.1/1 (smoothed), brevity penalty 1: (3/4 * 2/3 * 1/2 * 0.1) ** 0.25 = 0.025 ** 0.25
  ("abcdef", "abc")   precisions 3/3, 2/2, 1/1 and 0.1/1 (no 4-gram in a 3-character hypothesis: denominator max(1, 0)),
                      brevity penalty exp(1 - 6/3): exp(-1) * 0.1 ** 0.25
"""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_identical_strings_score_one():
    from clip_caption.metrics import sentence_bleu
    assert sentence_bleu("abcd", "abcd") == 1.0


def test_one_wrong_character():
    from clip_caption.metrics import sentence_bleu
    assert abs(sentence_bleu("abce", "abcd") - 0.025 ** 0.25) < 1e-12


def test_short_hypothesis_pays_the_brevity_penalty():
    from clip_caption.metrics import sentence_bleu
    assert abs(sentence_bleu("abcdef", "abc") - math.exp(-1) * 0.1 ** 0.25) < 1e-12


def test_longer_hypothesis_has_no_brevity_penalty_and_counts_are_clipped():
    from clip_caption.metrics import sentence_bleu
    # hypothesis "aaaa" against "ab": unigram 'a' clipped to the reference's single 'a' -> 1/4; no 2-, 3-, 4-gram matches ->
    # 0.1/3, 0.1/2, 0.1/1; longer than the reference: no penalty
    want = (1 / 4 * 0.1 / 3 * 0.1 / 2 * 0.1) ** 0.25
    assert abs(sentence_bleu("ab", "aaaa") - want) < 1e-12


def test_nothing_shared_and_empty_hypothesis_score_zero():
    from clip_caption.metrics import sentence_bleu
    assert sentence_bleu("abcd", "wxyz") == 0.0
    assert sentence_bleu("abcd", "") == 0.0


def test_chinese_pair_from_the_annotation_fixture():
    from clip_caption.metrics import sentence_bleu
    labels = json.load(open(os.path.join(ROOT, "tests", "golden", "all_json_summary.json"), encoding="utf-8"))["keys"]["violation_type"]["labels"]
    ref, hyp = labels[7] + labels[8], labels[7] + labels[0]          # two class names each: four shared characters, two different
    assert len(ref) == len(hyp) == 6 and ref != hyp
    a, b = sentence_bleu(ref, hyp), sentence_bleu(ref, hyp)
    assert a == b and 0.0 < a <= 1.0
    # 4/6, 3/5, 2/4, 1/3 matching 1- .. 4-grams, equal lengths
    assert abs(a - (4 / 6 * 3 / 5 * 2 / 4 * 1 / 3) ** 0.25) < 1e-12


def test_corpus_mean_and_exports():
    import clip_caption
    from clip_caption.metrics import corpus_bleu_mean, sentence_bleu
    assert clip_caption.sentence_bleu is sentence_bleu and clip_caption.corpus_bleu_mean is corpus_bleu_mean
    assert hasattr(clip_caption, "evaluate_captions") and hasattr(clip_caption, "CaptionScores")
    assert hasattr(clip_caption.ClipCaptionModel, "score")
    log = {"caption": [dict(prediction="abcd", caption="abcd"), dict(prediction="abcd", caption="abce")]}
    res = corpus_bleu_mean(log)
    assert res["n"] == 2 and res["scores"] == [1.0, sentence_bleu("abce", "abcd")]
    assert abs(res["bleu"] - (1.0 + 0.025 ** 0.25) / 2) < 1e-12
    assert corpus_bleu_mean({"caption": []})["bleu"] == 0.0


def test_score_captions_script(tmp_path):
    from clip_caption.metrics import sentence_bleu
    items = [dict(prediction="abcd", caption="abcd", file_name="a.jpg"), dict(prediction="abcd", caption="abce", file_name="b.jpg"),
             dict(prediction="abc", caption="abcdef", file_name="c.jpg")]
    path = tmp_path / "output_caption.json"
    path.write_text(json.dumps({"caption": items}, ensure_ascii=False, indent=2), encoding="utf-8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "score_captions.py"), str(path)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and lines[0]["n"] == 3
    want = sum(sentence_bleu(d["caption"], d["prediction"]) for d in items) / 3
    assert abs(lines[0]["bleu"] - want) < 1e-12
    assert abs(want - (1.0 + 0.025 ** 0.25 + math.exp(-1) * 0.1 ** 0.25) / 3) < 1e-12
