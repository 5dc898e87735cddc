"""Captioner.describe(best_of=K) on the MI355X: K drawn captions per image, CLIP's choice among them (cclip_caption_select),
against the pieces it is made of - generate_sample_batch on the same prefixes and uniforms, encode_text of the drawn texts and
the float64 selection reference (tests/caption_select_ref.py) - plus clip.clip_score and the two scripts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.dirname(os.path.abspath(__file__))]
import caption_select_ref as R  # noqa: E402

TYPES = {"s": "a", "v": "b"}
VIOS = ["c", "d", "e", "f", "g", "h", "i", "j", "k"]
FEATURE_TOL = 2e-3        # relative row error of fp16 tower features between two batch compositions (tests/test_clip_parity_gpu.py)
ENTRY = 10
_CACHE = {}


def _setup():
    """(captioner, clip model, caption model, tokenizer, clip tokenize, caption geometry) on seeded test-tiny state dicts, fp16"""
    if "s" in _CACHE:
        return _CACHE["s"]
    import _common as C
    import clip
    from clip.weights import MODELS, init_state_dict
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    clip_model = clip.build_model(init_state_dict(MODELS["test-tiny"], 3)).cuda().eval().half()
    geo = GPT2_MODELS["test-tiny"]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval().half()
    tok = C.ByteCaptionTokenizer(geo.vocab_size)
    ctok = C.get_tokenize(clip_model)
    cap = Captioner(clip_model, model, tok, clip_tokenize=ctok, caption_types=TYPES, violation_types=VIOS,
                    prefix_length=geo.prefix_length, attribute_length=geo.attribute_length)
    _CACHE["s"] = (cap, clip_model, model, tok, ctok, geo)
    return _CACHE["s"]


def _images(clip_model, n, seed=4):
    from clip.weights import synthetic_images
    return synthetic_images(n, clip_model.geo, seed).cuda()


def _uniforms(n, K, seed=5):
    return torch.rand(ENTRY, n * K, generator=torch.Generator().manual_seed(seed))


def _described(N=3, K=4):
    """one describe(best_of=K) call shared by the tests that only read it"""
    key = ("d", N, K)
    if key not in _CACHE:
        cap, clip_model, *_ = _setup()
        images, U = _images(clip_model, N), _uniforms(N, K)
        kw = dict(best_of=K, uniforms=U, entry_length=ENTRY, temperature=1.0, top_p=0.9, return_tokens=True)
        _CACHE[key] = (images, U, kw, cap.describe(images, **kw))
    return _CACHE[key]


def _embeds(cap, model, images):
    with torch.no_grad():
        feat = cap._features_one_by_one(images)
        _, _, ids = cap._classify(feat)
        proj = cap._project(feat)
        return feat, torch.cat((proj.view(images.shape[0], cap.prefix_length, -1), model.gpt.transformer.wte(ids.long())), dim=1)


def test_candidates_are_the_samplers_draws_and_the_selection_is_the_float64_reference():
    from clip_caption import generate_sample_batch
    cap, clip_model, model, tok, ctok, geo = _setup()
    N, K = 3, 4
    images, U, kw, (records, extra) = _described(N, K)
    feat, emb = _embeds(cap, model, images)
    per = generate_sample_batch(model, tok, emb, num_samples=K, entry_length=ENTRY, top_p=0.9, temperature=1.0, uniforms=U,
                                return_tokens=True)
    E = feat.shape[1]
    tf, order = extra["text_features"], extra["order"].cpu().numpy()
    assert tf.shape == (N * K, E) and tf.dtype == torch.float32 and order.shape == (N, K)
    draws, lm = [], []
    for i in range(N):
        texts, tokens, lengths, total = per[i]
        assert torch.equal(extra["tokens"][i][1], tokens) and torch.equal(extra["tokens"][i][2], lengths)
        by_lm = (total / lengths).argsort(descending=True, stable=True).tolist()
        row = [None] * K
        for place, k in enumerate(by_lm):                                  # generate_sample_batch lists its texts best first
            row[k] = texts[place]
        draws += row
        lm.append((total / lengths).float().cpu())
        assert sorted(c["text"] for c in records[i]["candidates"]) == sorted(texts)
    lm = torch.cat(lm).numpy()
    # the rows the kernel saw are the text tower's features of exactly these texts
    with torch.no_grad():
        own = clip_model.encode_text(ctok(draws).cuda()).float()
    rel = ((tf - own).norm(dim=1) / own.norm(dim=1)).max().item()
    assert rel < FEATURE_TOL, rel
    for a in range(N * K):                                                 # equal texts were encoded once: equal bits
        for b in range(a):
            if draws[a] == draws[b]:
                assert torch.equal(tf[a], tf[b])
    # the selection: the float64 reference on the returned text features and the image features
    r = R.caption_select_ref(feat.cpu().numpy(), tf.cpu().numpy(), K, lm_mean=lm, lm_weight=0.0)
    b_cos, b_cs, _, b_sc = R.bounds(r, E, 2.5, lm, 0.0)
    rank = np.argsort(order, axis=1)
    assert (np.sort(order, axis=1) == np.arange(K)[None]).all()
    for i, rec in enumerate(records):
        cands = rec["candidates"]
        assert len(cands) == K and [c["text"] for c in cands] == [draws[i * K + k] for k in order[i]]
        assert rec["prediction"] == cands[0]["text"] and rec["clip_score"] == cands[0]["clip_score"]
        assert set(rec) >= {"caption_type", "violation_type", "attribute", "prediction", "type_probs", "violation_probs",
                            "clip_score", "candidates"}
        for place, k in enumerate(order[i]):
            c = cands[place]
            assert abs(c["cos"] - r.cos[i, k]) <= b_cos[i, k] and abs(c["clip_score"] - r.clip_score[i, k]) <= b_cs[i, k]
            assert abs(c["lm_logprob"] - lm[i * K + k]) <= 1e-6 * max(1.0, abs(lm[i * K + k]))
        for j in range(K):
            for k in range(j + 1, K):
                gap = r.score[i, j] - r.score[i, k]
                if draws[i * K + j] == draws[i * K + k]:
                    assert rank[i, j] < rank[i, k]                         # duplicate draws tie exactly: the lower index first
                elif abs(gap) > 2 * max(b_sc[i, j], b_sc[i, k]):
                    assert (rank[i, j] < rank[i, k]) == (gap > 0), (i, j, k, gap)


def test_lm_weight_enters_the_order():
    cap, clip_model, model, tok, ctok, geo = _setup()
    N, K = 3, 4
    images, U, kw, (records, extra) = _described(N, K)
    rec2, extra2 = cap.describe(images, **dict(kw, lm_weight=50.0))        # the language model decides
    assert torch.equal(extra2["text_features"], extra["text_features"])
    for a, b in zip(records, rec2):
        lps = [c["lm_logprob"] for c in b["candidates"]]
        texts = [c["text"] for c in b["candidates"]]
        assert sorted(texts) == sorted(c["text"] for c in a["candidates"])
        for x, y, tx, ty in zip(lps, lps[1:], texts, texts[1:]):
            assert x >= y - 2.0 / 50.0 or tx == ty                         # |cos| <= 1 moves a score by at most 1 / 50 of lm


def test_same_uniforms_same_records_and_chunks_agree():
    cap, clip_model, *_ = _setup()
    N, K = 3, 4
    images, U, kw, (records, extra) = _described(N, K)
    again, extra2 = cap.describe(images, **kw)
    assert again == records and torch.equal(extra2["order"], extra["order"])
    assert torch.equal(extra2["text_features"], extra["text_features"])
    # 64 // 24 = 2 images per chunk: three images go in two chunks, each the call on its own images and uniform columns
    K2 = 24
    U2 = _uniforms(N, K2, seed=6)
    kw2 = dict(best_of=K2, entry_length=ENTRY, temperature=1.0, top_p=0.9)
    whole = cap.describe(images, uniforms=U2, **kw2)
    parts = cap.describe(images[:2], uniforms=U2[:, :2 * K2], **kw2) + cap.describe(images[2:], uniforms=U2[:, 2 * K2:], **kw2)
    assert len(whole) == N and all(len(r["candidates"]) == K2 for r in whole)
    assert whole == parts


def test_best_of_one_returns_the_single_draw():
    from clip_caption import generate_sample_batch
    cap, clip_model, model, tok, ctok, geo = _setup()
    images = _images(clip_model, 2, seed=12)
    U = _uniforms(2, 1, seed=8)
    records = cap.describe(images, best_of=1, uniforms=U, entry_length=ENTRY, temperature=1.0)
    _, emb = _embeds(cap, model, images)
    texts = generate_sample_batch(model, tok, emb, num_samples=1, entry_length=ENTRY, top_p=0.8, temperature=1.0, uniforms=U)
    for rec, t in zip(records, texts):
        assert rec["prediction"] == t[0] and len(rec["candidates"]) == 1 and rec["candidates"][0]["text"] == t[0]


def test_best_of_zero_is_the_call_without_the_argument():
    cap, clip_model, *_ = _setup()
    images = _images(clip_model, 3, seed=13)
    kw = dict(beam_size=3, entry_length=ENTRY, temperature=0.5)
    want, e0 = cap.describe(images, return_tokens=True, **kw)
    got, e1 = cap.describe(images, return_tokens=True, best_of=0, lm_weight=3.0, uniforms=None, generator=None, **kw)
    assert got == want and set(e1) == set(e0) == {"ids", "index", "tokens"}
    assert all("clip_score" not in r and "candidates" not in r for r in got)
    with pytest.raises(ValueError, match="best_of"):
        cap.describe(images, best_of=-1)
    with pytest.raises(NotImplementedError, match="best_of = 65"):
        cap.describe(images, best_of=65)
    with pytest.raises(ValueError, match="uniforms must be"):
        cap.describe(images, best_of=2, uniforms=torch.rand(ENTRY, 5), entry_length=ENTRY)


def test_training_flags_are_left_as_found():
    cap, clip_model, model, *_ = _setup()
    images = _images(clip_model, 2, seed=14)
    cap.describe(images, best_of=2, entry_length=4, generator=torch.Generator(device="cuda").manual_seed(1))
    assert not clip_model.training and not model.training
    try:
        model.train()
        cap.describe(images, best_of=2, entry_length=4)
        assert model.training and not clip_model.training
    finally:
        model.eval()


def test_explain_best_of_explains_the_selected_caption():
    cap, clip_model, *_ = _setup()
    images = _images(clip_model, 2, seed=15)
    U = _uniforms(2, 3, seed=9)
    kw = dict(best_of=3, uniforms=U, entry_length=ENTRY, temperature=1.0)
    plain = cap.describe(images, **kw)
    recs = cap.explain(images, size=32, score_model=clip_model, **kw)
    for a, b in zip(plain, recs):
        assert b["prediction"] == a["prediction"] and b["candidates"] == a["candidates"]
        assert torch.equal(b["clip_tokens"].cpu(), cap._caption_tokens([a["prediction"]])[0].cpu())
        assert b["overlay"].shape == (32, 32, 3)


def test_clip_score_on_images_and_tokens_equals_clip_score_features():
    import clip
    cap, clip_model, model, tok, ctok, geo = _setup()
    N, K = 3, 4
    images = _images(clip_model, N, seed=16)
    texts = [f"caption {n} {k % 3}" for n in range(N) for k in range(K)]   # k = 0 and 3 of every image are one text
    tokens = ctok(texts).cuda().view(N, K, -1)
    refs = [ctok([f"truth {n} {j}" for j in range(c)]).cuda() if c else tokens.new_zeros(0, tokens.shape[2]) for n, c in enumerate((2, 0, 1))]
    res = clip.clip_score(clip_model, images, tokens, references=refs)
    with torch.no_grad():
        fi = clip_model.encode_image(images).float()
        every = torch.cat([tokens.view(N * K, -1)] + refs)
        uniq, inv = clip.unique_texts(every)
        ft = clip_model.encode_text(uniq).float()[inv.long()]
    want = clip.clip_score_features(fi, ft[:N * K], reference_features=ft[N * K:], reference_offsets=[0, 2, 2, 3])
    for a, b in zip(res, want):
        assert torch.equal(a, b)
    assert res.cos.is_cuda and res.order.shape == (N, K) and (res.ref_clip_score[1] == 0).all()
    rank = res.order.long().argsort(dim=1)
    assert bool((res.cos[:, 0] == res.cos[:, 3]).all()) and bool((rank[:, 0] < rank[:, 3]).all())   # duplicates: exact tie, lower first
    # the [N, L] form and image features in place of images
    one = clip.clip_score(clip_model, fi, tokens[:, 1])
    assert one.cos.shape == (N, 1) and one.ref_clip_score is None and bool((one.best == 0).all())
    assert torch.allclose(one.cos[:, 0], res.cos[:, 1], atol=2 * FEATURE_TOL)
    assert torch.equal(one.clip_score, 2.5 * one.cos.clamp(min=0))


def test_scripts_emit_the_new_keys(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "describe_images.py"), "--synthetic", "--n_images", "5", "--bs", "4",
                        "--entry_length", "8", "--best-of", "3", "--lm-weight", "0.1", "--seed", "7", "--out_dir", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = json.loads((out / "output_ct.json").read_text())["caption"]
    assert len(recs) == 5
    for rec in recs:
        assert set(rec) == {"caption_type", "violation_type", "prediction", "caption", "file_name", "clip_score", "candidates"}
        assert len(rec["candidates"]) == 3 and rec["prediction"] == rec["candidates"][0]["text"]
        assert set(rec["candidates"][0]) == {"text", "cos", "clip_score", "lm_logprob"}
        assert rec["clip_score"] == rec["candidates"][0]["clip_score"] >= 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "score_captions.py"), "--clip-score", "--synthetic"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(line) == {"bleu", "n", "clip_score", "ref_clip_score", "n_clip"} and line["n"] == line["n_clip"] == 9
    assert 0 <= line["clip_score"] <= 2.5 and 0 <= line["ref_clip_score"] <= 2.5
