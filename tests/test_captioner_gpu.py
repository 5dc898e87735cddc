"""clip_caption.Captioner on the MI355X: `describe(images)` against the composition of the public pieces it replaces, image by
image (encode_image -> two ZeroShotClassifiers -> tokenizer.encode -> clip_project -> wte / cat -> generate_beam_batch), its
chunking, that `submit` does not make the host wait for the device, that it leaves the models as it found them, and the two
scripts built on it."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

TYPES = {"s": "a", "v": "b"}
VIOS = ["c", "d", "e", "f", "g", "h", "i", "j", "k"]
_CACHE = {}


def _setup(name, half):
    """(captioner, clip model, caption model, tokenizer, clip tokenize, caption geometry, label sets) on seeded state dicts"""
    key = (name, half)
    if key in _CACHE:
        return _CACHE[key]
    import _common as C
    import clip
    from clip.weights import MODELS, init_state_dict
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    from clip_caption.data import CAPTION_TYPES, VIOLATION_TYPES
    cname, gname = ("test-tiny", "test-tiny") if name == "tiny" else ("ViT-B/32", "ckiplab/gpt2-base-chinese")
    clip_model = clip.build_model(init_state_dict(MODELS[cname], 3)).cuda().eval()
    geo = GPT2_MODELS[gname]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval()
    if half:
        clip_model.half()
        model.half()
    else:
        clip_model.bfloat16()
        model.bfloat16()
    tok = C.ByteCaptionTokenizer(geo.vocab_size)
    ctok = C.get_tokenize(clip_model)
    labels = (TYPES, VIOS) if name == "tiny" else (CAPTION_TYPES, VIOLATION_TYPES)
    cap = Captioner(clip_model, model, tok, clip_tokenize=ctok, caption_types=labels[0], violation_types=labels[1],
                    prefix_length=geo.prefix_length, attribute_length=geo.attribute_length)
    _CACHE[key] = (cap, clip_model, model, tok, ctok, geo, labels)
    return _CACHE[key]


def _images(clip_model, n, seed=4):
    from clip.weights import synthetic_images
    return synthetic_images(n, clip_model.geo, seed).cuda()


def _compose(clip_model, model, tok, ctok, geo, labels, images):
    """the reference's predict() (test.py:516-546) per image from the public pieces: (labels, attribute ids [N, A], embeds)"""
    from clip.data import ZeroShotClassifier
    types, vios = labels
    cap_cls = ZeroShotClassifier(clip_model, ctok(list(types.keys())), list(types.values()))
    vio_cls = ZeroShotClassifier(clip_model, ctok(list(vios)), list(vios))
    out, ids, embeds = [], [], []
    with torch.no_grad():
        for i in range(images.shape[0]):
            f = clip_model.encode_image(images[i:i + 1])
            _, _, c = cap_cls(image_features=f)
            _, _, v = vio_cls(image_features=f)
            attribute = f"{c[0]} {v[0]} "
            enc = torch.tensor(tok.encode(attribute), dtype=torch.int64)
            enc = torch.cat((enc, torch.zeros(geo.attribute_length - enc.shape[0], dtype=torch.int64))).cuda()
            pre = model.clip_project(f.float()).reshape(1, geo.prefix_length, -1)
            embeds.append(torch.cat((pre, model.gpt.transformer.wte(enc).unsqueeze(0)), dim=1))
            out.append((c[0], v[0], attribute))
            ids.append(enc.cpu())
    return out, torch.stack(ids), torch.cat(embeds)


def _same_best_beam(got, ref):
    """the criterion of tests/test_decode_batch_gpu.py:124-151: equal lengths, equal tokens for the best beam"""
    (t1, l1, s1), (t0, l0, s0) = got, ref
    assert torch.equal(l1.cpu(), l0.cpu()), (l1, l0)
    b1, b0 = int(s1.argsort(descending=True)[0]), int(s0.argsort(descending=True)[0])
    assert torch.equal(t1[b1].cpu(), t0[b0].cpu()), (t1, t0)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("greedy", [False, True])
def test_describe_equals_the_composition_of_public_pieces(half, greedy):
    from clip_caption import generate2_batch, generate_beam_batch
    cap, clip_model, model, tok, ctok, geo, labels = _setup("tiny", half)
    images = _images(clip_model, 6)
    kw = dict(entry_length=14, temperature=0.5, stop_token=102)
    ref_labels, ref_ids, embeds = _compose(clip_model, model, tok, ctok, geo, labels, images)
    assert model.beam_batch_native_ok(1 if greedy else 3, embeds.shape[1], 14)
    records, extra = cap.describe(images, beam_size=3, greedy=greedy, return_tokens=True, **kw)
    if greedy:
        texts, rows = generate2_batch(model, tok, embeds, return_tokens=True, **kw)
    else:
        texts, per = generate_beam_batch(model, tok, embeds, beam_size=3, return_tokens=True, **kw)
    assert torch.equal(extra["ids"].long(), ref_ids)
    for i, rec in enumerate(records):
        assert (rec["caption_type"], rec["violation_type"], rec["attribute"]) == ref_labels[i]
        assert abs(sum(rec["type_probs"]) - 1) < 1e-5 and abs(sum(rec["violation_probs"]) - 1) < 1e-5
        if greedy:
            assert torch.equal(extra["tokens"][i].cpu(), rows[i].cpu())
            assert rec["prediction"] == texts[i]
        else:
            _same_best_beam(extra["tokens"][i], per[i])
            assert rec["prediction"] == texts[i][0]


def test_describe_at_vit_b32_gpt2_small_geometry_with_the_real_labels():
    from clip_caption import generate_beam_batch
    cap, clip_model, model, tok, ctok, geo, labels = _setup("b32", True)
    assert cap.table.shape == (18, 20) and cap.prompts.shape == (11, 512)
    images = _images(clip_model, 3)
    kw = dict(entry_length=10, temperature=0.5, stop_token=102)
    ref_labels, ref_ids, embeds = _compose(clip_model, model, tok, ctok, geo, labels, images)
    records, extra = cap.describe(images, beam_size=3, return_tokens=True, **kw)
    texts, per = generate_beam_batch(model, tok, embeds, beam_size=3, return_tokens=True, **kw)
    assert torch.equal(extra["ids"].long(), ref_ids)
    for i, rec in enumerate(records):
        assert (rec["caption_type"], rec["violation_type"], rec["attribute"]) == ref_labels[i]
        assert rec["caption_type"] in ("現況", "缺失")                               # the values, not application.py's keys
        _same_best_beam(extra["tokens"][i], per[i])
        assert rec["prediction"] == texts[i][0]


def test_chunked_and_single_image_calls_agree():
    cap, clip_model, model, tok, ctok, geo, labels = _setup("tiny", True)
    per = 64 // 3
    images = _images(clip_model, per + 3, seed=8)
    kw = dict(beam_size=3, entry_length=10, temperature=0.5, stop_token=102)
    singles = [cap.describe(images[i:i + 1], return_tokens=True, **kw) for i in range(per + 3)]
    for n in (1, per, per + 3):
        records, extra = cap.describe(images[:n], return_tokens=True, **kw)
        assert len(records) == n
        for i in range(n):
            (r1,), e1 = singles[i]
            assert records[i] == r1
            assert torch.equal(extra["ids"][i], e1["ids"][0]) and torch.equal(extra["index"][i], e1["index"][0])
            for a, b in zip(extra["tokens"][i], e1["tokens"][0]):
                assert torch.equal(a, b), (n, i, a, b)


@pytest.mark.parametrize("greedy", [False, True])
def test_submit_does_not_wait_for_the_device(greedy):
    cap, clip_model, model, tok, ctok, geo, labels = _setup("tiny", True)
    images = _images(clip_model, 5, seed=9)
    kw = dict(beam_size=3, entry_length=10, temperature=0.5, stop_token=102, greedy=greedy)
    want = cap.describe(images, **kw)                      # (first call: arenas, weight shadows, GEMM choices are set up here)
    assert model.beam_batch_native_ok(1 if greedy else 3, geo.prefix_length + geo.attribute_length, 10)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                  # (the mode is live: a read-back raises)
            torch.ones(1, device="cuda").item()
        handle = cap.submit(images, **kw)                  # raises on .item() / .tolist() / .cpu() / bool(device tensor) / blocking copies
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert handle.result() == want
    src = open(os.path.join(ROOT, "construction-clip_amd", "clip_caption", "pipeline.py")).read()
    assert not re.search(r"synchronize", src)              # (the debug mode does not see a raw stream wait)


def test_fallback_when_the_batched_kernel_does_not_apply(monkeypatch):
    cap, clip_model, model, tok, ctok, geo, labels = _setup("tiny", True)
    images = _images(clip_model, 3, seed=10)
    kw = dict(beam_size=3, entry_length=10, temperature=0.5, stop_token=102)
    want, extra = cap.describe(images, return_tokens=True, **kw)
    monkeypatch.setenv("CCLIP_BEAM_NATIVE", "0")
    assert not model.beam_batch_native_ok(3, geo.prefix_length + geo.attribute_length, 10)
    got, extra2 = cap.describe(images, return_tokens=True, **kw)
    assert torch.equal(extra["ids"], extra2["ids"])
    for a, b in zip(got, want):
        assert {k: a[k] for k in ("caption_type", "violation_type", "attribute")} == {k: b[k] for k in ("caption_type", "violation_type", "attribute")}
    assert all(isinstance(r["prediction"], str) for r in got)


def test_describe_leaves_the_models_as_it_found_them():
    cap, clip_model, model, tok, ctok, geo, labels = _setup("tiny", True)
    images = _images(clip_model, 4, seed=11)
    cap.describe(images, entry_length=6)                   # runtime built
    try:
        clip_model.train()
        model.train()
        marks = []
        for m in (clip_model, model):
            m.arena.gflat.fill_(0.25)
            p = next(q for q in m.parameters() if q.requires_grad)
            p.grad = torch.full_like(p, 2.0)
            marks.append((p, p.grad))
        grads_before = [{n: (None if q.grad is None else q.grad.clone()) for n, q in m.named_parameters()} for m in (clip_model, model)]
        cap.describe(images, entry_length=6)
        cap.describe(images, entry_length=6, greedy=True)
        assert clip_model.training and model.training
        for m, before in zip((clip_model, model), grads_before):
            assert torch.equal(m.arena.gflat, torch.full_like(m.arena.gflat, 0.25))
            for n, q in m.named_parameters():
                assert (q.grad is None) == (before[n] is None), n
                if q.grad is not None:
                    assert torch.equal(q.grad, before[n]), n
        for p, g in marks:
            assert p.grad is g
    finally:
        for m in (clip_model, model):
            m.eval()
            m.arena.gflat.zero_()
            for q in m.parameters():
                q.grad = None


def test_describe_images_and_extract_embeddings_scripts(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "describe_images.py"), "--synthetic", "--n_images", "7", "--bs", "4",
                        "--entry_length", "10", "--out_dir", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = json.loads((out / "output_ct.json").read_text())["caption"]
    assert len(recs) == 7
    for rec in recs:
        assert set(rec) == {"caption_type", "violation_type", "prediction", "caption", "file_name"}
        assert rec["caption_type"] in ("a", "b") and rec["violation_type"] in VIOS and rec["file_name"].startswith("images/")
    pkl = tmp_path / "emb" / "embedding.pkl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "extract_embeddings.py"), "--synthetic", "--n_images", "11", "--bs", "4",
                        "--attribute_length", "4", "--out", str(pkl)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    import _common as C
    from clip_caption.data import ClipCocoDataset, load_embeddings
    data = load_embeddings(str(pkl))
    assert data["clip_embedding"].shape == (11, 64) and len(data["captions"]) == 11
    for i, a in enumerate(data["captions"]):
        assert a["clip_embedding"] == i and re.fullmatch(r"[ab] [c-k] ", a["attribute"]), a
    ds = ClipCocoDataset(str(pkl), 4, 4, tokenizer=C.ByteCaptionTokenizer(300), write_tokens_cache=False)
    tokens, mask, prefix, attribute = ds[3]
    assert len(ds) == 11 and prefix.shape == (64,) and attribute.shape == (4,) and int(attribute[0]) in (1 + ord("a"), 1 + ord("b"))
