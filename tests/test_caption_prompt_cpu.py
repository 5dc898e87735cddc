"""CPU side of the image-to-caption pipeline (clip_caption/pipeline.py, csrc/caption_prompt.hip):

  * `prompt_reference64` - the float64 statement of cclip_caption_prompt's formula.  It is the checker the GPU test imports
    (tests/test_caption_prompt_gpu.py); here it is pinned against ZeroShotClassifier's arithmetic (normalized_logits -> softmax ->
    argmax) run on the CPU restatement of the launchers (tests/cpu_ops_shim.py);
  * the attribute table (18 rows, caption type slowest, zero padded; an over-long string raises);
  * record assembly and chunking of Captioner.describe on CPU stub models, whose decoding goes through the host-side loops of
    generate_beam_batch / generate2_batch as in tests/test_generate_cpu.py;
  * the C ABI: cclip_caption_prompt is declared (one form, no _f16 twin) and exported.
"""
import math
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.dirname(os.path.abspath(__file__))]


# ------------------------------------------------------------------------------------------------------------------------
# the float64 checker
# ------------------------------------------------------------------------------------------------------------------------
def prompt_reference64(feat, prompts, head_start, log_scale, table=None):
    """float64: logit = exp(log_scale) * cos(feat_n, prompt_k); per head softmax / arg-max (lowest index on a tie); the table
    row of the combination (head 0 slowest).  Returns (probs [N, K], index [N, G], ids [N, A] or None, gap [N, G]) with gap the
    difference of a head's two largest logits (inf for a head of one prompt)."""
    f, p = feat.detach().double().cpu(), prompts.detach().double().cpu()
    f = f / f.norm(dim=1, keepdim=True)
    p = p / p.norm(dim=1, keepdim=True)
    logits = math.exp(float(log_scale)) * (f @ p.t())
    N, G = f.shape[0], len(head_start) - 1
    probs = torch.empty_like(logits)
    index = torch.empty(N, G, dtype=torch.int64)
    gap = torch.full((N, G), float("inf"), dtype=torch.float64)
    comb = torch.zeros(N, dtype=torch.int64)
    for g in range(G):
        k0, k1 = head_start[g], head_start[g + 1]
        lg = logits[:, k0:k1]
        probs[:, k0:k1] = lg.softmax(dim=1)
        index[:, g] = lg.argmax(dim=1)                      # torch.argmax: the first of equal maxima
        if k1 - k0 > 1:
            top = lg.topk(2, dim=1).values
            gap[:, g] = top[:, 0] - top[:, 1]
        comb = comb * (k1 - k0) + index[:, g]
    ids = None if table is None else table.cpu().long()[comb]
    return probs, index, ids, gap


class OpsShim:
    """stands in for cclip_hip.ops in clip_caption.pipeline on CPU tensors: caption_prompt restated from its contract"""
    BEAM_BATCH_MAX_ROWS = 64

    @staticmethod
    def caption_prompt(feat, prompts, head_start, logit_scale, table, probs, index, ids):
        p, i, t, _ = prompt_reference64(feat, prompts, list(head_start), float(logit_scale.reshape(-1)[0]), table)
        probs.copy_(p.float())
        index.copy_(i.to(torch.int32))
        ids.copy_(t.to(torch.int32))


class _WordTok:
    """caption-side tokenizer stub: one id per character (ord mod vocab), a [CLS]-like id in front"""

    def __init__(self, vocab=300, cls=7):
        self.vocab, self.cls = vocab, cls

    def encode(self, s):
        return [self.cls] + [1 + ord(c) % (self.vocab - 1) for c in s]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


# ------------------------------------------------------------------------------------------------------------------------
# 1. attribute table
# ------------------------------------------------------------------------------------------------------------------------
def test_attribute_table_rows_order_and_padding():
    from clip_caption import build_attribute_table
    from clip_caption.data import CAPTION_TYPES, VIOLATION_TYPES
    tok = _WordTok()
    types, vios = list(CAPTION_TYPES.values()), VIOLATION_TYPES
    table = build_attribute_table(tok, types, vios, 20)
    assert table.shape == (18, 20) and table.dtype == torch.int32
    for i, t in enumerate(types):
        for j, v in enumerate(vios):
            enc = tok.encode(f"{t} {v} ")
            row = table[i * len(vios) + j].tolist()
            assert row[:len(enc)] == enc and all(x == 0 for x in row[len(enc):]), (i, j, row)
    longest = max(len(tok.encode(f"{t} {v} ")) for t in types for v in vios)
    assert build_attribute_table(tok, types, vios, longest).shape == (18, longest)      # an exact fit is not over-long


def test_over_long_attribute_raises_naming_the_string():
    from clip_caption import build_attribute_table
    with pytest.raises(ValueError, match=re.escape(repr("status a-very-long-violation-name "))):
        build_attribute_table(_WordTok(), ["status"], ["fall", "a-very-long-violation-name"], 16)


# ------------------------------------------------------------------------------------------------------------------------
# 2. the formula against ZeroShotClassifier's arithmetic
# ------------------------------------------------------------------------------------------------------------------------
class _FixedTextModel:
    def __init__(self, text_features, log_scale):
        self.text_features, self.logit_scale = text_features, torch.tensor(log_scale)

    def encode_text(self, tokens):
        return self.text_features[tokens.view(-1).long()]


@pytest.mark.parametrize("log_scale", [math.log(100.0), math.log(1 / 0.07)])
def test_reference64_equals_zero_shot_classifier_arithmetic(monkeypatch, log_scale):
    import clip.model as cm
    import cpu_ops_shim
    from clip.data import ZeroShotClassifier
    monkeypatch.setattr(cm, "ops", cpu_ops_shim)
    g = torch.Generator().manual_seed(567)
    E, heads = 512, (2, 9)
    feat = torch.randn(64, E, generator=g)
    prompts = [torch.randn(k, E, generator=g) for k in heads]
    allp = torch.cat(prompts)
    head_start = [0, 2, 11]
    probs, index, _, gap = prompt_reference64(feat, allp, head_start, log_scale)
    for h, (k0, k1) in enumerate(zip(head_start[:-1], head_start[1:])):
        cls = ZeroShotClassifier(_FixedTextModel(allp, log_scale), torch.arange(k0, k1), [str(i) for i in range(k1 - k0)])
        sim, idx, labels = cls(image_features=feat)
        assert (sim.double() - probs[:, k0:k1]).abs().max() < 1e-5          # fp32 arithmetic against float64
        assert gap[:, h].min() > 1e-3 and torch.equal(idx, index[:, h])
        assert labels == [str(int(i)) for i in index[:, h]]


def test_reference64_ties_take_the_lowest_index_and_table_rows():
    g = torch.Generator().manual_seed(1)
    feat = torch.randn(20, 32, generator=g)
    p = torch.randn(9, 32, generator=g)
    head_start = [0, 3, 7, 9]
    winner = prompt_reference64(feat, p, head_start, 2.0)[1]
    table = torch.arange(3 * 4 * 2 * 5, dtype=torch.int32).view(24, 5)
    p2 = p.clone()
    p2[6] = p2[4]                                           # rows 1 and 3 of head 1 are the same prompt
    probs, index, ids, gap = prompt_reference64(feat, p2, head_start, 2.0, table)
    assert (index[:, 1] != 3).all()                         # row 3 can only tie with row 1, which comes first
    assert torch.equal(index[:, 0], winner[:, 0]) and torch.equal(index[:, 2], winner[:, 2])
    comb = (index[:, 0] * 4 + index[:, 1]) * 2 + index[:, 2]
    assert torch.equal(ids, table.long()[comb])
    for k0, k1 in zip(head_start[:-1], head_start[1:]):
        assert torch.allclose(probs[:, k0:k1].sum(1), torch.ones(20, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------------
# 3. Captioner on CPU stubs: record assembly, chunking, the fallback decode
# ------------------------------------------------------------------------------------------------------------------------
class _StubClip:
    """encode_image = a fixed linear map of the pixels, encode_text = rows of a fixed table picked by the first token"""

    def __init__(self, E=64, R=8, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.w = torch.randn(3 * R * R, E, generator=g)
        self.text = torch.randn(64, E, generator=g)
        self.logit_scale = torch.tensor(math.log(100.0))
        self.visual = SimpleNamespace(input_resolution=R)

    def encode_image(self, image):
        return image.reshape(image.shape[0], -1) @ self.w

    def encode_text(self, tokens):
        return self.text[tokens[:, 0].long()]


def _clip_tokenize(texts):
    return torch.tensor([[sum(t.encode("utf-8")) % 64] for t in texts], dtype=torch.int32)


def _stub_caption_model():
    from clip_caption.weights import GPT2_MODELS, init_caption_state_dict
    from test_generate_cpu import _StubModel
    geo = GPT2_MODELS["test-tiny"]
    sd = init_caption_state_dict(geo, 31)
    model = _StubModel(sd, geo.n_head)
    model.prefix_length = geo.prefix_length
    model.clip_project = lambda prefix: model.CO.mlp_mapper(sd, prefix)
    return geo, model


TYPES = {"s": "a", "v": "b"}
VIOS = ["c", "d", "e", "f", "g", "h", "i", "j", "k"]


class _CharTok:
    def encode(self, s):
        return [1 + ord(c) % 299 for c in s]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def _captioner(monkeypatch, max_rows=64):
    import clip_caption.pipeline as pl
    shim = type("Shim", (OpsShim,), {"BEAM_BATCH_MAX_ROWS": max_rows})
    monkeypatch.setattr(pl, "ops", shim)
    geo, model = _stub_caption_model()
    clip_model = _StubClip(E=geo.prefix_size)
    cap = pl.Captioner(clip_model, model, _CharTok(), clip_tokenize=_clip_tokenize, caption_types=TYPES, violation_types=VIOS,
                       prefix_length=geo.prefix_length, attribute_length=geo.attribute_length)
    return geo, model, clip_model, cap


def _compose_one(geo, model, clip_model, image, greedy, **kw):
    """the reference's predict() for one image from the public pieces (test.py:516-549), all on the CPU stubs"""
    from clip_caption import generate2, generate_beam
    tok = _CharTok()
    f = clip_model.encode_image(image[None]).float()
    heads = [clip_model.encode_text(_clip_tokenize(list(TYPES.keys()))), clip_model.encode_text(_clip_tokenize(VIOS))]
    probs, index, _, _ = prompt_reference64(f, torch.cat(heads), [0, 2, 11], clip_model.logit_scale)
    t, v = list(TYPES.values())[int(index[0, 0])], VIOS[int(index[0, 1])]
    attribute = f"{t} {v} "
    enc = torch.tensor(tok.encode(attribute), dtype=torch.int64)
    enc = torch.cat((enc, torch.zeros(geo.attribute_length - enc.shape[0], dtype=torch.int64)))
    emb = torch.cat((model.clip_project(f).reshape(1, geo.prefix_length, -1), model.gpt.transformer.wte(enc)[None]), dim=1)
    if greedy:
        text = generate2(model, tok, embed=emb, **kw)
    else:
        text = generate_beam(model, tok, embed=emb, **kw)[0]
    return dict(caption_type=t, violation_type=v, attribute=attribute, prediction=text, probs=probs[0], ids=enc)


@pytest.mark.parametrize("greedy", [False, True])
def test_describe_records_and_chunking_on_cpu_stubs(monkeypatch, greedy):
    geo, model, clip_model, cap = _captioner(monkeypatch, max_rows=6)       # 6 rows: 2 captions of 3 beams per chunk
    assert cap.table.shape == (18, geo.attribute_length) and cap.head_start == (0, 2, 11)
    g = torch.Generator().manual_seed(9)
    images = torch.randn(5, 3, 8, 8, generator=g)
    kw = dict(entry_length=6, stop_token=7)
    dkw = dict(kw, beam_size=3) if not greedy else dict(kw, top_p=0.8)
    calls = []
    orig = cap.submit
    monkeypatch.setattr(cap, "submit", lambda im, **k: (calls.append(im.shape[0]), orig(im, **k))[1])
    records, extra = cap.describe(images, greedy=greedy, return_tokens=True, **dkw)
    assert calls == ([5] if greedy else [2, 2, 1])
    assert len(records) == 5 and extra["ids"].shape == (5, geo.attribute_length) and extra["index"].shape == (5, 2)
    assert len(extra["tokens"]) == 5
    for i, rec in enumerate(records):
        assert set(rec) == {"caption_type", "violation_type", "attribute", "prediction", "type_probs", "violation_probs"}
        ref = _compose_one(geo, model, clip_model, images[i], greedy, **dkw)
        for key in ("caption_type", "violation_type", "attribute", "prediction"):
            assert rec[key] == ref[key], (i, key, rec[key], ref[key])
        assert torch.equal(extra["ids"][i].long(), ref["ids"])
        assert len(rec["type_probs"]) == 2 and len(rec["violation_probs"]) == 9
        assert torch.allclose(torch.tensor(rec["type_probs"] + rec["violation_probs"], dtype=torch.float64), ref["probs"], atol=1e-6)
    assert cap.describe(images[:1], greedy=greedy, **dkw) == records[:1]


def test_describe_reports_values_not_keys_and_rejects_bad_input(monkeypatch):
    geo, model, clip_model, cap = _captioner(monkeypatch)
    assert cap.caption_labels == ["a", "b"] and cap.attributes[0] == "a c " and cap.attributes[17] == "b k "
    rec = cap.describe(torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(2)), entry_length=3)[0]
    assert rec["caption_type"] in ("a", "b") and rec["violation_type"] in VIOS
    with pytest.raises(ValueError):
        cap.describe(torch.randn(3, 8, 8))
    with pytest.raises(ValueError):
        cap.describe(torch.zeros(0, 3, 8, 8))
    # images that are not float tensors go through `preprocess`
    import clip_caption.pipeline as pl
    cap2 = pl.Captioner(clip_model, model, _CharTok(), clip_tokenize=_clip_tokenize, caption_types=TYPES, violation_types=VIOS,
                        prefix_length=geo.prefix_length, attribute_length=geo.attribute_length,
                        preprocess=lambda im: torch.as_tensor(im).permute(2, 0, 1).float() / 255.0)
    u8 = torch.randint(0, 255, (2, 8, 8, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    a = cap2.describe([u8[0].numpy(), u8[1].numpy()], entry_length=3)
    b = cap2.describe(u8.permute(0, 3, 1, 2).float() / 255.0, entry_length=3)
    assert a == b


def test_embed_returns_features_index_ids(monkeypatch):
    geo, model, clip_model, cap = _captioner(monkeypatch)
    images = torch.randn(7, 3, 8, 8, generator=torch.Generator().manual_seed(5))
    feat, index, ids = cap.embed(images, batch_size=3)
    assert torch.equal(feat, torch.cat([clip_model.encode_image(images[s:s + 3]) for s in (0, 3, 6)]).float())   # towers run per batch
    _, ref_index, ref_ids, _ = prompt_reference64(feat, cap.prompts, list(cap.head_start), clip_model.logit_scale, cap.table)
    assert torch.equal(index.long(), ref_index) and torch.equal(ids.long(), ref_ids)


# ------------------------------------------------------------------------------------------------------------------------
# 4. ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_caption_prompt_is_declared_once_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(re.findall(r"\bint\s+cclip_caption_prompt\s*\(", code)) == 1
    assert "cclip_caption_prompt_f16" not in code                    # fp32 only: one form
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+cclip_caption_prompt\s*\(", hdr, flags=re.S)
    assert m and "exp(" in m.group(1) and "arg-max" in m.group(1) and "table[" in m.group(1)     # the comment states the formula
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip import load_library, ops
    lib = load_library()
    assert hasattr(lib, "cclip_caption_prompt") and not hasattr(lib, "cclip_caption_prompt_f16")
    assert callable(ops.caption_prompt)
