"""Caption attention maps, the parts that need no GPU:

1. `gpt2_attentions64` - the float64 restatement of GPT-2's per-layer attention probabilities (the loop of
   oracle/caption_oracle.gpt2_forward, returning the softmax instead of the logits) that the GPU tests compare the kernels
   against - is itself pinned against transformers' eager GPT-2 with output_attentions=True (<= 1e-5 absolute, the level
   test_oracle_pinning.py holds fp32 against HF);
2. `caption_attention_map` against the reference's `attention_map` formula (CLIP_prefix_caption/test.py:342-349), restated;
3. the property the replay rests on: row S0-1+j of ONE causal forward over the finished sequence is the attention of the
   step-by-step forward on the sequence grown to that position;
4. the library exports the new entry points.
"""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

from clip_caption.weights import GPT2_MODELS, init_caption_state_dict, synthetic_caption_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpt2_attentions64(sd, inputs_embeds, attention_mask, n_head, p="model."):
    """Per layer softmax(q k^T / sqrt(dh) + causal + key padding) of GPT2LMHeadModel(inputs_embeds=..., attention_mask=...),
    all in float64: a list of n_layer tensors [B, n_head, S, S].  Masked keys get HF's additive finfo(float32).min, which
    leaves an exact 0 after the softmax."""
    f = lambda k: sd[k].double()
    x = inputs_embeds.double()
    b, s, d = x.shape
    dh = d // n_head
    x = x + f(p + "transformer.wpe.weight")[:s]
    causal = torch.full((s, s), float("-inf"), dtype=torch.float64).triu_(1)
    pad = None
    if attention_mask is not None:
        pad = (1.0 - attention_mask.double())[:, None, None, :] * torch.finfo(torch.float32).min
    n_layer = len({k.split(".")[3] for k in sd if k.startswith(p + "transformer.h.")})
    out = []
    for i in range(n_layer):
        q = f"{p}transformer.h.{i}."
        h = F.layer_norm(x, (d,), f(q + "ln_1.weight"), f(q + "ln_1.bias"), 1e-5)
        qkv = h @ f(q + "attn.c_attn.weight") + f(q + "attn.c_attn.bias")
        qq, kk, vv = (t.view(b, s, n_head, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
        sc = (qq @ kk.transpose(-1, -2)) / math.sqrt(dh) + causal
        if pad is not None:
            sc = sc + pad
        pr = torch.softmax(sc, dim=-1)
        out.append(pr)
        a = (pr @ vv).transpose(1, 2).reshape(b, s, d)
        x = x + a @ f(q + "attn.c_proj.weight") + f(q + "attn.c_proj.bias")
        h = F.layer_norm(x, (d,), f(q + "ln_2.weight"), f(q + "ln_2.bias"), 1e-5)
        h = h @ f(q + "mlp.c_fc.weight") + f(q + "mlp.c_fc.bias")
        h = 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))          # gelu_new
        x = x + h @ f(q + "mlp.c_proj.weight") + f(q + "mlp.c_proj.bias")
    return out


def _tiny_inputs(seed=5, b=3, lc=10):
    from oracle import caption_oracle as CO
    geo = GPT2_MODELS["test-tiny"]
    sd = init_caption_state_dict(geo, seed)
    tokens, mask, prefix, attribute = synthetic_caption_batch(b, geo, lc, seed + 2)
    with torch.no_grad():
        emb = torch.cat((CO.mlp_mapper(sd, prefix).view(-1, geo.prefix_length, geo.n_embd),
                         sd["model.transformer.wte.weight"][torch.cat((attribute, tokens), 1)]), 1)
    return geo, sd, emb, mask


@pytest.mark.parametrize("masked", [False, True])
def test_attentions64_match_hf_eager(masked):
    pytest.importorskip("transformers")
    from oracle import hf_crosscheck as H
    geo, sd, emb, mask = _tiny_inputs()
    mask = mask.clone()
    if masked:
        mask[1, -3:] = 0
        mask[2, 2] = 0                                   # a hole inside the sequence, not only right padding
    hf = H.build_hf_gpt2(sd, geo.n_head)
    with torch.no_grad():
        ref = hf(inputs_embeds=emb, attention_mask=mask if masked else None, output_attentions=True).attentions
        got = gpt2_attentions64(sd, emb, mask if masked else None, geo.n_head)
    assert len(ref) == len(got) == geo.n_layer
    for l, (r, g) in enumerate(zip(ref, got)):
        assert r.shape == g.shape == (emb.shape[0], geo.n_head, emb.shape[1], emb.shape[1])
        err = (g - r.double()).abs().max().item()
        assert err <= 1e-5, (l, err)
        assert torch.equal(g.triu(1), torch.zeros_like(g))                 # exact zeros above the diagonal
        if masked:
            assert g[1, :, :, -3:].abs().max() == 0 and g[2, :, 3:, 2].abs().max() == 0
        assert (g.sum(-1) - 1).abs().max() < 1e-12


def _reference_attention_map(attention_list):
    """test.py:342-349 without the plot: every row appended with 1 up to the last row's length"""
    import numpy as np
    rows = []
    for attention in attention_list:
        while len(attention) < len(attention_list[-1]):
            attention = np.append(attention, 1)
        rows.append(attention)
    return np.array(rows)


@pytest.mark.parametrize("head", [-1, None, 0])
def test_caption_attention_map_is_the_references(head):
    from clip_caption import caption_attention_map
    g = torch.Generator().manual_seed(3)
    H, n, S0 = 4, 6, 5
    att = torch.rand(H, n, S0 + n - 1, generator=g)
    att = att * (torch.arange(S0 + n - 1)[None, :] < (S0 + torch.arange(n))[:, None])      # zeros right of the causal frontier
    rows = att.mean(0) if head is None else att[head]
    want = _reference_attention_map([rows[j, :S0 + j].numpy() for j in range(n)])         # what the step loop collects
    got = caption_attention_map(att, head=head) if head != -1 else caption_attention_map(att)
    assert got.shape == (n, S0 + n - 1) and got.dtype == torch.float32
    assert torch.equal(got, torch.from_numpy(want).float())
    assert torch.equal(caption_attention_map(att, head=head, pad_value=0.0), rows)
    with pytest.raises(ValueError):
        caption_attention_map(att[0])


def test_replay_rows_equal_step_by_step_rows():
    """float64: the distribution the decode step at position S0-1+j forms (a forward over the sequence grown to that
    position, its last row - what the reference logs, test.py:381-383) is row S0-1+j of one forward over the whole
    sequence.  Keys right of a query are masked, so what is appended later cannot reach an earlier row."""
    geo, sd, emb, _ = _tiny_inputs(seed=11, b=1, lc=9)
    S0 = geo.prefix_length + geo.attribute_length
    S = emb.shape[1]
    n = S - S0 + 1                                        # generated tokens: the last one is never fed
    with torch.no_grad():
        full = gpt2_attentions64(sd, emb, None, geo.n_head)
        for j in range(n):
            t = S0 - 1 + j
            step = gpt2_attentions64(sd, emb[:, :t + 1], None, geo.n_head)
            for l in range(geo.n_layer):
                assert (step[l][0, :, -1, :] - full[l][0, :, t, :t + 1]).abs().max() < 1e-13
                assert not full[l][0, :, t, t + 1:].any()
        # right padding (the batched replay): rows below a sequence's length do not see it
        padded = torch.cat((emb, torch.randn(1, 5, emb.shape[2], generator=torch.Generator().manual_seed(1))), dim=1)
        wide = gpt2_attentions64(sd, padded, None, geo.n_head)
        for l in range(geo.n_layer):
            assert (wide[l][0, :, :S, :S] - full[l]).abs().max() < 1e-13


def test_library_exports_attention_probs():
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip._lib import LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cclip_attention_probs", "cclip_attention_probs_f16"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    assert "int cclip_attention_probs(" in hdr and "int cclip_attention_probs_f16(" in hdr
    assert "#define CCLIP_ABI_VERSION 3" in hdr


def test_generate_signatures_carry_the_new_keywords():
    import inspect
    import clip_caption as cc
    for fn in (cc.generate_beam, cc.generate2, cc.generate_beam_batch, cc.generate2_batch):
        sig = inspect.signature(fn)
        assert sig.parameters["return_attention"].default is False
        assert sig.parameters["attention_layer"].default == -1
