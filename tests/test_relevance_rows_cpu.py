"""Relevance rows without a GPU: the public surface of clip.interpret_rows / clip.text_row_scores, the C ABI declaration of
the row kernel, and the row recurrence itself in float64 - r <- r + r C_l, top-down from the one-hot of the pooled position,
is the class-token row (image tower) / the EOT row (text tower) of the reference's rollout, which test_relevance_cpu.py pins.
tests/test_relevance_rows_gpu.py measures the HIP path against these rows."""
import inspect
import os
import re

import pytest
import torch

from test_relevance_cpu import _fixture, cams, forward64, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row_rollout(cs, start_layer, pos):
    """r <- r + r C_l for the blocks l >= start (start -1: the last block), from the last block down; r starts as e_pos[b]."""
    L = len(cs)
    s = L - 1 if start_layer == -1 else start_layer
    n, t = cs[0].shape[0], cs[0].shape[-1]
    r = torch.zeros(n, t, dtype=cs[0].dtype)
    r[torch.arange(n), pos] = 1
    for i in range(L - 1, -1, -1):
        if i >= s:
            r = r + torch.bmm(r[:, None, :], cs[i])[:, 0]
    return r


def test_rows_are_exported():
    import clip
    from clip.explain import interpret_rows, text_row_scores
    assert clip.interpret_rows is interpret_rows and clip.text_row_scores is text_row_scores
    assert list(inspect.signature(interpret_rows).parameters) == ["image", "texts", "model", "device", "start_layer",
                                                                  "start_layer_text"]
    assert list(inspect.signature(text_row_scores).parameters) == ["text_relevance_row", "tokens"]


def test_header_declares_the_row_kernel_and_its_twin():
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("cclip_attention_relevance_row", "cclip_attention_relevance_row_f16"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared"
        args = " ".join(m.group(1).split())
        assert args == ("const cclip_attn_desc* d, float grad_scale, const float* r_in, float* r_out, hipStream_t stream"), args


@pytest.mark.parametrize("start", [-1, 0, 1])
@pytest.mark.parametrize("name", ["test-small", "test-long"])
def test_row_recurrence_is_the_rollouts_row(name, start):
    sd, img, txt = _fixture(name)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.enable_grad():
        logits, pi, pt = forward64(sd64, img, txt)
        logits.diagonal().sum().backward()
    n = img.shape[0]
    ci, ct = cams(pi), cams(pt)
    r_img = row_rollout(ci, start, torch.zeros(n, dtype=torch.long))
    assert (r_img - rollout(ci, start)[:, 0]).abs().max().item() < 1e-12
    eot = txt.long().argmax(dim=-1)
    r_txt = row_rollout(ct, start, eot)
    assert (r_txt - rollout(ct, start)[torch.arange(n), eot]).abs().max().item() < 1e-12
    assert r_img.abs().sum() > n and r_txt.abs().sum() > n          # (more than the one-hot: the maps are not empty)


def test_text_row_scores_are_text_token_scores_of_the_matrix():
    from clip import text_row_scores, text_token_scores
    g = torch.Generator().manual_seed(4)
    R = torch.rand(2, 16, 16, generator=g)
    tok = torch.zeros(2, 16, dtype=torch.int32)
    tok[0, :6] = torch.tensor([510, 7, 8, 9, 10, 511])
    tok[1, :3] = torch.tensor([510, 7, 511])
    eot = tok.long().argmax(dim=-1)
    rows = R[torch.arange(2), eot]
    got, ref = text_row_scores(rows, tok), text_token_scores(R, tok)
    assert isinstance(got, list) and len(got) == 2
    for b in range(2):
        assert torch.equal(got[b], ref[b])
        assert torch.equal(text_row_scores(rows[b], tok[b]), ref[b])
