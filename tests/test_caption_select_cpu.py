"""CPU: the float64 restatement of the caption-selection contract (tests/caption_select_ref.py) against torch's own cosine
similarity and stable argsort, its edge rules (zero norm, no references, the harmonic mean and its zero denominator, ties),
and the argument checks of the Python layer (cclip_hip.ops.caption_select, clip.clip_score_features, clip.clip_score), which
all fire before anything touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caption_select_ref as R  # noqa: E402


def _case(N, K, E, seed, Rn=None):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(N, E, generator=g)
    txt = torch.randn(N * K, E, generator=g) + 0.5 * img.repeat_interleave(K, 0)
    lm = -torch.rand(N * K, generator=g)
    ref, off = None, None
    if Rn is not None:
        off = [0] + list(np.cumsum(Rn))
        ref = torch.randn(int(off[-1]), E, generator=g)
    return img, txt, lm, ref, off


@pytest.mark.parametrize("N,K,E", [(1, 1, 4), (3, 5, 260), (2, 64, 512)])
def test_ref_equals_torch_cosine_and_stable_argsort(N, K, E):
    img, txt, lm, ref, off = _case(N, K, E, 11, Rn=[2, 0, 5][:N])
    r = R.caption_select_ref(img.numpy(), txt.numpy(), K, lm_mean=lm.numpy(), ref=ref.numpy(), ref_off=off, w=2.5, lm_weight=0.25)
    i64, t64 = img.double(), txt.double().view(N, K, E)
    cos = torch.nn.functional.cosine_similarity(i64[:, None, :], t64, dim=2, eps=0.0)
    assert np.allclose(r.cos, cos.numpy(), rtol=0, atol=1e-14)
    assert np.allclose(r.clip_score, 2.5 * cos.clamp(min=0).numpy(), rtol=0, atol=1e-14)
    score = cos + float(np.float32(0.25)) * lm.double().view(N, K)
    assert np.allclose(r.score, score.numpy(), rtol=0, atol=1e-14)
    assert np.array_equal(r.order, score.argsort(dim=1, descending=True, stable=True).numpy())
    assert np.array_equal(r.best, r.order[:, 0])
    for n in range(N):
        rows = ref.double()[off[n]:off[n + 1]]
        if rows.shape[0] == 0:
            assert (r.rmax[n] == 0).all() and (r.ref_score[n] == 0).all()                  # the empty-reference rule
            continue
        rc = torch.nn.functional.cosine_similarity(t64[n][:, None, :], rows[None], dim=2, eps=0.0).max(dim=1).values.clamp(min=0)
        assert np.allclose(r.rmax[n], rc.numpy(), rtol=0, atol=1e-14)
        a, m = r.clip_score[n], r.rmax[n]
        want = np.where(a + m == 0, 0.0, 2 * a * m / np.where(a + m == 0, 1, a + m))
        assert np.allclose(r.ref_score[n], want, rtol=0, atol=1e-14)


def test_zero_norm_rule():
    img, txt, *_ = _case(2, 3, 8, 5)
    img[1] = 0
    txt[1] = 0
    r = R.caption_select_ref(img.numpy(), txt.numpy(), 3)
    assert r.cos[0, 1] == 0 and (r.cos[1] == 0).all() and r.cos[0, 0] != 0
    assert np.isfinite(r.cos).all() and (r.clip_score[1] == 0).all()
    assert list(r.order[1]) == [0, 1, 2]                                                   # all tied at 0: index order


def test_harmonic_mean_rule_and_its_zero_denominator():
    e = np.eye(4, dtype=np.float32)
    img = e[:1]                                                            # image = e0
    txt = np.stack([e[0], e[1], -e[0], (e[0] + e[1])])                     # cos 1, 0, -1, 1/sqrt2
    ref = np.stack([e[1], e[2]])                                           # rmax 0, 1, 0, 1/sqrt2
    r = R.caption_select_ref(img, txt, 4, ref=ref, ref_off=[0, 2], w=2.0)
    s = 1 / np.sqrt(2)
    assert np.allclose(r.cos[0], [1, 0, -1, s]) and np.allclose(r.clip_score[0], [2, 0, 0, 2 * s])
    assert np.allclose(r.rmax[0], [0, 1, 0, s])
    # (2, 0) -> 0; (0, 1) -> 0; (0, 0): zero denominator -> 0; (2s, s) -> 2 * 2s * s / (3s) = 4s / 3
    assert np.allclose(r.ref_score[0], [0, 0, 0, 4 * s / 3]) and r.ref_score[0, 2] == 0
    assert list(r.order[0]) == [0, 3, 1, 2]
    assert R.caption_select_ref(img, txt, 4).ref_score is None


def test_tie_order_and_signed_zero():
    img, txt, *_ = _case(1, 6, 16, 9)
    txt[4] = txt[1]
    txt[5] = txt[1]
    r = R.caption_select_ref(img.numpy(), txt.numpy(), 6)
    place = {int(k): i for i, k in enumerate(r.order[0])}
    assert place[1] + 1 == place[4] and place[4] + 1 == place[5]
    assert list(R.order_ref(np.array([[-0.0, 0.0, -0.0, 1.0]]))[0]) == [3, 0, 1, 2]
    lm = np.zeros(6, dtype=np.float32)
    lm[int(r.order[0][-1])] = 100.0                                        # the language model's favourite wins with enough weight
    r2 = R.caption_select_ref(img.numpy(), txt.numpy(), 6, lm_mean=lm, lm_weight=1.0)
    assert r2.best[0] == r.order[0][-1] != r.best[0]


def test_bounds_follow_the_formulas():
    assert R.cos_bound(512) == 4 * 16 * 2.0 ** -24 and R.cos_bound(4) == 4 * (4 / 64 + 8) * 2.0 ** -24
    img, txt, lm, ref, off = _case(2, 4, 64, 3, Rn=[1, 2])
    r = R.caption_select_ref(img.numpy(), txt.numpy(), 4, lm_mean=lm.numpy(), ref=ref.numpy(), ref_off=off, lm_weight=0.5)
    b_cos, b_cs, b_rs, b_sc = R.bounds(r, 64, 2.5, lm.numpy(), 0.5)
    assert (b_cs >= 2.5 * b_cos).all() and (b_rs >= 2 * (b_cs + b_cos)).all() and (b_sc >= b_cos).all()
    assert b_rs.max() < 1e-4 and b_sc.max() < 1e-5
    ratios, loose = R.check_outputs(r, 64, (r.cos, r.clip_score, r.ref_score, r.score, r.order, r.best), 2.5, lm.numpy(), 0.5)
    assert loose == 0 and max(ratios.values()) == 0


# ---- the Python layer: every one of these raises before a device is needed --------------------------------------------------
def test_ops_argument_checks():
    from cclip_hip import ops
    assert ops.CAPTION_SELECT_MAX_K == 64 and ops.CAPTION_SELECT_MAX_E == 1024
    img, txt = torch.zeros(2, 8), torch.zeros(6, 8)
    with pytest.raises(ValueError, match=r"txt must be \[N \* K, E\]"):
        ops.caption_select(img, txt, 2)
    with pytest.raises(ValueError, match="txt must be"):
        ops.caption_select(img, torch.zeros(6, 12), 3)
    with pytest.raises(ValueError, match="float32"):
        ops.caption_select(img.double(), txt, 3)
    with pytest.raises(ValueError, match="inner stride 1"):
        ops.caption_select(img, torch.zeros(8, 6).t(), 3)
    with pytest.raises(ValueError, match="K must be"):
        ops.caption_select(img, txt, 0)
    with pytest.raises(ValueError, match="lm_mean"):
        ops.caption_select(img, txt, 3, lm_mean=torch.zeros(5))
    with pytest.raises(NotImplementedError, match="K = 65"):
        ops.caption_select(img, torch.zeros(130, 8), 65)
    with pytest.raises(NotImplementedError, match="E = 6"):
        ops.caption_select(torch.zeros(2, 6), torch.zeros(6, 6), 3)
    with pytest.raises(NotImplementedError, match="E = 1028"):
        ops.caption_select(torch.zeros(1, 1028), torch.zeros(1, 1028), 1)
    ref = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="both ref and ref_off"):
        ops.caption_select(img, txt, 3, ref=ref)
    with pytest.raises(ValueError, match="both ref and ref_off"):
        ops.caption_select(img, txt, 3, ref_off=[0, 1, 2])
    with pytest.raises(ValueError, match="columns"):
        ops.caption_select(img, txt, 3, ref=torch.zeros(4, 12), ref_off=[0, 2, 4])
    with pytest.raises(ValueError, match="never decrease"):
        ops.caption_select(img, txt, 3, ref=ref, ref_off=[0, 3, 2])
    with pytest.raises(ValueError, match="never decrease"):
        ops.caption_select(img, txt, 3, ref=ref, ref_off=torch.tensor([1, 2, 4]))
    with pytest.raises(ValueError, match="N \\+ 1 = 3 entries"):
        ops.caption_select(img, txt, 3, ref=ref, ref_off=[0, 4])
    with pytest.raises(ValueError, match="ends at 5"):
        ops.caption_select(img, txt, 3, ref=ref, ref_off=[0, 2, 5])
    with pytest.raises(TypeError, match="no CPU path"):                   # everything valid: only the device is missing
        ops.caption_select(img, txt, 3, ref=ref, ref_off=[0, 0, 4])


def test_clip_score_features_argument_checks():
    import clip
    with pytest.raises(ValueError, match="K rows per image"):
        clip.clip_score_features(torch.zeros(2, 8), torch.zeros(5, 8))
    with pytest.raises(ValueError, match="K rows per image"):
        clip.clip_score_features(torch.zeros(2, 8), torch.zeros(0, 8))
    with pytest.raises(ValueError, match="columns"):
        clip.clip_score_features(torch.zeros(2, 8), torch.zeros(4, 12))
    with pytest.raises(ValueError, match="2-D float"):
        clip.clip_score_features(torch.zeros(2, 8, 1), torch.zeros(4, 8))
    with pytest.raises(ValueError, match="both reference_features and reference_offsets"):
        clip.clip_score_features(torch.zeros(2, 8), torch.zeros(4, 8), reference_features=torch.zeros(1, 8))
    with pytest.raises(NotImplementedError, match="K = 65"):
        clip.clip_score_features(torch.zeros(1, 8), torch.zeros(65, 8))
    with pytest.raises(ValueError, match="never decrease"):
        clip.clip_score_features(torch.zeros(2, 8), torch.zeros(4, 8), reference_features=torch.zeros(3, 8), reference_offsets=[0, 2, 1])


class _NoTower:
    logit_scale = torch.zeros(())

    def encode_text(self, tokens):
        raise AssertionError("the token forms are checked before any tower runs")

    encode_image = encode_text


def test_clip_score_token_forms():
    import clip
    from clip.score import candidate_tokens, csr_offsets
    flat, K = candidate_tokens(torch.arange(3 * 77).view(3, 77), 3)
    assert K == 1 and flat.shape == (3, 77)
    t3 = torch.arange(3 * 5 * 77).view(3, 5, 77)
    flat, K = candidate_tokens(t3, 3)
    assert K == 5 and flat.shape == (15, 77) and torch.equal(flat[1 * 5 + 2], t3[1, 2])          # row n * K + k
    assert csr_offsets([2, 0, 5]) == [0, 2, 2, 7]
    m = _NoTower()
    with pytest.raises(ValueError, match=r"\[N, L\] or \[N, K, L\]"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer tensor"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(3, 77))
    with pytest.raises(ValueError, match="for 2 images, there are 3"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(2, 77, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="K = 65"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(3, 65, 77, dtype=torch.int32))
    with pytest.raises(ValueError, match="one tensor per image"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(3, 77, dtype=torch.int32), references=[torch.zeros(1, 77, dtype=torch.int32)])
    with pytest.raises(ValueError, match="token rows"):
        clip.clip_score(m, torch.zeros(3, 8), torch.zeros(3, 77, dtype=torch.int32), references=[torch.zeros(1, 76, dtype=torch.int32)] * 3)
    with pytest.raises(ValueError, match="images must be"):
        clip.clip_score(m, torch.zeros(3, 8, 8), torch.zeros(3, 77, dtype=torch.int32))


def test_captioner_best_of_argument_checks():
    import inspect
    from clip_caption import Captioner
    for fn in (Captioner.describe, Captioner.submit):
        p = inspect.signature(fn).parameters
        assert p["best_of"].default == 0 and p["lm_weight"].default == 0.0                  # the default is today's path
        assert p["generator"].default is None and p["uniforms"].default is None and p["score_model"].default is None
