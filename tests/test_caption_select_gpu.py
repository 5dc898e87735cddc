"""cclip_caption_select on the MI355X (csrc/caption_select.hip) against its float64 restatement (tests/caption_select_ref.py)
on the same fp32 inputs.

Tolerance, derived (caption_select_ref.cos_bound / bounds): a lane adds E / 256 float4 products one after the other and six
butterfly levels follow, so each of the dot and the two squared norms errs by at most (E / 64 + 6) 2^-24 of sum |a_i b_i| <=
|a| |b|; with the square roots, their product and the division |cos - exact| <= 4 (E / 64 + 8) 2^-24.  clip_score scales that
by w, ref_score and score carry it through their formulas.  `order` must equal the float64 order for every pair of candidates
whose float64 scores differ by more than twice the bound; the seeds below leave NO pair inside it (asserted), apart from the
deliberately duplicated rows, which must come lower index first.

Shapes: E = 4 (one float4, 63 idle lanes), 252 / 256 / 260 (around 64 lanes x one float4), 512, 1024 (the limit); K = 1, 3, 4, 5
(the four-wave trip and its remainder), 64 (the limit); N = 1, 3."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caption_select_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ES, KS, NS = (4, 252, 256, 260, 512, 1024), (1, 3, 4, 5, 64), (1, 3)
W, LMW = 2.5, 0.05
# the seed of a shape is the first of 1, 2, .. for which no pair of candidates has float64 scores within twice the bound
# (found with the reference alone, on the CPU); test_seeds_leave_no_pair_inside_the_bound re-derives the property
SEEDS = {(252, 64, 3): 2}


def _inputs(E, K, N, seed=None, pad=4):
    """seeded fp32 (img [N, E], txt [N K, E], lm [N K], ref [Rtot, E], ref_off) on the host; references 0 / 1 / 5 per image"""
    g = torch.Generator().manual_seed(SEEDS.get((E, K, N), 1) if seed is None else seed)
    img = torch.randn(N, E, generator=g)
    txt = torch.randn(N * K, E, generator=g) + torch.rand(N * K, 1, generator=g) * img.repeat_interleave(K, 0)
    lm = -3.0 * torch.rand(N * K, generator=g)
    counts = [5, 0, 1][:N]
    off = [0] + [int(v) for v in np.cumsum(counts)]
    ref = torch.randn(off[-1], E, generator=g) + 0.5 * txt[:1]
    return img, txt, lm, ref, off


def _strided(t, pad):
    """the rows of t in a cuda buffer whose row stride is pad floats more than its width"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def _host(outs):
    return tuple(None if o is None else o.cpu().numpy() for o in outs)


def _launch(img, txt, K, lm=None, ref=None, off=None, w=W, lm_weight=0.0, pad=4):
    from cclip_hip import ops
    return ops.caption_select(_strided(img, pad), _strided(txt, pad), K, lm_mean=None if lm is None else lm.cuda(),
                              ref=None if ref is None else _strided(ref, pad), ref_off=off, w=w, lm_weight=lm_weight)


def _no_close_pairs(ref, E, lm, lm_weight):
    return len(R.close_pairs(ref, R.bounds(ref, E, W, lm, lm_weight)[3])) == 0


@pytest.mark.parametrize("E", ES)
def test_against_float64_at_every_shape(E):
    worst = {}
    for K in KS:
        for N in NS:
            img, txt, lm, ref, off = _inputs(E, K, N)
            r = R.caption_select_ref(img.numpy(), txt.numpy(), K, lm_mean=lm.numpy(), ref=ref.numpy(), ref_off=off, w=W, lm_weight=LMW)
            assert _no_close_pairs(r, E, lm.numpy(), LMW), ("the seed leaves a pair inside the bound", E, K, N)
            got = _host(_launch(img, txt, K, lm, ref, off, lm_weight=LMW))
            ratios, loose = R.check_outputs(r, E, got, W, lm.numpy(), LMW)
            assert loose == 0
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"E = {E}: bound {R.cos_bound(E):.3e}; worst error / bound {worst}")


def test_seeds_leave_no_pair_inside_the_bound():
    """the excluded share of the order rule is 0: re-derived here for the largest K of every E, reference alone"""
    for E in ES:
        for N in NS:
            img, txt, lm, ref, off = _inputs(E, 64, N)
            r = R.caption_select_ref(img.numpy(), txt.numpy(), 64, lm_mean=lm.numpy(), lm_weight=LMW)
            assert _no_close_pairs(r, E, lm.numpy(), LMW), (E, N)


def test_without_lm_mean_and_without_references():
    img, txt, lm, ref, off = _inputs(260, 5, 3)
    r = R.caption_select_ref(img.numpy(), txt.numpy(), 5, w=W)
    assert _no_close_pairs(r, 260, None, 0.0)
    outs = _launch(img, txt, 5)
    assert outs[2] is None
    _, loose = R.check_outputs(r, 260, _host(outs), W)
    assert loose == 0
    assert torch.equal(outs[0], outs[3])                                   # score is cos itself, bit for bit
    outs2 = _launch(img, txt, 5, lm, lm_weight=0.0)                        # a weight of 0 changes nothing
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2) if a is not None)
    outs3 = _launch(img, txt, 5, pad=0)                                    # contiguous rows: the same bits as strided ones
    assert all(torch.equal(a, b) for a, b in zip(outs, outs3) if a is not None)


def test_lm_weight_flips_best_on_a_constructed_case():
    E = 64
    img = torch.zeros(1, E)
    img[0, 0] = 1.0
    txt = torch.zeros(3, E)
    txt[0, 0], txt[0, 1] = 1.0, 0.1                                        # cos 0.995: CLIP's favourite
    txt[1, 0], txt[1, 1] = 1.0, 1.0                                        # cos 0.707: the language model's favourite
    txt[2, 1] = 1.0                                                        # cos 0
    lm = torch.tensor([-2.0, -0.5, -3.0])
    for lmw, want in ((0.0, [0, 1, 2]), (0.1, [0, 1, 2]), (0.5, [1, 0, 2])):
        r = R.caption_select_ref(img.numpy(), txt.numpy(), 3, lm_mean=lm.numpy(), lm_weight=lmw)
        assert list(r.order[0]) == want
        got = _host(_launch(img, txt, 3, lm, lm_weight=lmw))
        R.check_outputs(r, E, got, W, lm.numpy(), lmw)
        assert list(got[4][0]) == want and got[5][0] == want[0]


def test_reference_identical_to_a_candidate_and_mixed_counts():
    E, K, N = 252, 4, 3
    img, txt, lm, ref, off = _inputs(E, K, N)
    ref = ref.clone()
    ref[2] = txt[1]                                                        # image 0, candidate 1: rmax = 1
    ref[5] = 3.0 * txt[2 * K + 3]                                          # image 2's only reference = candidate 3, rescaled
    r = R.caption_select_ref(img.numpy(), txt.numpy(), K, ref=ref.numpy(), ref_off=off, w=W)
    assert abs(r.rmax[0, 1] - 1) < 1e-12 and abs(r.rmax[2, 3] - 1) < 1e-12 and (r.rmax[1] == 0).all() and off == [0, 5, 5, 6]
    got = _host(_launch(img, txt, K, None, ref, off))
    R.check_outputs(r, E, got, W)
    b = R.cos_bound(E)
    a = got[1][0, 1]
    assert abs(got[2][0, 1] - 2 * a / (a + 1)) <= 4 * b + 1e-6             # harmonic mean of (clip_score, 1)
    assert (got[2][1] == 0).all()                                          # no references: exactly 0
    # no reference at all in the call
    got0 = _host(_launch(img, txt, K, None, torch.zeros(0, E), [0, 0, 0, 0]))
    assert (got0[2] == 0).all() and np.array_equal(got0[0], got[0])


def test_zero_rows_give_cos_exactly_zero():
    E, K, N = 256, 5, 3
    img, txt, lm, ref, off = _inputs(E, K, N)
    img, txt, ref = img.clone(), txt.clone(), ref.clone()
    img[1] = 0                                                             # an all-zero image row
    txt[2] = 0                                                             # an all-zero text row (image 0, candidate 2)
    ref[0] = 0                                                             # and an all-zero reference
    r = R.caption_select_ref(img.numpy(), txt.numpy(), K, lm_mean=lm.numpy(), ref=ref.numpy(), ref_off=off, w=W, lm_weight=LMW)
    got = _host(_launch(img, txt, K, lm, ref, off, lm_weight=LMW))
    assert (got[0][1] == 0).all() and got[0][0, 2] == 0 and (got[1][1] == 0).all() and got[2][0, 2] == 0
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    R.check_outputs(r, E, got, W, lm.numpy(), LMW)
    # all of image 1's scores are lm terms only; with no lm_mean they tie at 0 and come in index order
    got = _host(_launch(img, txt, K))
    assert list(got[4][1]) == list(range(K)) and got[5][1] == 0


def test_duplicated_candidates_tie_lower_index_first():
    E, K, N = 512, 5, 3
    img, txt, lm, ref, off = _inputs(E, K, N)
    txt, lm = txt.clone(), lm.clone()
    txt[K + 4] = txt[K + 1]                                                # image 1: candidates 1 and 4 are one row
    lm[K + 4] = lm[K + 1]
    txt[2 * K + 0] = txt[2 * K + 3]                                        # image 2: 0 and 3, and 2 as well
    txt[2 * K + 2] = txt[2 * K + 3]
    lm[2 * K + 0] = lm[2 * K + 2] = lm[2 * K + 3]
    ties = [(1, 1, 4), (2, 0, 2), (2, 0, 3), (2, 2, 3)]
    r = R.caption_select_ref(img.numpy(), txt.numpy(), K, lm_mean=lm.numpy(), w=W, lm_weight=LMW)
    close = R.close_pairs(r, R.bounds(r, E, W, lm.numpy(), LMW)[3])
    assert sorted(close) == ties                                           # nothing but the deliberate duplicates
    got = _host(_launch(img, txt, K, lm, lm_weight=LMW))
    R.check_outputs(r, E, got, W, lm.numpy(), LMW, ties=ties)


def test_two_launches_are_bitwise_equal_and_a_row_does_not_depend_on_n():
    E, K = 1024, 5
    img, txt, lm, ref, off = _inputs(E, K, 3)
    a = _launch(img, txt, K, lm, ref, off, lm_weight=LMW)
    b = _launch(img, txt, K, lm, ref, off, lm_weight=LMW)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # image 1 of 3 (no references) alone, and in the middle of 7 images
    solo = _launch(img[1:2], txt[K:2 * K], K, lm[K:2 * K], ref[:0], [0, 0], lm_weight=LMW)
    g = torch.Generator().manual_seed(77)
    big_i = torch.randn(7, E, generator=g)
    big_t = torch.randn(7 * K, E, generator=g)
    big_l = -torch.rand(7 * K, generator=g)
    big_i[4], big_t[4 * K:5 * K], big_l[4 * K:5 * K] = img[1], txt[K:2 * K], lm[K:2 * K]
    big_r = torch.randn(6, E, generator=g)
    wide = _launch(big_i, big_t, K, big_l, big_r, [0, 1, 2, 3, 3, 3, 4, 6], lm_weight=LMW)
    for s, x, y in zip(solo, a, wide):
        assert torch.equal(s[0], x[1]) and torch.equal(s[0], y[4])


def test_a_nan_row_still_yields_a_permutation():
    E, K, N = 260, 64, 3
    img, txt, lm, ref, off = _inputs(E, K, N)
    txt, img = txt.clone(), img.clone()
    txt[7, 3] = float("nan")
    txt[K + 9] = float("inf")
    img[2, 0] = float("nan")                                               # every score of image 2 is NaN
    got = _host(_launch(img, txt, K, lm, ref, off, lm_weight=LMW))
    order, best = got[4], got[5]
    assert (np.sort(order, axis=1) == np.arange(K)[None]).all() and (best == order[:, 0]).all()
    assert np.isnan(got[0][0, 7]) and np.isnan(got[0][2]).all()
    r = R.caption_select_ref(img[1:2].numpy(), txt[K:2 * K].numpy(), K)     # the finite candidates keep their values
    fin = np.arange(K) != 9
    assert (np.abs(got[0][1][fin] - r.cos[0][fin]) <= R.cos_bound(E)).all()


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    from cclip_hip._lib import lib
    c_int, c_long, c_float, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    N, K, E, ld = 2, 3, 8, 12
    big = torch.randn(N * 70 * 1040 + 64, device="cuda")                   # room for every shape tried below
    off = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    outs = [torch.full((N * 70,), -7.0, device="cuda") for _ in range(4)] + [torch.full((N * 70,), -7, dtype=torch.int32, device="cuda")
                                                                             for _ in range(2)]
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(img=big.data_ptr(), ldi=ld, txt=big.data_ptr(), ldt=ld, N=N, K=K, E=E, lm=0, ref=0, ldr=ld, off=0,
                 cos=outs[0].data_ptr(), cs=outs[1].data_ptr(), rs=outs[2].data_ptr(), sc=outs[3].data_ptr(),
                 order=outs[4].data_ptr(), best=outs[5].data_ptr())
        a.update(kw)
        return lib.cclip_caption_select(vp(a["img"]), c_long(a["ldi"]), vp(a["txt"]), c_long(a["ldt"]), c_int(a["N"]), c_int(a["K"]),
                                        c_int(a["E"]), vp(a["lm"]), vp(a["ref"]), c_long(a["ldr"]), vp(a["off"]), c_float(2.5),
                                        c_float(0.0), vp(a["cos"]), vp(a["cs"]), vp(a["rs"]), vp(a["sc"]), vp(a["order"]),
                                        vp(a["best"]), stream)

    misaligned = big[1:].data_ptr()                                        # an offset view: 4 bytes past a 16-byte boundary
    assert misaligned % 16 == 4
    bad = [dict(K=65), dict(K=0), dict(E=6, ldi=8, ldt=8), dict(E=1028, ldi=1028, ldt=1028), dict(E=0), dict(N=0),
           dict(ldi=E - 4), dict(ldt=E - 4), dict(ldt=E + 2), dict(img=misaligned), dict(txt=misaligned), dict(img=0), dict(order=0),
           dict(ref=big.data_ptr()), dict(off=off.data_ptr()), dict(ref=misaligned, off=off.data_ptr()),
           dict(ref=big.data_ptr(), off=off.data_ptr(), ldr=E - 4), dict(ref=big.data_ptr(), off=off.data_ptr(), rs=0)]
    for kw in bad:
        assert call(**kw) == 1, kw                                         # CCLIP_ERR_ARG
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all()), "a refused call wrote to its outputs"
    assert call() == 0 and call(ref=big.data_ptr(), off=off.data_ptr()) == 0   # the same arguments, valid: launched
    torch.cuda.synchronize()
    assert bool((outs[0][:N * K] != -7).all()) and bool((outs[0][N * K:] == -7).all())


def test_python_layer_refuses_what_the_kernel_would():
    from cclip_hip import ops
    buf = torch.zeros(4 * 16 + 8, device="cuda")
    img = torch.zeros(1, 16, device="cuda")
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.caption_select(img, buf[1:65].view(4, 16), 4)
    with pytest.raises(ValueError, match="16-byte aligned"):               # a row stride that is no multiple of 4 floats
        ops.caption_select(img, buf[:72].view(4, 18)[:, :16], 4)
    with pytest.raises(TypeError, match="host tensor"):
        ops.caption_select(img, buf[:64].view(4, 16), 4, ref=img, ref_off=torch.tensor([0, 1], device="cuda"))


def test_clip_score_features_is_the_kernel():
    import clip
    from cclip_hip import ops
    img, txt, lm, ref, off = _inputs(512, 4, 3)
    res, score = clip.clip_score_features(img.cuda().half(), txt.cuda().half(), reference_features=ref.cuda().half(), reference_offsets=off,
                                          lm_mean=lm.cuda(), lm_weight=LMW, return_score=True)
    assert isinstance(res, clip.ClipScores)
    want = ops.caption_select(img.cuda().half().float(), txt.cuda().half().float(), 4, lm_mean=lm.cuda(), ref=ref.cuda().half().float(),
                              ref_off=off, lm_weight=LMW)
    for a, b in zip((res.cos, res.clip_score, res.ref_clip_score, score, res.order, res.best), want):
        assert torch.equal(a, b)
    plain = clip.clip_score_features(img.cuda(), txt.cuda())
    assert plain.ref_clip_score is None and plain.cos.shape == (3, 4) and plain.order.dtype == torch.int32
