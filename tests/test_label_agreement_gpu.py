"""GPU: the label-agreement counts (csrc/label_agreement.hip, ops.label_agreement, clip.evaluate_labels, .evaluate) on the MI355X
against the numpy reference of tests/label_agreement_ref.py.  Every output is an integer sum, so every comparison of counts is
for exact equality; the scores are float64 functions of the counts and compared for equality too.  The native call always runs
on guarded int64 buffers pre-filled with junk (accumulate == 0 must set them), the guards are checked, and every case runs twice
for equal bytes.  The shapes (label_agreement_ref.CASES) are the smallest at which each mechanism can go wrong: sides below, at
and past the 64 x 64 tile, widths that are no multiple of the four pixels a thread owns, class boundaries on the tile border and
d and d + 1 past it, a band wider than the image, C on both sides of the LDS-histogram switch (44 | 45), C = 1 and C = 255.

Behaviour (section 6.32's own case, 64 x 96, band 2): measured on the MI355X, unrefined -> after 10 default iterations
  mIoU 0.600000 -> 0.738048, mean boundary IoU 0.276413 -> 0.418694, pixel accuracy 0.750000 -> 0.849284 (the test prints them;
  mIoU and mean boundary IoU must rise)."""
from __future__ import annotations

import functools
import os
import sys
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dense_refine_ref as RR  # noqa: E402
import label_agreement_ref as AR  # noqa: E402

GUARD = 64
JUNK = -77
KEYS = ("confusion", "bad", "bands")


def _ops():
    from cclip_hip import ops
    return ops


def _guarded(shape, fill=JUNK):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=torch.int64)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf, fill=JUNK):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _outputs(B, C, d, per_image, fill=JUNK):
    R = B if per_image else 1
    out = {"confusion": _guarded((R, C, C + 1), fill), "bad": _guarded((R, 2), fill)}
    out["bands"] = _guarded((R, C, 3), fill) if d > 0 else (None, None)
    return out


def _run(pred, gt, C, d, per_image, outs, accumulate=False):
    """the native call into guarded buffers (the guards checked) -> the counts as numpy arrays"""
    _ops().label_agreement(pred, gt, C, d, outs["confusion"][1], outs["bad"][1], outs["bands"][1], per_image=per_image, accumulate=accumulate)
    torch.cuda.synchronize()
    for k in KEYS:
        assert outs[k][0] is None or _intact(outs[k][0]), k
    return {k: None if outs[k][1] is None else outs[k][1].cpu().numpy() for k in KEYS}


def _device(pred_np, gt_np, C, d, per_image=False):
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    return _run(pred, gt, C, d, per_image, _outputs(pred.shape[0], C, d, per_image))


def _same(got, ref, tag):
    for k in KEYS:
        if ref[k] is None:
            assert got[k] is None, f"{tag}: {k}"
            continue
        assert got[k].dtype == np.int64 and got[k].shape == ref[k].shape, f"{tag}: {k} {got[k].dtype} {got[k].shape}"
        bad = np.flatnonzero((got[k] != ref[k]).reshape(-1))
        assert bad.size == 0, (f"{tag}: {k} differs at {bad.size} places, first flat index {bad[0]}: "
                               f"{got[k].reshape(-1)[bad[0]]} != {ref[k].reshape(-1)[bad[0]]}")


@functools.lru_cache(maxsize=None)
def _ref(name, d=None, per_image=False):
    pred, gt, C, d0 = AR.CASES[name]
    return AR.counts(pred, gt, C, d0 if d is None else d, per_image)


# ---- 1. the counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_counts_equal_the_reference(name):
    pred, gt, C, d = AR.CASES[name]
    got = _device(pred, gt, C, d)
    _same(got, _ref(name), name)
    again = _device(pred, gt, C, d)                                            # two calls, equal bytes
    assert all(got[k].tobytes() == again[k].tobytes() for k in KEYS)
    if pred.shape[0] > 1:
        per = _device(pred, gt, C, d, per_image=True)
        _same(per, _ref(name, per_image=True), name + " per image")
        assert all(np.array_equal(per[k].sum(axis=0, keepdims=True), got[k]) for k in KEYS)


@pytest.mark.parametrize("name", ["1x5x7_C3_d1", "side_65x63_d2", "stairs_131x135_d1", "bad_2x33x70_d2", "pairs_C44_d1", "pairs_C45_d1",
                                  "C255_20x67_d2", "C1_30x41_d1", "batch_3x40x70_d2"])
def test_band_zero_has_no_bands(name):
    pred, gt, C, _ = AR.CASES[name]
    for per_image in (False, True):
        got = _device(pred, gt, C, 0, per_image)
        assert got["bands"] is None
        _same(got, _ref(name, 0, per_image), f"{name} d = 0 per_image {per_image}")
        full = _ref(name, per_image=per_image)                                  # the band does not change the other counts
        assert np.array_equal(got["confusion"], full["confusion"]) and np.array_equal(got["bad"], full["bad"])


def test_known_answers_on_the_device():
    u = _device(np.zeros((1, 130, 130), np.uint8), np.zeros((1, 130, 130), np.uint8), 2, 32)
    assert u["confusion"].tolist() == [[[16900, 0, 0], [0, 0, 0]]] and u["bands"].tolist() == [[[16900 - 66 * 66] * 3, [0, 0, 0]]]
    one = _device(np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8), 1, 1)
    assert one["confusion"].tolist() == [[[1, 0]]] and one["bands"].tolist() == [[[1, 1, 1]]] and one["bad"].tolist() == [[0, 0]]


@pytest.mark.parametrize("name", ["side_65x63_d2", "side_63x65_d32", "pairs_C45_d1", "batch_3x40x70_d2"])
def test_maps_one_byte_into_their_allocation(name):
    pred_np, gt_np, C, d = AR.CASES[name]
    n = pred_np.size
    pred = torch.empty(n + 1, device="cuda", dtype=torch.uint8)[1:].view(pred_np.shape)
    gt = torch.empty(n + 3, device="cuda", dtype=torch.uint8)[3:].view(gt_np.shape)
    pred.copy_(torch.from_numpy(pred_np)), gt.copy_(torch.from_numpy(gt_np))
    assert pred.data_ptr() % 4 == 1 and gt.data_ptr() % 4 == 3
    for dd in (d, 0):
        _same(_run(pred, gt, C, dd, False, _outputs(pred.shape[0], C, dd, False)), _ref(name, dd), f"{name} d = {dd}, offset maps")


@pytest.mark.parametrize("per_image", [False, True])
def test_accumulate_adds_to_what_the_buffers_hold(per_image):
    (p1, g1), (p2, g2) = AR.blocky(2, 70, 66, 6, seed=31), AR.blocky(2, 70, 66, 6, seed=32, shift=(1, 0))
    C, d = 6, 3
    r1, r2 = AR.counts(p1, g1, C, d, per_image), AR.counts(p2, g2, C, d, per_image)
    outs = _outputs(2, C, d, per_image)
    first = _run(torch.from_numpy(p1).cuda(), torch.from_numpy(g1).cuda(), C, d, per_image, outs)            # sets, over the junk
    _same(first, r1, "first call")
    both = _run(torch.from_numpy(p2).cuda(), torch.from_numpy(g2).cuda(), C, d, per_image, outs, accumulate=True)
    _same(both, {k: r1[k] + r2[k] for k in KEYS}, "accumulated")
    outs0 = _outputs(2, C, 0, per_image, fill=5)                                                           # adds to 5 in every cell, d == 0
    for k in ("confusion", "bad"):
        outs0[k][0][:GUARD] = JUNK
        outs0[k][0][-GUARD:] = JUNK
    got = _run(torch.from_numpy(p2).cuda(), torch.from_numpy(g2).cuda(), C, 0, per_image, outs0, accumulate=True)
    assert np.array_equal(got["confusion"], r2["confusion"] + 5) and np.array_equal(got["bad"], r2["bad"] + 5)


# ---- 2. refusals --------------------------------------------------------------------------------------
def test_raw_library_argument_errors():
    from cclip_hip import load_library
    lib = load_library()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, W, C = 2, 5, 7, 3
    pred = torch.zeros(B * H * W + 8, device="cuda", dtype=torch.uint8)
    gt = torch.zeros(B * H * W + 8, device="cuda", dtype=torch.uint8)
    cbuf, conf = _guarded((B, C, C + 1))
    bbuf, bad = _guarded((B, 2))
    dbuf, bands = _guarded((B, C, 3))
    ERR_ARG = 1
    good = dict(pred=pred.data_ptr(), gt=gt.data_ptr(), B=B, H=H, W=W, C=C, band=2, per_image=1, accumulate=0, confusion=conf.data_ptr(),
                bad=bad.data_ptr(), bands=bands.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.cclip_label_agreement(c_void_p(a["pred"]), c_void_p(a["gt"]), c_int(a["B"]), c_int(a["H"]), c_int(a["W"]), c_int(a["C"]),
                                         c_int(a["band"]), c_int(a["per_image"]), c_int(a["accumulate"]), c_void_p(a["confusion"]),
                                         c_void_p(a["bad"]), c_void_p(a["bands"]), stream)

    refused = [dict(pred=0), dict(gt=0), dict(confusion=0), dict(bad=0), dict(bands=0), dict(band=0), dict(C=0), dict(C=256), dict(band=-1),
               dict(band=33), dict(B=0), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(B=8, H=16384, W=16384),
               dict(B=1 << 30, H=2, W=1), dict(per_image=2), dict(accumulate=-1), dict(confusion=conf.data_ptr() + 4),
               dict(bad=bad.data_ptr() + 4), dict(bands=bands.data_ptr() + 2),
               dict(bad=conf.data_ptr() + 8), dict(bands=conf.data_ptr()), dict(bands=bad.data_ptr()),      # outputs that overlap
               dict(confusion=bands.data_ptr() + 8, per_image=0)]
    for kw in refused:
        assert call(**kw) == ERR_ARG, kw
    for accumulate in (0, 1):
        assert call(accumulate=accumulate, bands=0) == ERR_ARG and call(accumulate=accumulate, band=0) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((cbuf == JUNK).all()) and bool((bbuf == JUNK).all()) and bool((dbuf == JUNK).all())          # nothing launched, nothing written
    assert call() == 0 and call(band=0, bands=0) == 0 and call(pred=pred.data_ptr() + 1, gt=gt.data_ptr() + 3) == 0
    torch.cuda.synchronize()
    assert conf[:, 0, 0].tolist() == [H * W, H * W] and _intact(cbuf) and _intact(bbuf) and _intact(dbuf)


def test_wrapper_argument_errors():
    import clip
    ops = _ops()
    lab = torch.zeros(2, 5, 7, device="cuda", dtype=torch.uint8)
    conf, bad, bands = (torch.empty(s, device="cuda", dtype=torch.int64) for s in ((1, 3, 4), (1, 2), (1, 3, 3)))
    la = ops.label_agreement
    la(lab, lab, 3, 2, conf, bad, bands)
    cases = [
        ("label_agreement: pred must be a cuda tensor", lambda: la(lab.cpu(), lab, 3, 2, conf, bad, bands)),
        ("label_agreement: gt must be torch.uint8", lambda: la(lab, lab.int(), 3, 2, conf, bad, bands)),
        ("label_agreement: pred must be contiguous", lambda: la(lab.transpose(1, 2), lab, 3, 2, conf, bad, bands)),
        ("label_agreement: pred must be \\[B, H, W\\]", lambda: la(lab[0], lab[0], 3, 2, conf, bad, bands)),
        ("label_agreement: gt must be \\[2, 5, 7\\]", lambda: la(lab, lab[:1], 3, 2, conf, bad, bands)),
        ("label_agreement: n_classes must be an integer in \\[1, 255\\]", lambda: la(lab, lab, 256, 2, conf, bad, bands)),
        ("label_agreement: band must be an integer in \\[0, 32\\]", lambda: la(lab, lab, 3, 33, conf, bad, bands)),
        ("label_agreement: bands goes with band > 0", lambda: la(lab, lab, 3, 2, conf, bad)),
        ("label_agreement: bands goes with band > 0", lambda: la(lab, lab, 3, 0, conf, bad, bands)),
        ("label_agreement: confusion must be torch.int64", lambda: la(lab, lab, 3, 2, conf.int(), bad, bands)),
        ("label_agreement: confusion must be \\[2, 3, 4\\]", lambda: la(lab, lab, 3, 2, conf, bad, bands, per_image=True)),
        ("label_agreement: bad must be a cuda tensor", lambda: la(lab, lab, 3, 2, conf, bad.cpu(), bands)),
        ("label_agreement: bands must be \\[1, 3, 3\\]", lambda: la(lab, lab, 3, 2, conf, bad, bands.view(1, 9, 1))),
        ("label_agreement: height 1, width 16385", lambda: la(torch.zeros(1, 1, 16385, device="cuda", dtype=torch.uint8),
                                                              torch.zeros(1, 1, 16385, device="cuda", dtype=torch.uint8), 3, 2, conf, bad, bands)),
        ("evaluate_labels: gt must have pred's shape \\[2, 5, 7\\], got \\[5, 7\\]", lambda: clip.evaluate_labels(lab, lab[0], 3)),
        ("evaluate_labels: pred must be torch.uint8", lambda: clip.evaluate_labels(lab.int(), lab, 3)),
        ("evaluate_labels: n_classes must be an integer", lambda: clip.evaluate_labels(lab, lab, 0)),
        ("evaluate_labels: band must be None or an integer in \\[0, 32\\]", lambda: clip.evaluate_labels(lab, lab, 3, band=40)),
        ("evaluate_labels: 2 class names for 3 classes", lambda: clip.evaluate_labels(lab, lab, 3, class_names=["a", "b"])),
    ]
    for match, fn in cases:
        with pytest.raises(ValueError, match=match):
            fn()


# ---- 3. the Python surface ----------------------------------------------------------------------------
def _check_scores(s, ref_counts, r=None):
    """SegmentationScores against the reference's float64 scores of row r of the reference's counts (None: a pooled result)"""
    conf = ref_counts["confusion"][0 if r is None else r]
    bands = None if ref_counts["bands"] is None else ref_counts["bands"][0 if r is None else r]
    want = AR.scores(conf, bands)
    for k, v in want.items():
        got = getattr(s, k)
        if got is not None and r is not None:
            got = got[r]
        got = got.tolist() if isinstance(got, torch.Tensor) else got
        v = v.tolist() if isinstance(v, np.ndarray) else v
        assert np.array_equal(np.array(got, dtype=np.float64), np.array(v, dtype=np.float64), equal_nan=True), (k, got, v)


@pytest.mark.parametrize("name", ["side_65x63_d2", "batch_3x40x70_d2", "pairs_C45_d1", "C255_20x67_d2"])
def test_evaluate_labels_equals_the_reference_scores(name):
    import clip
    pred_np, gt_np, C, d = AR.CASES[name]
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    names = [f"c{i}" for i in range(C)]
    s = clip.evaluate_labels(pred, gt, C, band=d, class_names=names)
    ref = _ref(name)
    assert isinstance(s, clip.SegmentationScores) and not s.per_image and s.band == d and s.class_names == names
    assert np.array_equal(s.confusion.numpy(), ref["confusion"][0]) and np.array_equal(s.bands.numpy(), ref["bands"][0])
    _check_scores(s, ref)
    per = clip.evaluate_labels(pred, gt, C, band=d, per_image=True)
    refp = _ref(name, per_image=True)
    assert per.per_image and np.array_equal(per.confusion.numpy(), refp["confusion"]) and per.miou.shape == (pred.shape[0],)
    for r in range(pred.shape[0]):
        _check_scores(per, refp, r)
    tot = per.total()
    assert torch.equal(tot.confusion, s.confusion) and torch.equal(tot.bands, s.bands) and tot.miou == s.miou
    zero = clip.evaluate_labels(pred, gt, C, band=0)
    assert zero.bands is None and zero.band == 0 and zero.boundary_iou is None and torch.equal(zero.confusion, s.confusion)
    if pred.shape[0] == 1:                                                     # [H, W] in: the same counts
        flat = clip.evaluate_labels(pred[0], gt[0], C, band=d)
        assert torch.equal(flat.confusion, s.confusion) and torch.equal(flat.bands, s.bands)
    else:                                                                      # the images one by one, summed: the batch
        parts = [clip.evaluate_labels(pred[b], gt[b], C, band=d) for b in range(pred.shape[0])]
        acc = parts[0] + parts[1]
        for p in parts[2:]:
            acc += p
        assert torch.equal(acc.confusion, s.confusion) and torch.equal(acc.bands, s.bands) and acc.miou == s.miou


def test_out_of_range_labels_are_a_value_error_and_the_default_band():
    import clip
    pred_np, gt_np, C, d = AR.CASES["bad_2x33x70_d2"]
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    nb = _ref("bad_2x33x70_d2")["bad"][0].tolist()
    with pytest.raises(ValueError, match=f"{nb[0]} pixels of gt hold a label in \\[4, 254\\] and {nb[1]} pixels of pred hold a label in \\[4, 254\\]"):
        clip.evaluate_labels(pred, gt, C)
    with pytest.raises(ValueError, match="evaluate_labels: [0-9]+ pixels of pred hold"):
        clip.evaluate_labels(pred, torch.where(gt >= C, torch.full_like(gt, 255), gt), C, band=0)
    ok = torch.zeros(64, 96, device="cuda", dtype=torch.uint8)
    assert clip.evaluate_labels(ok, ok, 2).band == AR.default_band(64, 96) == 2
    assert clip.evaluate_labels(ok[:5, :7].contiguous(), ok[:5, :7].contiguous(), 2).band == 1
    big = torch.zeros(1080, 1920, device="cuda", dtype=torch.uint8)
    s = clip.evaluate_labels(big, big, 9)
    assert s.band == 32 and s.miou == 1.0 and s.bands[0].tolist() == [1080 * 1920 - (1080 - 64) * (1920 - 64)] * 3


def _toy(grid, dtype=torch.bfloat16, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)
    return geo, clip.build_model(init_state_dict(geo, seed), dtype).cuda().eval()


def _check_result(res, gt, band=None):
    import clip
    s = res.evaluate(gt, band=band)
    direct = clip.evaluate_labels(res.labels, gt.reshape(res.labels.shape), res.n_classes, band=band, class_names=res.class_names)
    assert torch.equal(s.confusion, direct.confusion) and torch.equal(s.bands, direct.bands) and s.band == direct.band
    assert s.class_names == res.class_names and s.n_classes == res.n_classes
    valid = int(s.confusion.sum())
    assert valid == int((gt != 255).sum())
    hits = int((res.labels == gt.reshape(res.labels.shape)).sum())             # 255 == 255 never counts: gt 255 is ignored, and
    hits -= int(((res.labels == 255) & (gt.reshape(res.labels.shape) == 255)).sum())   # pred 255 is no hit
    # pixel_accuracy valid == hits, stated without a second rounding: the diagonal sums to hits, and the one division is hits / valid
    assert int(torch.diagonal(s.confusion[:, :-1]).sum()) == hits and s.pixel_accuracy == hits / valid
    ref = AR.counts(res.labels.reshape(-1, *res.labels.shape[-2:]).cpu().numpy(), gt.reshape(-1, *gt.shape[-2:]).cpu().numpy(), res.n_classes, s.band)
    assert np.array_equal(s.confusion.numpy(), ref["confusion"][0]) and np.array_equal(s.bands.numpy(), ref["bands"][0])
    return s


def test_results_evaluate_on_the_toy_tower():
    import clip
    from clip.weights import synthetic_images
    geo, model = _toy(2)
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    gen = torch.Generator().manual_seed(8)
    photo = torch.randint(0, 256, (45, 61, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
    gt = torch.randint(0, 4, (45, 61), generator=gen, dtype=torch.uint8)
    gt[:, 30:33] = 255
    gt = gt.cuda()
    res = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=4)
    assert _check_result(res, gt).band == 2
    _check_result(res.refine(photo, iterations=2), gt, band=3)
    img = synthetic_images(2, geo, 4).cuda()
    dense = clip.segment(model, img, text, size=(29, 43), min_conf=0.3)
    gtb = torch.randint(0, 4, (2, 29, 43), generator=gen, dtype=torch.uint8).cuda()
    s = _check_result(dense, gtb, band=1)
    per = dense.evaluate(gtb, band=1, per_image=True)
    assert per.per_image and torch.equal(per.total().confusion, s.confusion) and torch.equal(per.total().bands, s.bands)
    with pytest.raises(ValueError, match="evaluate: gt must have the labels' shape \\[45, 61\\], got \\[45, 60\\]"):
        res.evaluate(gt[:, :60])
    with pytest.raises(ValueError, match="evaluate: gt must have the labels' shape \\[2, 29, 43\\], got \\[29, 43\\]"):
        dense.evaluate(gtb[0])


# ---- 4. behaviour: refinement raises both scores on section 6.32's case ---------------------------------
def test_refinement_raises_miou_and_boundary_iou_on_the_diagonal_case():
    import clip
    maps, guide, truth = RR.diagonal_case()
    gt = truth.to(torch.uint8).cuda()
    lab = torch.empty(1, 64, 96, device="cuda", dtype=torch.uint8)
    conf = torch.empty(1, 64, 96, device="cuda")
    _ops().dense_maps_label(maps.cuda(), lab, conf)
    before = clip.evaluate_labels(lab[0], gt, 2, band=2)
    _ops().dense_maps_label(clip.refine_maps(maps.cuda(), guide.cuda()), lab, conf)
    after = clip.evaluate_labels(lab[0], gt, 2, band=2)
    print(f"diagonal case, band 2: mIoU {before.miou:.6f} -> {after.miou:.6f}, mean boundary IoU {before.mean_boundary_iou:.6f} -> "
          f"{after.mean_boundary_iou:.6f}, pixel accuracy {before.pixel_accuracy:.6f} -> {after.pixel_accuracy:.6f}")
    assert before.pixel_accuracy == RR.DIAGONAL_BEFORE
    assert after.miou > before.miou and after.mean_boundary_iou > before.mean_boundary_iou
