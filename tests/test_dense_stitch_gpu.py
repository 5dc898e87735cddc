"""GPU: the window stitch (csrc/dense_stitch.hip, ops.dense_stitch, clip.segment_photo, clip.segment(size=(h, w))) on the MI355X
against the float64 reference of tests/dense_stitch_ref.py.

Bounds.
  labels   equal outside the fragile set (float64 top-two margin in (0, FRAGILE = 1e-5): either class), dense_ref.compare_labels.
  conf     |conf - conf64| <= CONF_TOL = 1e-6 on the shared cases (cover <= 6): the project's bound for ONE sample (measured
           1.5e-7); the n - 1 <= 5 fp32 adds of values <= 1 add at most 5 x 2^-24 x n / n ~ 3e-7 after the division.  The hand-made
           cases with n windows on a pixel use CONF_TOL + (n - 1) x 2^-24: each of the n - 1 adds rounds a partial sum <= n by at
           most n x 2^-25, in all (n - 1) x n x 2^-25 before and (n - 1) x 2^-25 after the division by n; the bound takes twice
           that.  With n <= 64 twice the bound stays below FRAGILE, so the label comparison keeps its width.
           Measured on the MI355X: 7.1e-8 / 1.3e-7 / 1.0e-7 / 1.2e-7 / 9.8e-8 on the five shared cases, 9.8e-8 at 40 windows.
  cover    exact; picture bytes exactly the integer formula on the returned labels.
Paths.  DS_FAST = 4 covering windows of a pixel keep their axes in registers, the rest go through the recompute loop (the
40-window test, and every case with cover > 4).  A work-group lists up to DS_LIST = 512 windows that meet its 1024-pixel band
in LDS (K = 300 small windows: the list path, as every other test here); more than 512 meeting one band (K = 600 full-height
columns) makes the group walk all K boxes from global memory instead."""
import json
import os
import subprocess
import sys
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dense_ref as R  # noqa: E402
import dense_stitch_ref as SR  # noqa: E402

GUARD = 64
FEAT_TOL = {torch.bfloat16: 1.2e-2, torch.float16: 1.0e-3}      # DESIGN 6.29, encode_image_dense rel L2


def _ops():
    from cclip_hip import ops
    return ops


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _boxes(b):
    return torch.as_tensor(np.asarray(b), dtype=torch.int32).reshape(-1, 4).cuda()


def _run(probs, boxes, H, W, min_conf=0.0, overlay=False, palette=None, photo=None, alpha8=256):
    """(labels, conf, cover, overlay) in guarded buffers, the guards checked"""
    lbuf, labels = _guarded((H, W), torch.uint8, 77)
    cbuf, conf = _guarded((H, W), torch.float32, -7.0)
    vbuf, cover = _guarded((H, W), torch.uint8, 77)
    obuf, out = _guarded((H, W, 3), torch.uint8, 77) if overlay else (None, None)
    _ops().dense_stitch(probs.cuda(), _boxes(boxes), H, W, labels, conf, min_conf=min_conf, cover=cover, overlay=out, palette=palette,
                        photo=photo, alpha8=alpha8)
    torch.cuda.synchronize()
    assert _intact(lbuf, 77) and _intact(cbuf, -7.0) and _intact(vbuf, 77) and (obuf is None or _intact(obuf, 77))
    return labels, conf, cover, out


def _tol(nmax):
    return R.CONF_TOL + max(nmax - 1, 0) * 2.0 ** -24


def _check(got, ref, tol=R.CONF_TOL, tag=""):
    labels, conf, cover, _ = got
    wrong, share = R.compare_labels(labels, ref)
    cerr = (conf.double().cpu() - ref["conf"]).abs().max().item()
    print(f"dense_stitch {tag}: wrong {wrong}, fragile share {share:.2e}, max |dconf| {cerr:.3e} (bound {tol:.2e}), "
          f"cover {int(ref['cover'].min())}-{int(ref['cover'].max())}")
    assert wrong == 0
    assert cerr <= tol
    assert torch.equal(cover.cpu().long(), ref["cover"].clamp_max(255))
    return cerr


# ---- kernel against float64 --------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.STITCH_CASES)
def test_stitch_against_float64(case):
    import clip
    probs, boxes, H, W = SR.stitch_case(case)
    ref = SR.stitch_ref(probs, boxes, H, W)
    C = probs.shape[1]
    gen = torch.Generator().manual_seed(5)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    photo = torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).cuda()
    got = _run(probs, boxes, H, W, overlay=True, palette=pal)
    _check(got, ref, tag=str(case))
    labels, conf, cover, out = got
    assert torch.equal(out.cpu(), R.overlay_ref(labels, pal))
    for a8 in (0, 77, 256):
        l2, c2, v2, o2 = _run(probs, boxes, H, W, overlay=True, palette=pal, photo=photo, alpha8=a8)
        assert torch.equal(l2, labels) and torch.equal(c2, conf) and torch.equal(v2, cover)       # two calls, equal bytes
        assert torch.equal(o2.cpu(), R.overlay_ref(labels, pal, photo, a8)), a8
    l3, c3, v3, _ = _run(probs, boxes, H, W)                                                      # the picture changes none
    assert torch.equal(l3, labels) and torch.equal(c3, conf) and torch.equal(v3, cover)
    thr = float(ref["conf"].median())
    rt = SR.stitch_ref(probs, boxes, H, W, min_conf=thr)
    lt, ct, _, _ = _run(probs, boxes, H, W, min_conf=thr)
    assert R.compare_labels(lt, rt)[0] == 0 and torch.equal(ct, conf)
    assert bool((lt[ct < thr] == 255).all()) and bool((lt[ct >= thr] < C).all())
    assert torch.equal(clip.default_palette(C)[255], torch.tensor([96, 96, 96], dtype=torch.uint8))


# ---- bitwise identities ------------------------------------------------------------------------
@pytest.mark.parametrize("g,S", [(7, 224), (2, 5), (1, 9)])
def test_one_full_window_is_dense_label_map_bit_for_bit(g, S):
    C = 5
    probs = R.label_case(g, S, C, 1, seed=1).cuda()
    gen = torch.Generator().manual_seed(6)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    photo = torch.randint(0, 256, (S, S, 3), generator=gen, dtype=torch.uint8).cuda()
    lab = torch.empty(1, S, S, device="cuda", dtype=torch.uint8)
    conf = torch.empty(1, S, S, device="cuda")
    ov = torch.empty(1, S, S, 3, device="cuda", dtype=torch.uint8)
    for mc in (0.0, 0.5):
        _ops().dense_label_map(probs, S, lab, conf, min_conf=mc, overlay=ov, palette=pal, photo=photo[None], alpha8=77)
        l2, c2, v2, o2 = _run(probs, [[0, 0, S, S]], S, S, min_conf=mc, overlay=True, palette=pal, photo=photo, alpha8=77)
        assert torch.equal(l2, lab[0]) and torch.equal(c2, conf[0]) and torch.equal(o2, ov[0])
        assert bool((v2 == 1).all())


def test_permutation_that_keeps_each_pixels_order_gives_equal_bytes():
    """two groups of windows that share no pixel (left and right of column 24), interleaved two ways: every pixel sees its own
    windows in the same order"""
    H, W, g, C = 20, 50, 3, 4
    left = [[0, 0, 16, 16], [6, 2, 22, 20], [3, 5, 24, 14]]
    right = [[26, 0, 50, 12], [30, 4, 46, 20], [24, 8, 40, 18]]
    probs = SR.stitch_maps(6, C, g, seed=11)
    order_a, order_b = [0, 1, 2, 3, 4, 5], [3, 0, 4, 1, 5, 2]
    boxes = np.array(left + right)
    a = _run(probs[order_a], boxes[order_a], H, W)
    b = _run(probs[order_b], boxes[order_b], H, W)
    _check(a, SR.stitch_ref(probs, boxes, H, W), tag="permutation")
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


# ---- hand-made boxes ---------------------------------------------------------------------------
def test_hole_and_identical_windows():
    H, W, g = 12, 19, 3
    base = SR.stitch_maps(1, 2, g, seed=12)[0]                                # [2, g, g]
    twin = torch.stack([torch.zeros_like(base[0]), base[0], base[0], base[1]]).contiguous()      # classes 1 and 2 identical
    probs = torch.stack([twin, twin])
    boxes = [[2, 1, 12, 11], [2, 1, 12, 11]]
    pal = torch.arange(768, dtype=torch.int64).remainder(251).to(torch.uint8).view(256, 3).cuda()
    labels, conf, cover, out = _run(probs, boxes, H, W, overlay=True, palette=pal)
    ref = SR.stitch_ref(probs, torch.tensor(boxes), H, W)
    assert R.compare_labels(labels, ref)[0] == 0
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[1:11, 2:12] = True
    assert bool((cover.cpu()[inside] == 2).all()) and bool((cover.cpu()[~inside] == 0).all())
    assert bool((labels.cpu()[~inside] == 255).all()) and bool((conf.cpu()[~inside] == 0).all())       # the hole
    assert bool((out.cpu()[~inside] == pal[255].cpu()).all())
    l1, c1, v1, _ = _run(probs[:1], boxes[:1], H, W)
    assert torch.equal(conf, c1) and torch.equal(labels, l1)                  # (s + s) / 2 == s / 1, bit for bit
    won = labels.cpu()[inside]
    assert bool(((won == 1) | (won == 3)).all()) and bool((won == 1).any())   # an exact tie of 1 and 2: never the higher index


def test_box_hanging_over_every_edge_and_one_rectangle():
    H, W, g, C = 21, 34, 4, 3
    probs = SR.stitch_maps(2, C, g, seed=13)
    boxes = [[-5, -4, W + 3, H + 6], [-9, 3, 17, H + 40]]
    _check(_run(probs, boxes, H, W), SR.stitch_ref(probs, torch.tensor(boxes), H, W), tag="hanging")
    _check(_run(probs[:1], [[0, 0, W, H]], H, W), SR.stitch_ref(probs[:1], torch.tensor([[0, 0, W, H]]), H, W), tag="rectangle")


def test_bad_boxes_among_valid_ones_change_nothing():
    H, W, g, C = 23, 37, 2, 3
    probs, boxes, _, _ = SR.stitch_case(SR.STITCH_CASES[0])
    K = boxes.shape[0]
    want = _run(probs, boxes, H, W)
    i32 = 2 ** 31
    bad = [[5, 5, 5, 9], [9, 2, 4, 11], [0, 0, 16385, 4], [3, -16380, 7, 6], [-i32, -i32, i32 - 1, i32 - 1], [i32 - 1, 0, -i32, 4],
           [0, i32 - 1, 4, -i32], [-i32, 0, 10, 10]]
    mixed_boxes = torch.cat([torch.tensor(bad[:4]), boxes[:3], torch.tensor(bad[4:]), boxes[3:]])
    filler = SR.stitch_maps(len(bad), C, g, seed=14)
    mixed_probs = torch.cat([filler[:4], probs[:3], filler[4:], probs[3:]])
    assert mixed_boxes.shape[0] == K + len(bad)
    got = _run(mixed_probs, mixed_boxes, H, W)                                # (_run checks the guard bytes)
    for x, y in zip(got[:3], want[:3]):
        assert torch.equal(x, y)


def test_forty_windows_on_a_pixel():
    """cover 40 in the middle: 4 windows from registers, 36 through the recompute loop"""
    H, W, g, C = 30, 41, 3, 4
    rng = np.random.default_rng(15)
    boxes = np.array([[rng.integers(0, 15), rng.integers(0, 10), rng.integers(26, 42), rng.integers(20, 31)] for _ in range(40)])
    probs = SR.stitch_maps(40, C, g, seed=15)
    ref = SR.stitch_ref(probs, torch.from_numpy(boxes), H, W)
    assert int(ref["cover"].max()) == 40
    _check(_run(probs, boxes, H, W), ref, tol=_tol(40), tag="40 windows")


@pytest.mark.parametrize("K,kind", [(300, "small"), (600, "columns")])
def test_many_windows_list_path_and_overflow_fallback(K, kind):
    """64 x 48 = three work-groups of 16 rows.  300 small windows: at most 300 <= 512 meet a band - the LDS list.  600 columns of
    the picture's height meet every band: 600 > 512, each group walks all K boxes from global memory."""
    H, W, g, C = 48, 64, 2, 3
    rng = np.random.default_rng(16)
    if kind == "small":
        x0, y0 = rng.integers(-3, W - 2, K), rng.integers(-3, H - 2, K)
        boxes = np.stack([x0, y0, x0 + rng.integers(4, 13, K), y0 + rng.integers(4, 13, K)], axis=1)
    else:
        x0 = rng.integers(0, W - 1, K)
        boxes = np.stack([x0, np.zeros(K, dtype=np.int64), x0 + rng.integers(1, 3, K), np.full(K, H)], axis=1)
    probs = SR.stitch_maps(K, C, g, seed=16)
    ref = SR.stitch_ref(probs, torch.from_numpy(boxes), H, W)
    nmax = int(ref["cover"].max())
    assert 4 < nmax <= 64
    got = _run(probs, boxes, H, W)
    _check(got, ref, tol=_tol(nmax), tag=f"K={K} {kind}")
    again = _run(probs, boxes, H, W)
    assert all(torch.equal(x, y) for x, y in zip(got[:3], again[:3]))


def test_misaligned_buffers():
    probs, boxes, H, W = SR.stitch_case(SR.STITCH_CASES[0])
    gen = torch.Generator().manual_seed(4)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    photo = torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).cuda()
    labels, conf, cover, out = _run(probs, boxes, H, W, overlay=True, palette=pal, photo=photo, alpha8=100)
    n = H * W
    lb = torch.full((n + 9,), 77, device="cuda", dtype=torch.uint8)
    vb = torch.full((n + 9,), 77, device="cuda", dtype=torch.uint8)
    ob = torch.full((3 * n + 9,), 77, device="cuda", dtype=torch.uint8)
    pb = torch.zeros(3 * n + 3, device="cuda", dtype=torch.uint8)
    pb[3:] = photo.flatten()
    pb1 = torch.zeros(3 * n + 1, device="cuda", dtype=torch.uint8)
    pb1[1:] = photo.flatten()
    cb = torch.full((n + 5,), -7.0, device="cuda")
    _ops().dense_stitch(probs.cuda(), _boxes(boxes), H, W, lb[1:1 + n].view(H, W), cb[1:1 + n].view(H, W), cover=vb[1:1 + n].view(H, W),
                        overlay=ob[1:1 + 3 * n].view(H, W, 3), palette=pal, photo=pb1[1:].view(H, W, 3), alpha8=100)
    assert torch.equal(lb[1:1 + n].view(H, W), labels) and torch.equal(ob[1:1 + 3 * n].view(H, W, 3), out)
    assert torch.equal(vb[1:1 + n].view(H, W), cover) and torch.equal(cb[1:1 + n].view(H, W), conf)
    for b, fill, m in ((lb, 77, n), (vb, 77, n), (ob, 77, 3 * n), (cb, -7.0, n)):
        assert b[0] == fill and bool((b[1 + m:] == fill).all())
    o2 = torch.empty(H, W, 3, device="cuda", dtype=torch.uint8)
    _ops().dense_stitch(probs.cuda(), _boxes(boxes), H, W, torch.empty_like(labels), torch.empty_like(conf), overlay=o2, palette=pal,
                        photo=pb[3:].view(H, W, 3), alpha8=100)               # a photo 3 bytes off a dword
    assert torch.equal(o2, out)


# ---- argument errors ---------------------------------------------------------------------------
def test_raw_library_argument_errors():
    from cclip_hip import load_library
    lib = load_library()
    ERR_ARG = lib.cclip_dense_stitch(c_void_p(0), c_int(1), c_int(1), c_int(1), c_void_p(0), c_int(1), c_int(1), c_float(0.0), c_void_p(0),
                                     c_void_p(0), c_void_p(0), c_void_p(0), c_void_p(0), c_int(0), c_void_p(0), c_void_p(0))
    assert ERR_ARG != 0
    probs = torch.rand(2, 3, 2, 2, device="cuda")
    boxes = _boxes([[0, 0, 5, 5], [1, 1, 4, 4]])
    lab, conf = torch.zeros(5, 5, device="cuda", dtype=torch.uint8), torch.zeros(5, 5, device="cuda")
    pal = torch.zeros(256, 3, device="cuda", dtype=torch.uint8)
    ov, ph = torch.zeros(5, 5, 3, device="cuda", dtype=torch.uint8), torch.zeros(5, 5, 3, device="cuda", dtype=torch.uint8)
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(probs=probs.data_ptr(), K=2, C=3, g=2, boxes=boxes.data_ptr(), H=5, W=5, labels=lab.data_ptr(), conf=conf.data_ptr(),
                cover=0, palette=pal.data_ptr(), photo=ph.data_ptr(), a8=128, overlay=ov.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.cclip_dense_stitch(c_void_p(a["probs"]), c_int(a["K"]), c_int(a["C"]), c_int(a["g"]), c_void_p(a["boxes"]), c_int(a["H"]),
                                      c_int(a["W"]), c_float(0.0), c_void_p(a["labels"]), c_void_p(a["conf"]), c_void_p(a["cover"]),
                                      c_void_p(a["palette"]), c_void_p(a["photo"]), c_int(a["a8"]), c_void_p(a["overlay"]), stream)

    assert call() == 0
    assert call(palette=0, photo=0, overlay=0) == 0
    bad = [dict(probs=0), dict(boxes=0), dict(labels=0), dict(conf=0), dict(K=0), dict(K=65536), dict(C=0), dict(C=256), dict(g=0),
           dict(g=16385), dict(H=0), dict(H=16385), dict(W=0), dict(W=16385), dict(palette=0), dict(overlay=0), dict(a8=-1), dict(a8=257),
           dict(probs=probs.data_ptr() + 2), dict(conf=conf.data_ptr() + 2), dict(boxes=boxes.data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()


def test_wrapper_argument_errors():
    ops = _ops()
    probs = torch.rand(2, 3, 2, 2, device="cuda")
    boxes = _boxes([[0, 0, 7, 5], [1, 1, 4, 4]])
    lab, conf = torch.empty(5, 7, device="cuda", dtype=torch.uint8), torch.empty(5, 7, device="cuda")
    pal = torch.zeros(256, 3, device="cuda", dtype=torch.uint8)
    ov = torch.empty(5, 7, 3, device="cuda", dtype=torch.uint8)
    ops.dense_stitch(probs, boxes, 5, 7, lab, conf, cover=torch.empty_like(lab), overlay=ov, palette=pal)
    cases = [
        ("probs must be a cuda tensor", lambda: ops.dense_stitch(probs.cpu(), boxes, 5, 7, lab, conf)),
        ("boxes must be a cuda tensor", lambda: ops.dense_stitch(probs, boxes.cpu(), 5, 7, lab, conf)),
        ("boxes must be torch.int32", lambda: ops.dense_stitch(probs, boxes.long(), 5, 7, lab, conf)),
        ("boxes must be contiguous", lambda: ops.dense_stitch(probs, _boxes([[0, 1], [0, 1], [7, 4], [5, 4]]).t(), 5, 7, lab, conf)),
        ("boxes must be \\[2, 4\\]", lambda: ops.dense_stitch(probs, boxes[:1], 5, 7, lab, conf)),
        ("labels must be torch.uint8", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab.int(), conf)),
        ("probs must be \\[K, C, g, g\\]", lambda: ops.dense_stitch(probs[:, :, :1].contiguous(), boxes, 5, 7, lab, conf)),
        ("256 classes", lambda: ops.dense_stitch(torch.rand(2, 256, 2, 2, device="cuda"), boxes, 5, 7, lab, conf)),
        ("65536 windows", lambda: ops.dense_stitch(torch.zeros(65536, 1, 1, 1, device="cuda"),
                                                   torch.zeros(65536, 4, device="cuda", dtype=torch.int32), 5, 7, lab, conf)),
        ("height 0", lambda: ops.dense_stitch(probs, boxes, 0, 7, lab, conf)),
        ("width 16385", lambda: ops.dense_stitch(probs, boxes, 5, 16385, lab, conf)),
        ("labels must be \\[5, 7\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab.view(7, 5), conf)),
        ("conf must be \\[5, 7\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf.view(7, 5))),
        ("cover must be \\[5, 7\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, cover=lab.view(7, 5))),
        ("cover must be torch.uint8", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, cover=conf)),
        ("palette must be uint8 \\[256, 3\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, overlay=ov)),
        ("give overlay too", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, palette=pal)),
        ("overlay must be \\[5, 7, 3\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, overlay=ov.view(7, 5, 3), palette=pal)),
        ("photo must be \\[5, 7, 3\\]", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, overlay=ov, palette=pal,
                                                                 photo=torch.zeros(7, 5, 3, device="cuda", dtype=torch.uint8))),
        ("alpha8", lambda: ops.dense_stitch(probs, boxes, 5, 7, lab, conf, overlay=ov, palette=pal, alpha8=257)),
    ]
    for match, fn in cases:
        with pytest.raises(ValueError, match=match):
            fn()


# ---- segment_photo / segment(size=(h, w)) on a toy model ---------------------------------------
def _toy(grid, dtype, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)       # width 128, 2 heads of 64, 2 layers
    sd = init_state_dict(geo, seed)
    return geo, sd, clip.build_model(sd, dtype).cuda().eval()


def _photo(W, H, seed):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("grid", [2, 3])
def test_segment_photo_is_the_composition_by_hand(grid):
    import clip
    from clip.preprocess_device import DevicePreprocess
    geo, sd, model = _toy(grid, torch.bfloat16)
    R_px, C, batch = geo.image_resolution, 4, 4
    photo = _photo(61, 45, 21)
    text = torch.randn(C, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    res = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=batch)
    boxes = clip.plan_windows(61, 45, 24, 12)
    K = len(boxes)
    assert K == 15 and torch.equal(res.boxes, torch.from_numpy(boxes)) and res.boxes.dtype == torch.int64
    crops = DevicePreprocess(R_px).regions(photo, boxes)
    scale = float(model.logit_scale.detach().exp())
    probs = torch.empty(K, C, grid, grid, device="cuda")
    for i in range(0, K, batch):
        f = model.encode_image_dense(crops[i:i + batch])
        b = f.shape[0]
        _ops().dense_class_probs(f.view(b * grid * grid, -1), text, scale, grid * grid, probs[i:i + b].view(b, C, grid * grid))
    labels, conf = torch.empty(45, 61, device="cuda", dtype=torch.uint8), torch.empty(45, 61, device="cuda")
    cover = torch.empty_like(labels)
    _ops().dense_stitch(probs, _boxes(boxes), 45, 61, labels, conf, min_conf=0.3, cover=cover)
    assert torch.equal(res.probs, probs) and torch.equal(res.labels, labels) and torch.equal(res.conf, conf) and torch.equal(res.cover, cover)
    assert res.class_names is None and res.n_classes == C and res.min_conf == 0.3
    ref = SR.stitch_ref(probs.cpu(), torch.from_numpy(boxes), 45, 61, min_conf=0.3)
    _check((res.labels, res.conf, res.cover, None), ref, tol=_tol(int(ref["cover"].max())), tag=f"segment_photo grid {grid}")
    fr = res.area_fractions()
    assert fr.shape == (C + 1,) and abs(float(fr.sum()) - 1.0) < 1e-12
    pal = clip.default_palette(C)
    assert torch.equal(res.overlay().cpu(), R.overlay_ref(labels, pal))
    assert torch.equal(res.overlay(photo=photo, alpha=0.25).cpu(), R.overlay_ref(labels, pal, photo, 64))
    top = res.top_class()
    if top is not None:
        bx = res.class_boxes(top)
        assert bx and all(0 <= x0 < x1 <= 61 and 0 <= y0 < y1 <= 45 for x0, y0, x1, y1 in bx)
        assert sum(int((res.labels[y0:y1, x0:x1] == top).sum()) for x0, y0, x1, y1 in bx) >= int((res.labels == top).sum())

    # batch = 1 against batch = 64: not bitwise (the GEMM tile may follow the row count).  Two runs of the 16-bit tower are each
    # within FEAT_TOL (rel L2) of float64, a cosine moves by at most twice that, a logit by scale times that and a
    # softmax probability by no more than its logits: |dp| <= 4 FEAT_TOL scale.  Labels may differ only where the float64
    # margin of one run is below twice the largest probability change (plus the usual fragile width).
    one = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=1)
    many = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=64)
    dp = (one.probs - many.probs).abs().max().item()
    dc = (one.conf - many.conf).abs().max().item()
    print(f"segment_photo grid {grid}: batch 1 vs 64 max |dp| {dp:.3e}, max |dconf| {dc:.3e}")
    bound = 4 * FEAT_TOL[torch.bfloat16] * scale
    assert dp <= bound and dc <= bound + 2 * R.CONF_TOL
    ref_many = SR.stitch_ref(many.probs.cpu(), torch.from_numpy(boxes), 45, 61, min_conf=0.3)
    assert R.compare_labels(one.labels, ref_many, fragile=2 * dp + R.FRAGILE, conf_tol=dp + R.CONF_TOL)[0] == 0


def test_segment_photo_square_photo_is_segment_and_multi_scale_covers_twice():
    import clip
    from clip.preprocess_device import DevicePreprocess
    geo, sd, model = _toy(2, torch.bfloat16)
    R_px = geo.image_resolution
    text = torch.randn(3, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    photo = _photo(R_px, R_px, 22)
    res = clip.segment_photo(model, photo, text, window=R_px)
    want = clip.segment(model, DevicePreprocess(R_px)(photo.numpy())[None], text)      # (its single-image call takes PIL / numpy)
    assert res.probs.shape[0] == 1 and torch.equal(res.labels, want.labels[0]) and torch.equal(res.conf, want.conf[0])
    assert bool((res.cover == 1).all())
    big = _photo(150, 131, 23)
    ms = clip.segment_photo(model, big, text, window=(R_px, 2 * R_px), batch=8)
    k1, k2 = len(clip.plan_windows(150, 131, R_px)), len(clip.plan_windows(150, 131, 2 * R_px))
    assert ms.probs.shape[0] == k1 + k2 and ms.labels.shape == (131, 150)
    assert int(ms.cover.min()) >= 2
    assert bool((ms.labels < 3).all()) and torch.isfinite(ms.conf).all()
    with pytest.raises(ValueError, match="downscale factor"):
        clip.segment_photo(model, torch.zeros(4200, 4200, 3, dtype=torch.uint8), text, window=4200)      # 4200 / 64 > 64: before any upload


def test_segment_rectangular_size_against_float64():
    import clip
    from clip.weights import synthetic_images
    geo, sd, model = _toy(3, torch.bfloat16)
    img = synthetic_images(2, geo, 4).cuda()
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    H, W = 29, 43
    res = clip.segment(model, img, text, size=(H, W), min_conf=0.3)
    assert res.labels.shape == (2, H, W) and res.conf.shape == (2, H, W)
    sq = clip.segment(model, img, text, size=40, min_conf=0.3)
    assert torch.equal(sq.probs, res.probs)
    pal = clip.default_palette(4)
    photo = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    ov, ovp = res.overlay().cpu(), res.overlay(photo=photo, alpha=0.25).cpu()
    for b in range(2):
        ref = SR.stitch_ref(res.probs[b:b + 1].cpu(), torch.tensor([[0, 0, W, H]]), H, W, min_conf=0.3)
        cover = torch.ones(H, W, dtype=torch.uint8)
        _check((res.labels[b], res.conf[b], cover, None), ref, tag=f"segment size=({H}, {W}) image {b}")
    assert torch.equal(ov, R.overlay_ref(res.labels, pal)) and torch.equal(ovp, R.overlay_ref(res.labels, pal, photo, 64))
    same = clip.segment(model, img, text, size=(40, 40), min_conf=0.3)        # a square tuple: the same bytes as the int
    assert torch.equal(same.labels, sq.labels) and torch.equal(same.conf, sq.conf)
    with pytest.raises(ValueError, match="height, width"):
        clip.segment(model, img, text, size=(1, 2, 3))


# ---- the script --------------------------------------------------------------------------------
def test_segment_images_script_with_windows(tmp_path):
    out = tmp_path / "maps"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "segment_images.py"), "--synthetic", "--n_images", "2", "--window", "224",
                        "--stride", "112", "--png", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    from PIL import Image
    for line in lines:
        assert abs(sum(line["area"]) - 1.0) < 1e-5 and len(line["area"]) == len(line["classes"]) + 1
        assert line["top_class"] in line["classes"]
        src = Image.open(line["file"]).size if os.path.exists(line["file"]) else (line["width"], line["height"])
        assert (line["width"], line["height"]) == src and line["windows"] >= 1
        assert Image.open(line["png"]).size == (line["width"], line["height"])
    assert len(os.listdir(out)) == 2
