"""GPU: the image-guided refinement (csrc/dense_refine.hip: ops.dense_refine_prepare, dense_refine_step; the maps it starts from
and their labels, csrc/dense_stitch.hip: ops.dense_stitch_maps, csrc/dense_classes.hip: ops.dense_maps_label; clip.refine_maps,
DenseResult.refine, PhotoDenseResult.refine) on the MI355X against the float64 references of tests/dense_refine_ref.py and
tests/dense_stitch_ref.py.

Exact (==): stitch_maps + maps_label(cover=) against dense_stitch, also where a pixel has 40 windows (the recompute loop), on
the LDS list of K = 300 and on the walk of all K = 600 boxes; max_c maps against conf; two calls of every kernel; a flat guide
of one colour against a flat guide of another; overlay bytes against the integer formula.
Every class of dense_stitch_maps against float64 within CONF_TOL + (nmax - 1) 2^-24, test_dense_stitch_gpu.py's bound for conf.
Bounds: dense_refine_ref.BOUNDS, per case and guide 4 x the error of the fp32 torch restatement against float64 (measured by
tests/test_dense_refine_ref_cpu.py): the key's factors (relative), L, the maps after 1, 2 and 10 steps.  Labels are compared
outside the fragile set (float64 top-two margin in (0, FRAGILE_T10 = 2.9e-5)); conf is held to the map bound and the class sums
to C x the map bound.  Every test prints the device's figures beside the bounds; DESIGN.md 6.32 lists them.
Measured on the MI355X, the largest over the four guides (its bound in brackets):
  case                  factors            L                  1 step             T = 2              T = 10
  1x1x1x1 (1)           0 (0)              5.7e-9 (2.3e-8)    2.2e-16 (8.9e-16)
  1x3x5x7 default       2.1e-7 (4.6e-7)    7.9e-7 (1.1e-6)    9.7e-7 (1.7e-6)
  2x3x33x65 (1, 2)      2.3e-7 (7.2e-7)    1.5e-6 (6.2e-6)    5.2e-7 (2.3e-6)    7.6e-7 (3.7e-6)    3.2e-6 (1.4e-5)
  1x9x70x97 default     2.3e-7 (7.3e-7)    1.4e-6 (3.9e-6)    9.2e-7 (2.0e-6)    8.6e-7 (2.4e-6)    3.7e-6 (8.3e-6)
  1x2x40x31 (3)         2.4e-7 (7.7e-7)    1.8e-6 (7.0e-6)    6.0e-7 (2.0e-6)
  1x255x9x9 (24)        1.7e-7 (5.8e-7)    8.7e-7 (4.8e-6)    7.7e-8 (5.3e-7)
  wrong labels 0 in every T = 2 / T = 10 run; segment_photo(...).refine after 10 iterations 4.0e-6 (8.3e-6).
Tile: 32 x 32, so the 33 x 65, 70 x 97 and 40 x 31 cases run one past a tile, several tiles and one below a tile."""
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
import dense_refine_ref as RR  # noqa: E402
import dense_stitch_ref as SR  # noqa: E402

GUARD = 64


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


def _prepare(guide, ds):
    kbuf, key = _guarded((*guide.shape[:3], 4), torch.float32, -7.0)
    _ops().dense_refine_prepare(guide, ds, key)
    torch.cuda.synchronize()
    assert _intact(kbuf, -7.0)
    return key


def _step(m, guide, key, ds):
    obuf, out = _guarded(tuple(m.shape), torch.float32, -7.0)
    _ops().dense_refine_step(m, out, guide, key, ds)
    torch.cuda.synchronize()
    assert _intact(obuf, -7.0)
    return out


def _device_run(maps, guide, ds, ts):
    """the device's results in the form dense_refine_ref.errors takes, from guarded buffers"""
    m, g = maps.cuda(), guide.cuda()
    key = _prepare(g, ds)
    out = {"key": {"factors": key[..., :3].cpu(), "L": key[..., 3].cpu()}}
    for t in range(1, max(ts) + 1):
        m = _step(m, g, key, ds)
        if t in ts:
            out[t] = m.cpu()
    return out, key


_REF = {}


def _reference(i, kind):
    """float64 results of a shared case, computed once"""
    if (i, kind) not in _REF:
        maps, guide, ds = RR.case_inputs(i, kind)
        ts = (1,) + (RR.LONG_T if i in RR.LONG_CASES else ())
        _REF[(i, kind)] = (maps, guide, ds, ts, RR.refine_ref(maps, guide, ds, max(ts), keep=ts))
    return _REF[(i, kind)]


# ---- 1. exact identities -------------------------------------------------------------------------
def _stitch_both(probs, boxes, H, W, min_conf=0.0, photo=None, pal=None, a8=256):
    ops = _ops()
    p, bx = probs.cuda(), _boxes(boxes)
    C = probs.shape[1]
    lab, conf, cov = (torch.empty(H, W, device="cuda", dtype=dt) for dt in (torch.uint8, torch.float32, torch.uint8))
    ov = torch.empty(H, W, 3, device="cuda", dtype=torch.uint8)
    ops.dense_stitch(p, bx, H, W, lab, conf, min_conf=min_conf, cover=cov, overlay=ov, palette=pal, photo=photo, alpha8=a8)
    mbuf, maps = _guarded((C, H, W), torch.float32, -7.0)
    vbuf, cov2 = _guarded((H, W), torch.uint8, 77)
    ops.dense_stitch_maps(p, bx, H, W, maps, cover=cov2)
    lbuf, lab2 = _guarded((1, H, W), torch.uint8, 77)
    cbuf, conf2 = _guarded((1, H, W), torch.float32, -7.0)
    obuf, ov2 = _guarded((1, H, W, 3), torch.uint8, 77)
    ops.dense_maps_label(maps[None], lab2, conf2, min_conf=min_conf, cover=cov2[None], overlay=ov2, palette=pal,
                         photo=None if photo is None else photo[None], alpha8=a8)
    torch.cuda.synchronize()
    assert _intact(mbuf, -7.0) and _intact(vbuf, 77) and _intact(lbuf, 77) and _intact(cbuf, -7.0) and _intact(obuf, 77)
    assert torch.equal(lab2[0], lab) and torch.equal(conf2[0], conf) and torch.equal(cov2, cov) and torch.equal(ov2[0], ov)
    covered = cov > 0
    assert torch.equal(maps.max(dim=0).values[covered], conf[covered])        # max_c of the stitched maps IS conf, bitwise
    assert bool((maps[:, ~covered] == 0).all())
    maps_b = torch.empty_like(maps)
    ops.dense_stitch_maps(p, bx, H, W, maps_b)                                # two calls, equal bytes; cover is optional
    lab3, conf3 = torch.empty_like(lab2), torch.empty_like(conf2)
    ops.dense_maps_label(maps[None], lab3, conf3, min_conf=min_conf, cover=cov2[None])
    assert torch.equal(maps_b, maps) and torch.equal(lab3, lab2) and torch.equal(conf3, conf2)
    return maps, cov


@pytest.mark.parametrize("case", [SR.STITCH_CASES[0], SR.STITCH_CASES[2], SR.STITCH_CASES[3]])
def test_stitch_maps_then_maps_label_is_dense_stitch(case):
    probs, boxes, H, W = SR.stitch_case(case)
    gen = torch.Generator().manual_seed(5)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    photo = torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).cuda()
    _stitch_both(probs, boxes, H, W, pal=pal)
    _stitch_both(probs, boxes, H, W, min_conf=0.5, photo=photo, pal=pal, a8=77)


def _path_case(name):
    """(probs, boxes, H, W, the cover to expect) of test_dense_stitch_gpu.py's path cases, generators and seeds as there: "forty"
    - 40 windows on a pixel, 36 of them through the recompute loop; "small" - K = 300, the LDS list; "columns" - K = 600 columns
    of the picture's height meet every band, 600 > 512: each group walks all K boxes from global memory"""
    if name == "forty":
        H, W, g, C = 30, 41, 3, 4
        rng = np.random.default_rng(15)
        boxes = np.array([[rng.integers(0, 15), rng.integers(0, 10), rng.integers(26, 42), rng.integers(20, 31)] for _ in range(40)])
        return SR.stitch_maps(40, C, g, seed=15), boxes, H, W, (40, 40)
    K = {"small": 300, "columns": 600}[name]
    H, W, g, C = 48, 64, 2, 3
    rng = np.random.default_rng(16)
    if name == "small":
        x0, y0 = rng.integers(-3, W - 2, K), rng.integers(-3, H - 2, K)
        boxes = np.stack([x0, y0, x0 + rng.integers(4, 13, K), y0 + rng.integers(4, 13, K)], axis=1)
    else:
        x0 = rng.integers(0, W - 1, K)
        boxes = np.stack([x0, np.zeros(K, dtype=np.int64), x0 + rng.integers(1, 3, K), np.full(K, H)], axis=1)
    return SR.stitch_maps(K, C, g, seed=16), boxes, H, W, (5, 64)


PATH_CASES = ("forty", "small", "columns")
_STITCH_REF = {}


def _stitch_reference(case):
    """(probs, boxes, H, W, float64 stitch_ref, its largest cover) of a STITCH_CASES entry or a path case, computed once; the
    reference is finite and its largest cover is what the case is there for"""
    if case not in _STITCH_REF:
        if case in PATH_CASES:
            probs, boxes, H, W, (lo, hi) = _path_case(case)
        else:
            probs, boxes, H, W = SR.stitch_case(case)
            lo, hi = 1, 6                                                     # the shared cases: what CONF_TOL alone was stated for
        ref = SR.stitch_ref(probs, torch.as_tensor(np.asarray(boxes)), H, W)
        nmax = int(ref["cover"].max())
        assert bool(torch.isfinite(ref["up"]).all()) and lo <= nmax <= hi, (case, nmax)
        _STITCH_REF[case] = (probs, boxes, H, W, ref, nmax)
    return _STITCH_REF[case]


@pytest.mark.parametrize("name", PATH_CASES)
def test_stitch_maps_identity_on_the_recompute_list_and_overflow_paths(name):
    probs, boxes, H, W, _ = _path_case(name)
    pal = torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    _stitch_both(probs, boxes, H, W, min_conf=0.3, pal=pal)


@pytest.mark.parametrize("case", [SR.STITCH_CASES[0], SR.STITCH_CASES[2], SR.STITCH_CASES[3], *PATH_CASES])
def test_stitch_maps_classes_against_float64(case):
    """every class of dense_stitch_maps against stitch_ref's "up" within CONF_TOL + (nmax - 1) 2^-24 (test_dense_stitch_gpu.py's
    _tol, nmax the reference's largest cover); cover exactly"""
    probs, boxes, H, W, ref, nmax = _stitch_reference(case)
    C = probs.shape[1]
    mbuf, maps = _guarded((C, H, W), torch.float32, -7.0)
    vbuf, cover = _guarded((H, W), torch.uint8, 77)
    _ops().dense_stitch_maps(probs.cuda(), _boxes(boxes), H, W, maps, cover=cover)
    torch.cuda.synchronize()
    assert _intact(mbuf, -7.0) and _intact(vbuf, 77)
    tol = R.CONF_TOL + (nmax - 1) * 2.0 ** -24
    err = (maps.double().cpu() - ref["up"]).abs().amax(dim=(1, 2))
    print(f"dense_stitch_maps {case}: cover up to {nmax}, max |du_c| per class {[f'{e:.2e}' for e in err.tolist()]} (bound {tol:.2e})")
    assert torch.equal(cover.cpu().long(), ref["cover"].clamp_max(255))
    assert float(err.max()) <= tol


def test_stitch_maps_with_hanging_boxes_and_an_uncovered_strip():
    gen = torch.Generator().manual_seed(6)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    H, W, g, C = 21, 34, 4, 3
    probs = SR.stitch_maps(2, C, g, seed=13)
    _stitch_both(probs, [[-5, -4, W + 3, H + 6], [-9, 3, 17, H + 40]], H, W, pal=pal)
    H, W = 30, 41
    probs = SR.stitch_maps(6, C, g, seed=14)
    boxes = [[0, 0, 16, 30], [8, 0, 24, 20], [3, 5, 20, 30], [28, 0, 41, 30], [26, 4, 40, 22], [0, 0, 10, 10]]      # columns 24, 25: none
    maps, cov = _stitch_both(probs, boxes, H, W, min_conf=0.3, pal=pal)
    assert bool((cov[:, 24:26] == 0).all()) and int(cov.max()) >= 3


def test_maps_label_without_cover_and_straddling_images():
    """B = 3 images of 5 x 7: a thread's four pixels straddle two images (35 is no multiple of 4)"""
    B, C, H, W = 3, 4, 5, 7
    maps = RR.make_maps(B, C, H, W, seed=9).cuda()
    lbuf, lab = _guarded((B, H, W), torch.uint8, 77)
    cbuf, conf = _guarded((B, H, W), torch.float32, -7.0)
    _ops().dense_maps_label(maps, lab, conf, min_conf=0.4)
    torch.cuda.synchronize()
    assert _intact(lbuf, 77) and _intact(cbuf, -7.0)
    best, arg = maps.max(dim=1)
    assert torch.equal(conf, best)
    assert torch.equal(lab.long(), torch.where(best < 0.4, torch.full_like(arg, 255), arg))


@pytest.mark.parametrize("i", [1, 2, 3])
def test_flat_guides_of_two_colours_give_equal_bytes(i):
    B, C, H, W, ds = RR.CASES[i]
    maps = RR.make_maps(B, C, H, W, seed=i).cuda()
    outs = []
    for colour in ([37, 200, 111], [0, 0, 0], [255, 3, 128]):
        g = torch.tensor(colour, dtype=torch.uint8).expand(B, H, W, 3).contiguous().cuda()
        key = _prepare(g, ds)
        outs.append((key.clone(), _step(maps, g, key, ds).clone()))
    for key, out in outs[1:]:
        assert torch.equal(key, outs[0][0]) and torch.equal(out, outs[0][1])
    N = 8 * len(ds)
    assert (outs[0][0][..., 3].double().cpu() - float(np.log(N))).abs().max() < 1e-6


# ---- 2. prepare and one step against float64 -------------------------------------------------------
@pytest.mark.parametrize("kind", RR.GUIDES)
@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_prepare_and_steps_against_float64(i, kind):
    """the key's factors (relative), L and the maps after one step - and, on the long cases, after T = 2 and T = 10 with their
    labels, conf and class sums - each within dense_refine_ref.BOUNDS[(i, kind)]"""
    maps, guide, ds, ts, ref = _reference(i, kind)
    got, key = _device_run(maps, guide, ds, ts)
    e = RR.errors(got, ref, ts)
    b = RR.BOUNDS[(i, kind)]
    print(f"dense_refine case {i} {RR.CASES[i]} guide {kind}: " + ", ".join(f"{k}: {v:.3e} (bound {b[k]:.3e})" for k, v in e.items()))
    again, key2 = _device_run(maps, guide, ds, ts)                            # two calls, equal bytes
    assert torch.equal(key, key2) and all(torch.equal(got[t], again[t]) for t in ts)
    C = maps.shape[1]
    for t in ts:
        if t == 1:
            continue
        lab = torch.empty(maps.shape[0], *maps.shape[2:], device="cuda", dtype=torch.uint8)
        conf = torch.empty(lab.shape, device="cuda")
        _ops().dense_maps_label(got[t].cuda(), lab, conf)
        lref = RR.label_ref(ref[t])
        wrong, share = RR.compare_labels(lab, lref, fragile=RR.FRAGILE_T10, conf_tol=0.0)
        cerr = (conf.double().cpu() - lref["conf"]).abs().max().item()
        serr = (got[t].double().sum(dim=1) - 1.0).abs().max().item()
        print(f"dense_refine case {i} guide {kind} T = {t}: wrong labels {wrong}, fragile share {share:.2e}, max |dconf| {cerr:.3e} "
              f"(bound {b[t]:.3e}), max |sum_c - 1| {serr:.3e} (bound {C * b[t]:.3e})")
        assert wrong == 0 and cerr <= b[t] and serr <= C * b[t]
    for k, v in e.items():
        assert v <= b[k], (k, v, b[k])


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_raw_library_argument_errors():
    from cclip_hip import load_library
    lib = load_library()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    B, C, H, W = 1, 2, 5, 7
    mbuf, m_in = _guarded((B, C, H, W), torch.float32, 0.25)
    obuf, m_out = _guarded((B, C, H, W), torch.float32, -7.0)
    kbuf, key = _guarded((B, H, W, 4), torch.float32, -7.0)
    guide = torch.zeros(B, H, W, 3, device="cuda", dtype=torch.uint8)
    ERR_ARG = 1

    def prepare(guide_p=guide.data_ptr(), B=B, H=H, W=W, ds=(1, 2), D=None, key_p=key.data_ptr(), ds_null=False):
        arr = (c_int * max(len(ds), 1))(*ds)
        return lib.cclip_dense_refine_prepare(c_void_p(guide_p), c_int(B), c_int(H), c_int(W), None if ds_null else arr,
                                              c_int(len(ds) if D is None else D), c_void_p(key_p), stream)

    def step(in_p=m_in.data_ptr(), out_p=m_out.data_ptr(), guide_p=guide.data_ptr(), key_p=key.data_ptr(), B=B, C=C, H=H, W=W, ds=(1, 2),
             D=None, ds_null=False):
        arr = (c_int * max(len(ds), 1))(*ds)
        return lib.cclip_dense_refine_step(c_void_p(in_p), c_void_p(out_p), c_void_p(guide_p), c_void_p(key_p), c_int(B), c_int(C),
                                           c_int(H), c_int(W), None if ds_null else arr, c_int(len(ds) if D is None else D), stream)

    bad_prepare = [dict(guide_p=0), dict(key_p=0), dict(ds_null=True), dict(B=0), dict(H=0), dict(H=16385), dict(W=0), dict(W=16385),
                   dict(ds=()), dict(ds=(1,) * 7), dict(ds=(1, 0)), dict(ds=(25,)), dict(key_p=key.data_ptr() + 4),
                   dict(key_p=key.data_ptr() + 8), dict(B=9, H=16384, W=16384)]
    for kw in bad_prepare:
        assert prepare(**kw) == ERR_ARG, kw
    bad_step = [dict(in_p=0), dict(out_p=0), dict(guide_p=0), dict(key_p=0), dict(ds_null=True), dict(C=0), dict(C=256), dict(B=0),
                dict(H=0), dict(W=16385), dict(ds=()), dict(ds=(1,) * 7), dict(ds=(0,)), dict(ds=(25,)), dict(out_p=m_in.data_ptr()),
                dict(out_p=m_in.data_ptr() + 8), dict(in_p=m_in.data_ptr() + 2), dict(key_p=key.data_ptr() + 4),
                dict(B=1, C=9, H=16384, W=16384), dict(B=2 ** 20, C=255, H=16, W=16)]      # B C H W past 2^31 - 1: arguments only
    for kw in bad_step:
        assert step(**kw) == ERR_ARG, kw
    maps_label = lambda **kw: lib.cclip_dense_maps_label(                     # noqa: E731
        c_void_p(kw.get("maps", m_in.data_ptr())), c_int(kw.get("B", B)), c_int(kw.get("C", C)), c_int(H), c_int(kw.get("W", W)), c_void_p(0),
        c_float(0.0), c_void_p(kw.get("labels", guide.data_ptr())), c_void_p(kw.get("conf", m_out.data_ptr())), c_void_p(0), c_void_p(0),
        c_int(kw.get("a8", 256)), c_void_p(kw.get("overlay", 0)), stream)
    for kw in [dict(maps=0), dict(labels=0), dict(conf=0), dict(C=0), dict(C=256), dict(B=0), dict(W=16385), dict(a8=257),
               dict(overlay=guide.data_ptr()), dict(maps=m_in.data_ptr() + 2), dict(B=2 ** 23, C=255)]:
        assert maps_label(**kw) == ERR_ARG, kw
    probs = torch.rand(1, C, 2, 2, device="cuda")
    box = _boxes([[0, 0, W, H]])
    stitch_maps = lambda **kw: lib.cclip_dense_stitch_maps(                   # noqa: E731
        c_void_p(kw.get("probs", probs.data_ptr())), c_int(kw.get("K", 1)), c_int(kw.get("C", C)), c_int(kw.get("g", 2)),
        c_void_p(kw.get("boxes", box.data_ptr())), c_int(kw.get("H", H)), c_int(kw.get("W", W)), c_void_p(kw.get("maps", m_out.data_ptr())),
        c_void_p(0), stream)
    for kw in [dict(probs=0), dict(boxes=0), dict(maps=0), dict(K=0), dict(K=65536), dict(C=0), dict(C=256), dict(g=0), dict(H=0),
               dict(W=16385), dict(maps=m_out.data_ptr() + 2), dict(C=9, H=16384, W=16384)]:
        assert stitch_maps(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert _intact(mbuf, 0.25) and _intact(obuf, -7.0) and _intact(kbuf, -7.0)
    assert bool((m_out == -7.0).all()) and bool((key == -7.0).all())           # nothing was launched
    assert prepare() == 0 and step() == 0 and maps_label() == 0 and stitch_maps() == 0
    torch.cuda.synchronize()


def test_wrapper_argument_errors():
    import clip
    ops = _ops()
    B, C, H, W = 1, 2, 5, 7
    m, out = torch.rand(B, C, H, W, device="cuda"), torch.empty(B, C, H, W, device="cuda")
    guide = torch.zeros(B, H, W, 3, device="cuda", dtype=torch.uint8)
    key = torch.empty(B, H, W, 4, device="cuda")
    lab, conf = torch.empty(B, H, W, device="cuda", dtype=torch.uint8), torch.empty(B, H, W, device="cuda")
    probs, box = torch.rand(1, C, 2, 2, device="cuda"), _boxes([[0, 0, W, H]])
    ops.dense_refine_prepare(guide, (1,), key)
    ops.dense_refine_step(m, out, guide, key, (1,))
    off = torch.empty(B * H * W * 4 + 1, device="cuda")[1:].view(B, H, W, 4)
    both = torch.empty(m.numel() + 4, device="cuda")                          # two maps that share all but four values
    cases = [
        ("guide must be a cuda tensor", lambda: ops.dense_refine_prepare(guide.cpu(), (1,), key)),
        ("guide must be torch.uint8", lambda: ops.dense_refine_prepare(guide.float(), (1,), key)),
        ("key must be \\[1, 5, 7, 4\\]", lambda: ops.dense_refine_prepare(guide, (1,), key.view(B, W, H, 4))),
        ("16-byte boundary", lambda: ops.dense_refine_prepare(guide, (1,), off)),
        ("0 dilations", lambda: ops.dense_refine_prepare(guide, (), key)),
        ("two buffers", lambda: ops.dense_refine_step(m, m, guide, key, (1,))),
        ("overlap", lambda: ops.dense_refine_step(both[:m.numel()].view(m.shape), both[4:].view(m.shape), guide, key, (1,))),
        ("maps_out must be \\[1, 2, 5, 7\\]", lambda: ops.dense_refine_step(m, out.view(B, C, W, H), guide, key, (1,))),
        ("guide must be \\[1, 5, 7, 3\\]", lambda: ops.dense_refine_step(m, out, guide.view(B, W, H, 3), key, (1,))),
        ("maps_in must be torch.float32", lambda: ops.dense_refine_step(m.double(), out, guide, key, (1,))),
        ("256 classes", lambda: ops.dense_refine_step(torch.empty(1, 256, 2, 2, device="cuda"), torch.empty(1, 256, 2, 2, device="cuda"),
                                                      guide[:, :2, :2].contiguous(), key[:, :2, :2].contiguous(), (1,))),
        ("dilation 25", lambda: ops.dense_refine_step(m, out, guide, key, (25,))),
        ("maps must be \\[B, C, H, W\\]", lambda: ops.dense_maps_label(m[0], lab, conf)),
        ("labels must be \\[1, 5, 7\\]", lambda: ops.dense_maps_label(m, lab[0], conf)),
        ("cover must be torch.uint8", lambda: ops.dense_maps_label(m, lab, conf, cover=conf)),
        ("give overlay too", lambda: ops.dense_maps_label(m, lab, conf, palette=torch.zeros(256, 3, device="cuda", dtype=torch.uint8))),
        ("maps must be \\[2, 5, 7\\]", lambda: ops.dense_stitch_maps(probs, box, H, W, out)),
        ("boxes must be torch.int32", lambda: ops.dense_stitch_maps(probs, box.long(), H, W, out[0])),
        ("cover must be \\[5, 7\\]", lambda: ops.dense_stitch_maps(probs, box, H, W, out[0], cover=lab)),
        ("iterations must be an integer", lambda: clip.refine_maps(m, guide, iterations=0)),
    ]
    for match, fn in cases:
        with pytest.raises(ValueError, match=match):
            fn()


# ---- 6. the Python surface -------------------------------------------------------------------------
def _toy(grid, dtype=torch.bfloat16, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)
    return geo, clip.build_model(init_state_dict(geo, seed), dtype).cuda().eval()


def test_refine_maps_is_prepare_and_steps_and_leaves_its_input():
    import clip
    maps, guide, ds, ts, ref = _reference(2, "noise")
    m = maps.cuda()
    keep = m.clone()
    out = clip.refine_maps(m, guide.cuda(), dilations=ds, iterations=2)
    got, _ = _device_run(maps, guide, ds, (2,))
    assert torch.equal(m, keep) and out.shape == m.shape and torch.equal(out.cpu(), got[2])
    one = clip.refine_maps(m[1], guide[1].cuda(), dilations=ds, iterations=2)           # [C, H, W] in, the same out; images apart
    assert one.shape == m.shape[1:] and torch.equal(one, out[1])
    assert torch.equal(clip.refine_maps(m, guide.cuda(), dilations=ds, iterations=1).cpu(), _device_run(maps, guide, ds, (1,))[0][1])


def test_segment_refine_surface():
    import clip
    from clip.weights import synthetic_images
    geo, model = _toy(3)
    img = synthetic_images(2, geo, 4).cuda()
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    pal = clip.default_palette(4)
    for size in (40, (29, 43)):
        res = clip.segment(model, img, text, size=size, min_conf=0.3)
        H, W = res.labels.shape[1:]
        photo = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
        ref = res.refine(photo, iterations=3, dilations=(1, 2, 4))
        assert isinstance(ref, clip.RefinedDenseResult) and ref.dilations == (1, 2, 4) and ref.iterations == 3 and ref.min_conf == 0.3
        assert ref.maps.shape == (2, 4, H, W) and ref.maps.dtype == torch.float32
        assert ref.labels.shape == (2, H, W) and ref.labels.dtype == torch.uint8 and ref.conf.shape == (2, H, W) and ref.conf.dtype == torch.float32
        assert torch.equal(ref.conf, ref.maps.max(dim=1).values)
        assert torch.equal(ref.overlay().cpu(), R.overlay_ref(ref.labels, pal))
        assert torch.equal(ref.overlay(photo=photo, alpha=0.25).cpu(), R.overlay_ref(ref.labels, pal, photo, 64))
        fr = ref.area_fractions()
        assert fr.shape == (2, 5) and (fr.sum(dim=1) - 1.0).abs().max() < 1e-12 and len(ref.top_class()) == 2
        comps = ref.components()
        assert comps.n >= 1 and len(ref.instances()) == comps.n
        # the maps it started from are the stitch's: zero iterations are not offered, so compare the initialiser by hand
        maps0 = torch.empty(4, H, W, device="cuda")
        _ops().dense_stitch_maps(res.probs[:1], _boxes([[0, 0, W, H]]), H, W, maps0)
        lab0, conf0 = torch.empty(1, H, W, device="cuda", dtype=torch.uint8), torch.empty(1, H, W, device="cuda")
        _ops().dense_maps_label(maps0[None], lab0, conf0, min_conf=0.3)
        assert torch.equal(lab0[0], res.labels[0]) and torch.equal(conf0[0], res.conf[0])
        with pytest.raises(ValueError, match="overlay: photo must be"):
            res.refine(photo[:, :-1])
        with pytest.raises(ValueError, match="overlay: photo must be a uint8 tensor"):
            res.refine(photo.float())


def test_segment_photo_refine_surface():
    import clip
    geo, model = _toy(2)
    photo = torch.randint(0, 256, (45, 61, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    res = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=4)
    keep = (res.labels.clone(), res.conf.clone(), res.cover.clone())
    ref = res.refine(photo, min_conf=0.2)
    assert ref.maps.shape == (4, 45, 61) and ref.labels.shape == (45, 61) and ref.conf.shape == (45, 61) and ref.min_conf == 0.2
    assert ref.dilations == RR.DEFAULT_DILATIONS and ref.iterations == 10
    assert torch.equal(ref.conf, ref.maps.max(dim=0).values)
    assert torch.equal(res.labels, keep[0]) and torch.equal(res.conf, keep[1]) and torch.equal(res.cover, keep[2])
    pal = clip.default_palette(4)
    assert torch.equal(ref.overlay().cpu(), R.overlay_ref(ref.labels, pal))
    assert torch.equal(ref.overlay(photo=photo, alpha=0.25).cpu(), R.overlay_ref(ref.labels, pal, photo, 64))
    assert ref.area_fractions().shape == (5,) and (ref.top_class() is None or 0 <= ref.top_class() < 4)
    comps = ref.components(connectivity=8)
    assert comps.n >= 1 and len(ref.instances(connectivity=8)) == comps.n
    maps0 = torch.empty(4, 45, 61, device="cuda")                              # against float64 from the stitched maps on
    _ops().dense_stitch_maps(res.probs, _boxes(res.boxes.numpy()), 45, 61, maps0)
    want = RR.refine_ref(maps0.cpu()[None], photo[None], RR.DEFAULT_DILATIONS, 10)[10][0]
    err = (ref.maps.double().cpu() - want).abs().max().item()
    print(f"segment_photo(...).refine: max |dm| after 10 iterations {err:.3e}")
    assert err <= RR.BOUNDS[(3, "noise")][10]                                # the shared case of the same dilations, T and kind of guide
    with pytest.raises(ValueError, match="overlay: photo must be \\[45, 61, 3\\]"):
        res.refine(photo[:44])


def _script(*args):
    """the script as a fresh child process: its JSON lines, without the temporary file names"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "segment_images.py"), "--synthetic", "--n_images", "2", *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    for line in lines:
        line["file"] = os.path.basename(line["file"])
    return lines


def test_segment_images_script_with_refine(tmp_path):
    base = ["--window", "224", "--stride", "112", "--instances"]
    plain = _script(*base)
    refined = _script(*base, "--refine", "--refine-iterations", "3", "--refine-dilations", "1", "2", "4", "--png", str(tmp_path / "maps"))
    assert len(refined) == 2 and len(plain) == 2 and all("refine" not in line for line in plain)
    from PIL import Image
    for line, was in zip(refined, plain):
        assert line["refine"] == {"iterations": 3, "dilations": [1, 2, 4]}
        assert abs(sum(line["area"]) - 1.0) < 1e-5 and len(line["area"]) == len(line["classes"]) + 1
        assert line["top_class"] in line["classes"] and isinstance(line["instances"], list) and line["instances"]
        assert all(set(r) == {"class", "name", "box", "area", "score"} for r in line["instances"])
        assert [line[k] for k in ("file", "width", "height", "windows", "classes")] == [was[k] for k in ("file", "width", "height", "windows", "classes")]
        assert Image.open(line["png"]).size == (line["width"], line["height"])
    small = _script("--refine", "--refine-iterations", "2")                   # the batch path (clip.segment) under the same flag
    assert len(small) == 2 and all(line["refine"]["iterations"] == 2 and abs(sum(line["area"]) - 1.0) < 1e-5 for line in small)


def test_segment_images_script_without_refine_is_segment_photo(tmp_path):
    """without the flag the script prints what clip.segment_photo returns directly, made here the way the script makes it"""
    import clip
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import segment_images as S
    lines = _script("--window", "224", "--stride", "112", "--instances")
    C.make_synthetic_annotations(str(tmp_path), per_class=1 + (2 - 1) // len(C.CLASSES))
    d = os.path.join(str(tmp_path), "images")
    files = [os.path.join(d, f) for f in sorted(os.listdir(d))][:2]
    model, _ = clip.load("test-tiny", device=torch.device("cuda:0"), jit=False)
    model.eval()
    args = S.build_parser().parse_args(["--synthetic", "--window", "224", "--stride", "112", "--instances"])
    prompts = S.class_prompts(args)
    with torch.no_grad():
        text = model.encode_text(C.get_tokenize(model)(prompts).to("cuda:0")).float()
    assert [line["file"] for line in lines] == [os.path.basename(f) for f in files]
    for line, f in zip(lines, files):
        res = clip.segment_photo(model, Image.open(f).convert("RGB"), text, window=224, stride=112, batch=args.bs)
        top = res.top_class()
        assert line["area"] == [round(v, 6) for v in res.area_fractions().tolist()]
        assert line["top_class"] == (None if top is None else prompts[top]) and line["mean_conf"] == round(float(res.conf.mean()), 5)
        assert (line["windows"], line["height"], line["width"]) == (int(res.boxes.shape[0]), *res.labels.shape)
        assert line["instances"] == S.instance_records(res.components(4), args, prompts)
        assert set(line) == {"file", "classes", "area", "top_class", "mean_conf", "windows", "height", "width", "instances"}


# ---- 7. behaviour: the labels follow the photo's edge ----------------------------------------------
def test_refinement_moves_a_vertical_band_to_the_diagonal_edge():
    """64 x 96, two flat colours split by a diagonal; class maps from a 4 x 6 grid whose boundary is a vertical band.  Before:
    0.75 of the pixels carry their colour region's label.  After 10 default iterations the float64 reference reaches 0.84928;
    the device must gain at least DIAGONAL_MARGIN = 0.09."""
    import clip
    maps, guide, truth = RR.diagonal_case()
    lab0 = torch.empty(1, 64, 96, device="cuda", dtype=torch.uint8)
    conf = torch.empty(1, 64, 96, device="cuda")
    _ops().dense_maps_label(maps.cuda(), lab0, conf)
    before = RR.agreement(lab0, truth)
    out = clip.refine_maps(maps.cuda(), guide.cuda())
    lab1 = torch.empty_like(lab0)
    _ops().dense_maps_label(out, lab1, conf)
    after = RR.agreement(lab1, truth)
    print(f"diagonal case on the device: agreement before {before:.5f}, after {after:.5f}")
    assert before == RR.DIAGONAL_BEFORE
    assert after - before >= RR.DIAGONAL_MARGIN
