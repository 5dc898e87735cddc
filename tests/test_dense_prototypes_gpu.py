"""GPU: the dense class prototypes (csrc/dense_prototypes.hip, ops.dense_prototypes, clip.DensePrototypes) on the MI355X against
the numpy reference of tests/dense_prototypes_ref.py.  Every native call writes into guarded buffers pre-filled with junk
(accumulate == 0 must set them), the guards are checked, and every case runs twice for equal bytes.  patches, pixels and bad are
compared for exact equality; sums and weight per element against float64 with the derived bounds
  |sums[c][e] - ref| <= 2^-24 (n_c + E / 2 + 8) sum_p w_pc |f^_pe| + 1e-30      |weight[c] - ref| <= 2^-24 (n_c + 2) sum_p w_pc
(n_c = patches[c]: any summation order of n_c terms; E / 2: the E-term sum of squares under the root; 8: the roundings of weight,
reciprocal, product and one accumulate add).  tests/test_dense_prototypes_ref_cpu.py shows these bounds trip on planted faults.

End to end on the toy tower (random weights, two flat textures): measured on the MI355X,
  mIoU with fitted prototypes 1.000000, blended with text (0.3) 1.000000, with text prompts 0.125000 (the test prints
  them; nothing is asserted beyond their being finite - with random toy weights no ordering can be derived in advance)."""
from __future__ import annotations

import functools
import math
import os
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

ROOT = os.path.dirname(HERE)
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "construction-clip_amd")) if p not in sys.path]

import dense_prototypes_ref as PR  # noqa: E402
from cclip_hip.ops import dense_prototypes  # noqa: E402,F401  (the file is about the feature: without it, no collection)
from clip import DensePrototypes  # noqa: E402,F401

GUARD = 64
JUNK_I, JUNK_F = -77, -1234.5
INT_KEYS, ALL_KEYS = ("patches", "pixels", "bad"), ("sums", "weight", "patches", "pixels", "bad")


def _ops():
    from cclip_hip import ops
    return ops


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _outputs(C, E):
    return {"sums": _guarded((C, E), torch.float32, JUNK_F), "weight": _guarded((C,), torch.float32, JUNK_F),
            "patches": _guarded((C,), torch.int64, JUNK_I), "pixels": _guarded((C,), torch.int64, JUNK_I),
            "bad": _guarded((1,), torch.int64, JUNK_I)}


def _feat_dev(feat_np, pad=0):
    f = torch.from_numpy(feat_np).cuda()
    if pad:
        wide = torch.full((f.shape[0], f.shape[1] + pad), 9.0e9, device="cuda")
        wide[:, :f.shape[1]] = f
        f = wide[:, :f.shape[1]]
        assert f.stride(0) == feat_np.shape[1] + pad
    return f


def _run(feat, masks, boxes, g, C, s8, outs, image=None, accumulate=False):
    _ops().dense_prototypes(feat, masks, boxes, g, C, s8, *(outs[k][1] for k in ALL_KEYS), image=image, accumulate=accumulate)
    torch.cuda.synchronize()
    for k in ALL_KEYS:
        assert _intact(outs[k][0], JUNK_F if k in ("sums", "weight") else JUNK_I), k
    return {k: outs[k][1].cpu().numpy() for k in ALL_KEYS}


def _device(case, masks=None, order=None):
    boxes, image, feat = case["boxes"], case["image"], case["feat"]
    g = case["g"]
    if order is not None:
        boxes = boxes[order]
        image = None if image is None else image[order]
        feat = feat.reshape(len(order), g * g, -1)[order].reshape(feat.shape)
    masks = torch.from_numpy(case["masks"]).cuda() if masks is None else masks
    img = None if image is None else torch.from_numpy(image.astype(np.int32)).cuda()
    return _run(_feat_dev(feat, case["ldf_pad"]), masks, torch.from_numpy(boxes.astype(np.int32)).cuda(), g, case["C"], case["min_share8"],
                _outputs(case["C"], feat.shape[1]), image=img)


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = PR.CASES[name]
    return PR.reference(c["feat"], c["masks"], c["boxes"], c["g"], c["C"], c["min_share8"], c["image"])


def _check(got, ref, tag, n=None):
    for k in INT_KEYS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), f"{tag}: {k} {got[k].tolist()} != {ref[k].tolist()}"
    es = np.abs(got["sums"].astype(np.float64) - ref["sums"])
    ew = np.abs(got["weight"].astype(np.float64) - ref["weight"])
    bs, bw = PR.sums_bound(ref, n), PR.weight_bound(ref, n)
    print(f"{tag}: max |dsums| / bound {np.max(es / bs):.3f}, max |dweight| {ew.max():.3e} (bound {bw.max():.3e})")
    assert (es <= bs).all(), f"{tag}: sums off by {es.max():.3e} at {np.unravel_index(np.argmax(es - bs), es.shape)}"
    assert (ew <= bw).all(), f"{tag}: weight off by {ew.max():.3e}"
    dead = ref["patches"] == 0                                # a class nothing contributes to: exactly 0
    assert not got["sums"][dead].any() and not got["weight"][dead].any()


# ---- 1. the cases against the reference --------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_cases_against_the_reference(name):
    got = _device(PR.CASES[name])
    _check(got, _ref(name), name)
    again = _device(PR.CASES[name])
    assert all(got[k].tobytes() == again[k].tobytes() for k in ALL_KEYS)       # two calls, equal bytes


def test_known_answers_on_the_device():
    t = {s: _device(PR.CASES[f"threshold_{s}"]) for s in (128, 129, 0, 256, 64)}
    assert t[128]["patches"].tolist() == [2, 2, 1] and t[129]["patches"].tolist() == [1, 1, 1] and t[0]["patches"].tolist() == [3, 3, 2]
    assert t[256]["patches"].tolist() == [0, 0, 1] and t[64]["patches"].tolist() == [3, 2, 1]
    assert t[64]["weight"].tolist() == [0.5 + 15 / 16 + 0.25, 0.5 + 9 / 16, 1.0]
    ig = _device(PR.CASES["mask_all_ignore"])
    assert not any(ig[k].any() for k in ALL_KEYS)
    bad = _device(PR.CASES["batch_image_bad"])                                  # image -1 and image B contribute nothing: window 1 alone
    c = PR.CASES["batch_image_bad"]
    only = PR.reference(c["feat"][9:18], c["masks"], c["boxes"][1:2], 3, 3, c["min_share8"], image=np.array([1]))
    _check(bad, only, "image out of range")
    z = _device(PR.CASES["zero_row"])
    assert np.array_equal(z["patches"], _ref("zero_row")["patches"])


@pytest.mark.parametrize("name", ["boxes_edges", "accumulate", "batch_image_101", "cells_65"])
def test_window_order_does_not_change_the_integers(name):
    case = PR.CASES[name]
    K = case["boxes"].shape[0]
    order = np.random.default_rng(3).permutation(K)
    a, b = _device(case), _device(case, order=order)
    assert all(np.array_equal(a[k], b[k]) for k in INT_KEYS)
    _check(b, _ref(name), name + " permuted")


@pytest.mark.parametrize("name", ["g3_side10", "mask_values", "large_cell", "batch_image_101"])
def test_masks_one_byte_into_their_allocation(name):
    m = PR.CASES[name]["masks"]
    dev = torch.empty(m.size + 1, device="cuda", dtype=torch.uint8)[1:].view(m.shape)
    dev.copy_(torch.from_numpy(m))
    assert dev.data_ptr() % 4 == 1
    _check(_device(PR.CASES[name], masks=dev), _ref(name), name + " offset mask")


def test_accumulate_equals_one_call_over_all_windows():
    c = PR.CASES["accumulate"]
    g, C, E = c["g"], c["C"], c["feat"].shape[1]
    masks = torch.from_numpy(c["masks"]).cuda()
    boxes = torch.from_numpy(c["boxes"].astype(np.int32)).cuda()
    feat = torch.from_numpy(c["feat"]).cuda()
    outs = _outputs(C, E)
    first = _run(feat[:2 * g * g], masks, boxes[:2].contiguous(), g, C, c["min_share8"], outs)                   # sets, over the junk
    _check(first, PR.reference(c["feat"][:2 * g * g], c["masks"], c["boxes"][:2], g, C, c["min_share8"]), "first call")
    both = _run(feat[2 * g * g:], masks, boxes[2:].contiguous(), g, C, c["min_share8"], outs, accumulate=True)
    one = _device(c)
    assert all(np.array_equal(both[k], one[k]) for k in INT_KEYS)
    _check(both, _ref("accumulate"), "two calls", n=_ref("accumulate")["patches"])


# ---- 2. refusals -------------------------------------------------------------------------------------
def test_raw_library_argument_errors():
    from cclip_hip import load_library
    lib = load_library()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    K, g, C, E, B, H, W = 2, 3, 3, 8, 2, 9, 11
    feat = torch.randn(K * g * g, E + 4, device="cuda")
    masks = torch.zeros(B * H * W + 8, device="cuda", dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 11, 9], [1, 1, 8, 8], [0, 0, 1, 1]], device="cuda", dtype=torch.int32)
    image = torch.tensor([0, 1, 0, 0], device="cuda", dtype=torch.int32)
    outs = _outputs(C, E)
    need = _ops().dense_prototypes_workspace(K, g, C, E)
    ws = torch.full((need + 64,), 7, device="cuda", dtype=torch.uint8)
    ERR_ARG = 1
    ptr = {k: outs[k][1].data_ptr() for k in ALL_KEYS}
    good = dict(feat=feat.data_ptr(), ldf=E + 4, masks=masks.data_ptr(), boxes=boxes.data_ptr(), image=image.data_ptr(), K=K, g=g, C=C, E=E,
                B=B, H=H, W=W, s8=128, acc=0, ws=ws.data_ptr(), ws_bytes=need, **ptr)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cclip_dense_prototypes(c_void_p(a["feat"]), c_int64(a["ldf"]), c_void_p(a["masks"]), c_void_p(a["boxes"]), c_void_p(a["image"]),
                                          c_int(a["K"]), c_int(a["g"]), c_int(a["C"]), c_int(a["E"]), c_int(a["B"]), c_int(a["H"]), c_int(a["W"]),
                                          c_int(a["s8"]), c_int(a["acc"]), c_void_p(a["sums"]), c_void_p(a["weight"]), c_void_p(a["patches"]),
                                          c_void_p(a["pixels"]), c_void_p(a["bad"]), c_void_p(a["ws"]), c_int64(a["ws_bytes"]), stream)

    refused = [dict(feat=0), dict(masks=0), dict(boxes=0), dict(sums=0), dict(weight=0), dict(patches=0), dict(pixels=0), dict(bad=0), dict(ws=0),
               dict(K=0), dict(K=65536), dict(C=0), dict(C=256), dict(g=0), dict(g=16385), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385),
               dict(B=0), dict(B=8, H=16384, W=16384), dict(B=1 << 30, H=2, W=1),
               dict(E=0), dict(E=6), dict(E=1028), dict(ldf=E - 4), dict(ldf=E + 2), dict(feat=feat.data_ptr() + 4),
               dict(sums=ptr["sums"] + 2), dict(weight=ptr["weight"] + 2), dict(boxes=boxes.data_ptr() + 2), dict(image=image.data_ptr() + 2),
               dict(patches=ptr["patches"] + 4), dict(pixels=ptr["pixels"] + 4), dict(bad=ptr["bad"] + 4),
               dict(ldf=1 << 62), dict(ldf=((1 << 62) // (K * g * g) + 4) & ~3), dict(s8=-1), dict(s8=257), dict(acc=2), dict(acc=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ws.data_ptr() + 8),
               dict(weight=ptr["sums"] + 4), dict(pixels=ptr["patches"]), dict(bad=ptr["pixels"] + 8), dict(patches=ptr["bad"]),   # output | output
               dict(ws=ptr["sums"] - 16), dict(sums=feat.data_ptr() + 16), dict(weight=boxes.data_ptr() + 4), dict(bad=image.data_ptr()),
               dict(patches=masks.data_ptr() + 8), dict(ws=feat.data_ptr())]                                                         # output | input
    for accumulate in (0, 1):
        for kw in refused:
            assert call(**dict(dict(acc=accumulate), **kw)) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert all(bool((outs[k][0] == (JUNK_F if k in ("sums", "weight") else JUNK_I)).all()) for k in ALL_KEYS)      # nothing written
    assert bool((ws == 7).all())
    assert call() == 0 and call(image=0) == 0 and call(masks=masks.data_ptr() + 1) == 0
    torch.cuda.synchronize()
    assert outs["pixels"][1].tolist() == [H * W + 49, 0, 0] and outs["bad"][1].item() == 0
    assert all(_intact(outs[k][0], JUNK_F if k in ("sums", "weight") else JUNK_I) for k in ALL_KEYS) and bool((ws[need:] == 7).all())


def test_wrapper_argument_errors():
    ops = _ops()
    C, E, g = 3, 8, 3
    feat = torch.randn(9, E, device="cuda")
    masks = torch.zeros(1, 9, 11, device="cuda", dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 11, 9]], device="cuda", dtype=torch.int32)
    o = {k: v[1] for k, v in _outputs(C, E).items()}

    def dp(feat=feat, masks=masks, boxes=boxes, g=g, C=C, s8=128, **kw):
        out = dict(o, **{k: kw.pop(k) for k in list(kw) if k in ALL_KEYS})
        return ops.dense_prototypes(feat, masks, boxes, g, C, s8, *(out[k] for k in ALL_KEYS), **kw)

    dp()
    cases = [("feat must be a cuda tensor", lambda: dp(feat=feat.cpu())), ("masks must be torch.uint8", lambda: dp(masks=masks.int())),
             ("boxes must be torch.int32", lambda: dp(boxes=boxes.long())), ("feat must be 2-D with inner stride 1", lambda: dp(feat=feat.t())),
             ("grid must be an integer", lambda: dp(g=0)), ("n_classes must be an integer in \\[1, 255\\]", lambda: dp(C=256)),
             ("min_share8 must be an integer in \\[0, 256\\]", lambda: dp(s8=257)), ("min_share8 must be an integer", lambda: dp(s8=0.5)),
             ("feat has embedding width 6", lambda: dp(feat=torch.randn(9, 6, device="cuda"))), ("feat has 9 rows", lambda: dp(g=2)),
             ("masks must be \\[B, H, W\\]", lambda: dp(masks=masks[0])), ("boxes must be \\[1, 4\\]", lambda: dp(boxes=boxes.repeat(2, 1))),
             ("image must be \\[1\\]", lambda: dp(image=torch.zeros(2, device="cuda", dtype=torch.int32))),
             ("image must be torch.int32", lambda: dp(image=torch.zeros(1, device="cuda", dtype=torch.int64))),
             ("sums must be \\[3, 8\\]", lambda: dp(sums=torch.zeros(3, 4, device="cuda"))),
             ("patches must be torch.int64", lambda: dp(patches=torch.zeros(3, device="cuda", dtype=torch.int32))),
             ("bad must be a cuda tensor", lambda: dp(bad=torch.zeros(1, dtype=torch.int64))),
             ("workspace must be a uint8 or float32 tensor of at least", lambda: dp(workspace=torch.zeros(16, device="cuda", dtype=torch.uint8))),
             ("workspace must be a contiguous cuda tensor", lambda: dp(workspace=torch.zeros(4096, dtype=torch.uint8))),
             ("height 1, width 16385", lambda: dp(masks=torch.zeros(1, 1, 16385, device="cuda", dtype=torch.uint8)))]
    for match, fn in cases:
        with pytest.raises(ValueError, match="dense_prototypes: " + match):
            fn()
    dp(workspace=torch.empty(ops.dense_prototypes_workspace(1, g, C, E) // 4, device="cuda"))               # a float32 workspace of the exact size


# ---- 3. behaviour with planted features ----------------------------------------------------------------
def test_planted_centres_are_recovered_and_label_their_cells():
    """E = 64, features centre_c + 0.05 noise (noise ~ N(0, I)), centres random unit vectors.  A unit feature is the centre plus a
    perpendicular part of length about 0.05 sqrt(63) = 0.40, so one cell has cosine about 1 / sqrt(1 + 0.16) = 0.93 to its centre.
    The prototype averages n >= 40 cells per class: the centre parts add up coherently (n x 0.93), the noise parts like
    0.40 x 0.93 sqrt(n), so the prototype's cosine is 1 / sqrt(1 + 0.16 / n) >= 1 / sqrt(1.004) = 0.998 - the floor 0.99 leaves a
    factor four in the noise energy.  Between classes, random unit centres at E = 64 have |cosine| about 1 / 8, far below 0.93."""
    import clip
    C, E, g, K, cell = 4, 64, 8, 3, 5
    rng = np.random.default_rng(77)
    centres = rng.standard_normal((C, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    H = W = g * cell
    cls = rng.integers(0, C, size=(K, g, g))                                    # constant per cell
    masks = np.repeat(np.repeat(cls, cell, axis=1), cell, axis=2).astype(np.uint8)
    assert min(np.bincount(cls.ravel(), minlength=C)) >= 40
    feat = (centres[cls.reshape(-1)] + 0.05 * rng.standard_normal((K * g * g, E))).astype(np.float32)
    p = clip.DensePrototypes(C, E, min_share=1.0)
    boxes = np.tile(np.array([[0, 0, W, H]]), (K, 1))
    p.add_features(torch.from_numpy(feat).cuda().view(K, g, g, E), torch.from_numpy(masks).cuda(), boxes, g, image=np.arange(K))
    assert p.patches.tolist() == np.bincount(cls.ravel(), minlength=C).tolist() and p.pixels.sum().item() == K * H * W and p.bad.item() == 0
    protos = p.features()
    cos = (protos.double().cpu().numpy() * centres).sum(axis=1)
    print(f"planted centres: cosines {np.round(cos, 5).tolist()}")
    assert (cos >= 0.99).all()
    probs = torch.empty(K, C, g * g, device="cuda")
    _ops().dense_class_probs(torch.from_numpy(feat).cuda(), protos, 100.0, g * g, probs)
    assert np.array_equal(probs.argmax(dim=1).cpu().numpy().reshape(K, g, g), cls)     # every pure cell takes its own class


# ---- 4. end to end on the toy tower ------------------------------------------------------------------
def _toy(grid, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)
    return geo, clip.build_model(init_state_dict(geo, seed), torch.bfloat16).cuda().eval()


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ALL_KEYS)


def test_add_equals_add_features_on_the_same_features():
    import clip
    from clip.weights import synthetic_images
    geo, model = _toy(3)
    img = synthetic_images(2, geo, 4).cuda()
    before = model.encode_image(img).clone()
    masks = torch.randint(0, 3, (2, 50, 71), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    masks[:, :, 30:34] = 255
    a = clip.DensePrototypes(3, geo.embed_dim, min_share=0.3).add(model, img, masks.cuda())
    feats = model.encode_image_dense(img)
    b = clip.DensePrototypes(3, geo.embed_dim, min_share=0.3)
    b.add_features(feats, masks.cuda(), np.array([[0, 0, 71, 50]] * 2), 3, image=[0, 1])
    assert _same(a, b) and a.patches.sum().item() > 0 and a.pixels.sum().item() == int((masks != 255).sum())
    res = clip.segment(model, img, a.features())
    assert isinstance(res, clip.DenseResult) and res.n_classes == 3
    assert torch.equal(model.encode_image(img), before)                          # the pooled path is untouched
    with pytest.raises(ValueError, match="masks must be uint8 \\[2, H, W\\]"):
        a.add(model, img, masks[0].cuda())


def test_add_photo_equals_add_features_chunk_by_chunk():
    import clip
    geo, model = _toy(2)
    gen = torch.Generator().manual_seed(9)
    photo = torch.randint(0, 256, (260, 300, 3), generator=gen, dtype=torch.uint8)
    mask = torch.randint(0, 4, (26, 30), generator=gen, dtype=torch.uint8).repeat_interleave(10, 0).repeat_interleave(10, 1).contiguous()
    a = clip.DensePrototypes(4, geo.embed_dim).add_photo(model, photo, mask, window=[64, 96], batch=16)
    boxes = clip.plan_windows(300, 260, [64, 96])
    crops = clip.DevicePreprocess(64, torch.device("cuda")).regions(photo, boxes)
    b = clip.DensePrototypes(4, geo.embed_dim)
    for i in range(0, len(boxes), 16):
        feats = model.encode_image_dense(crops[i:i + 16])
        b.add_features(feats, mask.cuda()[None], boxes[i:i + 16], 2)
    assert len(boxes) > 32 and _same(a, b) and a.patches.sum().item() > 0
    with pytest.raises(ValueError, match="mask must be uint8 \\[260, 300\\]"):
        a.add_photo(model, photo, mask[:, :299].contiguous())


def _textured(layout, seed):
    """a 128 x 128 photo of two flat textures (grey levels 40 and 215 with a little noise) in the given 2 x 2 layout of 64-blocks"""
    lay = torch.tensor(layout, dtype=torch.uint8).repeat_interleave(64, 0).repeat_interleave(64, 1).contiguous()
    base = torch.where(lay == 0, 40, 215).to(torch.int16)
    noise = torch.randint(-8, 9, (128, 128, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.int16)
    return (base[:, :, None] + noise).clamp(0, 255).to(torch.uint8), lay


def test_fitted_prototypes_against_text_on_a_second_photo():
    import clip
    geo, model = _toy(2)
    fit_photo, fit_mask = _textured([[0, 1], [1, 0]], 1)
    new_photo, new_mask = _textured([[1, 1], [0, 1]], 2)
    p = clip.DensePrototypes(2, geo.embed_dim, class_names=["dark", "light"]).add_photo(model, fit_photo, fit_mask, window=64, stride=32)
    assert p.unsupported() == [] and p.support()["pixels"][0] > 0
    from clip.weights import synthetic_text
    prompts = ["a dark texture", "a light texture"]
    tokenize = lambda names: synthetic_text(len(names), geo, 7)                  # noqa: E731  (the toy vocabulary has no BPE: seeded token rows)
    clip.dense.class_features(model, prompts, tokenize)                          # the first call may time GEMM candidates: not compared
    text, names = clip.dense.class_features(model, prompts, tokenize)
    assert names == prompts and tuple(text.shape) == (2, geo.embed_dim)
    for tw in (0.0, 0.3):                                                        # prompt strings take the path of the feature tensor
        assert torch.equal(p.features(prompts, tw, model=model, tokenize=tokenize), p.features(text, tw))
    half = clip.DensePrototypes(2, geo.embed_dim)                                # no support at all: every row is its text row
    assert torch.equal(half.features(prompts, 0.5, model=model, tokenize=tokenize), text / text.norm(dim=1, keepdim=True))
    few = clip.segment_photo(model, new_photo, p.features(), window=64, stride=32).evaluate(new_mask.cuda())
    blend = clip.segment_photo(model, new_photo, p.features(text, 0.3), window=64, stride=32).evaluate(new_mask.cuda())
    zero = clip.segment_photo(model, new_photo, prompts, window=64, stride=32, tokenize=tokenize).evaluate(new_mask.cuda())
    print(f"toy textures: mIoU with fitted prototypes {few.miou:.6f}, blended with text (0.3) {blend.miou:.6f}, with text prompts {zero.miou:.6f}")
    assert math.isfinite(few.miou) and math.isfinite(zero.miou) and math.isfinite(blend.miou)
