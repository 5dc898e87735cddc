"""CPU: the host reference of the dense prototypes (tests/dense_prototypes_ref.py) against an independent brute-force statement
on every case of the table, the GPU test's bounds against five planted faults, the declarations the feature adds (header, ops
constants, the workspace closed form, the library symbols, clip's name), and the host arithmetic of clip.DensePrototypes on
accumulators filled by hand (the class keeps them on the CPU when asked to; only adding needs the device)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "construction-clip_amd")) if p not in sys.path]

import dense_prototypes_ref as PR  # noqa: E402
from cclip_hip.ops import dense_prototypes, dense_prototypes_workspace  # noqa: E402,F401  (the file is about the feature: without it, no collection)
from clip import DensePrototypes  # noqa: E402,F401


# ---- the reference against a brute-force statement -------------------------------------------------
def brute_force(case):
    """One one-hot mask per class, then per-cell means by a Python loop over the pixels of each window."""
    feat, masks, boxes, g, C, s8, image = (case[k] for k in ("feat", "masks", "boxes", "g", "C", "min_share8", "image"))
    B, H, W = masks.shape
    K, E = boxes.shape[0], feat.shape[1]
    onehot = [(masks == c) for c in range(C)]
    badmask = (masks >= C) & (masks != 255)
    sums, weight = np.zeros((C, E)), np.zeros(C)
    patches, pixels, bad = np.zeros(C, np.int64), np.zeros(C, np.int64), 0
    for k in range(K):
        x0, y0, x1, y1 = (int(v) for v in boxes[k])
        b = 0 if image is None else int(image[k])
        w, h = x1 - x0, y1 - y0
        if w < 1 or h < 1 or w > 16384 or h > 16384 or b < 0 or b >= B:
            continue
        area = np.zeros((g, g), np.int64)
        hits = np.zeros((C, g, g), np.int64)
        for v in range(h):
            i = ((2 * v + 1) * g) // (2 * h)
            for u in range(w):
                j = ((2 * u + 1) * g) // (2 * w)
                area[i, j] += 1
                x, y = x0 + u, y0 + v
                if 0 <= x < W and 0 <= y < H:
                    bad += int(badmask[b, y, x])
                    for c in range(C):
                        hits[c, i, j] += int(onehot[c][b, y, x])
        for c in range(C):
            pixels[c] += hits[c].sum()
            for i in range(g):
                for j in range(g):
                    n, a = int(hits[c, i, j]), int(area[i, j])
                    if a == 0 or n == 0 or n / a < s8 / 256:              # shares are exact binary fractions of small integers here
                        continue
                    f = feat[k * g * g + i * g + j].astype(np.float64)
                    nf = np.linalg.norm(f)
                    mean = float(np.float32(n) / np.float32(a))
                    if nf > 0:
                        sums[c] += mean * f / nf
                    weight[c] += mean
                    patches[c] += 1
    return dict(sums=sums, weight=weight, patches=patches, pixels=pixels, bad=np.array([bad], np.int64))


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_reference_equals_the_brute_force_statement(name):
    case = PR.CASES[name]
    ref = PR.reference(case["feat"], case["masks"], case["boxes"], case["g"], case["C"], case["min_share8"], case["image"])
    bf = brute_force(case)
    for k in ("patches", "pixels", "bad"):
        assert np.array_equal(ref[k], bf[k]), (name, k, ref[k], bf[k])
    assert np.allclose(ref["sums"], bf["sums"], rtol=0, atol=1e-12) and np.allclose(ref["weight"], bf["weight"], rtol=0, atol=1e-12)
    if name == "C255":                                        # support on classes 0, 128 and 254 only
        assert sorted(np.flatnonzero(ref["patches"]).tolist()) == [0, 128, 254] and ref["pixels"].sum() == 4 * 12 + 4 * 12 + 4 * 6
        assert ref["patches"].tolist()[0] == 3 and not ref["sums"][1:128].any() and not ref["weight"][129:254].any()


def test_hand_counted_cases():
    r = {s: PR.reference(**{k: PR.CASES[f"threshold_{s}"][k] for k in ("feat", "masks", "boxes", "g", "C", "min_share8")}) for s in (128, 129, 0, 256, 64)}
    assert r[128]["patches"].tolist() == [2, 2, 1]            # cell 00: 8 | 8 of 16, both at the threshold; 01: class 0; 10: class 1; 11: class 2
    assert r[129]["patches"].tolist() == [1, 1, 1]            # 8 of 16 no longer passes
    assert r[0]["patches"].tolist() == [3, 3, 2]              # any overlap
    assert r[256]["patches"].tolist() == [0, 0, 1]            # one stray pixel disqualifies cell 01
    assert r[64]["patches"].tolist() == [3, 2, 1]             # cell 10: 4 of 16 passes at exactly 64, 9 passes, 3 does not
    assert all(v["pixels"].tolist() == [8 + 15 + 4, 8 + 1 + 9, 3 + 16] for v in r.values())
    assert r[64]["weight"].tolist() == [0.5 + 15 / 16 + 0.25, 0.5 + 9 / 16, 1.0]
    s = PR.reference(**{k: PR.CASES["g3_side2"][k] for k in ("feat", "masks", "boxes", "g", "C", "min_share8")})
    assert s["patches"].sum() <= 4                            # side 2 at g = 3: the middle row and column of cells are empty
    assert PR.cell_of(np.arange(10), 10, 3).tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    assert PR.cell_of(np.arange(2), 2, 3).tolist() == [0, 2] and PR.cell_of(np.arange(1), 1, 3).tolist() == [1]
    e = PR.CASES["boxes_edges"]
    assert [PR.valid_window(b, 0, 1) for b in e["boxes"]] == [True] * 6 + [False] * 6 + [True, True, False, True]
    z = PR.reference(**{k: PR.CASES["zero_row"][k] for k in ("feat", "masks", "boxes", "g", "C", "min_share8")})
    full = PR.CASES["zero_row"]["feat"].copy()
    full[4] = 1.0
    nz = PR.reference(full, *(PR.CASES["zero_row"][k] for k in ("masks", "boxes", "g", "C", "min_share8")))
    assert np.array_equal(z["patches"], nz["patches"]) and np.array_equal(z["weight"], nz["weight"]) and not np.array_equal(z["sums"], nz["sums"])


# ---- the bounds trip on planted faults -------------------------------------------------------------
@pytest.mark.parametrize("fault,name", [("drop_cell", "g3_side10"), ("floor_rule", "g3_side10"), ("floor_rule", "g7_side225"),
                                        ("strict", "threshold_128"), ("strict", "threshold_64"), ("no_area", "g3_box10x7"),
                                        ("slab_twice", "cells_65"), ("slab_twice", "slabs_4_last_cell"), ("drop_cell", "E1024")])
def test_the_bounds_trip_on_a_planted_fault(fault, name):
    case = PR.CASES[name]
    args = (case["feat"], case["masks"], case["boxes"], case["g"], case["C"], case["min_share8"], case["image"])
    ref, wrong = PR.reference(*args), PR.reference(*args, fault=fault)
    assert PR.within(ref["sums"].astype(np.float32), ref["weight"].astype(np.float32), ref)       # fp32 rounding of the truth passes
    assert not (np.abs(wrong["sums"] - ref["sums"]) <= PR.sums_bound(ref)).all(), "the sums bound does not see the fault"
    assert not (np.abs(wrong["weight"] - ref["weight"]) <= PR.weight_bound(ref)).all(), "the weight bound does not see the fault"


# ---- declarations ----------------------------------------------------------------------------------
def test_header_ops_library_and_names():
    text = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    assert re.search(r"\bint\s+cclip_dense_prototypes\s*\(const float\*\s*feat,\s*int64_t ldf,\s*const uint8_t\*\s*masks,", text)
    assert re.search(r"\bint64_t\s+cclip_dense_prototypes_workspace\s*\(", text)
    slab = int(re.search(r"#define\s+CCLIP_PROTOTYPES_SLAB\s+(\d+)", text).group(1))
    side = int(re.search(r"#define\s+CCLIP_OVERLAY_MAX_SIDE\s+(\d+)", text).group(1))
    assert "ceil(K g g / CCLIP_PROTOTYPES_SLAB) * C * (E + 2) * 4" in text
    import clip
    from cclip_hip import load_library, ops
    assert slab == ops.PROTOTYPES_SLAB == PR.SLAB and side == ops.OVERLAY_MAX_SIDE == PR.MAX_SIDE
    lib = load_library()
    q = lib.cclip_dense_prototypes_workspace
    q.restype = ctypes.c_int64
    for K, g, C, E in [(1, 1, 1, 4), (7, 3, 3, 8), (1, 8, 3, 8), (65, 1, 3, 8), (1, 14, 255, 1024), (108, 14, 9, 512), (65535, 14, 255, 1024),
                       (65535, 16384, 255, 1024)]:
        closed = -(-(K * g * g) // slab) * C * (E + 2) * 4
        assert q(K, g, C, E) == ops.dense_prototypes_workspace(K, g, C, E) == closed, (K, g, C, E)
    assert hasattr(lib, "cclip_dense_prototypes") and clip.DensePrototypes.__name__ == "DensePrototypes"
    with pytest.raises(ValueError, match="dense_prototypes: feat must be a cuda tensor"):
        z = torch.zeros(1, dtype=torch.int64)
        ops.dense_prototypes(torch.zeros(9, 8), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, dtype=torch.int32), 3, 2, 128,
                             torch.zeros(2, 8), torch.zeros(2), z.repeat(2), z.repeat(2), z)


# ---- the host arithmetic of DensePrototypes ----------------------------------------------------------
def _filled(seed=0, C=4, E=8, empty=(2,)):
    import clip
    g = torch.Generator().manual_seed(seed)
    p = clip.DensePrototypes(C, E, class_names=[f"n{c}" for c in range(C)], min_share=0.5, device="cpu")
    p.sums.copy_(torch.randn(C, E, generator=g) * 3)
    p.weight.copy_(torch.rand(C, generator=g) * 5 + 1)
    p.patches.copy_(torch.randint(1, 9, (C,), generator=g))
    p.pixels.copy_(torch.randint(10, 99, (C,), generator=g))
    p.bad.fill_(3)
    for c in empty:
        p.sums[c], p.weight[c], p.patches[c] = 0.0, 0.0, 0
    return p


def test_features_blend_fallback_and_errors():
    import clip
    p = _filled()
    assert p.min_share8 == 128 and clip.DensePrototypes(2, 8, min_share=0.3, device="cpu").min_share8 == 77      # round(76.8)
    with pytest.raises(ValueError, match=r"no support for class 2 \(n2\)"):
        p.features()
    text = torch.randn(4, 8, generator=torch.Generator().manual_seed(5)) * 2
    t = text / text.norm(dim=1, keepdim=True)
    proto = p.sums / p.sums.norm(dim=1, keepdim=True).clamp_min(1e-30)
    f0 = p.features(text, 0.0)
    assert torch.allclose(f0[[0, 1, 3]], proto[[0, 1, 3]], atol=1e-6) and torch.allclose(f0[2], t[2], atol=1e-6)   # the fall-back is the text row
    f = p.features(text, 0.25)
    want = 0.75 * proto + 0.25 * t
    want = want / want.norm(dim=1, keepdim=True)
    assert torch.allclose(f[[0, 1, 3]], want[[0, 1, 3]], atol=1e-6) and torch.allclose(f[2], t[2], atol=1e-6)
    assert torch.allclose(f.norm(dim=1), torch.ones(4), atol=1e-6) and f.dtype == torch.float32 and f.is_contiguous()
    assert torch.allclose(p.features(text, 1.0), t, atol=1e-6)
    full = _filled(empty=())
    assert torch.allclose(full.features(), full.sums / full.sums.norm(dim=1, keepdim=True), atol=1e-6)
    two = _filled(empty=(0, 3))
    with pytest.raises(ValueError, match=r"no support for class 0 \(n0\), 3 \(n3\)"):
        two.features()
    for bad, match in ((lambda: p.features(text[:3]), r"text must be \[4, 8\]"), (lambda: p.features(text, 1.5), "text_weight must lie"),
                       (lambda: p.features(["a", "b", "c", "d"]), "prompt strings need model="),
                       (lambda: clip.DensePrototypes(0, 8, device="cpu"), "n_classes must be"),
                       (lambda: clip.DensePrototypes(2, 6, device="cpu"), "embed_dim must be"),
                       (lambda: clip.DensePrototypes(2, 8, min_share=1.5, device="cpu"), "min_share must lie"),
                       (lambda: clip.DensePrototypes(2, 8, class_names=["a"], device="cpu"), "1 class names for 2 classes")):
        with pytest.raises(ValueError, match=match):
            bad()
    s = p.support()
    assert s["unsupported"] == [2] and s["unsupported_names"] == ["n2"] and s["bad"] == 3 and s["patches"] == p.patches.tolist()
    assert s["pixels"] == p.pixels.tolist() and s["weight"] == p.weight.tolist()


def test_state_dict_round_trip_and_iadd():
    import clip
    p, q = _filled(1), _filled(2, empty=())
    sd = p.state_dict()
    r = clip.DensePrototypes.from_state_dict(sd, device="cpu")
    assert r.class_names == p.class_names and r.min_share8 == p.min_share8
    assert all(torch.equal(getattr(r, k), getattr(p, k)) for k in ("sums", "weight", "patches", "pixels", "bad"))
    fresh = clip.DensePrototypes(4, 8, device="cpu").load_state_dict(sd)
    assert torch.equal(fresh.sums, p.sums) and fresh.class_names == p.class_names
    sd["sums"][0, 0] += 1                                     # the state is a copy
    assert not torch.equal(sd["sums"], p.sums)
    with pytest.raises(ValueError, match="the state is for n_classes 4"):
        clip.DensePrototypes(3, 8, device="cpu").load_state_dict(sd)
    before = {k: getattr(p, k).clone() for k in ("sums", "weight", "patches", "pixels", "bad")}
    p += q
    assert all(torch.equal(getattr(p, k), before[k] + getattr(q, k)) for k in before)
    assert p.unsupported() == [] and p.bad.item() == 6
    with pytest.raises(ValueError, match="cannot add"):
        p += clip.DensePrototypes(4, 8, min_share=0.25, device="cpu")
