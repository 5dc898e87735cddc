"""CPU: the float64 reference of the image-guided refinement (tests/dense_refine_ref.py) on cases that can be worked out by hand,
the fp32 torch restatement's error against it on every shared case (printed: 4 x these figures are dense_refine_ref.BOUNDS, the
bounds of tests/test_dense_refine_gpu.py), the reference's own fragile share, the margin of the behavioural case, and the
refusals of clip.refine_maps / ops.dense_refine_* that need no device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_refine_ref as RR  # noqa: E402

FRAGILE_CAP = 1e-3


# ---- by hand -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", [(1,), (2, 5), RR.DEFAULT_DILATIONS])
def test_flat_guide_gives_the_neighbour_mean(ds):
    H, W, C = 11, 14, 3
    guide = RR.make_guide("flat", 1, H, W)
    maps = torch.rand(1, C, H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    wr = RR.weights_ref(guide, ds)
    N = 8 * len(ds)
    assert torch.equal(wr["factors"], torch.full_like(wr["factors"], 1.0 / 1e-8))        # sigma = 0 exactly
    assert (wr["w"] - 1.0 / N).abs().max() < 1e-15 and (wr["L"] - torch.log(torch.tensor(float(N), dtype=torch.float64))).abs().max() < 1e-15
    mean = torch.zeros_like(maps)
    for d in ds:                                              # the clamped neighbours, written out once more with Python indices
        for oy, ox in RR.OFFSETS:
            for y in range(H):
                for x in range(W):
                    mean[0, :, y, x] += maps[0, :, min(max(y + d * oy, 0), H - 1), min(max(x + d * ox, 0), W - 1)]
    assert (RR.step_ref(maps, wr) - mean / N).abs().max() < 1e-14


@pytest.mark.parametrize("kind", RR.GUIDES)
def test_constant_map_is_a_fixed_point_and_class_sums_stay_one_to_1e_12(kind):
    B, C, H, W = 2, 4, 19, 23
    guide = RR.make_guide(kind, B, H, W, seed=3)
    wr = RR.weights_ref(guide, RR.DEFAULT_DILATIONS)
    assert (wr["w"].sum(dim=1) - 1.0).abs().max() < 1e-12
    const = torch.full((B, 1, H, W), 0.37, dtype=torch.float64)
    assert (RR.step_ref(const, wr) - 0.37).abs().max() < 1e-12
    m = RR.make_maps(B, C, H, W, seed=3).double()
    m = m / m.sum(dim=1, keepdim=True)                        # sums of 1 to the last float64 bit (the fp32 maps' are within 2e-7)
    out = RR.refine_ref(m, guide, RR.DEFAULT_DILATIONS, 10)[10]
    assert (out.sum(dim=1) - 1.0).abs().max() < 1e-12
    assert float(out.min()) >= 0.0


def test_vertical_edge_keeps_a_step_map_on_its_side():
    H, W = 16, 20
    guide = RR.make_guide("edge", 1, H, W)
    left = (torch.arange(W) < (W + 1) // 2).double()
    m0 = left.expand(1, 1, H, W).contiguous()
    wr = RR.weights_ref(guide, (1,))
    m = m0
    for t in range(1, 6):
        m = RR.step_ref(m, wr)
        leak = (m - m0).abs().max().item()
        print(f"vertical edge, dilation 1: leakage after {t} iterations {leak:.3e}")
        assert leak < 1e-6 * t


def test_smaller_than_the_largest_dilation_is_all_clamping():
    B, C, H, W, ds = RR.CASES[1]
    qy, qx = RR.neighbours(H, W, ds)
    far = qy[8 * 5:]                                          # dilation 24 on a 5 x 7 picture: every neighbour is an edge pixel
    assert bool(((far == 0) | (far == H - 1) | (far == torch.arange(H)[None, :, None])).all())
    assert int(qy.min()) == 0 and int(qy.max()) == H - 1 and int(qx.min()) == 0 and int(qx.max()) == W - 1


# ---- the restatement sizes the bounds ----------------------------------------------------------
@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_fp32_restatement_sizes_the_bounds(i):
    """prints, per guide, the fp32 torch restatement's worst error against float64; BOUNDS holds 4 x these figures"""
    ts = (1,) + (RR.LONG_T if i in RR.LONG_CASES else ())
    for kind in RR.GUIDES:
        maps, guide, ds = RR.case_inputs(i, kind)
        ref = RR.refine_ref(maps, guide, ds, max(ts), keep=ts)
        e = RR.errors(RR.refine_fp32(maps, guide, ds, max(ts), keep=ts), ref, ts)
        b = RR.BOUNDS[(i, kind)]
        print(f"case {i} {RR.CASES[i]} guide {kind}: restatement error " + ", ".join(f"{k}: {v:.3e} (bound {b[k]:.3e})" for k, v in e.items()))
        assert set(b) == set(e)
        for k, v in e.items():
            assert v <= b[k], (kind, k)                       # the restatement itself, with its factor 4 of room
        for t in ts:
            if t > 1:                                         # a condition on the inputs: fp32 may decide few pixels either way
                share = RR.fragile_share(RR.label_ref(ref[t]), RR.FRAGILE_T10)
                print(f"case {i} guide {kind} T = {t}: fragile share {share:.2e}")
                assert share <= FRAGILE_CAP
    assert RR.FRAGILE_T10 >= RR.FRAGILE and RR.FRAGILE_T10 == max(RR.FRAGILE, 2 * max(b[10] for b in RR.BOUNDS.values() if 10 in b))


def test_diagonal_case_margin():
    maps, guide, truth = RR.diagonal_case()
    before = RR.agreement(maps.argmax(dim=1), truth)
    ref = RR.refine_ref(maps, guide, RR.DEFAULT_DILATIONS, 10)[10]
    after = RR.agreement(ref.argmax(dim=1), truth)
    print(f"diagonal case: agreement before {before:.5f}, after 10 default iterations {after:.5f} (float64)")
    assert before == RR.DIAGONAL_BEFORE and abs(after - RR.DIAGONAL_AFTER) < 1e-3
    assert after - before > RR.DIAGONAL_MARGIN
    assert RR.fragile_share(RR.label_ref(ref), RR.FRAGILE_T10) == 0.0


# ---- refusals that need no device --------------------------------------------------------------
def test_refine_maps_refusals():
    import clip
    m, g = torch.zeros(2, 3, 4), torch.zeros(3, 4, 3, dtype=torch.uint8)
    bad = [
        ("maps must be an fp32", lambda: clip.refine_maps(torch.zeros(3, 4), g)),
        ("maps must be an fp32", lambda: clip.refine_maps(m.double(), g)),
        ("guide must be a uint8", lambda: clip.refine_maps(m, g.float())),
        ("guide must be a uint8", lambda: clip.refine_maps(m, g[None])),
        ("guide must be \\[3, 4, 3\\]", lambda: clip.refine_maps(m, torch.zeros(4, 3, 3, dtype=torch.uint8))),
        ("guide must be \\[1, 3, 4, 3\\]", lambda: clip.refine_maps(m[None], torch.zeros(2, 3, 4, 3, dtype=torch.uint8))),
        ("0 dilations", lambda: clip.refine_maps(m, g, dilations=())),
        ("7 dilations", lambda: clip.refine_maps(m, g, dilations=(1,) * 7)),
        ("dilation 0", lambda: clip.refine_maps(m, g, dilations=(1, 0))),
        ("dilation 25", lambda: clip.refine_maps(m, g, dilations=(25,))),
        ("dilation 1.5", lambda: clip.refine_maps(m, g, dilations=(1.5,))),
        ("dilations must be a sequence", lambda: clip.refine_maps(m, g, dilations=3)),
        ("iterations must be an integer in \\[1, 64\\]", lambda: clip.refine_maps(m, g, iterations=0)),
        ("iterations must be an integer in \\[1, 64\\]", lambda: clip.refine_maps(m, g, iterations=65)),
        ("iterations must be an integer in \\[1, 64\\]", lambda: clip.refine_maps(m, g, iterations=2.5)),
        ("no CPU path", lambda: clip.refine_maps(m, g)),
    ]
    for match, fn in bad:
        with pytest.raises(ValueError, match=match):
            fn()


def test_step_refuses_in_place_before_anything_else():
    from cclip_hip import ops
    m = torch.zeros(1, 2, 3, 4)
    g, key = torch.zeros(1, 3, 4, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match="two buffers"):
        ops.dense_refine_step(m, m, g, key, (1,))
    with pytest.raises(ValueError, match="two buffers"):
        ops.dense_refine_step(m, m.view(1, 2, 3, 4), g, key, (1,))
    with pytest.raises(ValueError, match="dilation 25"):
        ops.dense_refine_step(m, torch.zeros_like(m), g, key, (25,))
    with pytest.raises(ValueError, match="7 dilations"):
        ops.dense_refine_prepare(g, (1,) * 7, key)
    with pytest.raises(ValueError, match="must be a cuda tensor"):
        ops.dense_refine_step(m, torch.zeros_like(m), g, key, (1,))
