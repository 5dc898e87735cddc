"""CPU: the derived bounds of tests/test_gemm_paths_f64_gpu.py (tests/gemm_refs_f64.py) without a kernel.  Clean side: an fp32
torch computation of the same formula on the same 16-bit operands - "a kernel that is correct to fp32" - passes every bound with
room to spare (half of it, the rounding of a 16-bit output aside).  Planted errors: one dropped k in one skinny chunk, one 4-column group missing from a partial, one
partial block skipped in the combine, the consumer reading the statistics of row m + 16, one missing K-tile in one sub-tile of
configuration 4 - each fails its bound.  The skinny cases are the GPU module's own operands (host generator), and the dropped
product clears TWICE the bound there, so whatever a kernel inside the bound returns, the GPU module's sensitivity check sees it."""
import pytest
import torch

import gemm_refs_f64 as GR

DTS = [torch.float16, torch.bfloat16]


def clean(name, got, ref, bound):
    """fp32 values: within half of the bound.  16-bit values: within the bound less half of everything but the output's own
    rounding, u |ref| + floor - that term is tight by construction (a value just above a power of two rounds by u times itself)"""
    err = (got.double() - ref).abs()
    own = 0.0 if got.dtype == torch.float32 else GR.U(got.dtype) * ref.abs() + GR.FLOOR(got.dtype)
    assert bool((err <= own + 0.5 * (bound - own)).all()), f"{name}: fp32 evaluation uses {(err / bound).max().item():.3g} of the bound"


def rejects(got, wrong, bound):
    return bool(((got.double() - wrong).abs() > bound).any())


def gelu_new32(v):
    return 0.5 * v * (1 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", GR.SKINNY_SHAPES)
def test_skinny_bound_separates_fp32_rounding_from_one_dropped_product(M, N, K, dt):
    A, B, bias, res = GR.skinny_operands(M, N, K, dt)
    Am, Bm = GR._mats(A, B, True, False)
    acc32 = A.float() @ B.float()
    # fp32 residual form, alpha = 0.5; its 16-bit rounding; GELU-new and its pre-activation
    for alpha, act, r in ((0.5, 0, res), (0.5, 0, None), (1.0, 3, None)):
        e = GR.epilogue_ref(Am, Bm, alpha, bias, act, r)
        bf, b16, bp = GR.skinny_bounds(Am, Bm, alpha, e, act, dt)
        pre32 = acc32 * alpha + bias
        y32 = (gelu_new32(pre32) if act else pre32) + (0 if r is None else r)
        sl = e["slope"] if act else None
        for nm, got, ref, bound, s in (("f32", y32, e["ref"], bf, sl), ("16-bit", y32.to(dt), e["ref"], b16, sl),
                                       ("pre", pre32.to(dt), e["pre"], bp, None)):
            clean(f"skinny {nm} act{act}", got, ref, bound)
            wrong, m, cs, ratio = GR.skinny_dropped_product(ref, bound, Am, Bm, alpha, s)
            assert ratio > 2.0, f"{nm}: the largest dropped product is only {ratio:.3g} of the bound"
            assert rejects(got[m:m + 1, cs], wrong[m:m + 1, cs], bound[m:m + 1, cs]), "the bound cannot see one dropped product"
            assert not rejects(got, ref, bound)
            GR.assert_skinny_sensitive(got, ref, bound, Am, Bm, alpha, s)


def test_skinny_bound_is_the_worst_case_where_sqrt_k_is_not():
    """K <= 64: one product per row slot, 18 roundings of the reduction; the project's 2 sqrt(K) term is smaller than that"""
    A, B = torch.ones(1, 64, dtype=torch.float64), torch.ones(8, 64, dtype=torch.float64)
    assert bool((GR._acc_bound(A, B) < GR.skinny_acc_bound(A, B)).all())
    assert GR.skinny_acc_bound(A, B)[0, 0].item() == 19 * 2.0 ** -24 * 64
    A, B = torch.ones(1, 3072, dtype=torch.float64), torch.ones(8, 3072, dtype=torch.float64)
    assert GR.skinny_acc_bound(A, B, 0.5)[0, 0].item() == 66 * 2.0 ** -24 * 0.5 * 3072


def test_partial_bound_separates_fp32_sums_from_a_missing_column_group():
    g = torch.Generator().manual_seed(3)
    M, N = 256, 256
    x = (torch.randn(M, N, generator=g) * 2 + 0.7).float()
    ref, bound = GR.rowstats_partials_ref(x)
    xb = x.view(M, N // 64, 64).permute(1, 0, 2)
    got = torch.stack((xb.sum(2), (xb * xb).sum(2)), 2)
    clean("partials", got, ref, bound)
    j, m = 2, 100
    grp = x[m, 64 * j + 8:64 * j + 12].double()
    wrong = ref.clone()
    wrong[j, m, 0] -= grp.sum()
    wrong[j, m, 1] -= (grp * grp).sum()
    for c in (0, 1):
        assert (got[j, m, c].double() - wrong[j, m, c]).abs() > bound[j, m, c], "the bound cannot see a missing 4-column group"
    assert not rejects(got, ref, bound)


@pytest.mark.parametrize("nblk", [1, 4, 12, 16])
def test_combine_bound_separates_fp32_evaluation_from_a_skipped_block(nblk):
    rows, D = 257, 64 * nblk
    part = GR.combine_partials(rows, nblk, torch.Generator().manual_seed(nblk))
    r = GR.rowstats_combine_ref(part, D)
    assert bool((r["dv"] <= 0.1 * (r["var"] + 1e-5)).all()) and r["raw"][0] <= 0

    def fp32_combine(p):
        s1, s2 = torch.zeros(rows), torch.zeros(rows)
        for j in range(p.shape[0]):
            s1 = s1 + p[j, :, 0]
            s2 = s2 + p[j, :, 1]
        mean = s1 / D
        var = (s2 / D - mean * mean).clamp_min(0.0)
        return mean, (var + 1e-5).rsqrt()

    mean, rstd = fp32_combine(part)
    clean("mean", mean, r["mean"], r["b_mean"])
    clean("rstd", rstd, r["rstd"], r["b_rstd"] * r["rstd"])
    skipped = part.clone()
    skipped[nblk // 2] = 0
    w = GR.rowstats_combine_ref(skipped, D)
    rows_seen = ((mean.double() - w["mean"]).abs() > r["b_mean"]) | ((rstd.double() - w["rstd"]).abs() > r["b_rstd"] * r["rstd"])
    assert bool(rows_seen.all()), "a skipped partial block must show in every row"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", [0, 1])
def test_consumer_bound_separates_fp32_evaluation_from_a_neighbours_statistics(act, dt):
    g = torch.Generator().manual_seed(5 + act)
    M, N, K = 256, 256, 128
    xb, ws = GR.host_rnd((M, K), dt, g), GR.host_rnd((N, K), dt, g, 0.1)
    stats = torch.stack((torch.rand(M, generator=g) * 4 - 2, 0.1 * 100.0 ** torch.rand(M, generator=g)), 1)
    c1, c2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    Am, Bm = GR._mats(xb, ws, True, True)
    r = GR.fold_consumer_ref(Am, Bm, 0.5, stats, c1, c2, act, dt)

    def fp32_consumer(st):
        v = ((xb.float() @ ws.float().t()) * 0.5 - st[:, 0:1] * c1[None, :]) * st[:, 1:2] + c2[None, :]
        return (v * torch.sigmoid(1.702 * v) if act else v).to(dt)

    got = fp32_consumer(stats)
    clean("consumer", got, r["y"], r["bound"])
    GR._assert_sensitive(got, r["y"], r["bound"], Am, Bm, 0.5, r["slope"] * r["rstd"])
    shifted = fp32_consumer(torch.roll(stats, -16, 0))                    # row m reads the statistics of row m + 16
    bad_rows = ((shifted.double() - r["y"]).abs() > r["bound"]).any(1)
    assert bool(bad_rows.all()), "statistics of the wrong row must show in every row"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("K", [512, 456])
def test_cfg4_bound_separates_fp32_rounding_from_a_missing_k_tile(K, dt):
    g = torch.Generator().manual_seed(K)
    M, N = 256, 128
    A, B = GR.host_rnd((M, K), dt, g, 0.1), GR.host_rnd((N, K), dt, g)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    Am, Bm = GR._mats(A, B, True, True)
    pre32 = (A.float() @ B.float().t()) * 0.5 + bias
    for act, r in ((0, None), (1, None), (0, res)):
        e = GR.epilogue_ref(Am, Bm, 0.5, bias, act, r)
        bf, b16, bp = GR.epilogue_bounds(GR._acc_bound(Am, Bm, 0.5), e, dt)
        y32 = (pre32 * torch.sigmoid(1.702 * pre32) if act else pre32) + (0 if r is None else r)
        got, bound = (y32, bf) if r is not None else (y32.to(dt), b16)
        clean(f"cfg4 act{act}", got, e["ref"], bound)
        GR._assert_sensitive(got, e["ref"], bound, Am, Bm, 0.5, e["slope"])
        if act:
            clean("cfg4 pre", pre32.to(dt), e["pre"], bp)
            GR._assert_sensitive(pre32.to(dt), e["pre"], bp, Am, Bm, 0.5)
