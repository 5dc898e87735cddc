"""Plain helpers of the float64 GEMM tests (tests/test_kernels_f16_gpu.py, tests/test_gemm_paths_f64_gpu.py and, for the
device-free parts, tests/test_gemm_path_bounds_cpu.py).

First part: the helpers test_kernels_f16_gpu.py has always used (the bound its docstring derives, NaN canvases with sentinel
padding, `within` with its WORST table, `_assert_sensitive`), moved here unchanged.

Second part: references and DERIVED bounds of the GEMM's side paths (skinny GEMV, folded-LayerNorm partials / combine /
consumer).  They are written for tensors on any device so that the CPU module can run every bound against "the same formula in
fp32" and against a planted error without a kernel.  Each constant counts roundings of the kernel's own summation order; none
comes from a measured error."""
import math

import pytest
import torch

C_ACC = 2.0
SENT = -7.25          # exact in bf16, fp16 and fp32


def U(dt):
    return 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8


def FLOOR(dt):
    return 2.0 ** -24 if dt == torch.float16 else 0.0


def rnd(shape, dt, g, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=g) * scale).to(dt)


def canvas(rows, cols, dt, rows_pad=3, cols_pad=8):
    """(buffer, logical view): NaN inside [rows, cols], SENT in the padding rows / columns; row stride = cols + cols_pad rounded to 8"""
    ld = (cols + cols_pad + 7) // 8 * 8
    buf = torch.full((rows + rows_pad, ld), SENT, device="cuda", dtype=dt)
    buf[:rows, :cols] = float("nan")
    return buf, buf[:rows, :cols]


def check_canvas(name, buf, rows, cols):
    pad = torch.ones_like(buf, dtype=torch.bool)
    pad[:rows, :cols] = False
    assert bool((buf[pad] == SENT).all()), f"{name}: a write landed outside the logical output"


WORST = {}            # (check family, dtype) -> largest err / bound seen; printed at the end of the module (pytest -s)


@pytest.fixture(scope="module", autouse=True)
def _worst_report():
    """imported by the test modules: prints the ratios THAT module added or raised"""
    before = dict(WORST)
    yield
    for (fam, dt), r in sorted(WORST.items()):
        if before.get((fam, dt)) != r:
            print(f"worst err/bound  {fam:<24} {dt:<9} {r:.3g}")


def within(name, got, ref, bound, dt=None):
    got64 = got.double()
    fin = torch.isfinite(got64)
    assert bool(fin.all()), f"{name}: {int((~fin).sum())} non-finite outputs, first {(~fin).nonzero()[:4].tolist()}"
    err = (got64 - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        t = tuple(idx[0])
        pytest.fail(f"{name}: {int(bad.sum())}/{bad.numel()} outside the bound; first {idx}; got {got64[t].item():.6g} ref {ref[t].item():.6g} "
                    f"bound {bound[t].item():.3g}; worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3g}")
    worst = (err / bound.clamp_min(1e-300)).max().item()
    key = (name.split(" ")[0] + (" f32" if got.dtype == torch.float32 else " 16-bit"), str(dt or got.dtype).replace("torch.", ""))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def _mats(A, B, akc, bkc):
    """A [M,K], B [N,K] in fp64 from the operands as stored"""
    Am = A.double() if akc else A.double().t()
    Bm = B.double() if bkc else B.double().t()
    return Am, Bm


def _acc_bound(Am, Bm, scale=1.0):
    K = Am.shape[1]
    return C_ACC * 2.0 ** -24 * math.sqrt(K) * scale * (Am.abs() @ Bm.abs().t())


def _assert_sensitive(got, ref, bound, Am, Bm, alpha=1.0, slope=None):
    """The bound must reject a reference with the LAST 64-deep K-tile's contribution removed from one 16x16 output sub-tile
    (the middle one of the logical output): an error the size of one MFMA step in one tile is visible."""
    M, N, K = Am.shape[0], Bm.shape[0], Am.shape[1]
    k0 = (K - 1) // 64 * 64
    m0, n0 = (M // 2) // 16 * 16, (N // 2) // 16 * 16
    m1, n1 = min(m0 + 16, M), min(n0 + 16, N)
    part = alpha * (Am[m0:m1, k0:] @ Bm[n0:n1, k0:].t())
    if slope is not None:
        part = part * slope[m0:m1, n0:n1]
    wrong = ref.clone()
    wrong[m0:m1, n0:n1] -= part
    err = (got.double() - wrong).abs()
    assert bool((err[m0:m1, n0:n1] > bound[m0:m1, n0:n1]).any()), "the bound cannot see one missing K-tile in one 16x16 sub-tile"
    full = ref - alpha * (Am[:, k0:] @ Bm[:, k0:].t()) * (1.0 if slope is None else slope)
    assert bool(((got.double() - full).abs() > bound).any()), "the bound cannot see one missing K-tile"


def _act64(v, act, aux):
    """fp64 activation and its slope d act / d v (the factor an accumulation error is multiplied by)"""
    c = math.sqrt(2 / math.pi)
    if act == 0:
        return v, torch.ones_like(v)
    if act == 1:
        s = torch.sigmoid(1.702 * v)
        return v * s, (s + 1.702 * v * s * (1 - s)).abs()
    if act == 2:
        t = torch.tanh(v)
        return t, 1 - t * t
    if act == 3:
        t = torch.tanh(c * (v + 0.044715 * v ** 3))
        y = 0.5 * v * (1 + t)
        d = 0.5 * (1 + t) + 0.5 * v * (1 - t * t) * c * (1 + 3 * 0.044715 * v * v)
        return y, d.abs()
    if act == 4:
        return torch.relu(v), (v > 0).double()
    a = aux.double()
    if act == 16:
        s = torch.sigmoid(1.702 * a)
        gd = s * (1 + 1.702 * a * (1 - s))
    elif act == 17:
        gd = 1 - a * a
    elif act == 18:
        t = torch.tanh(c * (a + 0.044715 * a ** 3))
        gd = 0.5 * (1 + t) + 0.5 * a * (1 - t * t) * c * (1 + 3 * 0.044715 * a * a)
    elif act == 19:
        gd = (a > 0).double()
    else:
        raise ValueError(act)
    return v * gd, gd.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# the side paths: references and derived bounds (any device)
# ---------------------------------------------------------------------------------------------------------------------------
E24, E20 = 2.0 ** -24, 2.0 ** -20


def host_rnd(shape, dt, g, scale=1.0):
    """16-bit operands from a HOST generator: the CPU module sees the very tensors the GPU module feeds the kernel"""
    return (torch.randn(shape, generator=g) * scale).to(dt)


# (M, N, K) of the skinny cases: one live 8-column chunk; K % 64 != 0 and a second 32-column block with one live chunk; MCAP 4 | 8 on
# either side of the split at one full 768-row pass; a second pass with one live row group; K % 8 != 0 (scalar staging); LDS
# exactly at the 96 KiB limit (four passes); just over it (the call falls back to the tile kernels)
SKINNY_SHAPES = [(1, 8, 64), (3, 40, 200), (4, 136, 768), (5, 136, 768), (8, 2304, 832), (3, 384, 100), (8, 768, 3072), (8, 768, 3080)]


def skinny_operands(M, N, K, dt):
    """A [M, K] (0.1 scale), B [K, N], bias [N], residual [M, N] on the host"""
    g = torch.Generator().manual_seed(M * 100003 + N * 101 + K)
    return host_rnd((M, K), dt, g, 0.1), host_rnd((K, N), dt, g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def epilogue_ref(Am, Bm, alpha, bias, act, res, aux=None):
    """pre-activation, activation, its slope and the output of the GEMM epilogue in fp64"""
    pre = alpha * (Am @ Bm.t())
    if bias is not None:
        pre = pre + bias.double()
    y, slope = _act64(pre, act, aux)
    r = torch.zeros_like(y) if res is None else res.double()
    return dict(pre=pre, y=y, slope=slope, res=r, ref=y + r)


def epilogue_bounds(acc, e, dt):
    """The bound of test_gemm_epilogues_f64 from an accumulation term `acc`: (fp32 output, 16-bit output, 16-bit pre-activation)"""
    ev = E20 * (e["ref"].abs() + e["pre"].abs() + e["res"].abs() + e["y"].abs())
    bf = acc * (1.0 + e["slope"]) + ev + 1e-30
    b16 = bf + U(dt) * e["ref"].abs() + FLOOR(dt)
    bp = acc + E20 * e["pre"].abs() + U(dt) * e["pre"].abs() + FLOOR(dt) + 1e-30
    return bf, b16, bp


def skinny_acc_bound(Am, Bm, alpha=1.0):
    """Skinny GEMV (csrc/gemm_skinny_impl.h): a row slot adds at most ceil(K / 64) exact products (one fp32 rounding each), two
    DPP adds join the four slots of a 16-lane row, 16 partials are added in order: at most ceil(K / 64) + 18 roundings, each of at
    most 2^-24 of a partial sum, and every partial sum is at most |A| . |B|.  Worst case, first order; no sqrt(K) statistics (for
    K <= 64 that term would be SMALLER than this worst case)."""
    K = Am.shape[1]
    return ((K + 63) // 64 + 18) * E24 * abs(alpha) * (Am.abs() @ Bm.abs().t())


def skinny_bounds(Am, Bm, alpha, e, act, dt):
    """(fp32 output, 16-bit output, 16-bit pre-activation): the derived accumulation term, times (1 + slope) behind GELU-new, plus the
    project's 2^-20 epilogue term, plus u |ref| + floor for a 16-bit output"""
    acc = skinny_acc_bound(Am, Bm, alpha)
    ev = E20 * (e["ref"].abs() + e["pre"].abs() + e["res"].abs() + e["y"].abs())
    bf = acc * ((1.0 + e["slope"]) if act else 1.0) + ev + 1e-30
    b16 = bf + U(dt) * e["ref"].abs() + FLOOR(dt)
    bp = acc + E20 * e["pre"].abs() + U(dt) * e["pre"].abs() + FLOOR(dt) + 1e-30
    return bf, b16, bp


def skinny_dropped_product(ref, bound, Am, Bm, alpha, slope=None):
    """A reference with the single product k = K - 1 removed from one 8-column chunk of one row - the (row, chunk) where that
    product is largest against the bound (a product next to zero is invisible to any bound; one row's activation A[m, K-1] is shared by
    the whole chunk).  Returns (wrong reference, row, column slice, largest |removed| / bound in the chunk)."""
    K = Am.shape[1]
    part = alpha * Am[:, K - 1:K] * Bm[:, K - 1][None, :]
    if slope is not None:
        part = part * slope
    ratio = (part.abs() / bound).view(Am.shape[0], -1, 8).amax(2)
    flat = int(ratio.argmax())
    m, c = flat // ratio.shape[1], flat % ratio.shape[1]
    sl = slice(8 * c, 8 * c + 8)
    wrong = ref.clone()
    wrong[m, sl] -= part[m, sl]
    return wrong, m, sl, ratio[m, c].item()


def assert_skinny_sensitive(got, ref, bound, Am, Bm, alpha, slope=None):
    wrong, m, sl, _ = skinny_dropped_product(ref, bound, Am, Bm, alpha, slope)
    err = (got.double() - wrong).abs()
    assert bool((err[m, sl] > bound[m, sl]).any()), "the bound cannot see one dropped product in one 8-column chunk"


def rowstats_partials_ref(x):
    """(sum, sum of squares) of every 64-column block of the fp32 rows x [M, N] in fp64, as [N / 64, M, 2], and their bounds:
    the kernel adds 4 values pairwise (2 roundings deep), then 4 DPP steps over 16 lanes: 6 roundings deep on the sum, one more (the
    squares) on the sum of squares; each at most 2^-24 of sum |x| (resp. sum x^2).  8 leaves one spare."""
    M, N = x.shape
    xb = x.double().contiguous().view(M, N // 64, 64).permute(1, 0, 2)
    ref = torch.stack((xb.sum(2), (xb * xb).sum(2)), 2)
    bound = 8 * E24 * torch.stack((xb.abs().sum(2), (xb * xb).sum(2)), 2) + 1e-300
    return ref, bound


def combine_partials(rows, nblk, g):
    """block sums of rows with mean in +-1 and std in 0.5 .. 2; row 0 is constant 0.25 (var == 0 exactly), row 1 constant 0.3"""
    D = 64 * nblk
    x = torch.randn(rows, D, generator=g, dtype=torch.float64) * (0.5 + 1.5 * torch.rand(rows, 1, generator=g, dtype=torch.float64)) \
        + (2 * torch.rand(rows, 1, generator=g, dtype=torch.float64) - 1)
    x[0] = 0.25
    if rows > 1:
        x[1] = 0.3
    xb = x.view(rows, nblk, 64).permute(1, 0, 2)
    return torch.stack((xb.sum(2), (xb * xb).sum(2)), 2).float().contiguous()


def rowstats_combine_ref(partials, D, eps=1e-5):
    """cclip_rowstats_combine in fp64 (same formula, clamp included) from the fp32 partials [nblk, rows, 2] as stored; returns
    mean, var, rstd, the bound on mean, delta_v and the RELATIVE bound on rstd:
      mean: nblk - 1 adds and one division, each 2^-24 of at most sum |s1| / D                        -> (nblk + 1) 2^-24 sum|s1| / D
      var : the same for s2 / D, plus mean^2 (mean's own error doubled, one product, one subtraction)   -> (nblk + 3) 2^-24 (sum|s2| / D + 2 mean^2)
      rstd: d rstd / rstd = -dv / (2 (var + eps)) to first order, the add of eps, and rsqrtf's own ulp -> dv / (2 (var + eps)) + 3 2^-24"""
    p = partials.double()
    nblk = p.shape[0]
    s1, s2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    mean = s1 / D
    raw = s2 / D - mean * mean
    var = raw.clamp_min(0.0)
    rstd = (var + eps).rsqrt()
    b_mean = (nblk + 1) * E24 * p[:, :, 0].abs().sum(0) / D + 1e-300
    dv = (nblk + 3) * E24 * (p[:, :, 1].abs().sum(0) / D + 2 * mean * mean)
    b_rstd = dv / (2 * (var + eps)) + 3 * E24
    return dict(mean=mean, var=var, raw=raw, rstd=rstd, b_mean=b_mean, dv=dv, b_rstd=b_rstd)


def fold_pipeline_bound(x, D, eps=1e-5):
    """Producer + combine against fp64 statistics of the fp32 rows x themselves (the conditioning measurement): the combine's terms
    with the partials' own error added - 8 2^-24 sum|x| on s1 and 8 2^-24 sum x^2 on s2, carried through var = s2 / D - mean^2.
    Returns fp64 mean, var, rstd and the relative bound on rstd (first order; valid while dv <= 0.1 (var + eps), returned too)."""
    nblk = D // 64
    xd = x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    a1, a2 = xd.abs().sum(1) / D, (xd * xd).sum(1) / D
    dv = (nblk + 3) * E24 * (a2 + 2 * mean * mean) + 8 * E24 * (a2 + 2 * mean.abs() * a1)
    return dict(mean=mean, var=var, rstd=(var + eps).rsqrt(), dv=dv, b_rstd=dv / (2 * (var + eps)) + 3 * E24)


def fold_consumer_ref(Am, Bm, alpha, stats, c1, c2, act, dt):
    """act(rstd (alpha x ws^T - mean c1) + c2) in fp64 and its bound (16-bit output): the accumulation error and the fp32
    evaluation of every term, scaled by the row's rstd and the activation's slope, then the output's own rounding"""
    mean, rstd = stats[:, 0:1].double(), stats[:, 1:2].double()
    acc = alpha * (Am @ Bm.t())
    mc = mean * c1.double()[None, :]
    pre = rstd * (acc - mc) + c2.double()[None, :]
    y, slope = _act64(pre, act, None)
    bound = (rstd * _acc_bound(Am, Bm, alpha) + E20 * (rstd * acc.abs() + rstd * mc.abs() + c2.double().abs()[None, :] + pre.abs())) * (1 + slope) \
        + E20 * y.abs() + U(dt) * y.abs() + FLOOR(dt) + 1e-30
    return dict(y=y, pre=pre, slope=slope, rstd=rstd, bound=bound)
