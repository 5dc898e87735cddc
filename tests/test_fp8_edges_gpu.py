"""GPU: the five fp8 kernels (csrc/gemm_bf16_fp8ops.hip quantize_rows_fp8 / quantize_mx_fp8 / ln_fwd_fp8 / gemm_fp8_kernel,
csrc/attention.hip attn_store_mx) at their boundaries, against the float64 reference of tests/fp8_ref.py.  Wherever the answer
is knowable exactly it is asserted exactly: operands are built so that every product, sum, scale and rounding is determined
(small-integer e4m3 bytes, power-of-two scales, block amax on the m * 2^k grid of fp8_ref.DYADIC_M, no value near an e4m3 tie
unless the tie itself is exact), so an exponent byte routed to a neighbouring block / head / K-tile, a scale taken from the next
row or column, or an off-by-one at a power-of-two amax changes the expected bytes and fails.

Every operand and output is a view of a wider buffer (ld > width).  Canaries: 0x7F (e4m3 NaN) in byte buffers - operand padding
included, so a read past an operand's edge poisons the result -, NaN in 16-bit / fp32 outputs, 0 in exponent buffers (legal
exponents are 1..253); everything outside the written region must come back untouched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp8_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTS = [torch.bfloat16, torch.float16]
NAN8 = 0x7F


def ops():
    from cclip_hip import ops as o
    return o


def U(dt):
    return 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8


def FLOOR(dt):
    return 2.0 ** -24 if dt == torch.float16 else 0.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def in_view(t, pad, fill):
    """a copy of the 2-D tensor t as the [:, pad : pad + C] slice of a buffer with `pad` more columns on either side and one
    more row, all `fill`: (buffer, view) on the GPU"""
    Rr, C = t.shape
    buf = torch.full((Rr + 1, C + 2 * pad), fill, dtype=t.dtype)
    buf[:Rr, pad:pad + C] = t
    buf = buf.cuda()
    return buf, buf[:Rr, pad:pad + C]


def out_view(rows, cols, dtype, fill, left=0, right=8, rows_pad=2):
    buf = torch.full((rows + rows_pad, left + cols + right), fill, dtype=dtype, device="cuda")
    return buf, buf[:rows, left:left + cols]


def assert_pad_untouched(name, buf, rows, cols, left, fill):
    pad = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    pad[:rows, left:left + cols] = False
    got = buf[pad]
    ok = torch.isnan(got).all() if isinstance(fill, float) and fill != fill else (got == fill).all()
    assert bool(ok), f"{name}: a write landed outside the logical output"


def assert_bytes(name, got, want):
    got, want = got.cpu(), want.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        t = tuple(bad[0].tolist())
        pytest.fail(f"{name}: {bad.shape[0]}/{got.numel()} differ; first at {t}: got {int(got[t])} want {int(want[t])}; "
                    f"rows {sorted(set(bad[:, 0].tolist()))[:8]} cols {sorted(set(bad[:, -1].tolist()))[:8]}")


# ---------------------------------------------------------------------------------------------------------------------------------
# quantisers
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows_input(Rr, C, dt, seed):
    """dyadic-amax rows with no element near an e4m3 tie of x / scale (there the kernel's fp32 x * (1 / s) and the float64
    quotient could round apart); from 5 rows up: row 1 = exact ties on a power-of-two scale, row 2 = +-amax only, row 3 = zeros"""
    x, _, _ = R.dyadic_amax_rows(Rr, C, dt, seed)
    x = x.double()
    s = R.rows_scale_ref(x.float().abs().amax(1)).double()
    tie = R.near_tie(x / s[:, None]) & (x.abs() < x.abs().amax(1, keepdim=True))
    x = torch.where(tie, torch.zeros_like(x), x)
    if Rr >= 5:
        s1 = 2.0 ** -3
        pat = torch.tensor([17.0, 27.0, -17.0, -27.0, 448.0, 1.0, -3.0, 0.0]) * s1          # 17 -> 16, 27 -> 28 (round to even), scale 2^-3
        x[1] = pat.repeat(C // 8).double()
        sg = torch.randint(0, 2, (C,), generator=gen(seed)).double() * 2 - 1
        x[2] = sg * 352.0 * 2.0 ** 5
        x[3] = 0.0
    x16 = x.to(dt)
    assert torch.equal(x16.double(), x)
    return x16


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Rr,C", [(1, 8), (5, 24), (7, 520), (9, 1032)])
def test_quantize_rows_exact(Rr, C, dt):
    """scale == fp32(amax) * fp32(1 / 448) bit for bit, bytes == RNE e4m3 of the float64 quotient x / scale; x a column slice of
    a buffer with ld = C + 8, out one with ld = C + 16; cols below one lane sweep (8, 24), past one (520) and two (1032)."""
    o = ops()
    x16 = _rows_input(Rr, C, dt, 11 + Rr)
    xb = torch.full((Rr + 1, C + 8), float("nan"), dtype=dt)
    xb[:Rr, :C] = x16
    xb = xb.cuda()
    qb, q = out_view(Rr, C, torch.uint8, NAN8, left=8, right=8)
    sb = torch.full((Rr + 2,), float("nan"), device="cuda")
    o.quantize_rows_fp8(xb[:Rr, :C], q, sb[:Rr])
    torch.cuda.synchronize()
    want_s = R.rows_scale_ref(x16.float().abs().amax(1))
    assert torch.equal(sb[:Rr].cpu(), want_s), (sb[:Rr].cpu(), want_s)
    assert bool(torch.isnan(sb[Rr:]).all())
    assert_bytes("bytes", q, R.encode_rne(x16.double() / want_s.double()[:, None]))
    assert_pad_untouched("out", qb, Rr, C, 8, NAN8)
    if Rr >= 5:
        assert want_s[1].item() == 2.0 ** -3 and want_s[3].item() == 1.0
        assert R.decode(q[1, :8].cpu()).tolist() == [16.0, 28.0, -16.0, -28.0, 448.0, 1.0, -3.0, 0.0]
        assert bool((q[3] == 0).all())
        assert set(R.decode(q[2].cpu()).tolist()) == {448.0, -448.0}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Rr,C,rows", [(1, 32, None), (3, 96, None), (5, 192, None), (130, 160, None), (9, 96, 6)])
def test_quantize_mx_exact(Rr, C, rows, dt):
    """Every block's amax is m * 2^k (fp8_ref.DYADIC_M), where the kernel's fp32 exponent rule and the exact one agree: EVERY
    exponent byte equals e8m0_exact and every e4m3 byte the float64 RNE (the scale is a power of two: x * 2^-(e-127) is exact).
    C % 128 != 0 (the last K-tile's spare bytes), 11 work-groups with a partial last quad (130 x 160), rows= below the buffer."""
    o = ops()
    x16, _, _ = R.dyadic_amax_rows(Rr, C, dt, 21 + Rr, block=32)
    n = Rr if rows is None else rows
    xb = torch.full((Rr + 1, C + 8), float("nan"), dtype=dt)
    xb[:Rr, :C] = x16
    xb = xb.cuda()
    qb, q = out_view(Rr, C, torch.uint8, NAN8, left=8, right=8)
    e3 = R.mx_buffer(n, C, rows_pad=2, fill=0).cuda()
    o.quantize_mx_fp8(xb[:Rr, :C], q, e3, rows=rows)
    torch.cuda.synchronize()
    want_e, want_q = R.quantize_mx_ref(x16.double()[:n])
    assert_bytes("exponents", R.mx_rows(e3, n, C), want_e.to(torch.uint8))
    assert_bytes("bytes", q[:n], want_q)
    assert bool((e3[~R.mx_written_mask(e3, n, C)] == 0).all()), "an exponent byte landed outside the operand's own"
    assert_pad_untouched("out", qb, n, C, 8, NAN8)


def _range_rows(dt, C=32):
    """rows whose amax runs from the type's smallest subnormal to its largest finite value; each row: +amax, -amax, zeros and
    +-amax / 2 (where amax / 2 exists in the type)"""
    if dt == torch.bfloat16:
        amax = [2.0 ** -133, 2.0 ** -132, 2.0 ** -130, 2.0 ** -127, 2.0 ** -126, 2.0 ** -123, 1.5 * 2.0 ** -120, 2.0 ** -118, 2.0 ** -100,
                2.0 ** -50, 1.0, 2.0 ** 50, 2.0 ** 100, 2.0 ** 126, torch.finfo(dt).max]
    else:
        amax = [2.0 ** -24, 2.0 ** -23, 2.0 ** -20, 2.0 ** -15, 2.0 ** -14, 1.5 * 2.0 ** -10, 1.0, 1000.0, 32768.0, torch.finfo(dt).max]
    a = torch.tensor(amax, dtype=F64)[:, None]
    pat = torch.tensor([1.0, 0.0, 0.5, -0.5, 0.0, -1.0, 0.5, 0.0], dtype=F64).repeat(C // 8)[None, :]
    x16 = (a * pat).to(dt)
    x = x16.double()
    assert torch.equal(x.abs().amax(1, keepdim=True), a)          # (amax / 2 of the smallest subnormal rounds to 0: a zero more)
    return x16


# fp32 evaluation of the row quantiser, relative to |x|: the scale's two roundings (1 / 448, the product), 1 / s and x * (1 / s)
# move x / s by < 2^-22 of itself - across a rounding boundary at worst, or past the 448 clamp; where the scale's product
# amax * (1 / 448) is an fp32 subnormal its rounding is absolute, <= 2^-150, and the clamp turns it into <= 448 * 2^-150 < 2^-141.
RANGE_REL, RANGE_ABS = 2.0 ** -22, 2.0 ** -141


@pytest.mark.parametrize("dt", DTS)
def test_quantize_rows_range(dt):
    """The whole range of the input type through the row quantiser: every scale finite and > 0, every dequantised element within
    quant_step(x, scale) + 2^-22 |x| + 2^-141 of x (RANGE_REL / RANGE_ABS above), every zero input a zero byte (0x00 / 0x80).

    Before the scale was floored at 2^-126 the bf16 rows with amax below 448 / FLT_MAX ~ 1.3e-36 failed here on an MI355X (fp32
    subnormals are not flushed, so the scale is a subnormal and 1 / scale = +inf): amax = 2^-133 = 1.84e-40 gave scale 4.1e-43
    and byte 0xFE (-448: 0 * inf = NaN through the clamp) for every zero input, i.e. zeros dequantised to -amax; the same for
    every row up to amax = 1.5 * 2^-120 = 1.13e-36 (scale 2.5e-39); amax = 2^-118 = 3.0e-36 (scale 6.7e-39, 1 / scale finite) and
    everything above passed, as did fp16 (smallest scale 2.7e-10).  With the floor those rows come back with scale 2^-126,
    zeros as 0x00 and amax as 2^126 amax (0x08 for 2^-133)."""
    o = ops()
    x16 = _range_rows(dt)
    Rr, C = x16.shape
    xb, xv = in_view(x16, 8, float("nan"))
    qb, q = out_view(Rr, C, torch.uint8, NAN8, left=8, right=8)
    s = torch.full((Rr,), float("nan"), device="cuda")
    o.quantize_rows_fp8(xv, q, s)
    torch.cuda.synchronize()
    x, sc, qc = x16.double(), s.cpu().double(), q.cpu()
    for r in range(Rr):
        print(f"range {dt} amax {x[r].abs().max().item():.4g}: scale {sc[r].item():.6g}, byte for a zero input 0x{int(qc[r, 1]):02X}, for amax 0x{int(qc[r, 0]):02X}")
    assert bool((torch.isfinite(sc) & (sc > 0)).all()), sc
    zero = x == 0
    assert bool(((qc[zero] & 0x7F) == 0).all()), f"zero inputs quantised to {sorted(set(qc[zero].tolist()))}"
    err = (R.dequant_rows(qc, sc) - x).abs()
    bound = R.quant_step(x, sc[:, None]) + RANGE_REL * x.abs() + RANGE_ABS
    assert bool((err <= bound).all()), (err / bound).amax(1)
    assert_pad_untouched("out", qb, Rr, C, 8, NAN8)


@pytest.mark.parametrize("dt", DTS)
def test_quantize_mx_range(dt):
    """the same rows through the block quantiser (its exponent is clamped to >= 1, so 1 / scale <= 2^126): exact exponents, exact
    bytes, zero inputs zero bytes"""
    o = ops()
    x16 = _range_rows(dt)
    Rr, C = x16.shape
    xb, xv = in_view(x16, 8, float("nan"))
    qb, q = out_view(Rr, C, torch.uint8, NAN8, left=8, right=8)
    e3 = R.mx_buffer(Rr, C, rows_pad=2, fill=0).cuda()
    o.quantize_mx_fp8(xv, q, e3)
    torch.cuda.synchronize()
    want_e, want_q = R.quantize_mx_ref(x16.double())
    assert_bytes("exponents", R.mx_rows(e3, Rr, C), want_e.to(torch.uint8))
    assert_bytes("bytes", q, want_q)
    x, qc = x16.double(), q.cpu()
    assert bool(((qc[x == 0] & 0x7F) == 0).all())
    err = (R.dequant_mx(qc, e3.cpu()) - x).abs()
    assert bool((err <= R.quant_step(x, torch.exp2(want_e.double() - 127).repeat_interleave(32, dim=1))).all())
    assert bool((e3[~R.mx_written_mask(e3, Rr, C)] == 0).all())
    assert_pad_untouched("out", qb, Rr, C, 8, NAN8)


# ---------------------------------------------------------------------------------------------------------------------------------
# layernorm_fwd_fp8
# ---------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(1, 4), (5, 100), (6, 256), (7, 260), (9, 768), (3, 1024)]      # NV = 1 (masked, full), 2 (masked), 3, 4; rows % 4 != 0; two work-groups


def _ln_run(x, gamma, beta):
    o = ops()
    rows, D = x.shape
    xb = torch.full((rows + 1, D + 4), float("nan"))
    xb[:rows, :D] = x
    xb = xb.cuda()
    qb, q = out_view(rows, D, torch.uint8, NAN8, left=0, right=12)
    s = torch.full((rows + 2,), float("nan"), device="cuda")
    o.layernorm_fwd_fp8(xb[:rows, :D], gamma.cuda(), beta.cuda(), q, s[:rows], rows=rows)
    torch.cuda.synchronize()
    assert_pad_untouched("ln out", qb, rows, D, 0, NAN8)
    assert bool(torch.isnan(s[rows:]).all())
    return q.cpu(), s[:rows].cpu()


def _ln_params(D, seed):
    g = gen(seed)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    for c in {1, D // 2, D - 1}:                                  # columns with gamma = beta = 0: y is exactly 0 there
        gamma[c] = 0.0
        beta[c] = 0.0
    return gamma, beta


def _ln_constant(D):
    """a constant c whose row the kernel's own mean formula, fp32(c D) * fp32(1 / D), gives back exactly (then x - mean = 0 and
    y = beta exactly); which small c do depends on how 1 / D rounds"""
    inv = torch.tensor(1.0) / torch.tensor(float(D))
    for c in (3.0, 5.0, 1.5, 7.0, 2.0, 0.75):
        if (torch.tensor(c * D) * inv).item() == c:
            return c
    raise AssertionError(D)


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_fp8_per_element(rows, D):
    """Per element |dequant - y| <= quant_step(y, scale) + 4 * 2^-24 * max_row |y| against the float64 LayerNorm y, and
    scale within 1e-5 of amax(y) / 448 (fp32 statistics against float64), at every D-dependent instantiation and mask; x with
    ldx = D + 4, out with ldo = D + 12.  Row 1 (from 5 rows up) is constant: y = beta exactly, so its scale and bytes are exact.
    Measured on an MI355X: scale off by at most 1.4e-7 relative (of 1e-5); no element used the 4 * 2^-24 term at all - the largest
    (err - quant_step) / (2^-24 max|y|) was -0.75 (9 x 768), i.e. every error stayed below its quantisation step."""
    g = gen(rows * 1000 + D)
    x = torch.randn(rows, D, generator=g)
    if rows >= 5:
        x[1] = _ln_constant(D)
    gamma, beta = _ln_params(D, D)
    q, s = _ln_run(x, gamma, beta)
    y = R.layernorm_ref(x, gamma, beta)
    ymax = y.abs().amax(1)
    assert bool(torch.isfinite(s).all())
    srel = ((s.double() - ymax / 448.0).abs() / (ymax / 448.0)).max().item()
    err = (R.dequant_rows(q, s) - y).abs()
    over = ((err - R.quant_step(y, s.double()[:, None])) / (2.0 ** -24 * ymax[:, None])).max().item()
    print(f"ln fp8 {rows}x{D}: scale rel {srel:.3g}, (err - quant_step) / (2^-24 rowmax) {over:.3g}")
    assert srel <= 1e-5, srel
    assert bool((err <= R.quant_step(y, s.double()[:, None]) + 4 * 2.0 ** -24 * ymax[:, None]).all()), over
    zc = (gamma == 0) & (beta == 0)
    assert bool(((q[:, zc] & 0x7F) == 0).all())                   # y = 0: a zero byte
    if rows >= 5:
        want_s = R.rows_scale_ref(beta.abs().amax()[None])
        assert s[1].item() == want_s.item()
        assert_bytes("constant row", q[1], R.encode_rne(beta.double() / want_s.double()))


def test_layernorm_fp8_large_mean_row():
    """mean >> std (1000 + randn): x - mean cancels three digits in fp32.  Held to the project's fp32 LayerNorm tolerance
    (test_kernels_gpu.py test_layernorm_fwd_bwd: atol 1e-5 + rtol 1e-5 of the largest |y|) on top of the quantisation step, and
    the scale to the same tolerance of amax(y) (plus the 2^-22 of the fp32 product).

    Measured on an MI355X: every row within its quantisation step (largest (err - quant_step) / tolerance -0.13; the large-mean
    row -0.17, like its ordinary neighbours) and |448 scale - amax(y)| - 2^-22 amax at most -0.006 of the tolerance.  Before
    ln_fwd_fp8_kernel corrected its fp32 mean (the mean of the centred values taken off again) the large-mean row missed this by
    12-13 %: tolerance 4.66e-5, scale term 5.24e-5, element term 5.27e-5 - near 1000 the fp32 mean alone is off by up to 3e-5."""
    D = 1024
    g = gen(5)
    x = torch.randn(3, D, generator=g)
    x[1] += 1000.0
    gamma, beta = _ln_params(D, 6)
    q, s = _ln_run(x, gamma, beta)
    y = R.layernorm_ref(x, gamma, beta)
    ymax = y.abs().amax(1)
    tol = 1e-5 + 1e-5 * ymax
    err = (R.dequant_rows(q, s) - y).abs()
    over = ((err - R.quant_step(y, s.double()[:, None])) / tol[:, None]).amax(1)
    sover = ((s.double() * 448.0 - ymax).abs() - 2.0 ** -22 * ymax) / tol
    print(f"ln fp8 large mean: (err - quant_step) / tol per row {over.tolist()}, (|448 scale - amax| - 2^-22 amax) / tol {sover.tolist()}")
    assert bool((sover <= 1.0).all()), sover
    assert bool((over <= 1.0).all()), over


# ---------------------------------------------------------------------------------------------------------------------------------
# gemm_fp8: exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact32(t, what):
    assert bool((t.float().double() == t).all()), f"test construction: {what} is not exact in fp32"
    return t


def _gemm_operands(M, N, K, seed, lo=-8, hi=8):
    A8, Av = R.int_operand(M, K, lo, hi, seed)
    B8, Bv = R.int_operand(N, K, lo, hi, seed + 1)
    return A8, Av, B8, Bv


def _row_col_scales(M, N):
    sa = torch.exp2((torch.arange(M) % 7 - 3).float())            # a scale from a neighbouring row or column is off by >= 2x
    sb = torch.exp2((torch.arange(N) % 5 - 2).float())
    return sa, sb


def _int_bias(N, seed):
    return torch.randint(-4, 5, (N,), generator=gen(seed)).float()


def _ld16(N):
    return 8 if N % 8 == 0 else (N + 7) // 8 * 8 - N             # 16-bit row stride: N + 8, or N rounded up to 8 (70 -> 72)


ROW_SHAPES = [(1, 8, 16), (15, 64, 128), (130, 72, 144), (300, 328, 384), (257, 70, 48)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act,with_bias", [(0, True), (0, False), (1, True), (1, False)])
@pytest.mark.parametrize("M,N,K", ROW_SHAPES)
def test_gemm_fp8_row_scales_exact(M, N, K, act, with_bias, dt):
    """Row / column scales, 16-bit output (OUT 0).  Integer operands in [-8, 8], power-of-two scales, integer bias: the fp32
    value is exact, so without activation the output is the single RNE rounding of the float64 result, bit for bit.  QuickGELU
    (expf / rcp) is not exact: held to the 16-bit unit roundoff plus the fp32-epilogue term of test_kernels_f16_gpu.py
    (2^-20 (|ref| + |pre| + |y|)), per element.  M = 1, M < 16, interior + fallback waves in one work-group (130 x 72),
    interior tile + three edge tiles with an odd K-tile count (300 x 328 x 384), one partial K-tile, N % 8 != 0 (scalar tail)."""
    o = ops()
    A8, Av, B8, Bv = _gemm_operands(M, N, K, M + N + K)
    sa, sb = _row_col_scales(M, N)
    bias = _int_bias(N, N) if with_bias else None
    pre = _exact32((Av @ Bv.t()) * sa.double()[:, None] * sb.double()[None, :] + (bias.double() if with_bias else 0.0), "pre-activation")
    Ab, A = in_view(A8, 16, NAN8)
    Bb, B = in_view(B8, 16, NAN8)
    ob, out = out_view(M, N, dt, float("nan"), left=0, right=_ld16(N))
    o.gemm_fp8(A, sa.cuda(), B, sb.cuda(), out, bias=None if bias is None else bias.cuda(), act=act)
    torch.cuda.synchronize()
    assert_pad_untouched("out16", ob, M, N, 0, float("nan"))
    got = out.cpu()
    if act == 0:
        want = pre.to(dt)
        assert torch.equal(got, want), (got.double() - want.double()).abs().max()
        return
    y = R.quickgelu_ref(pre)
    fin = y.abs() * (1 + 2.0 ** -9) < torch.finfo(dt).max          # (fp16: a few outputs of the largest shapes round to inf)
    assert not bool(torch.isnan(got).any())
    bound = U(dt) * y.abs() + FLOOR(dt) + 2.0 ** -20 * (2 * y.abs() + pre.abs())
    err = (got.double() - y).abs()
    assert bool((err[fin] <= bound[fin]).all()), (err[fin] / bound[fin]).max()


def _mxa_exponents(M, K, kind):
    m, b = torch.arange(M)[:, None], torch.arange(K // 32)[None, :]
    if kind == "unit":
        return torch.full((M, K // 32), 127)
    if kind == "equal":
        return torch.full((M, K // 32), 124)
    return 127 + ((3 * m + 5 * b) % 9 - 4)                         # mixed: neighbours in m and in b differ; span 2^-4 .. 2^4


def _mxa_setup(M, N, K, kind, seed):
    A8, Av, B8, Bv = _gemm_operands(M, N, K, seed)
    e = _mxa_exponents(M, K, kind)
    Aeff = Av * torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)
    ae = R.mx_put(R.mx_buffer(M, K, rows_pad=2, fill=0), e).cuda()
    _, sb = _row_col_scales(M, N)
    return A8, B8, Aeff @ Bv.t(), ae, sb


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,with_bias", [("unit", True), ("equal", False), ("mixed", True)])
@pytest.mark.parametrize("M,N,K", [(15, 64, 128), (130, 72, 256), (300, 328, 384)])
def test_gemm_fp8_block_scaled_a_exact(M, N, K, kind, with_bias, dt):
    """A with E8M0 exponent bytes 127 + ((3 m + 5 b) % 9 - 4) per (row m, k block b) (and all 127, all 124), 16-bit output: the
    sum's dynamic range stays below 2^24, the fp32 value is exact and the output its single rounding.  An exponent read from the
    neighbouring row, k block or K-tile changes some term by >= 2x.  The full span 2^-4 .. 2^4 is exact on an MI355X."""
    o = ops()
    A8, B8, acc, ae, sb = _mxa_setup(M, N, K, kind, M + N + K + 3)
    bias = _int_bias(N, N + 1) if with_bias else None
    ref = _exact32(_exact32(acc, "sum") * sb.double()[None, :] + (bias.double() if with_bias else 0.0), "result")
    Ab, A = in_view(A8, 16, NAN8)
    Bb, B = in_view(B8, 16, NAN8)
    ob, out = out_view(M, N, dt, float("nan"), left=0, right=_ld16(N))
    o.gemm_fp8(A, None, B, sb.cuda(), out, bias=None if bias is None else bias.cuda(), block_scale_a=ae)
    torch.cuda.synchronize()
    assert_pad_untouched("out16", ob, M, N, 0, float("nan"))
    want = ref.to(dt)
    assert torch.equal(out.cpu(), want), (out.cpu().double() - want.double()).abs().max()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,with_bias,alias", [("mixed", True, True), ("mixed", True, False), ("unit", False, False), ("equal", False, True)])
@pytest.mark.parametrize("M,N,K", [(40, 76, 128), (130, 328, 512), (300, 264, 384)])
def test_gemm_fp8_residual_f32_exact(M, N, K, kind, with_bias, alias, dt):
    """Block-scaled A onto the fp32 residual stream (OUT 2), integer residual, in place and into a separate buffer: the output
    equals the float64 reference bit for bit.  N % 8 != 0 (scalar tail, 40 x 76), interior + fallback waves (130 x 328, four
    K-tiles), three edge tiles and an odd K-tile count (300 x 264 x 384)."""
    o = ops()
    A8, B8, acc, ae, sb = _mxa_setup(M, N, K, kind, M + N + K + 4)
    bias = _int_bias(N, N + 2) if with_bias else None
    res = torch.randint(-16, 17, (M, N), generator=gen(M + N)).float()
    pre = _exact32(_exact32(acc, "sum") * sb.double()[None, :] + (bias.double() if with_bias else 0.0), "result")
    ref = _exact32(pre + res.double(), "result + residual")
    Ab, A = in_view(A8, 16, NAN8)
    Bb, B = in_view(B8, 16, NAN8)
    right = 4 if N % 4 == 0 else 8 - N % 4
    ob, out = out_view(M, N, torch.float32, float("nan"), left=0, right=right)
    if alias:
        out.copy_(res)
        resv = out
    else:
        rb, resv = out_view(M, N, torch.float32, float("nan"), left=0, right=right)
        resv.copy_(res)
    o.gemm_fp8(A, None, B, sb.cuda(), bias=None if bias is None else bias.cuda(), block_scale_a=ae, out_f32=out, residual=resv, half=dt)
    torch.cuda.synchronize()
    assert_pad_untouched("out_f32", ob, M, N, 0, float("nan"))
    assert torch.equal(out.cpu().double(), ref), (out.cpu().double() - ref).abs().max()
    if not alias:
        assert torch.equal(resv.cpu(), res)


MX_OUT_K, MX_OUT_HEAD = 256, 112


def _mx_out_setup(M, N, seed, positive):
    """Operands whose result has, in every (row, 32-column block), its amax at one known column n* with the exact value
    sa[m] * sb[n*] * 64 * cnt: A[m, k] = 8 for k < 112, B[n*, k] = +-8 for k < cnt (cnt = 112, 104, ... : amax mantissas 448,
    416, ..., 224 of fp8_ref.DYADIC_M) and 0 elsewhere in the row; every other row of B is 0 for k < 112 and holds integers in
    [-2, 2] beyond, as does A: |other| <= sa * 4 * (4 * 144) + 4 < amax.  n* is the block's first column with the largest sb."""
    K, H = MX_OUT_K, MX_OUT_HEAD
    g = gen(seed)
    Av = torch.randint(-2, 3, (M, K), generator=g).double()
    Bv = torch.randint(-2, 3, (N, K), generator=g).double()
    Av[:, :H] = 8.0
    Bv[:, :H] = 0.0
    cnts = [int(m) * 64 // 256 for m in R.DYADIC_M]              # 112, 104, 96, 88, 80, 72, 64, 60, 56
    nstar = []
    for blk in range(N // 32):
        n = next(c for c in range(32 * blk, 32 * blk + 32) if c % 5 == 4)
        sign = 1.0 if positive or blk % 2 == 0 else -1.0
        Bv[n] = 0.0
        Bv[n, :cnts[blk % len(cnts)]] = 8.0 * sign
        nstar.append(n)
    bias = _int_bias(N, seed + 7)
    bias[nstar] = 0.0
    return R.encode_rne(Av), Av, R.encode_rne(Bv), Bv, bias


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,act,with_bias", [(M, N, 0, True) for M in (1, 17, 260) for N in (64, 192, 320)] +
                         [(1, 192, 1, True), (17, 320, 1, False), (260, 64, 1, True), (260, 320, 0, False)])
def test_gemm_fp8_block_scaled_output_exact(M, N, act, with_bias, dt):
    """e4m3 + E8M0 output (OUT 1): every block's amax is sa[m] * sb[n*] * 64 * cnt, on the m * 2^k grid and different from row to
    row and block to block, so EVERY exponent byte equals e8m0_exact and every byte the RNE of the exact fp32 result (QuickGELU:
    the amax elements are large and positive, where the activation is the identity in fp32; the other bytes are compared where
    the float64 value is not within 2^-16 of an e4m3 tie).  N % 128 != 0 (64, 192, 320), M = 1, M < 16 and M > one tile."""
    o = ops()
    A8, Av, B8, Bv, bias = _mx_out_setup(M, N, M + N, positive=bool(act))
    if not with_bias:
        bias = None
    sa, sb = _row_col_scales(M, N)
    pre = _exact32((Av @ Bv.t()) * sa.double()[:, None] * sb.double()[None, :] + (bias.double() if with_bias else 0.0), "result")
    y = R.quickgelu_ref(pre) if act else pre
    amax = y.abs().view(M, N // 32, 32).amax(2)
    assert torch.equal(amax, pre.abs().view(M, N // 32, 32).amax(2))          # (the activation leaves the amax elements alone)
    Ab, A = in_view(A8, 16, NAN8)
    Bb, B = in_view(B8, 16, NAN8)
    qb, q = out_view(M, N, torch.uint8, NAN8, left=16, right=16)
    e3 = R.mx_buffer(M, N, rows_pad=2, fill=0).cuda()
    o.gemm_fp8(A, sa.cuda(), B, sb.cuda(), bias=None if bias is None else bias.cuda(), act=act, out_mx=(q, e3), half=dt)
    torch.cuda.synchronize()
    want_e, want_q = R.quantize_mx_ref(y)
    assert_bytes("exponents", R.mx_rows(e3, M, N), want_e.to(torch.uint8))
    assert bool((e3[~R.mx_written_mask(e3, M, N)] == 0).all()), "an exponent byte landed outside the output's own"
    assert_pad_untouched("out8", qb, M, N, 16, NAN8)
    got = q.cpu()
    if act:
        s = torch.exp2(want_e.double() - 127).repeat_interleave(32, dim=1)
        sure = ~R.near_tie(y / s, rel=2.0 ** -16) & (y.abs() / s > 2.0 ** -9)
        assert sure.float().mean() > 0.5
        assert_bytes("bytes", torch.where(sure, got, torch.zeros_like(got)), torch.where(sure, want_q, torch.zeros_like(got)))
        err = (R.dequant_mx(got, e3.cpu()) - y).abs()
        assert bool((err <= R.quant_step(y, s) + 2.0 ** -20 * (2 * y.abs() + pre.abs())).all())
    else:
        assert_bytes("bytes", got, want_q)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: block-scaled output
# ---------------------------------------------------------------------------------------------------------------------------------
_GRID = [v for v in R.E4M3[:0x7F].tolist() if 1.0 <= v <= 288.0]               # e4m3 values; between neighbours >= 6 % of the value


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,T,H,causal", [(2, 5, 2, False), (1, 50, 6, True), (2, 129, 4, False), (1, 257, 2, True)])
def test_attention_block_scaled_output_exact(B, T, H, causal, dt):
    """Every key of a (batch, head) carries the same V row, so the attention output is that row up to the rounding of the
    normalised probabilities (< 1 %, against >= 3 % to the nearest e4m3 tie).  The row's entries are e4m3 values times 2^k with
    amax 320 * 2^k and k = ((3 h + half) % 7) - 3 per 32-dim half of head h: EVERY exponent byte (127 + k) and EVERY e4m3 byte is
    determined.  Short kernel (T = 5, 50) and key-block-tiled kernel (T = 129, 257); the K-tile index h >> 1 and byte (2 h) & 3."""
    o = ops()
    D = H * 64
    g = gen(B * 1000 + T + H)
    vals = torch.tensor(_GRID, dtype=F64)
    scaled = vals[torch.randint(0, len(vals), (B, H, 2, 32), generator=g)]
    scaled = scaled * (torch.randint(0, 2, (B, H, 2, 32), generator=g).double() * 2 - 1)
    scaled = torch.where(torch.rand(B, H, 2, 32, generator=g) < 0.1, torch.zeros_like(scaled), scaled)
    pos = torch.randint(0, 32, (B, H, 2, 1), generator=g)
    scaled.scatter_(3, pos, 320.0 * (torch.randint(0, 2, (B, H, 2, 1), generator=g).double() * 2 - 1))
    k = ((3 * torch.arange(H)[:, None] + torch.arange(2)[None, :]) % 7 - 3).double()                      # [H, 2]
    vrow = (scaled * torch.exp2(k)[None, :, :, None]).reshape(B, 1, D)
    qkv = torch.randn(B * T, 3 * D + 8, generator=g)
    qkv[:, 2 * D:3 * D] = vrow.expand(B, T, D).reshape(B * T, D).float()
    qkv = qkv.to(dt).cuda()
    assert torch.equal(qkv[:, 2 * D:3 * D].cpu().double(), vrow.expand(B, T, D).reshape(B * T, D))
    wit = torch.full((B * T, D), float("nan"), dtype=dt, device="cuda")
    qb, q8 = out_view(B * T, D, torch.uint8, NAN8, left=16, right=16)
    e3 = R.mx_buffer(B * T, D, rows_pad=2, fill=0).cuda()
    o.attention_fwd(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], wit, B=B, T=T, H=H, causal=causal, out_mx=(q8, e3))
    torch.cuda.synchronize()
    want_e = (127 + k).reshape(1, 2 * H).expand(B * T, 2 * H).to(torch.uint8)
    want_q = R.encode_rne(scaled.reshape(B, 1, D).expand(B, T, D).reshape(B * T, D))
    assert_bytes("exponents", R.mx_rows(e3, B * T, D), want_e)
    assert_bytes("bytes", q8, want_q)
    assert bool((e3[~R.mx_written_mask(e3, B * T, D)] == 0).all()), "an exponent byte landed outside the output's own"
    assert_pad_untouched("o8", qb, B * T, D, 16, NAN8)
    assert bool(torch.isnan(wit).all())                           # the 16-bit output is only a dtype witness here
