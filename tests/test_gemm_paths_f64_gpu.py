"""GPU: the side paths behind `ops.gemm_bf16`, per element against float64 torch fed the operands exactly as stored, in both
dtypes: the skinny GEMV (csrc/gemm_skinny_impl.h), configuration 4 ("streaming", csrc/gemm_bf16_cfg4.hip), the folded-LayerNorm
forms of configuration 8 with cclip_rowstats_combine, and the fast epilogue forms of configurations 8 / 10 in fp16 as well as bf16.
Every logical output starts as NaN inside a canvas and must come back finite; the padding keeps its sentinel.

Bounds (tests/gemm_refs_f64.py; none is scaled by a tensor-wide maximum):
  * skinny: (ceil(K / 64) + 18) 2^-24 alpha |A| . |B| - the roundings of the kernel's own summation order, worst case - times
    (1 + slope) behind GELU-new, + 2^-20 (|ref| + |pre| + |residual| + |y|) + u |ref| + floor.  It must reject a reference with the
    single product k = K - 1 removed from one 8-column chunk of one row.
  * configuration 4, configurations 8 / 10, the producer's fp32 rows: the project bound exactly as test_gemm_epilogues_f64 builds it,
    with `_assert_sensitive` unchanged.
  * row-statistics partials: 8 2^-24 sum |x| and 8 2^-24 sum x^2 over the kernel's own 64 fp32 outputs of the block.
  * rowstats_combine: |d mean| <= (nblk + 1) 2^-24 sum|s1| / D, dv = (nblk + 3) 2^-24 (sum|s2| / D + 2 mean^2),
    |d rstd| / rstd <= dv / (2 (var + eps)) + 3 2^-24, on inputs with dv <= 0.1 (var + eps).
  * folded consumer: (rstd acc_bound + 2^-20 (rstd |acc| + rstd |mean c1| + |c2| + |pre|)) (1 + slope) + 2^-20 |y| + u |y| + floor.

Measured on an MI355X (largest err / bound per family; `pytest -s` prints them at the end of the module):
    family                       fp32 out   fp16 out   bf16 out
    skinny                        0.044      0.966      0.981
    cfg4 epilogue 0 / 1             -        0.953 / 0.966   0.990 / 0.991
    cfg4 epilogue 2               0.016        -          -
    cfg8, cfg10 QuickGELU (+pre)    -        0.955 (0.982)   0.987 (0.993)
    cfg8, cfg10 QuickGELU'          -        0.951      0.988
    producer rows                 0.028 (fp16 operands), 0.026 (bf16 operands)
    producer partial sum / sq     0.191 / 0.300 (fp16), 0.170 / 0.329 (bf16)
    combine mean / rstd           0.391 / 0.323
    folded consumer, act 0 / 1      -        0.975 / 0.974   0.993 / 0.990
  A 16-bit output sits just under 1 by construction: u |ref| is the rounding of the output itself and is reached by a value just
  above a power of two; what the kernels use of the rest of the bound is the fp32 column.

Conditioning of var = sum x^2 / D - mean^2 (producer + combine, D = 768, 256 fp32 rows of std 1): largest relative error of rstd
against float64 statistics of the same rows, next to cclip_layernorm_fwd (two-pass, centred) on the same rows, and the derived bound:
    mean / std    fold (producer + combine)    cclip_layernorm_fwd    derived bound
         0              1.4e-07                    1.2e-07              9.2e-07
         1              3.0e-07                    1.4e-07              3.5e-06
        10              2.0e-05                    1.3e-07              2.4e-04
       100              1.9e-03                    1.1e-07              2.3e-02
  (the same in both dtypes: the statistics are fp32).  The error grows with (mean / std)^2 as the formula predicts; the formula is not
  changed here.
"""
import pytest
import torch

from gemm_refs_f64 import (E24, FLOOR, SENT, SKINNY_SHAPES, U, WORST, _acc_bound, _assert_sensitive, _mats, _worst_report,  # noqa: F401
                           assert_skinny_sensitive, canvas, check_canvas, combine_partials, epilogue_bounds, epilogue_ref, fold_consumer_ref,
                           fold_pipeline_bound, rnd, rowstats_combine_ref, rowstats_partials_ref, skinny_bounds, skinny_operands, within)

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
NAN = float("nan")


def ops():
    from cclip_hip import ops as o
    return o


def err_type():
    from cclip_hip._lib import CclipError
    return CclipError


def G(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def dtn(dt):
    return str(dt).replace("torch.", "")


def in_canvas(t, rows_pad=2, left=8, right=16):
    """a copy of the fp32 matrix t inside a SENT frame (in-place residual on a padded row stride): (buffer, view)"""
    M, N = t.shape
    big = torch.full((M + rows_pad, left + N + right), SENT, device="cuda", dtype=t.dtype)
    v = big[:M, left:left + N]
    v.copy_(t)
    return big, v


def check_frame(name, big, v):
    keep = torch.ones_like(big, dtype=torch.bool)
    M, N = v.shape
    left = v.storage_offset() % big.stride(0)
    keep[:M, left:left + N] = False
    assert bool((big[keep] == SENT).all()), f"{name}: a write landed outside the logical output"


def col_slice(t, left=8, right=8):
    """the 16-bit matrix t as a column slice of a wider buffer (16-byte aligned start, row stride a multiple of 8).  The rest of
    the buffer is NaN - or, where K % 8 != 0, the sentinel: the entry point's contract wants finite pad columns there"""
    M, K = t.shape
    ld = left + (K + 7) // 8 * 8 + right
    wide = torch.full((M, ld), SENT if K % 8 else NAN, device=t.device, dtype=t.dtype)
    wide[:, left:left + K] = t
    return wide[:, left:left + K]


def refused(call, bufs, rows, cols):
    """the call raises CclipError and its canvases are untouched (NaN inside, SENT around)"""
    with pytest.raises(err_type()):
        call()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(b[:rows, :cols].isnan().all()), "a refused call wrote output"
        check_canvas("refused", b, rows, cols)


# ---------------------------------------------------------------------------------------------------------------------------
# skinny path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", SKINNY_SHAPES)
def test_skinny_f64(M, N, K, dt):
    """tile_config 0, layout (1, 0), N % 8 == 0, far below the autotune threshold: the call lands on the skinny kernel (K = 3080:
    over its LDS limit, on the tile kernels - same bound).  A's row stride is padded where K % 8 != 0 (the entry point takes
    multiples of 8 only), which is the scalar staging branch."""
    o = ops()
    assert 2.0 * M * N * K < o._TUNE_MIN_FLOPS / 16
    A_h, B_h, bias_h, res_h = skinny_operands(M, N, K, dt)
    A0, B, bias, res = A_h.cuda(), B_h.cuda(), bias_h.cuda(), res_h.cuda()
    A = A0 if K % 8 == 0 else col_slice(A0, left=0)
    assert A.stride(0) % 8 == 0
    Am, Bm = _mats(A, B, True, False)
    tag = f"skinny {M}x{N}x{K}"
    kw = dict(a_kcontig=True, b_kcontig=False, tile_config=0)

    # 1. 16-bit out, alpha = 0.5, bias
    e = epilogue_ref(Am, Bm, 0.5, bias, 0, None)
    bf, b16, _ = skinny_bounds(Am, Bm, 0.5, e, 0, dt)
    buf, out = canvas(M, N, dt)
    o.gemm_bf16(A, B, alpha=0.5, bias=bias, out_bf16=out, **kw)
    torch.cuda.synchronize()
    check_canvas("16-bit", buf, M, N)
    within(f"{tag} 16-bit", out, e["ref"], b16)
    assert_skinny_sensitive(out, e["ref"], b16, Am, Bm, 0.5)

    # 2. GELU-new with the pre-activation
    e = epilogue_ref(Am, Bm, 1.0, bias, 3, None)
    bf, b16, bp = skinny_bounds(Am, Bm, 1.0, e, 3, dt)
    (buf, out), (bufp, outp) = canvas(M, N, dt), canvas(M, N, dt)
    o.gemm_bf16(A, B, bias=bias, act=3, out_bf16=out, out_pre=outp, **kw)
    torch.cuda.synchronize()
    check_canvas("gelu", buf, M, N); check_canvas("pre", bufp, M, N)
    within(f"{tag} gelu", out, e["ref"], b16)
    within(f"{tag} pre", outp, e["pre"], bp)
    assert_skinny_sensitive(out, e["ref"], b16, Am, Bm, 1.0, e["slope"])
    assert_skinny_sensitive(outp, e["pre"], bp, Am, Bm, 1.0)

    # 3. fp32 residual in place on a padded ldc; configuration 1 on the same call meets the same bound
    e = epilogue_ref(Am, Bm, 0.5, bias, 0, res)
    bf, _, _ = skinny_bounds(Am, Bm, 0.5, e, 0, dt)
    for tc, nm in ((0, "residual"), (1, "residual-cfg1")):
        big, x = in_canvas(res)
        o.gemm_bf16(A, B, alpha=0.5, bias=bias, residual=x, out_f32=x, a_kcontig=True, b_kcontig=False, tile_config=tc)
        torch.cuda.synchronize()
        check_frame(nm, big, x)
        within(f"{tag} {nm}", x, e["ref"], bf)
        assert_skinny_sensitive(x, e["ref"], bf, Am, Bm, 0.5)

    # 4. fp32 and 16-bit outputs together
    e = epilogue_ref(Am, Bm, 1.0, bias, 0, None)
    bf, b16, _ = skinny_bounds(Am, Bm, 1.0, e, 0, dt)
    (buf, out), (buf16, out16) = canvas(M, N, torch.float32), canvas(M, N, dt)
    o.gemm_bf16(A, B, bias=bias, out_f32=out, out_bf16=out16, **kw)
    torch.cuda.synchronize()
    check_canvas("both f32", buf, M, N); check_canvas("both 16", buf16, M, N)
    within(f"{tag} both", out, e["ref"], bf)
    within(f"{tag} both", out16, e["ref"], b16)
    assert_skinny_sensitive(out, e["ref"], bf, Am, Bm, 1.0)
    assert torch.equal(out16, out.to(dt)), "the 16-bit output is the rounded fp32 output"

    # 5. no bias;  6. A with more rows than M (NaN rows, M=);  7. A as a column slice of a wider buffer
    e = epilogue_ref(Am, Bm, 1.0, None, 0, None)
    bf, b16, _ = skinny_bounds(Am, Bm, 1.0, e, 0, dt)
    A_wide = torch.full((M + 3, A.stride(0)), NAN, device="cuda", dtype=dt)
    if K % 8:
        A_wide[:M] = SENT                                     # finite pad columns of the live rows (the entry point's contract)
    A_more = A_wide[:, :K]
    A_more[:M] = A
    for nm, Ax, kx in (("nobias", A, {}), ("morerows", A_more, dict(M=M)), ("colslice", col_slice(A0), {})):
        assert Ax.stride(0) % 8 == 0 and Ax.data_ptr() % 16 == 0
        buf, out = canvas(M, N, torch.float32)
        o.gemm_bf16(Ax, B, out_f32=out, **kw, **kx)
        torch.cuda.synchronize()
        check_canvas(nm, buf, M, N)
        within(f"{tag} {nm}", out, e["ref"], bf)
        assert_skinny_sensitive(out, e["ref"], bf, Am, Bm, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# configuration 4
# ---------------------------------------------------------------------------------------------------------------------------
# (M, N, K, epilogue, act, bias, operands as column slices, in place)
CFG4 = [
    (256, 128, 512, 0, 0, True, False, False),       # kt == 8: the floor and the production depth
    (256, 128, 456, 0, 0, False, False, False),      # kt == 8 with a ragged last K-tile; no bias
    (512, 512, 512, 0, 1, True, True, False),        # the tuned production shape class, QuickGELU; lda, ldb > K
    (512, 512, 512, 1, 1, True, True, False),        # QuickGELU + out_pre; lda, ldb > K
    (512, 512, 512, 1, 1, False, False, False),      # ... without bias
    (256, 128, 640, 2, 0, True, True, True),         # kt == 10: the epilogue-2 floor, in place; lda, ldb > K
    (512, 256, 704, 2, 0, False, False, False),      # not in place, ldr != ldc (both multiples of 4); no bias
    (256, 4096, 512, 0, 0, True, False, False),      # the last columns of the LDS bias table
    (8448, 1024, 512, 0, 0, True, False, False),     # 264 tiles: work-groups 0..7 walk two tiles, the rest one
    (8448, 1024, 640, 2, 0, True, False, True),      # the same 264 tiles at epilogue 2's own floor, kt == 10 (it refuses K = 512: kt == 8)
    (66560, 128, 512, 0, 0, True, False, False),     # 260 tiles with tiles_n == 1
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,epi,act,has_bias,sliced,inplace", CFG4)
def test_cfg4_streaming_f64(M, N, K, epi, act, has_bias, sliced, inplace, dt):
    """Configuration 4 at its minimum depths, with alpha, with and without bias, padded lda / ldb / ldc, the full LDS bias table and
    unequal tile counts per work-group; each case launched twice into fresh canvases: bit-equal (a miscounted wait shows as a
    difference between runs)."""
    o = ops()
    g = G(M + 3 * N + 7 * K + epi)
    A, B = rnd((M, K), dt, g, 0.1), rnd((N, K), dt, g)
    if sliced:
        A, B = col_slice(A), col_slice(B)
        assert A.stride(0) > K and B.stride(0) > K
    bias = torch.randn(N, device="cuda", generator=g) if has_bias else None
    res = torch.randn(M, N, device="cuda", generator=g) if epi == 2 else None
    Am, Bm = _mats(A, B, True, True)
    e = epilogue_ref(Am, Bm, 0.5, bias, act, res)
    bf, b16, bp = epilogue_bounds(_acc_bound(Am, Bm, 0.5), e, dt)
    tag = f"cfg4-epi{epi} {M}x{N}x{K}"
    runs = []
    for _ in range(2):
        if epi == 2 and inplace:
            big, x = in_canvas(res)
            o.gemm_bf16(A, B, alpha=0.5, bias=bias, residual=x, out_f32=x, tile_config=4)
            torch.cuda.synchronize()
            check_frame(tag, big, x)
            runs.append((x,))
        elif epi == 2:
            rb = torch.full((M, N + 4), NAN, device="cuda")
            r = rb[:, :N]
            r.copy_(res)
            buf, out = canvas(M, N, torch.float32)
            assert r.stride(0) != out.stride(0) and r.stride(0) % 4 == 0
            o.gemm_bf16(A, B, alpha=0.5, bias=bias, residual=r, out_f32=out, tile_config=4)
            torch.cuda.synchronize()
            check_canvas(tag, buf, M, N)
            assert torch.equal(r, res), "the residual was written"
            runs.append((out,))
        else:
            (buf, out), (bufp, outp) = canvas(M, N, dt), canvas(M, N, dt)
            o.gemm_bf16(A, B, alpha=0.5, bias=bias, act=act, out_bf16=out, out_pre=outp if epi == 1 else None, tile_config=4)
            torch.cuda.synchronize()
            check_canvas(tag, buf, M, N)
            if epi == 1:
                check_canvas(tag + " pre", bufp, M, N)
            runs.append((out, outp) if epi == 1 else (out,))
    got = runs[0][0]
    bound = bf if epi == 2 else b16
    within(tag, got, e["ref"], bound)
    _assert_sensitive(got, e["ref"], bound, Am, Bm, 0.5, e["slope"])
    if epi == 1:
        within(tag + " pre", runs[0][1], e["pre"], bp)
        _assert_sensitive(runs[0][1], e["pre"], bp, Am, Bm, 0.5)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two launches of the same call differ"


@pytest.mark.parametrize("dt", DTS)
def test_cfg4_refusals_leave_the_output_alone(dt):
    o = ops()
    g = G(4)
    M = 256

    def ab(N, K):
        return rnd((M, K), dt, g, 0.1), rnd((N, K), dt, g)

    A, B = ab(4224, 512)                                     # one 128-column tile past the LDS bias table
    buf, out = canvas(M, 4224, dt)
    refused(lambda: o.gemm_bf16(A, B, out_bf16=out, tile_config=4), [buf], M, 4224)
    A, B = ab(128, 448)                                      # kt == 7, epilogue 0
    buf, out = canvas(M, 128, dt)
    refused(lambda: o.gemm_bf16(A, B, out_bf16=out, tile_config=4), [buf], M, 128)
    A, B = ab(128, 576)                                      # kt == 9, epilogue 2
    res = torch.randn(M, 136, device="cuda", generator=g)[:, :128]
    buf, out = canvas(M, 128, torch.float32)
    assert res.stride(0) == out.stride(0)
    refused(lambda: o.gemm_bf16(A, B, residual=res, out_f32=out, tile_config=4), [buf], M, 128)
    A, B = ab(128, 640)
    (buf, out), (buf16, out16) = canvas(M, 128, torch.float32), canvas(M, 128, dt)
    refused(lambda: o.gemm_bf16(A, B, out_f32=out, out_bf16=out16, tile_config=4), [buf, buf16], M, 128)
    aux = rnd((M, 136), dt, g)[:, :128]
    refused(lambda: o.gemm_bf16(A, B, act=16, aux=aux, out_bf16=out16, tile_config=4), [buf16], M, 128)
    refused(lambda: o.gemm_bf16(A, B, aux=aux, out_bf16=out16, tile_config=4), [buf16], M, 128)


# ---------------------------------------------------------------------------------------------------------------------------
# folded LayerNorm on configuration 8
# ---------------------------------------------------------------------------------------------------------------------------
def partial_canvas(nblk, M):
    n = nblk * M * 2
    flat = torch.full((n + 64,), SENT, device="cuda")
    flat[:n] = NAN
    return flat, flat[:n].view(nblk, M, 2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 320)])
def test_fold_producer_f64(M, N, K, inplace, dt):
    """rowstats_out: the fp32 rows against fp64, the 16-bit copy == the rounded fp32 rows, every (sum, sum of squares) partial against
    the fp64 sums of the kernel's own 64 fp32 outputs of its block."""
    o = ops()
    g = G(M + N + K + inplace)
    A, B = rnd((M, K), dt, g, 0.2), rnd((N, K), dt, g, 0.5)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g) * 2.0 + 0.7
    Am, Bm = _mats(A, B, True, True)
    e = epilogue_ref(Am, Bm, 0.5, bias, 0, res)
    bf, _, _ = epilogue_bounds(_acc_bound(Am, Bm, 0.5), e, dt)
    buf, out = canvas(M, N, torch.float32)
    buf16, out16 = canvas(M, N, dt)
    if inplace:
        out.copy_(res)
        r = out
    else:
        rbuf, r = canvas(M, N, torch.float32)
        r.copy_(res)
    flat, part = partial_canvas(N // 64, M)
    o.gemm_bf16(A, B, alpha=0.5, bias=bias, residual=r, out_f32=out, out_bf16=out16, rowstats_out=part)
    torch.cuda.synchronize()
    check_canvas("rows", buf, M, N); check_canvas("16-bit rows", buf16, M, N)
    assert bool((flat[part.numel():] == SENT).all()), "a partial landed past the buffer"
    if not inplace:
        assert torch.equal(r, res)
    within(f"fold-rows {M}x{N}x{K}", out, e["ref"], bf, dt=dt)
    _assert_sensitive(out, e["ref"], bf, Am, Bm, 0.5)
    assert torch.equal(out16, out.to(dt)), "the 16-bit copy is the rounded fp32 row"
    pref, pbound = rowstats_partials_ref(out)
    assert bool(torch.isfinite(part).all()), "a partial was not written"
    within("fold-partial-sum", part[:, :, 0], pref[:, :, 0], pbound[:, :, 0], dt=dt)
    within("fold-partial-sq", part[:, :, 1], pref[:, :, 1], pbound[:, :, 1], dt=dt)


@pytest.mark.parametrize("nblk", [1, 4, 12, 16])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_rowstats_combine_f64(rows, nblk):
    o = ops()
    D = 64 * nblk
    part = combine_partials(rows, nblk, torch.Generator().manual_seed(rows * 17 + nblk)).cuda()
    sbuf = torch.full((rows + 2, 2), SENT, device="cuda")
    sbuf[:rows] = NAN
    o.rowstats_combine(part, sbuf[:rows], rows=rows, D=D)
    torch.cuda.synchronize()
    assert bool((sbuf[rows:] == SENT).all()), "a row past `rows` was written"
    r = rowstats_combine_ref(part, D)
    assert bool((r["dv"] <= 0.1 * (r["var"] + 1e-5)).all()), "the first-order bound on rstd needs dv <= 0.1 (var + eps)"
    assert r["raw"][0] <= 0.0, "the constant row must reach the clamp"
    within("combine-mean", sbuf[:rows, 0], r["mean"], r["b_mean"])
    within("combine-rstd", sbuf[:rows, 1], r["rstd"], r["b_rstd"] * r["rstd"])


COND = {}


@pytest.mark.parametrize("dt", DTS)
def test_fold_statistics_conditioning(dt):
    """fp32 rows of std 1 and mean 0, 1, 10, 100 through producer (A = 0: the rows pass through unchanged) and combine, against
    float64 statistics of the same rows: asserted against the derived bound only; the measured errors are printed and recorded in
    the module docstring and DESIGN.md."""
    o = ops()
    M, D, K = 256, 768, 128
    A = torch.zeros(M, K, device="cuda", dtype=dt)
    B = rnd((D, K), dt, G(1))
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    for mu in (0.0, 1.0, 10.0, 100.0):
        x0 = (torch.randn(M, D, device="cuda", generator=G(int(mu) + 5)) + mu).contiguous()
        x = x0.clone()
        xb = torch.empty(M, D, device="cuda", dtype=dt)
        part = torch.full((D // 64, M, 2), NAN, device="cuda")
        o.gemm_bf16(A, B, residual=x, out_f32=x, out_bf16=xb, rowstats_out=part)
        assert torch.equal(x, x0)
        stats = torch.full((M, 2), NAN, device="cuda")
        o.rowstats_combine(part, stats, rows=M, D=D)
        mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        o.layernorm_fwd(x0, gamma, beta, rows=M, out_f32=torch.empty_like(x0), mean=mean, rstd=rstd)
        torch.cuda.synchronize()
        r = fold_pipeline_bound(x0, D)
        assert bool((r["dv"] <= 0.1 * (r["var"] + 1e-5)).all())
        rel_fold = ((stats[:, 1].double() - r["rstd"]).abs() / r["rstd"])
        rel_ln = ((rstd.double() - r["rstd"]).abs() / r["rstd"]).max().item()
        COND[(mu, dtn(dt))] = (rel_fold.max().item(), rel_ln, r["b_rstd"].max().item())
        print(f"conditioning mean/std {mu:>5g} {dtn(dt):<9} fold rstd rel err {rel_fold.max().item():.3g}  layernorm_fwd {rel_ln:.3g}  "
              f"bound {r['b_rstd'].max().item():.3g}")
        within(f"fold-cond-rstd-mean{mu:g}", stats[:, 1], r["rstd"], r["b_rstd"] * r["rstd"], dt=dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 320)])
def test_fold_consumer_f64(M, N, K, act, dt):
    """ln_stats / ln_c1 with statistics that are random per row and constants that are random per column: a row or column mix-up
    shows."""
    o = ops()
    g = G(M + N + K + act)
    xb, ws = rnd((M, K), dt, g), rnd((N, K), dt, g, 0.1)
    stats = torch.empty(M, 2, device="cuda")
    stats[:, 0] = torch.rand(M, device="cuda", generator=g) * 4 - 2
    stats[:, 1] = 0.1 * 100.0 ** torch.rand(M, device="cuda", generator=g)
    c1, c2 = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
    Am, Bm = _mats(xb, ws, True, True)
    r = fold_consumer_ref(Am, Bm, 0.5, stats, c1, c2, act, dt)
    buf, out = canvas(M, N, dt)
    o.gemm_bf16(xb, ws, alpha=0.5, bias=c2, act=act, out_bf16=out, ln_stats=stats, ln_c1=c1)
    torch.cuda.synchronize()
    check_canvas("fold consumer", buf, M, N)
    within(f"fold-consumer-act{act} {M}x{N}x{K}", out, r["y"], r["bound"])
    _assert_sensitive(out, r["y"], r["bound"], Am, Bm, 0.5, r["slope"] * r["rstd"])


@pytest.mark.parametrize("dt", DTS)
def test_fold_refusals_leave_the_output_alone(dt):
    o = ops()
    g = G(8)
    M, K = 256, 128
    A = rnd((M, K), dt, g)
    stats = torch.ones(M, 2, device="cuda")
    for N, kw in ((384, dict(ln_c1=True)), (256, dict(ln_c1=False)), (256, dict(ln_c1=True, residual=True))):
        B = rnd((N, K), dt, g)
        c1 = torch.zeros(N, device="cuda") if kw["ln_c1"] else None
        buf, out = canvas(M, N, dt)
        res = torch.zeros(M, out.stride(0), device="cuda")[:, :N] if kw.get("residual") else None
        refused(lambda: o.gemm_bf16(A, B, out_bf16=out, ln_stats=stats, ln_c1=c1, residual=res), [buf], M, N)
    N = 256
    B = rnd((N, K), dt, g)
    (buf, out), (buf16, out16) = canvas(M, N, torch.float32), canvas(M, N, dt)
    flat, part = partial_canvas(N // 64, M)
    res_other = torch.zeros(M, out.stride(0) + 4, device="cuda")[:, :N]
    refused(lambda: o.gemm_bf16(A, B, residual=res_other, out_f32=out, out_bf16=out16, rowstats_out=part), [buf, buf16], M, N)
    res_same = torch.zeros(M, out.stride(0), device="cuda")[:, :N]
    refused(lambda: o.gemm_bf16(A, B, act=1, residual=res_same, out_f32=out, out_bf16=out16, rowstats_out=part), [buf, buf16], M, N)
    assert bool(part.isnan().all()) and bool((flat[part.numel():] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------
# configurations 8 and 10: the fast epilogue forms and the persistent ring, in both dtypes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg", [8, 10])
@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (300, 264, 256)])
def test_cfg8_cfg10_fast_forms_equal_cfg3(M, N, K, cfg, dt):
    """16-bit out; 16-bit out + out_pre with QuickGELU; fp32 residual in place; QuickGELU' with ldaux == ldc and != ldc: each
    bit-equal to configuration 3; one form per shape also against fp64 (interior shape: QuickGELU + pre; ragged shape: QuickGELU')."""
    o = ops()
    g = G(M + N + K)
    A, B = rnd((M, K), dt, g, 0.1), rnd((N, K), dt, g)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g)
    aux0 = rnd((M, N), dt, g)
    Am, Bm = _mats(A, B, True, True)
    interior = M % 256 == 0

    def run(form, tc):
        """-> (outputs, frames to check)"""
        kw = dict(alpha=0.5, bias=bias, tile_config=tc)
        if form == "res":
            big, x = in_canvas(res)
            o.gemm_bf16(A, B, residual=x, out_f32=x, **kw)
            torch.cuda.synchronize()
            check_frame(form, big, x)
            return (x,)
        buf, out = canvas(M, N, dt)
        bufp, outp = canvas(M, N, dt)
        if form == "out16":
            o.gemm_bf16(A, B, out_bf16=out, **kw)
        elif form == "pre":
            o.gemm_bf16(A, B, act=1, out_bf16=out, out_pre=outp, **kw)
        else:
            ld = out.stride(0) + (0 if form == "dact" else 8)
            aux = torch.full((M, ld), NAN, device="cuda", dtype=dt)[:, :N]
            aux.copy_(aux0)
            o.gemm_bf16(A, B, act=16, aux=aux, out_bf16=out, **kw)
        torch.cuda.synchronize()
        check_canvas(form, buf, M, N)
        if form == "pre":
            check_canvas(form + " pre", bufp, M, N)
            return (out, outp)
        return (out,)

    for form in ("out16", "pre", "res", "dact", "dact-ldaux"):
        got, want = run(form, cfg), run(form, 3)
        for a, b in zip(got, want):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"configuration {cfg} differs from configuration 3 on form {form}"
        if form == "pre" and interior:
            e = epilogue_ref(Am, Bm, 0.5, bias, 1, None)
            bf, b16, bp = epilogue_bounds(_acc_bound(Am, Bm, 0.5), e, dt)
            within(f"cfg{cfg}-quickgelu", got[0], e["ref"], b16)
            within(f"cfg{cfg}-pre", got[1], e["pre"], bp)
            _assert_sensitive(got[0], e["ref"], b16, Am, Bm, 0.5, e["slope"])
            _assert_sensitive(got[1], e["pre"], bp, Am, Bm, 0.5)
        if form == "dact-ldaux" and not interior:
            e = epilogue_ref(Am, Bm, 0.5, bias, 16, None, aux0)
            bf, b16, bp = epilogue_bounds(_acc_bound(Am, Bm, 0.5), e, dt)
            within(f"cfg{cfg}-dquickgelu", got[0], e["ref"], b16)
            _assert_sensitive(got[0], e["ref"], b16, Am, Bm, 0.5, e["slope"])


@pytest.mark.parametrize("dt", DTS)
def test_cfg10_ring_with_unequal_tile_counts(dt):
    """(8448, 2048, 192): 264 tiles over the work-groups; bit-equal to configuration 3, and again on a second launch"""
    o = ops()
    M, N, K = 8448, 2048, 192
    g = G(10)
    A, B = rnd((M, K), dt, g), rnd((N, K), dt, g)
    bias = torch.randn(N, device="cuda", generator=g)
    outs = []
    for tc in (3, 10, 10):
        buf, out = canvas(M, N, dt)
        o.gemm_bf16(A, B, bias=bias, out_bf16=out, tile_config=tc)
        torch.cuda.synchronize()
        check_canvas(f"cfg{tc}", buf, M, N)
        assert bool(torch.isfinite(out).all())
        outs.append(out)
    assert torch.equal(outs[1], outs[0]), "configuration 10 differs from configuration 3"
    assert torch.equal(outs[2], outs[1]), "two launches of configuration 10 differ"
