"""GPU: the fp32 glue kernels every training and caption step runs between the GEMMs and the attention (csrc/layernorm.hip,
loss.hip, embed.hip, optim.hip, gemm_f32.hip and scale_f32) against the hand-written float64 references of
tests/kernel_refs_f64.py (pinned against torch's float64 operators by tests/test_kernel_refs_f64_cpu.py), per element, at the
shapes where such kernels go wrong: padded row strides, lanes that own no column and half-filled last chunks, the first row
count past every grid cap (with the narrowest row that crosses it), the second unrolled AdamW slot, ties, ignored rows,
constant and zero rows, clamped ids.

The bounds are those of tests/kernel_refs_f64.py (forms and derivations in its header); nothing is scaled by a tensor-wide
maximum, and the constants (C_RED = 2, EXP_F = 4, the per-expression rounding counts) were fixed before the first run.  Every
reduction family also shows that its bound REJECTS a reference with one planted error of the smallest structural size
(kernel_refs_f64.PLANTED).  Conventions of tests/test_kernels_f16_gpu.py, whose helpers are imported: logical outputs start as
NaN and must come back finite; padding columns of a wide row stride and rows past the logical end hold a sentinel that must
survive (input padding holds NaN, so a read of it poisons the result); the worst err / bound per family is printed at the end
of the module (pytest -s).

Measured on an MI355X, worst err / bound per family (a ratio above 1 would be a finding):
    ln.fwd 0.45 (16-bit out 0.99)   ln.bwd dx 0.15 (16-bit 0.99)   ln.bwd dgamma 0.29   ln.bwd dbeta 0.33   vit_embed_ln 0.39 (16390 rows)
    embed_grad segsum 0.42, atomics 0.48 - 0.58 (hardware order)   colsum 16-bit in 0.47, f32 in 0.38   l2norm.fwd 0.37   l2norm.bwd 0.54
    xent loss 0.065   xent dlogits 0.95 (16-bit 0.97)   xent rowdot 0.045   reduce_dot 0.086
    adamw p 0.71, m 0.27, v 0.20   gemm_f32 0.35
  xent dlogits: the 0.95 did not move when the argument-rounding term of the softmax bound was cut from EPS to E a, so it does
  not come from the rounding terms; the likely source is a probability in fp32's subnormal range (logits spanning 200) flushed
  to zero against the 2^-126 floor.  The 16-bit figures sit just under 1 by construction (the u |ref| term is exactly one
  rounding of the output).  Every bit-equality check (gathers, x0, shadows, casts, the scale, n = 4 against the long AdamW
  run, repeated launches) held; no kernel was changed.
"""
import pytest
import torch

import kernel_refs_f64 as KR
from test_kernels_f16_gpu import DTS, FLOOR, SENT, U, check_canvas

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST32 = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_report_f32():
    yield
    for fam, r in sorted(WORST32.items()):
        print(f"worst err/bound  {fam:<28} {r:.3g}")


def ops():
    from cclip_hip import ops as o
    return o


def err_type():
    from cclip_hip._lib import CclipError
    return CclipError


def cu(t):
    return None if t is None else t.cuda()


def chk(fam, what, got, ref, bound):
    """every output finite and |got - ref| <= bound per element, on the host (got: a device tensor); the largest err / bound is
    recorded under the family's name in this module's own table"""
    got64 = got.detach().cpu().double()
    fin = torch.isfinite(got64)
    assert bool(fin.all()), f"{fam} {what}: {int((~fin).sum())} non-finite outputs, first {(~fin).nonzero()[:4].tolist()}"
    err = (got64 - ref).abs()
    ratio = err / (bound + 1e-300)
    bad = ~(err <= bound + 1e-300)
    if bool(bad.any()):
        t = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"{fam} {what}: {int(bad.sum())}/{bad.numel()} outside the bound; first {list(t)}: got {got64[t].item():.9g} ref "
                    f"{ref[t].item():.9g} bound {bound[t].item():.3g}; worst err/bound {ratio.max().item():.3g}")
    WORST32[fam] = max(WORST32.get(fam, 0.0), ratio.max().item())


def b16(bound, ref, dt):
    """a 16-bit output adds one rounding"""
    return bound + U(dt) * ref.abs() + FLOOR(dt)


def out_buf(rows, cols, ld, dt=torch.float32, extra=2):
    """(buffer, logical view): NaN inside [rows, cols], SENT in the padding columns and in `extra` rows past the end"""
    buf = torch.full((rows + extra, ld), SENT, device="cuda", dtype=dt)
    buf[:rows, :cols] = NAN
    return buf, buf[:rows, :cols]


def in_pad(t, ld):
    """the operand on a row stride of ld elements, NaN in the padding columns"""
    rows, cols = t.shape
    buf = torch.full((rows, ld), NAN, device="cuda", dtype=t.dtype)
    buf[:, :cols] = t.cuda()
    return buf[:, :cols]


def vec(n, fill=NAN, dt=torch.float32, extra=2):
    """(buffer, logical view) of a vector output with `extra` sentinel elements behind it"""
    buf = torch.full((n + extra,), SENT if dt.is_floating_point else int(SENT), device="cuda", dtype=dt)
    buf[:n] = fill
    return buf, buf[:n]


def tail_ok(buf, n):
    return bool((buf[n:] == (SENT if buf.is_floating_point() else int(SENT))).all())


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
LN_DS = [4, 100, 260, 772, 1020, 1024]


def _ln_inputs(D, kind, n_src=11):
    g = KR.gen(D * 3 + (kind == "far"))
    x = torch.randn(n_src, D, generator=g) + 1e3 if kind == "far" else torch.randn(n_src, D, generator=g) * 2 + 0.5
    x[1] = 0.75                                            # a constant row: var = 0, rstd = 1 / sqrt(eps)
    x[2] = 0.0
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    idx = torch.tensor([9, 1, 2, 0, 10, 4, 6], dtype=torch.int32)          # a permuted subset; rows 3, 5, 7, 8 are not selected
    return g, x, gamma, beta, idx


@pytest.mark.parametrize("kind", ["plain", "far"])
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_fwd_f64(D, kind):
    """ln_fwd_kernel at every D class: lanes that own no column (D = 4, 100), a half-empty last 256-column chunk (260, 772, 1020),
    the full width; x and the outputs each on their own padded row stride; a constant row and a row of zeros; row_index as a
    permuted subset; fp32 and 16-bit outputs (both dtypes); mean / rstd present and absent.  kind 'far': row mean 1e3, std 1 -
    the error allowed is a rounding of the mean, (2 sqrt(D) + 1) E |mean| rstd (up to 65 half-ulps of x at D = 1024): a one-pass
    variance (E[x^2] - mean^2, error about E sqrt(D) 1e6 against a variance of 1) would miss it by about an order of magnitude."""
    o = ops()
    _, x, gamma, beta, idx = _ln_inputs(D, kind)
    rows = idx.numel()
    ref, bnd = KR.ln_fwd(x, gamma, beta, row_index=idx)
    xd, gd, bd, idxd = in_pad(x, D + 4), cu(gamma), cu(beta), cu(idx)
    buf, out = out_buf(rows, D, D + 12)
    mb, mean = vec(rows)
    rb, rstd = vec(rows)
    o.layernorm_fwd(xd, gd, bd, rows=rows, row_index=idxd, out_f32=out, mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    check_canvas("ln out", buf, rows, D)
    assert tail_ok(mb, rows) and tail_ok(rb, rows)
    chk("ln.fwd", f"y D{D} {kind}", out, ref["y"], bnd["y"])
    chk("ln.fwd", f"mean D{D} {kind}", mean, ref["mean"], bnd["mean"])
    chk("ln.fwd", f"rstd D{D} {kind}", rstd, ref["rstd"], bnd["rstd"])
    for dt in DTS:                                          # 16-bit copy next to the fp32 one (shared row stride), no statistics
        buf16, out16 = out_buf(rows, D, D + 12, dt)
        buf, out = out_buf(rows, D, D + 12)
        o.layernorm_fwd(xd, gd, bd, rows=rows, row_index=idxd, out_bf16=out16, out_f32=out)
        torch.cuda.synchronize()
        check_canvas("ln out16", buf16, rows, D)
        chk("ln.fwd 16-bit", f"y D{D} {kind} {dt}", out16, ref["y"], b16(bnd["y"], ref["y"], dt))
        chk("ln.fwd", f"y (with 16-bit) D{D} {kind}", out, ref["y"], bnd["y"])
    # no row_index: the first rows of x
    ref2, bnd2 = KR.ln_fwd(x[:rows], gamma, beta)
    buf, out = out_buf(rows, D, D + 12)
    o.layernorm_fwd(xd, gd, bd, rows=rows, out_f32=out)
    torch.cuda.synchronize()
    check_canvas("ln out", buf, rows, D)
    chk("ln.fwd", f"y no index D{D} {kind}", out, ref2["y"], bnd2["y"])


@pytest.mark.parametrize("kind", ["plain", "far"])
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_bwd_f64(D, kind):
    """ln_bwd_kernel + ln_bwd_reduce_kernel at every D class with the saved statistics as operands: dy, x and dx / dx_res on
    their own padded strides; row_index as a permuted subset - dx rows that are not selected keep their sentinel; accumulate
    on and off; the dgamma / dbeta pair, the fp32 dx and the 16-bit dx each absent once; 16-bit dy and dx in both dtypes; two
    launches bit-identical (dgamma and dbeta included)."""
    o = ops()
    g, x, gamma, beta, idx = _ln_inputs(D, kind)
    rows, n_src = idx.numel(), x.shape[0]
    st, _ = KR.ln_fwd(x, gamma, beta, row_index=idx)
    mean, rstd = st["mean"].float(), st["rstd"].float()                 # what the forward pass saves: operands from here on
    dy = torch.randn(rows, D, generator=g)
    res = torch.randn(n_src, D, generator=g)
    g0, b0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    sel = idx.long()
    xd, gd, md, rd, idxd = in_pad(x, D + 4), cu(gamma), cu(mean), cu(rstd), cu(idx)
    dyd, resd = in_pad(dy, D + 8), in_pad(res, D + 12)
    ws = torch.full((o.layernorm_bwd_ws_floats(rows, D),), NAN, device="cuda")

    def dx_buf(dt=torch.float32):
        buf = torch.full((n_src + 2, D + 12), SENT, device="cuda", dtype=dt)
        buf[sel.cuda(), :D] = NAN
        return buf

    def unselected_ok(buf):
        left = torch.ones(n_src + 2, dtype=torch.bool)
        left[sel] = False
        return bool((buf[left.cuda()] == SENT).all()) and bool((buf[:, D:] == SENT).all())

    # (a) everything at once, accumulated; twice
    ref, bnd = KR.ln_bwd(dy, x, gamma, mean, rstd, row_index=idx, dx_res=res[sel], dgamma0=g0, dbeta0=b0)
    runs = []
    for _ in range(2):
        dx, dx16 = dx_buf(), dx_buf(torch.bfloat16)
        dgb, dg = vec(D, 0.0)
        dbb, db = vec(D, 0.0)
        dg.copy_(g0); db.copy_(b0)
        o.layernorm_bwd(dyd, xd, gd, md, rd, rows=rows, row_index=idxd, dx_res=resd, dx_out=dx[:n_src, :D],
                        dx_out_bf16=dx16[:n_src, :D], dgamma=dg, dbeta=db, accumulate=True, ws=ws)
        torch.cuda.synchronize()
        runs.append((dx, dx16, dgb, dbb))
    dx, dx16, dgb, dbb = runs[0]
    assert unselected_ok(dx) and unselected_ok(dx16), "a dx row outside row_index, or padding, was written"
    assert tail_ok(dgb, D) and tail_ok(dbb, D)
    chk("ln.bwd dx", f"D{D} {kind}", dx[sel.cuda(), :D], ref["dx"], bnd["dx"])
    chk("ln.bwd dx 16-bit", f"D{D} {kind} bf16", dx16[sel.cuda(), :D], ref["dx"], b16(bnd["dx"], ref["dx"], torch.bfloat16))
    chk("ln.bwd dgamma", f"D{D} {kind}", dgb[:D], ref["dgamma"], bnd["dgamma"])
    chk("ln.bwd dbeta", f"D{D} {kind}", dbb[:D], ref["dbeta"], bnd["dbeta"])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a[sel.cuda(), :D] if a.dim() == 2 else a, b[sel.cuda(), :D] if b.dim() == 2 else b), "two launches differ"
    # (b) fp32 dx alone (no 16-bit copy, no residual), parameter gradients written, not accumulated
    ref, bnd = KR.ln_bwd(dy, x, gamma, mean, rstd, row_index=idx)
    dx = dx_buf()
    dgb, dg = vec(D)
    dbb, db = vec(D)
    o.layernorm_bwd(dyd, xd, gd, md, rd, rows=rows, row_index=idxd, dx_out=dx[:n_src, :D], dgamma=dg, dbeta=db, ws=ws)
    torch.cuda.synchronize()
    assert unselected_ok(dx) and tail_ok(dgb, D) and tail_ok(dbb, D)
    chk("ln.bwd dx", f"D{D} {kind} plain", dx[sel.cuda(), :D], ref["dx"], bnd["dx"])
    chk("ln.bwd dgamma", f"D{D} {kind} plain", dg, ref["dgamma"], bnd["dgamma"])
    chk("ln.bwd dbeta", f"D{D} {kind} plain", db, ref["dbeta"], bnd["dbeta"])
    # (c) 16-bit dy, 16-bit dx alone (no fp32 dx, no parameter gradients), both dtypes
    for dt in DTS:
        dy16 = dy.to(dt)
        ref, bnd = KR.ln_bwd(dy16, x, gamma, mean, rstd, row_index=idx, dx_res=res[sel])
        dx16 = dx_buf(dt)
        o.layernorm_bwd(in_pad(dy16, D + 8), xd, gd, md, rd, rows=rows, row_index=idxd, dx_res=resd, dx_out_bf16=dx16[:n_src, :D])
        torch.cuda.synchronize()
        assert unselected_ok(dx16)
        chk("ln.bwd dx 16-bit", f"D{D} {kind} {dt} dy", dx16[sel.cuda(), :D], ref["dx"], b16(bnd["dx"], ref["dx"], dt))


@pytest.mark.parametrize("rows,D", [(8200, 4), (4100, 4), (260, 1024), (5, 100)])
def test_layernorm_row_loops_f64(rows, D):
    """`r += gridDim.x * 4` and the per-block dgamma / dbeta accumulation over several row visits: 8200 rows pass the forward
    cap (2048 blocks x 4 waves), 4100 the backward cap (1024 x 4), each at the narrowest row (D = 4).  260 rows at D = 1024 make
    65 partial blocks: both loops of ln_bwd_reduce_kernel (the 4-way unrolled one and its remainder) run; 5 rows: a last block
    with idle waves."""
    o = ops()
    g = KR.gen(rows + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    ref, bnd = KR.ln_fwd(x, gamma, beta)
    xd, gd, bd = in_pad(x, D + 4), cu(gamma), cu(beta)
    buf, out = out_buf(rows, D, D + 4)
    mb, mean = vec(rows)
    rb, rstd = vec(rows)
    o.layernorm_fwd(xd, gd, bd, rows=rows, out_f32=out, mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    check_canvas("ln out", buf, rows, D)
    assert tail_ok(mb, rows) and tail_ok(rb, rows)
    chk("ln.fwd", f"y rows{rows}", out, ref["y"], bnd["y"])
    chk("ln.fwd", f"mean rows{rows}", mean, ref["mean"], bnd["mean"])
    chk("ln.fwd", f"rstd rows{rows}", rstd, ref["rstd"], bnd["rstd"])
    m32, r32 = ref["mean"].float(), ref["rstd"].float()
    rf, bn = KR.ln_bwd(dy, x, gamma, m32, r32)
    ws = torch.full((o.layernorm_bwd_ws_floats(rows, D),), NAN, device="cuda")
    outs = []
    for _ in range(2):
        dbuf, dx = out_buf(rows, D, D + 4)
        dgb, dg = vec(D)
        dbb, db = vec(D)
        o.layernorm_bwd(in_pad(dy, D + 8), xd, gd, cu(m32), cu(r32), rows=rows, dx_out=dx, dgamma=dg, dbeta=db, ws=ws)
        torch.cuda.synchronize()
        outs.append((dbuf, dgb, dbb))
    dbuf, dgb, dbb = outs[0]
    check_canvas("ln dx", dbuf, rows, D)
    assert tail_ok(dgb, D) and tail_ok(dbb, D)
    chk("ln.bwd dx", f"rows{rows}", dbuf[:rows, :D], rf["dx"], bn["dx"])
    chk("ln.bwd dgamma", f"rows{rows}", dgb[:D], rf["dgamma"], bn["dgamma"])
    chk("ln.bwd dbeta", f"rows{rows}", dbb[:D], rf["dbeta"], bn["dbeta"])
    assert all(torch.equal(a[:rows, :D] if a.dim() == 2 else a, b[:rows, :D] if b.dim() == 2 else b) for a, b in zip(*outs))


@pytest.mark.parametrize("D", [1024, 100])
def test_layernorm_bound_sees_a_short_mean(D):
    """the forward bound rejects a reference in which ONE row's mean left out one lane's four columns"""
    o = ops()
    c = KR.case_ln_short_mean(D=D)
    rows = c["x"].shape[0]
    out = torch.full((rows, D), NAN, device="cuda")
    o.layernorm_fwd(cu(c["x"]), cu(c["gamma"]), cu(c["beta"]), rows=rows, out_f32=out)
    torch.cuda.synchronize()
    chk("ln.fwd", f"planted case D{D}", out, c["ref"], c["bound"])
    assert KR.rejects(out.cpu(), c["wrong"], c["bound"]), "the bound cannot see a mean over D - 4 columns"


@pytest.mark.parametrize("D", LN_DS)
def test_vit_embed_ln_f64(D):
    """vit_embed_ln_kernel at every D class: T = 1 (every row is a class row) and T = 5 with 3 x 5 rows; x0 bit-equal to the fp32
    (patch + pos) + cls; the LayerNorm of it against fp64; x0, mean and rstd each absent once.  At D = 4 also 16390 = 3278 x 5
    rows: past the 4096-block x 4-wave grid cap, so the kernel's own `r += gridDim.x * 4` loop makes a second visit with the row
    registers reused and t = r % T re-derived; rows past the end keep their sentinel."""
    o = ops()
    for T, rows in ((1, 4), (5, 15)) + (((5, 16390),) if D == 4 else ()):
        g = KR.gen(D + T)
        patch, cls, pos = torch.randn(rows, D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g)
        gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
        x0 = KR.vit_x0(patch, cls, pos, T)
        ref, bnd = KR.ln_fwd(x0, gamma, beta)
        args = [cu(t) for t in (patch, cls, pos, gamma, beta)]
        for absent in (None, "x0", "mean", "rstd"):
            xb, x = out_buf(rows, D, D)
            x0b, x0o = out_buf(rows, D, D)
            mb, mean = vec(rows)
            rb, rstd = vec(rows)
            o.vit_embed_ln(*args, x, rows=rows, T=T, x0=None if absent == "x0" else x0o, mean=None if absent == "mean" else mean,
                           rstd=None if absent == "rstd" else rstd)
            torch.cuda.synchronize()
            check_canvas("x", xb, rows, D)
            assert tail_ok(mb, rows) and tail_ok(rb, rows) and bool((x0b[rows:] == SENT).all())
            chk("vit_embed_ln", f"x D{D} T{T} -{absent}", x, ref["y"], bnd["y"])
            if absent != "x0":
                assert torch.equal(x0o.cpu(), x0), "x0 is one or two fp32 adds per element: bit-equal"
            if absent != "mean":
                chk("vit_embed_ln", f"mean D{D} T{T}", mean, ref["mean"], bnd["mean"])
            if absent != "rstd":
                chk("vit_embed_ln", f"rstd D{D} T{T}", rstd, ref["rstd"], bnd["rstd"])


# ---------------------------------------------------------------------------------------------------------------------------
# embedding gathers, embedding gradient, column sums
# ---------------------------------------------------------------------------------------------------------------------------
def _gather_case(D, Bq, g):
    V, L, P, Lt = 9, 5, 2, 3
    emb, pos = torch.randn(V, D, generator=g), torch.randn(L, D, generator=g)
    ids = torch.randint(0, V, (Bq * L,), generator=g).to(torch.int32)
    ids[0], ids[1], ids[2] = -1, V, V + 5                              # clamped to the ends of the table
    prefix = torch.randn(Bq, P * D, generator=g)
    return V, L, P, Lt, emb, pos, ids, prefix


@pytest.mark.parametrize("D,Bq", [(4, 3), (260, 3), (768, 3), (4, 3278)])
def test_embedding_gathers_bit_exact(D, Bq):
    """text_embed (with and without pos), caption_embed (P = 0; Lt = 0 with ids = None) and add_positional: one fp32 add per
    element, so bit-equal to fp32 torch; ids -1, V and V + 5 clamp to the ends.  D = 4 / 260: lanes without a column and a second
    pass with one lane.  Bq = 3278: 16390 rows of D = 4 pass the 4096-block x 4-wave grid cap (`r += gridDim.x * 4`)."""
    o = ops()
    g = KR.gen(D + Bq)
    V, L, P, Lt, emb, pos, ids, prefix = _gather_case(D, Bq, g)
    embd, posd, idsd = cu(emb), cu(pos), cu(ids)
    rows = Bq * L

    def run(fn, want):
        buf, x = out_buf(rows if want.shape[0] == rows else want.shape[0], D, D)
        fn(x)
        torch.cuda.synchronize()
        assert bool((buf[want.shape[0]:] == SENT).all()), "rows past the end were written"
        assert torch.equal(x.cpu(), want)

    run(lambda x: o.text_embed(idsd, embd, posd, x, rows=rows, L=L), KR.text_embed(ids, emb, pos, L))
    run(lambda x: o.text_embed(idsd, embd, None, x, rows=rows, L=L), KR.text_embed(ids, emb, None, L))
    # caption_embed: S = P + Lt = 5 = L, ids [Bq, Lt]
    cid = ids[:Bq * Lt]
    run(lambda x: o.caption_embed(cu(prefix), cu(cid), embd, posd, x, B=Bq, P=P, Lt=Lt), KR.caption_embed(prefix, cid, emb, pos, Bq, P, Lt))
    none = torch.empty(Bq, 0, device="cuda")
    run(lambda x: o.caption_embed(none, cu(cid), embd, posd, x, B=Bq, P=0, Lt=Lt), KR.caption_embed(None, cid, emb, pos[:Lt], Bq, 0, Lt))
    run(lambda x: o.caption_embed(cu(prefix), None, embd, posd, x, B=Bq, P=P, Lt=0), KR.caption_embed(prefix, None, emb, pos[:P], Bq, P, 0))
    e = torch.randn(rows, D, generator=g)
    run(lambda x: o.add_positional(cu(e), posd, x, rows=rows, S=L), KR.add_positional(e, pos, L))


def _scatter(o, deterministic, fn):
    o.SCATTER_DETERMINISTIC = deterministic
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        o.SCATTER_DETERMINISTIC = True


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("D", [4, 260])
def test_embedding_gradient_f64(D, deterministic):
    """embed_segsum (+ finish) and the atomics kernel: runs of 63, 64, 65 and 129 rows of one id (one chunk, exactly one chunk,
    one row into a second chunk, three chunks through the ordered partials), ids out of range clamped to rows 0 and V - 1, dx on
    a padded row stride, accumulation onto a non-zero table; rows past the table keep their sentinel.  `keep` all False leaves
    the table bit-identical (deterministic path: the atomics path takes no `keep`)."""
    o = ops()
    g = KR.gen(D + deterministic)
    V = 7
    ids = torch.cat([torch.full((n,), t) for t, n in ((1, 63), (2, 64), (3, 65), (4, 129), (-1, 2), (V + 5, 3))])
    ids = ids[torch.randperm(ids.numel(), generator=g)].to(torch.int32)
    rows = ids.numel()
    dx = torch.randn(rows, D, generator=g)
    base = torch.randn(V, D, generator=g)
    ref, bound = KR.embed_grad(ids, dx, base)
    buf = torch.full((V + 2, D), SENT, device="cuda")
    buf[:V] = base.cuda()
    dxd, idsd = in_pad(dx, D + 4), cu(ids)
    _scatter(o, deterministic, lambda: o.embed_scatter_add(idsd, dxd, buf[:V], rows=rows))
    assert bool((buf[V:] == SENT).all()), "an id past the table was not clamped"
    chk("embed_grad " + ("segsum" if deterministic else "atomics"), f"D{D}", buf[:V], ref, bound)
    if deterministic:
        again = base.cuda()
        o.embed_scatter_add(idsd, dxd, again, rows=rows)
        assert torch.equal(again, buf[:V]), "two launches differ"
        kept = base.cuda()
        o.embed_scatter_add(idsd, dxd, kept, rows=rows, keep=torch.zeros(rows, dtype=torch.bool, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(kept.cpu(), base), "keep all False must leave the table untouched"


@pytest.mark.parametrize("deterministic", [True, False])
def test_embedding_gradient_bound_sees_a_missing_chunk(deterministic):
    """the bound (RED(run length) x sum|dx| of the run) rejects a reference with one 64-row chunk of a 129-row run left out"""
    o = ops()
    c = KR.case_embed_missing_chunk()
    demb = cu(c["demb0"]).clone()
    _scatter(o, deterministic, lambda: o.embed_scatter_add(cu(c["ids"]), cu(c["dx"]), demb, rows=c["ids"].numel()))
    chk("embed_grad " + ("segsum" if deterministic else "atomics"), "planted case", demb, c["ref"], c["bound"])
    assert KR.rejects(demb.cpu(), c["wrong"], c["bound"])


@pytest.mark.parametrize("dt", DTS + [torch.float32])
def test_colsum_f64(dt):
    """colsum_partial_kernel + colsum_final_kernel: 16-bit input at C = 4, 100, 516 (C % 8 == 4: the last lane is a HALF lane and
    takes the 4-column load) on ld = the next multiple of 8 above C, plus 8; fp32 input at C = 4 and 100 on ld = C + 4; R = 1, 63,
    65 (a second row split) and 4097 (65 splits: both loops of the final kernel); accumulate on and off.  Input padding is NaN."""
    o = ops()
    wide = dt == torch.float32
    for C in ((4, 100) if wide else (4, 100, 516)):
        ld = C + 4 if wide else (C + 8) // 8 * 8 + 8
        for R in (1, 63, 65, 4097):
            g = KR.gen(C * 7 + R)
            x = torch.randn(R, C, generator=g).to(dt)
            out0 = torch.randn(C, generator=g)
            xd = in_pad(x, ld)
            for acc in (True, False):
                ref, bound = KR.colsum(x, out0 if acc else None)
                ob, out = vec(C, NAN, extra=4)
                if acc:
                    out.copy_(out0)
                ws = torch.full((o.colsum_ws_floats(R, C),), NAN, device="cuda")
                o.colsum(xd, out, ws, R=R, C=C, ld=ld, accumulate=acc)
                torch.cuda.synchronize()
                assert tail_ok(ob, C), "columns past C were written"
                chk("colsum " + ("f32 in" if wide else "16-bit in"), f"R{R} C{C} acc{acc} {dt}", out, ref, bound)


@pytest.mark.parametrize("dt", DTS + [torch.float32])
def test_colsum_bound_sees_a_missing_lane(dt):
    """the bound rejects a reference in which one row's contribution to one lane's columns (the half lane of a 16-bit input, a
    full lane of an fp32 one) is left out of 4097 rows"""
    o = ops()
    c = KR.case_colsum_missing_lane(dt)
    R, C = c["x"].shape
    ld = C + 4
    out = cu(c["out0"]).clone()
    ws = torch.empty(o.colsum_ws_floats(R, C), device="cuda")
    o.colsum(in_pad(c["x"], ld), out, ws, R=R, C=C, ld=ld, accumulate=True)
    torch.cuda.synchronize()
    chk("colsum " + ("f32 in" if dt == torch.float32 else "16-bit in"), f"planted case {dt}", out, c["ref"], c["bound"])
    assert KR.rejects(out.cpu(), c["wrong"], c["bound"])


@pytest.mark.parametrize("dt", DTS)
def test_colsum_refuses_a_misaligned_16bit_pointer(dt):
    """a 16-bit input 8 bytes off a 16-byte boundary: refused before any launch, `out` untouched"""
    o = ops()
    R, C, ld = 5, 8, 16
    flat = torch.zeros(R * ld + 8, device="cuda", dtype=dt)
    x = flat[4:4 + R * ld].view(R, ld)
    assert x.data_ptr() % 16 == 8
    out = torch.full((C,), SENT, device="cuda")
    ws = torch.empty(o.colsum_ws_floats(R, C), device="cuda")
    with pytest.raises(err_type()):
        o.colsum(x, out, ws, R=R, C=C, ld=ld)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------
# l2norm, xent_rows, reduce_dot
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(5, 1), (5, 63), (5, 64), (5, 65), (5, 512), (5, 1000), (16390, 1)])
def test_l2norm_fwd_bwd_f64(rows, D):
    """l2norm_fwd_kernel / l2norm_bwd_kernel: D below, at and above one 64-lane pass and at the model widths; x, y, dy and dx each
    on its own padded stride; inv_norm absent; mul_dev present (0.37) and absent; 16390 rows of D = 1 pass the grid cap."""
    o = ops()
    g = KR.gen(rows + D)
    x = torch.randn(rows, D, generator=g) * 3
    dy = torch.randn(rows, D, generator=g)
    ref, bnd = KR.l2norm_fwd(x)
    xd = in_pad(x, D + 3)
    yb, y = out_buf(rows, D, D + 5)
    ib, inv = vec(rows)
    o.l2norm_fwd(xd, y, inv)
    yb2, y2 = out_buf(rows, D, D + 5)
    o.l2norm_fwd(xd, y2, None)
    torch.cuda.synchronize()
    check_canvas("y", yb, rows, D)
    assert tail_ok(ib, rows) and torch.equal(y, y2)
    chk("l2norm.fwd", f"y {rows}x{D}", y, ref["y"], bnd["y"])
    chk("l2norm.fwd", f"inv {rows}x{D}", inv, ref["inv"], bnd["inv"])
    y32, i32 = ref["y"].float(), ref["inv"].float()                       # operands of the backward pass
    mul = torch.tensor([0.37], device="cuda")
    for m in (None, mul):
        dxr, bdx = KR.l2norm_bwd(dy, y32, i32, 1.0 if m is None else mul.item())
        db, dx = out_buf(rows, D, D + 7)
        o.l2norm_bwd(in_pad(dy, D + 1), in_pad(y32, D + 5), cu(i32), dx, mul_dev=m)
        torch.cuda.synchronize()
        check_canvas("dx", db, rows, D)
        chk("l2norm.bwd", f"dx {rows}x{D} mul {m is not None}", dx, dxr, bdx)


def test_l2norm_zero_row_is_nan_like_torch():
    """pins include/cclip_hip.h: a zero row is 0 * rsqrt(0) = NaN with inv_norm = +inf - what x / x.norm() gives in torch; the
    rows around it are unaffected"""
    o = ops()
    x = torch.randn(3, 65, generator=KR.gen(1))
    x[1] = 0.0
    y = torch.full((3, 65), SENT, device="cuda")
    inv = torch.full((3,), SENT, device="cuda")
    o.l2norm_fwd(cu(x), y, inv)
    torch.cuda.synchronize()
    want = x / x.norm(dim=1, keepdim=True)
    assert torch.equal(y.isnan().cpu(), want.isnan()) and bool(y[1].isnan().all())
    assert inv[1].item() == float("inf")
    ref, bnd = KR.l2norm_fwd(x[[0, 2]])
    chk("l2norm.fwd", "rows next to a zero row", y[[0, 2]], ref["y"], bnd["y"])


def _xent_rows(C, g, R=9):
    z = torch.randn(R, C, generator=g) * 3
    labels = torch.randint(0, C, (R,), generator=g).to(torch.int32)
    if R >= 9:
        ign = 7 if C > 8 else -100                                        # a valid class as ignore_index where there is room
        labels[1], labels[2], labels[3] = ign, -1, C                      # ignored: == ignore_index, < 0, >= C
        if C > 1:
            z[4, 0] = z[4, C - 1] = z[4].max() + 1                        # tie across lanes (or in one lane when C - 1 = 64)
            z[5] = 0.25                                                   # all columns equal
        if C >= 71:
            z[6, 3] = z[6, 67] = z[6].max() + 1                           # tie inside one lane's stride (c, c + 64)
            z[7, 5] = z[7, 70] = z[7].max() + 1                           # tie between two lanes
    return z, labels, 7 if C > 8 else -100


@pytest.mark.parametrize("R,C", [(9, 1), (9, 2), (9, 63), (9, 64), (9, 65), (9, 1000), (16390, 1)])
def test_xent_rows_f64(R, C):
    """xent_rows_kernel<float>: C below / at / above one 64-lane pass (C < 64 leaves lanes at m = -inf, s = 0), 16390 rows of
    C = 1 past the grid cap; logits and dlogits on padded strides; loss, dlogits and rowdot per element / per row against fp64;
    the three ways a row is ignored give loss 0, a gradient row of exact zeros and rowdot 0; planted exact ties of the maximum
    (same lane, two lanes, first and last column, all equal) must give the LOWEST index; then in place on a padded stride."""
    o = ops()
    g = KR.gen(R * 31 + C)
    z, labels, ign = _xent_rows(C, g, R)
    ref, bnd = KR.xent(z, labels, ignore_index=ign, grad_scale=0.5)
    zd, ld = in_pad(z, C + 3), cu(labels)
    db, d = out_buf(R, C, C + 5)
    lb, loss = vec(R)
    rb, rowdot = vec(R)
    pb, pred = vec(R, -1, torch.int32)
    o.xent_rows(zd, ld, loss_row=loss, pred=pred, dlogits=d, grad_scale=0.5, ignore_index=ign, rowdot=rowdot)
    torch.cuda.synchronize()
    check_canvas("dlogits", db, R, C)
    assert tail_ok(lb, R) and tail_ok(rb, R) and tail_ok(pb, R)
    chk("xent loss", f"{R}x{C}", loss, ref["loss"], bnd["loss"])
    chk("xent dlogits", f"{R}x{C}", d, ref["dlogits"], bnd["dlogits"])
    chk("xent rowdot", f"{R}x{C}", rowdot, ref["rowdot"], bnd["rowdot"])
    assert torch.equal(pred.cpu().long(), ref["pred"]), "argmax: the lowest index of the maximum"
    ig = ref["ignored"]
    assert bool(ig.any()) or R != 9
    assert bool((loss.cpu()[ig] == 0).all()) and bool((d.cpu()[ig] == 0).all()) and bool((rowdot.cpu()[ig] == 0).all())
    # in place (dlogits is logits) on the padded stride
    buf = torch.full((R + 2, C + 3), SENT, device="cuda")
    zi = buf[:R, :C]
    zi.copy_(z)
    rb2, rowdot2 = vec(R)
    o.xent_rows(zi, ld, dlogits=zi, grad_scale=0.5, ignore_index=ign, rowdot=rowdot2)
    torch.cuda.synchronize()
    check_canvas("in place", buf, R, C)
    assert torch.equal(zi, d) and torch.equal(rowdot2, rowdot), "in place differs from out of place"
    for dt in DTS:                                                       # 16-bit gradient rows
        db16, d16 = out_buf(R, C, C + 5, dt)
        o.xent_rows(zd, ld, dlogits=d16, grad_scale=0.5, ignore_index=ign)
        torch.cuda.synchronize()
        check_canvas("dlogits 16", db16, R, C)
        chk("xent dlogits 16-bit", f"{R}x{C} {dt}", d16, ref["dlogits"], b16(bnd["dlogits"], ref["dlogits"], dt))


@pytest.mark.parametrize("C", [65, 1000])
def test_xent_rows_range_f64(C):
    """logits shifted by +80 and -80 (exp of the raw value would overflow / underflow) and logits spanning 200 (the small
    probabilities underflow to 0): nothing is NaN, everything inside the bound whose exp term is taken at the row's largest
    |logit - lse|"""
    o = ops()
    g = KR.gen(C)
    z = torch.randn(4, C, generator=g) * 3
    z[0] += 80.0
    z[1] -= 80.0
    z[2] = torch.linspace(-100.0, 100.0, C)[torch.randperm(C, generator=g)]
    z[3] = torch.linspace(100.0, -100.0, C)                              # descending: the running maximum is set once
    labels = torch.tensor([1, 2, 3, C - 1], dtype=torch.int32)
    ref, bnd = KR.xent(z, labels, grad_scale=1.0)
    d = torch.full((4, C), NAN, device="cuda")
    loss, rowdot = torch.full((4,), NAN, device="cuda"), torch.full((4,), NAN, device="cuda")
    pred = torch.full((4,), -1, device="cuda", dtype=torch.int32)
    o.xent_rows(cu(z), cu(labels), loss_row=loss, pred=pred, dlogits=d, rowdot=rowdot)
    torch.cuda.synchronize()
    chk("xent loss", f"range C{C}", loss, ref["loss"], bnd["loss"])
    chk("xent dlogits", f"range C{C}", d, ref["dlogits"], bnd["dlogits"])
    chk("xent rowdot", f"range C{C}", rowdot, ref["rowdot"], bnd["rowdot"])
    assert torch.equal(pred.cpu().long(), ref["pred"])


def test_xent_rows_minus_infinity_after_a_finite_logit():
    """include/cclip_hip.h: finite logits only (both callers feed GEMM outputs; nothing masks a logit).  Pinned here is the one
    -inf case the kernel does handle: a -inf that is NOT the first element of its lane (column >= 64) has probability 0, the
    loss, the gradient and the argmax are those of the finite columns."""
    o = ops()
    C = 100
    z = torch.randn(2, C, generator=KR.gen(5)) * 3
    z[0, 69] = float("-inf")
    z[1, 64] = z[1, 99] = float("-inf")
    labels = torch.tensor([3, 70], dtype=torch.int32)
    ref, bnd = KR.xent(z, labels)
    d = torch.full((2, C), NAN, device="cuda")
    loss = torch.full((2,), NAN, device="cuda")
    pred = torch.full((2,), -1, device="cuda", dtype=torch.int32)
    o.xent_rows(cu(z), cu(labels), loss_row=loss, pred=pred, dlogits=d)
    torch.cuda.synchronize()
    chk("xent loss", "-inf", loss, ref["loss"], bnd["loss"])
    chk("xent dlogits", "-inf", d, ref["dlogits"], bnd["dlogits"])
    assert d[0, 69] == 0 and d[1, 64] == 0 and d[1, 99] == 0 and torch.equal(pred.cpu().long(), ref["pred"])


@pytest.mark.parametrize("dt", DTS)
def test_xent_rows_refuses_16bit_dlogits_over_the_logits(dt):
    """the launcher's alias check: a 16-bit dlogits at the address of the fp32 logits (each lane would overwrite logits another
    lane still reads) is refused before any launch, in both 16-bit twins, and the logits are untouched"""
    o = ops()
    z = torch.randn(4, 16, device="cuda")
    before = z.clone()
    alias = z.view(dt)[:, :16]
    assert alias.data_ptr() == z.data_ptr()
    with pytest.raises(err_type()):
        o.xent_rows(z, torch.zeros(4, device="cuda", dtype=torch.int32), dlogits=alias)
    torch.cuda.synchronize()
    assert torch.equal(z, before)


@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 100003])
def test_reduce_dot_f64(n):
    """reduce_dot_kernel: fewer elements than lanes, one full pass of the 1024 threads, one element into a second pass, a long
    vector; b = None; alpha, mul_dev and accumulation onto a non-zero value; two launches bit-identical"""
    o = ops()
    g = KR.gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = cu(a), cu(b)
    mul = torch.tensor([0.37], device="cuda")
    for bb, alpha, m, acc in ((b, 0.5, mul, True), (None, 1.0, None, False), (b, -1.5, None, True), (None, 0.25, mul, False)):
        ref, bound = KR.reduce_dot(a, bb, alpha=alpha, mul=1.0 if m is None else m.item(), out0=1.25 if acc else 0.0)
        outs = []
        for _ in range(2):
            ob, out = vec(1, 1.25 if acc else NAN)
            o.reduce_dot(ad, None if bb is None else bd, out, alpha=alpha, mul_dev=m, accumulate=acc)
            torch.cuda.synchronize()
            assert tail_ok(ob, 1)
            outs.append(out)
        chk("reduce_dot", f"n{n} b{bb is not None} acc{acc}", outs[0], ref.reshape(1), bound.reshape(1))
        assert torch.equal(outs[0], outs[1])


def test_reduce_dot_bound_sees_a_missing_wave_partial():
    """reduce_dot_kernel's second stage (16 wave partials through LDS, added by thread 0): the bound rejects a reference with one
    of the 16 partials left out of a 100003-element dot product"""
    o = ops()
    c = KR.case_reduce_dot_missing_wave()
    out = torch.tensor([1.25], device="cuda")
    o.reduce_dot(cu(c["a"]), cu(c["b"]), out, alpha=0.5, mul_dev=torch.tensor([0.37], device="cuda"), accumulate=True)
    torch.cuda.synchronize()
    chk("reduce_dot", "planted case", out, c["ref"], c["bound"])
    assert KR.rejects(out.cpu(), c["wrong"], c["bound"]), "the bound cannot see one of the 16 wave partials"


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW, cast, scale
# ---------------------------------------------------------------------------------------------------------------------------
N_BIG = 4 * (8192 * 256) + 4 * 300 + 4        # the first size class in which the second unrolled slot and the grid stride run
PAT = 32                                       # the value pattern: 8 float4 groups


def _adam_pattern(g):
    p = torch.randn(PAT, generator=g)
    gr = torch.randn(PAT, generator=g)
    m = 0.1 * torch.randn(PAT, generator=g)
    v = 0.01 * torch.rand(PAT, generator=g)
    gr[:4] = 0.0; m[:4] = 0.0; v[:4] = 0.0       # g = 0, m = v = 0: may not move without decay
    gr[4:8] = torch.tensor([1e-20, -1e-20, 1e-20, -1e-20]); m[4:8] = 0.0; v[4:8] = 0.0       # g^2 underflows
    p[8] = 0.0
    return p, gr, m, v


ADAM_CFGS = [dict(mode=0, weight_decay=0.0, steps=(1, 2, 3)), dict(mode=0, weight_decay=0.01, steps=(100000, 100001, 100002)),
             dict(mode=0, weight_decay=0.01, steps=(1, 2, 3), correct_bias=False, grad_scale=0.25),
             dict(mode=1, weight_decay=0.01, steps=(1, 2, 3), grad_scale=0.25), dict(mode=1, weight_decay=0.0, steps=(100000, 100001, 100002)),
             dict(mode=1, weight_decay=0.01, steps=(1, 2, 3), correct_bias=False)]
HYP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6)


def _adam_run(o, p, gr, m, v, cfg, shadow=None):
    kw = {k: cfg[k] for k in ("mode", "weight_decay", "correct_bias", "grad_scale") if k in cfg}
    for step in cfg["steps"]:
        o.adamw_step(p, gr, m, v, step=step, bf16_shadow=shadow, **HYP, **kw)


@pytest.mark.parametrize("shadow_dt", [None] + DTS)
@pytest.mark.parametrize("ci", range(len(ADAM_CFGS)))
def test_adamw_three_steps_f64(ci, shadow_dt):
    """adamw_kernel, three steps per element against fp64 fed the fp32 hyper-parameters the entry point receives: both modes,
    grad_scale, correct_bias off, decay 0 and 0.01, first steps and step 100000; elements with g = 0 and m = v = 0 (no move in
    mode 0 without decay) and with |g| = 1e-20 (g^2 underflows); with and without a 16-bit shadow (the rounded fp32 parameter,
    bit for bit); the same values run group by group at n = 4 agree bit for bit (the update is element-wise)."""
    o = ops()
    cfg = ADAM_CFGS[ci]
    p0, gr, m0, v0 = _adam_pattern(KR.gen(ci))
    ref, bnd = KR.adamw(p0, gr, m0, v0, **HYP, **cfg)
    bufs = [vec(PAT, 0.0) for _ in range(3)]
    for (_, view), src in zip(bufs, (p0, m0, v0)):
        view.copy_(src)
    (pb, p), (mb, m), (vb, v) = bufs
    sb, sh = vec(PAT, NAN, shadow_dt) if shadow_dt else (None, None)
    grd = cu(gr)
    _adam_run(o, p, grd, m, v, cfg, sh)
    torch.cuda.synchronize()
    assert tail_ok(pb, PAT) and tail_ok(mb, PAT) and tail_ok(vb, PAT) and (sb is None or tail_ok(sb, PAT))
    for nm, got in (("p", p), ("m", m), ("v", v)):
        chk("adamw " + nm, f"cfg{ci}", got, ref[nm], bnd[nm])
    if sh is not None:
        assert torch.equal(sh, p.to(shadow_dt)), "the shadow is the rounded copy of the fp32 parameter"
    if cfg["mode"] == 0 and cfg["weight_decay"] == 0.0:
        assert torch.equal(p[:4].cpu(), p0[:4]), "g = 0, m = v = 0, no decay: the parameter moved"
    # group by group at n = 4
    p4, m4, v4 = cu(p0).clone(), cu(m0).clone(), cu(v0).clone()
    for k in range(0, PAT, 4):
        _adam_run(o, p4[k:k + 4], grd[k:k + 4], m4[k:k + 4], v4[k:k + 4], cfg)
    torch.cuda.synchronize()
    assert torch.equal(p4, p) and torch.equal(m4, m) and torch.equal(v4, v), "the result of an element depends on n or its position"


def _tile(pat, n):
    return pat.cuda().repeat((n + pat.numel() - 1) // pat.numel())[:n].contiguous()


def _same_everywhere(name, big, small):
    """every element of the long run equals the element of the short run that holds the same values - start, slot boundary
    (float4 group 8192 * 256) and tail included"""
    n, k = big.numel(), small.numel()
    full = n // k * k
    assert torch.equal(big[:full].view(-1, k), small[None, :].expand(full // k, k)), f"{name}: an element of the long run differs"
    assert torch.equal(big[full:], small[:n - full]), f"{name}: the tail of the long run differs"


@pytest.mark.parametrize("ci,shadow_dt", [(1, torch.bfloat16), (3, torch.float16), (0, None)])
def test_adamw_second_slot_and_grid_stride_bit_identical(ci, shadow_dt):
    """n = 4 (8192 x 256) + 4 x 300 + 4: the grid is capped at 8192 blocks, so the second unrolled slot (U = 2) holds groups
    8192 x 256 .. and its `break` fires in the tail.  The update is element-wise: every element of the long run is bit-identical
    to the same (p, g, m, v) run at n = 32 (itself pinned to n = 4 and to fp64 above) - an exact check, no tolerance."""
    o = ops()
    cfg = ADAM_CFGS[ci]
    p0, gr, m0, v0 = _adam_pattern(KR.gen(ci))
    small = [cu(t).clone() for t in (p0, gr, m0, v0)]
    ssh = torch.full((PAT,), NAN, device="cuda", dtype=shadow_dt) if shadow_dt else None
    _adam_run(o, small[0], small[1], small[2], small[3], cfg, ssh)
    big = [_tile(t, N_BIG) for t in (p0, gr, m0, v0)]
    bsh = torch.full((N_BIG,), NAN, device="cuda", dtype=shadow_dt) if shadow_dt else None
    _adam_run(o, big[0], big[1], big[2], big[3], cfg, bsh)
    torch.cuda.synchronize()
    for nm, i in (("p", 0), ("m", 2), ("v", 3)):
        _same_everywhere(nm, big[i], small[i])
    if shadow_dt:
        _same_everywhere("shadow", bsh.view(torch.int16), ssh.view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
def test_cast_and_scale_past_the_grid_cap_bit_identical(dt):
    """cast_bf16_kernel / scale_f32_kernel past their 8192-block caps (the grid-stride loop): bit-identical, element for element,
    to the same values at n = 4 and to torch's own rounding / fp32 product"""
    o = ops()
    pat = torch.randn(PAT, generator=KR.gen(11)) * torch.tensor([1.0, 1e-6, 3e4, 1e-3]).repeat(PAT // 4)
    src = _tile(pat, N_BIG)
    dst = torch.full((N_BIG,), NAN, device="cuda", dtype=dt)
    o.cast_f32_to_bf16(src, dst)
    small = torch.full((PAT,), NAN, device="cuda", dtype=dt)
    for k in range(0, PAT, 4):
        o.cast_f32_to_bf16(cu(pat)[k:k + 4].clone(), small[k:k + 4])
    torch.cuda.synchronize()
    assert torch.equal(small.view(torch.int16), cu(pat).to(dt).view(torch.int16))
    _same_everywhere("cast", dst.view(torch.int16), small.view(torch.int16))
    if dt == DTS[0]:                                                     # the scale has no 16-bit side: once
        o.scale_f32(src, 0.37)
        s4 = cu(pat).clone()
        for k in range(0, PAT, 4):
            o.scale_f32(s4[k:k + 4], 0.37)
        torch.cuda.synchronize()
        assert torch.equal(s4, cu(pat) * torch.tensor(0.37, device="cuda")), "one fp32 product per element"
        _same_everywhere("scale", src, s4)


def test_adamw_cast_scale_refusals():
    """arguments the launchers reject before any launch: n % 4 != 0, a pointer off its alignment, step = 0"""
    o = ops()
    E = err_type()
    t = [torch.ones(16, device="cuda") for _ in range(4)]
    keep = [x.clone() for x in t]
    kw = dict(lr=1e-3)
    with pytest.raises(E):
        o.adamw_step(t[0][:6], t[1][:6], t[2][:6], t[3][:6], step=1, **kw)
    with pytest.raises(E):
        o.adamw_step(t[0][1:9], t[1][:8], t[2][:8], t[3][:8], step=1, **kw)
    with pytest.raises(E):
        o.adamw_step(t[0][:8], t[1][:8], t[2][1:9], t[3][:8], step=1, **kw)
    with pytest.raises(E):
        o.adamw_step(*t, step=0, **kw)
    d16 = torch.zeros(16, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(E):
        o.cast_f32_to_bf16(t[0][:6], d16[:6])
    with pytest.raises(E):
        o.cast_f32_to_bf16(t[0][1:9], d16[:8])
    with pytest.raises(E):
        o.cast_f32_to_bf16(t[0][:8], d16[1:9])                          # 2 bytes off: the 8-byte store alignment
    with pytest.raises(E):
        o.scale_f32(t[0][:6], 2.0)
    with pytest.raises(E):
        o.scale_f32(t[0][1:9], 2.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(t, keep)) and bool((d16 == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 GEMM
# ---------------------------------------------------------------------------------------------------------------------------
GEMM_TILE, GEMM_KSTEP = 32, 32                # FBM = FBN, FBK of csrc/gemm_f32.hip
EDGE = (GEMM_TILE - 1, GEMM_TILE, GEMM_TILE + 1)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_f32_tile_edges_f64(ta, tb):
    """gemm_f32_kernel with M, N and K one below, at and one above the 32 x 32 tile and the 32-deep K step (27 shapes), in the
    four operand layouts (K-fast and K-strided staging loops), C on a padded row stride, alpha and a non-zero beta; then beta = 0
    over a C full of NaN (include/cclip_hip.h: C is not read) and alpha = 0."""
    o = ops()
    for M in EDGE:
        for N in EDGE:
            for K in (GEMM_KSTEP - 1, GEMM_KSTEP, GEMM_KSTEP + 1):
                g = KR.gen(M * 10000 + N * 100 + K)
                A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
                C0 = torch.randn(M, N, generator=g)
                Av = cu(A.t().contiguous()).t() if ta else cu(A)
                Bv = cu(B.t().contiguous()).t() if tb else cu(B)
                for alpha, beta in ((0.5, 2.0), (1.5, 0.0), (0.0, 2.0)):
                    ref, bound = KR.gemm_f32(A, B, C0, alpha=alpha, beta=beta)
                    buf, C = out_buf(M, N, N + 5)
                    if beta != 0.0:
                        C.copy_(C0)
                    o.gemm_f32(Av, Bv, C, alpha=alpha, beta=beta)
                    torch.cuda.synchronize()
                    check_canvas("C", buf, M, N)
                    chk("gemm_f32", f"{M}x{N}x{K} t{ta}{tb} a{alpha} b{beta}", C, ref, bound)


def test_gemm_f32_bound_sees_a_missing_k_step():
    """the bound rejects a reference with the last 32-deep K step left out of the last (ragged) 32 x 32 tile"""
    o = ops()
    c = KR.case_gemm_missing_kstep(tile=GEMM_TILE, kstep=GEMM_KSTEP)
    C = cu(c["C0"]).clone()
    o.gemm_f32(cu(c["A"]), cu(c["B"]), C, alpha=0.5, beta=2.0)
    torch.cuda.synchronize()
    chk("gemm_f32", "planted case", C, c["ref"], c["bound"])
    assert KR.rejects(C.cpu(), c["wrong"], c["bound"])
