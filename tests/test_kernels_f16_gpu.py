"""GPU: the fp16 twins of every dual-built kernel (csrc/build.py DUAL; `*_f16` entry points, the `model.half()` mode) and the
bf16 builds of the same paths, against plain torch in float64 fed the exact 16-bit operands the kernel receives.

GEMM bound, per element (S = |A| . |B|^T in fp64, scaled like the output: |alpha| and the activation's slope):
    |got - ref| <= C * 2^-24 * sqrt(K) * S  +  2^-20 * (|ref| + |pre| + |residual|)  +  u * |ref|  +  floor
  * C = 2: fp32 accumulation of exact 16-bit products (both products fit in fp32) has a worst-case error of K * 2^-24 * S; the
    sqrt(K) form is the usual probabilistic one for sums whose rounding errors do not line up, and C = 2 leaves a factor of two
    over it.  C was fixed before the first run; on an MI355X the largest err / (2^-24 sqrt(K) S) over every configuration and
    both dtypes was 0.18 (fp32 outputs), so the accumulation term has about ten times the headroom it needs.
  * 2^-20 * (...): fp32 evaluation of the epilogue (bias / residual adds, expf / tanhf of the activations: a few ulp each).
  * u * |ref|: the one rounding of a 16-bit output, u = 2^-8 (bf16) or 2^-11 (fp16), the unit roundoff (half an ulp of 1.0):
    this term alone is tight by construction - a value just above a power of two rounds by up to u times itself.
  * floor: 2^-24 for fp16 outputs (one subnormal ulp), 0 otherwise.
Every GEMM test also shows that the same bound REJECTS a reference with one 64-deep K-tile's contribution removed from a single
16x16 output sub-tile (`_assert_sensitive`): the tolerance sees an error confined to one MFMA tile and one K step.

Attention bound, also per element, from the magnitudes the exact computation goes through (P = softmax, fp64):
    o: 4u * P|V|,  dv: 4u * P^T|dO|,  dq / dk: 4u * scale * |dS|' |K|  (resp. |dS|'^T |Q|),  |dS|' = P * (|dO||V|^T + rowsum(|dO| P|V|))
  plus the subnormal floors of the 16-bit intermediates (P and dS are rounded to 16 bits inside the kernels).  A wrong head or a
  wrong packed sequence cannot hide under a larger one: nothing is scaled by a tensor-wide maximum.

Unwritten-region canaries: logical outputs start as NaN and must come back finite; rows / columns outside them (padded row
strides, rows past a packed batch) hold a sentinel that must survive."""
import math

import pytest
import torch

from gemm_refs_f64 import (C_ACC, FLOOR, SENT, U, WORST, _acc_bound, _act64, _assert_sensitive, _mats, _worst_report, canvas,  # noqa: F401
                           check_canvas, rnd, within)
from attn_refs_f64 import _attn64, _attn_bounds, _split_heads

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]


def ops():
    from cclip_hip import ops as o
    return o


def G(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# the GEMM helpers (U, FLOOR, rnd, canvas, check_canvas, within / WORST, _mats, _acc_bound, _assert_sensitive, _act64) live in
# tests/gemm_refs_f64.py, shared with tests/test_gemm_paths_f64_gpu.py


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------
# (cfg, layouts it accepts)
CFG_LAYOUTS = {1: [(1, 1), (1, 0), (0, 0)], 2: [(1, 1), (1, 0), (0, 0)], 3: [(1, 1), (1, 0), (0, 0)], 5: [(1, 1), (1, 0), (0, 0)],
               7: [(1, 1)], 8: [(1, 1)], 11: [(0, 0)]}
SHAPES = [(264, 200, 640), (72, 40, 200), (296, 392, 128), (520, 136, 1088)]      # (M % 8 == 0: the K-strided A of the wgrad layout has row stride M)
# configurations 8 / 11 take whole 64-deep K-tiles only (their refusal of the rest is tested in test_gemm_gpu.py)
PLAIN = [(cfg, akc, bkc, M, N, K) for cfg, lays in CFG_LAYOUTS.items() for (akc, bkc) in lays for (M, N, K) in SHAPES
         if not (cfg in (8, 11) and K % 64)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg,akc,bkc,M,N,K", PLAIN)
def test_gemm_plain_f64(cfg, akc, bkc, M, N, K, dt):
    """Every tile configuration in every layout it accepts: ragged M / N edges, M and N below one tile, K = 64 n and K % 64 != 0
    (the hand-scheduled configurations 8 / 11 need whole K-tiles and are given those only); fp32 and 16-bit outputs."""
    o = ops()
    g = G(cfg * 1000 + M + N + K)
    A = rnd((M, K) if akc else (K, M), dt, g)
    B = rnd((N, K) if bkc else (K, N), dt, g)
    Am, Bm = _mats(A, B, akc, bkc)
    ref = Am @ Bm.t()
    bound = _acc_bound(Am, Bm) + 1e-30
    buf, out = canvas(M, N, torch.float32)
    o.gemm_bf16(A, B, a_kcontig=bool(akc), b_kcontig=bool(bkc), out_f32=out, tile_config=cfg)
    torch.cuda.synchronize()
    check_canvas("f32 out", buf, M, N)
    within(f"cfg{cfg} {akc}{bkc} {M}x{N}x{K} f32", out, ref, bound)
    _assert_sensitive(out, ref, bound, Am, Bm)
    # 16-bit output of the same product
    buf16, out16 = canvas(M, N, dt)
    o.gemm_bf16(A, B, a_kcontig=bool(akc), b_kcontig=bool(bkc), out_bf16=out16, tile_config=cfg)
    torch.cuda.synchronize()
    check_canvas("16-bit out", buf16, M, N)
    b16 = bound + U(dt) * ref.abs() + FLOOR(dt)
    within(f"cfg{cfg} {akc}{bkc} {M}x{N}x{K} 16-bit", out16, ref, b16)
    _assert_sensitive(out16, ref, b16, Am, Bm)


# the epilogue instantiations (csrc/gemm_bf16_impl.h gemm_launch_cfg; configuration 8: csrc/gemm_bf16_cfg8.hip): anything else is
# refused with status 1, which test_gemm_gpu.py covers
# (configurations 7 / 8: forward layout only; 8: the plain, QuickGELU and QuickGELU' epilogues only)
EPI = [(a, 1, 1, cfg) for a in (0, 1, 2, 4, 16, 18, 19) for cfg in (1, 2, 3, 5, 7, 8) if cfg != 8 or a in (0, 1, 16)] + \
      [(a, 1, 0, cfg) for a in (0, 3, 16, 17, 19) for cfg in (1, 2, 3, 5)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act,akc,bkc,cfg", EPI)
def test_gemm_epilogues_f64(act, akc, bkc, cfg, dt):
    """alpha, bias, activation (16-bit aux for the derivative forms), residual, fp32 + 16-bit + pre-activation outputs at once on
    a padded row stride; ragged edges.  Then the residual form in place (out_f32 is residual, ldc > N)."""
    o = ops()
    M, N, K = 300, 264, 320
    g = G(act * 100 + cfg * 7 + akc + 2 * bkc)
    A = rnd((M, K), dt, g, 0.1)
    B = rnd((N, K) if bkc else (K, N), dt, g)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g)
    aux = rnd((M, N), dt, g)
    if act == 17:
        aux = torch.tanh(aux.float()).to(dt)
    Am, Bm = _mats(A, B, True, bkc)
    pre = 0.5 * (Am @ Bm.t()) + bias.double()
    y, slope = _act64(pre, act, aux)
    ref = y + res.double()
    acc = _acc_bound(Am, Bm, 0.5)
    ev = 2.0 ** -20 * (ref.abs() + pre.abs() + res.double().abs() + y.abs())
    bf = acc * (1.0 + slope) + ev + 1e-30               # (1 + slope): the pre-activation error and the activation's slope
    bufs = [canvas(M, N, t) for t in (torch.float32, dt, dt)]
    o.gemm_bf16(A, B, a_kcontig=True, b_kcontig=bool(bkc), alpha=0.5, bias=bias, act=act, aux=aux if act >= 16 else None,
                residual=res, out_f32=bufs[0][1], out_bf16=bufs[1][1], out_pre=bufs[2][1] if act else None, tile_config=cfg)
    torch.cuda.synchronize()
    for (b, _), nm in zip(bufs, ("f32", "16", "pre")):
        check_canvas(nm, b, M, N)
    within(f"act{act} cfg{cfg} f32", bufs[0][1], ref, bf)
    _assert_sensitive(bufs[0][1], ref, bf, Am, Bm, 0.5, slope)
    b16 = bf + U(dt) * ref.abs() + FLOOR(dt)
    within(f"act{act} cfg{cfg} 16-bit", bufs[1][1], ref, b16)
    if act:
        bp = acc + 2.0 ** -20 * pre.abs() + U(dt) * pre.abs() + FLOOR(dt) + 1e-30
        within(f"act{act} cfg{cfg} pre", bufs[2][1], pre, bp)
        _assert_sensitive(bufs[2][1], pre, bp, Am, Bm, 0.5)
    if act == 0:
        big = torch.full((M + 2, N + 24), SENT, device="cuda")
        x = big[:M, 8:8 + N]
        x.copy_(res)
        o.gemm_bf16(A, B, a_kcontig=True, b_kcontig=bool(bkc), alpha=0.5, bias=bias, residual=x, out_f32=x, tile_config=cfg)
        torch.cuda.synchronize()
        within(f"in-place residual cfg{cfg}", x, ref, bf)
        assert bool((big[:, :8] == SENT).all() and (big[:, 8 + N:] == SENT).all() and (big[M:] == SENT).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cfg,split,of_b", [(c, s, b) for c, s in ((1, 3), (2, 5), (5, 4), (1, 16), (11, 5), (11, 3), (11, 1))
                                            for b in (False, True) if not (c == 11 and b)])
def test_gemm_splitk_colsum_f64(cfg, split, of_b, dt):
    """Weight-gradient layout with split-K slabs (configuration 3 forms no bias gradient: refused) and the fused bias gradient (row sums of A, or with colsum_of_b of B), accumulated
    into existing gradients (configuration 11 forms no sums of B: refused, never tuned there).  K = 640 at split 5 is configuration 11's exact boundary: 2 K-tiles per split, 2 in the last one."""
    o = ops()
    M, N, K = 520, 264, 640
    g = G(cfg * 10 + split + of_b)
    A = rnd((K, M), dt, g)
    B = rnd((K, N), dt, g)
    Am, Bm = _mats(A, B, False, False)
    gw0 = torch.randn(M, N, device="cuda", generator=g)
    gb0 = torch.randn(N if of_b else M, device="cuda", generator=g)
    ref = gw0.double() + Am @ Bm.t()
    csrc = Bm if of_b else Am
    ref_b = gb0.double() + csrc.sum(1)
    bw = _acc_bound(Am, Bm) + 2.0 ** -20 * ref.abs() + 1e-30
    bb = C_ACC * 2.0 ** -24 * math.sqrt(K) * csrc.abs().sum(1) + 2.0 ** -20 * ref_b.abs() + 1e-30
    buf, gw = canvas(M, N, torch.float32)
    gw.copy_(gw0)
    gb = gb0.clone()
    ws = torch.full((split * (M * N + max(M, N)),), float("nan"), device="cuda") if split > 1 else None
    o.gemm_bf16(A, B, a_kcontig=False, b_kcontig=False, residual=gw, out_f32=gw, split_k=split, split_ws=ws, tile_config=cfg,
                colsum_out=gb, colsum_accumulate=True, colsum_of_b=of_b)
    torch.cuda.synchronize()
    check_canvas("wgrad", buf, M, N)
    within(f"wgrad cfg{cfg} split{split}", gw, ref, bw)
    _assert_sensitive(gw, ref, bw, Am, Bm)
    within(f"bias grad cfg{cfg} split{split}", gb, ref_b, bb)
    if cfg == 11:             # configuration 11 == configuration 2 at the same split, bit for bit (gradient and bias gradient)
        gw2, gb2 = gw0.clone(), gb0.clone()
        o.gemm_bf16(A, B, a_kcontig=False, b_kcontig=False, residual=gw2, out_f32=gw2, split_k=split, split_ws=ws, tile_config=2,
                    colsum_out=gb2, colsum_accumulate=True)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(450, 768, 768), (264, 200, 192), (1000, 2304, 256)])
def test_gemm_bit_identities_f64(M, N, K, dt):
    """configuration 8 == configuration 3, and the column-grouped tile orders == row-major, bit for bit - in both dtypes; and the
    shared result against fp64."""
    o = ops()
    g = G(M + N + K)
    A, B = rnd((M, K), dt, g), rnd((N, K), dt, g)
    bias = torch.randn(N, device="cuda", generator=g)
    Am, Bm = _mats(A, B, 1, 1)
    ref = Am @ Bm.t() + bias.double()
    outs = {}
    for tc in (3, 8, 2, 3 + 256 * 3, 8 + 256 * 4, 2 + 256 * 6):
        ob = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
        x = torch.zeros(M, N, device="cuda")
        o.gemm_bf16(A, B, bias=bias, out_bf16=ob, tile_config=tc)
        o.gemm_bf16(A, B, bias=bias, residual=x, out_f32=x, tile_config=tc)
        outs[tc] = (ob, x)
    torch.cuda.synchronize()
    bound = _acc_bound(Am, Bm) + 2.0 ** -20 * ref.abs() + 1e-30
    within("cfg3 f32", outs[3][1], ref, bound)
    within("cfg3 16-bit", outs[3][0], ref, bound + U(dt) * ref.abs() + FLOOR(dt))
    _assert_sensitive(outs[3][1], ref, bound, Am, Bm)
    for a, b in ((8, 3), (3 + 256 * 3, 3), (8 + 256 * 4, 8), (2 + 256 * 6, 2)):
        assert torch.equal(outs[a][0], outs[b][0]) and torch.equal(outs[a][1], outs[b][1]), (a, b)


@pytest.mark.parametrize("dt", DTS)
def test_gemm_derived_cfg11_choice_at_reproduced_count(dt):
    """56384 tokens through the 512x512 weight gradient with the committed table: the derived choice (nearest entry 78848 tokens,
    configuration 11 at split 64, scaled) launches, matches fp64, and equals configuration 2 at the split it ends up with."""
    from cclip_hip.stack import Scratch, wgrad_candidates
    o = ops()
    o.load_tuned_table()
    T, n = 56384, 512
    key = f"{str(dt).replace('torch.', '')}|{n}|{n}|{T}|0|0|0|1|0|0|0|0|-1|1|0"
    assert key not in o._TUNED
    o._DERIVED.pop(key, None)
    choice = o._nearest_tuned(key)
    assert choice[0] == 11 and o.cfg11_splits_ok(T // 64, choice[1]), choice
    g = G(56384)
    A, B = rnd((T, n), dt, g), rnd((T, n), dt, g)
    gw = torch.full((n, n), float("nan"), device="cuda")
    gb = torch.full((n,), float("nan"), device="cuda")
    o.gemm_bf16(A, B, a_kcontig=False, b_kcontig=False, out_f32=gw, colsum_out=gb, split_candidates=wgrad_candidates(n, n, T),
                scratch=Scratch(torch.device("cuda")).floats)
    assert o._DERIVED.get(key) == choice
    Am, Bm = _mats(A, B, False, False)
    ref = Am @ Bm.t()
    bound = _acc_bound(Am, Bm) + 1e-30
    within("derived cfg11", gw, ref, bound)
    _assert_sensitive(gw, ref, bound, Am, Bm)
    within("derived cfg11 bias", gb, Am.sum(1), C_ACC * 2.0 ** -24 * math.sqrt(T) * Am.abs().sum(1) + 1e-30)
    sp = choice[1]
    gw2, gb2 = torch.empty_like(gw), torch.empty_like(gb)
    o.gemm_bf16(A, B, a_kcontig=False, b_kcontig=False, out_f32=gw2, colsum_out=gb2, tile_config=2, split_k=sp,
                split_ws=torch.empty(sp * (n * n + n), device="cuda"))
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


# ---- fp16 range: outputs near and past 65504, and in the subnormal range ----------------------------------------------
F16_MAX_RND = 65520.0          # the smallest magnitude IEEE fp16 round-to-nearest takes to infinity


@pytest.mark.parametrize("cfg", [1, 3, 8])
@pytest.mark.parametrize("act", [0, 1, 16])
def test_gemm_f16_overflow_range(cfg, act):
    """Outputs of +-several 10^4 (some past the fp16 maximum): where IEEE rounding of the fp64 value gives +-inf (clear of the
    threshold by more than the accumulation bound) the kernel must too; below it, finite and within the bound; never NaN.
    act 16 (QuickGELU') with aux of +-6e4: expf overflows inside the derivative."""
    o = ops()
    dt = torch.float16
    M, N, K = 256, 264, 256
    g = G(cfg + act)
    A, B = rnd((M, K), dt, g, 50.0), rnd((N, K), dt, g, 50.0)
    aux = (torch.rand(M, N, device="cuda", generator=g) * 2 - 1).mul(65000).to(dt) if act == 16 else None
    Am, Bm = _mats(A, B, 1, 1)
    pre = Am @ Bm.t()
    y, slope = _act64(pre, act, aux)
    acc = _acc_bound(Am, Bm) * (1 + slope) + 2.0 ** -20 * (pre.abs() + y.abs()) + 1e-30
    out = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
    outp = torch.full((M, N), float("nan"), device="cuda", dtype=dt) if act in (1,) else None
    o.gemm_bf16(A, B, act=act, aux=aux, out_bf16=out, out_pre=outp, tile_config=cfg)
    torch.cuda.synchronize()
    for got, ref, bnd in ((out, y, acc),) + (((outp, pre, _acc_bound(Am, Bm) + 1e-30),) if outp is not None else ()):
        assert not bool(got.isnan().any()), "NaN from a finite product"
        sure_inf = ref.abs() > F16_MAX_RND + bnd
        sure_fin = ref.abs() < 65504.0 - bnd
        assert bool(sure_inf.any()) and bool(sure_fin.any()), "the case must reach past the fp16 range"
        gi = got[sure_inf].double()
        assert bool((gi.isinf() & (gi.sign() == ref[sure_inf].sign())).all()), "overflow must give +-inf like IEEE fp16 rounding"
        m = sure_fin
        b16 = bnd + U(dt) * ref.abs() + FLOOR(dt)
        within(f"cfg{cfg} act{act} finite part", got.double().where(m, ref), ref, b16.where(m, torch.ones_like(ref)))
        _assert_sensitive(got.double().where(m, ref), ref, b16, Am, Bm, 1.0, slope if ref is y else None)


@pytest.mark.parametrize("cfg,akc,bkc", [(1, 1, 1), (3, 1, 0), (8, 1, 1), (2, 0, 0), (11, 0, 0)])
@pytest.mark.parametrize("sub_operands", [False, True])
def test_gemm_f16_subnormal_range(cfg, akc, bkc, sub_operands):
    """Outputs in the fp16 subnormal range (< 6.1e-5) from normal operands (2^-9 scale), and from operands that are themselves
    fp16 subnormals (one operand scaled by 2^-16): a flush to zero at either end shows up against fp64."""
    o = ops()
    dt = torch.float16
    M, N, K = 264, 136, 256
    g = G(cfg + 17 * sub_operands)
    sa, sb = (2.0 ** -16, 2.0 ** -4) if sub_operands else (2.0 ** -9, 2.0 ** -9)
    A = rnd((M, K) if akc else (K, M), dt, g, sa)
    B = rnd((N, K) if bkc else (K, N), dt, g, sb)
    if sub_operands:
        assert bool(((A.abs() < 2.0 ** -14) & (A != 0)).float().mean() > 0.9)
    Am, Bm = _mats(A, B, akc, bkc)
    ref = Am @ Bm.t()
    assert bool((ref.abs() < 2.0 ** -14).float().mean() > 0.5), "most outputs must be fp16 subnormals"
    out = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
    outf = torch.full((M, N), float("nan"), device="cuda")
    o.gemm_bf16(A, B, a_kcontig=bool(akc), b_kcontig=bool(bkc), out_bf16=out, tile_config=cfg)
    o.gemm_bf16(A, B, a_kcontig=bool(akc), b_kcontig=bool(bkc), out_f32=outf, tile_config=cfg)
    torch.cuda.synchronize()
    bound = _acc_bound(Am, Bm) + 1e-30
    within("subnormal f32 out", outf, ref, bound)
    _assert_sensitive(outf, ref, bound, Am, Bm)
    b16 = bound + U(dt) * ref.abs() + FLOOR(dt)
    within("subnormal 16-bit out", out, ref, b16)
    assert bool((out != 0).float().mean() > 0.9), "subnormal outputs flushed to zero"


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
# _split_heads, _attn64 and _attn_bounds live in tests/attn_refs_f64.py, shared with the BlockStack tests (tests/stack_ref_f64.py)


def _run_attention(dt, B, T, H, causal, keep, g, qs=1.0, ks=1.0, vs=1.0, ds=1.0, q_zero=False):
    o = ops()
    D = H * 64
    qkv = torch.randn(B * T, 3 * D, device="cuda", generator=g)
    qkv[:, :D] *= qs; qkv[:, D:2 * D] *= ks; qkv[:, 2 * D:] *= vs
    qkv[:, 2 * D:].clamp_(-60000.0, 60000.0)                 # finite in fp16
    if q_zero:
        qkv[:, :D] = 0
    qkv = qkv.to(dt)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out = torch.full((B * T, D), float("nan"), device="cuda", dtype=dt)
    lse = torch.full((B, H, T), float("nan"), device="cuda")
    o.attention_fwd(q, k, v, out, B=B, T=T, H=H, causal=causal, key_keep=keep, lse=lse)
    dout = (torch.randn(B * T, D, device="cuda", generator=g) * ds).to(dt)
    dqkv = torch.full((B * T, 3 * D), float("nan"), device="cuda", dtype=dt)
    o.attention_bwd(q, k, v, out, lse, dout, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=B, T=T, H=H, causal=causal, key_keep=keep)
    torch.cuda.synchronize()
    ref = _attn64(_split_heads(q, B, T, H), _split_heads(k, B, T, H), _split_heads(v, B, T, H), _split_heads(dout, B, T, H),
                  causal, keep, 0.125)
    got = dict(o=_split_heads(out, B, T, H), dq=_split_heads(dqkv[:, :D], B, T, H), dk=_split_heads(dqkv[:, D:2 * D], B, T, H),
               dv=_split_heads(dqkv[:, 2 * D:], B, T, H))
    return got, lse, ref


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T,causal", [(5, False), (50, False), (77, True), (128, False), (129, True), (197, False), (257, True), (577, False)])
def test_attention_fwd_bwd_f64(T, causal, dt):
    """Short (T <= 128, one work-group per (sequence, head)) and long kernels (T > 128: attn_long_fwd / bwd_dkv / bwd_dq), with
    key padding in two of the sequences; o, lse, dq, dk, dv per element against fp64."""
    B, H = 3, 2
    g = G(T * 7 + causal)
    keep = torch.ones(B, T, device="cuda")
    keep[0, max(1, T - 3):] = 0
    keep[2, max(1, T // 2):] = 0
    got, lse, ref = _run_attention(dt, B, T, H, causal, keep, g)
    o_r, lse_r, dq_r, dk_r, dv_r, mag = ref
    bnd = _attn_bounds(mag, 0.125, dt)
    within(f"attn o T{T}", got["o"], o_r, bnd["o"], dt=dt)
    within(f"attn lse T{T}", lse, lse_r, 1e-5 * (1 + lse_r.abs()))
    for nm, r in (("dq", dq_r), ("dk", dk_r), ("dv", dv_r)):
        within(f"attn {nm} T{T}", got[nm], r, bnd[nm], dt=dt)


def test_attention_f16_range_cases():
    """fp16 attention at the ends of the range.  (1) values of up to 6e4: o stays finite and within the bound.  (2) uniform
    attention (q = 0) with a large upstream gradient in one column: dv of the first keys passes 65504 and must be +inf exactly
    where IEEE rounding of the fp64 value is; nothing is NaN.  (3) an upstream gradient of 2^-13: dS = P (dP - delta) falls in
    the fp16 subnormal range; a flush to zero would zero dq / dk."""
    dt, B, H, T = torch.float16, 2, 2, 128
    got, _, ref = _run_attention(dt, B, T, H, True, None, G(1), vs=2.0e4)
    bnd = _attn_bounds(ref[5], 0.125, dt)
    assert ref[0].abs().max() > 2e4
    within("large v: o", got["o"], ref[0], bnd["o"], dt=dt)
    # (2)
    o = ops()
    D = H * 64
    g = G(2)
    qkv = torch.randn(B * T, 3 * D, device="cuda", generator=g) * 0.5
    qkv[:, :D] = 0
    qkv = qkv.to(dt)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out = torch.empty(B * T, D, device="cuda", dtype=dt)
    lse = torch.empty(B, H, T, device="cuda")
    o.attention_fwd(q, k, v, out, B=B, T=T, H=H, causal=True, lse=lse)
    dout = torch.zeros(B * T, D, device="cuda", dtype=dt)
    dout[:, 3] = 2.0e4                                         # head 0, column 3
    dqkv = torch.full((B * T, 3 * D), float("nan"), device="cuda", dtype=dt)
    o.attention_bwd(q, k, v, out, lse, dout, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=B, T=T, H=H, causal=True)
    torch.cuda.synchronize()
    assert not bool(dqkv.isnan().any()), "NaN in the gradients of a finite problem"
    r = _attn64(_split_heads(q, B, T, H), _split_heads(k, B, T, H), _split_heads(v, B, T, H), _split_heads(dout, B, T, H), True, None, 0.125)
    dv, dv_r = _split_heads(dqkv[:, 2 * D:], B, T, H), r[4]
    bdv = _attn_bounds(r[5], 0.125, dt)["dv"]
    sure_inf = dv_r.abs() > F16_MAX_RND + bdv
    sure_fin = dv_r.abs() < 65504.0 - bdv
    assert bool(sure_inf.any())
    assert bool((dv[sure_inf].isinf() & (dv[sure_inf].sign() == dv_r[sure_inf].sign())).all())
    within("large dO: finite dv", dv.where(sure_fin, dv_r), dv_r, bdv.where(sure_fin, torch.ones_like(bdv)))
    # (3)
    got, _, ref = _run_attention(dt, B, 50, H, False, None, G(3), ds=2.0 ** -13)
    bnd = _attn_bounds(ref[5], 0.125, dt)
    for nm, i in (("dq", 2), ("dk", 3), ("dv", 4)):
        within(f"subnormal dS: {nm}", got[nm], ref[i], bnd[nm], dt=dt)
        assert bool((got[nm] != 0).float().mean() > 0.9), f"{nm} flushed to zero"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("lens,causal", [([1, 77, 30, 64, 77, 2], True), ([128, 1, 100, 17], False)])
def test_attention_packed_cu_seqlens_f64(lens, causal, dt):
    """Packed batches (cu_seqlens, the text tower's default path): sequence b = rows [cu[b], cu[b+1]), lengths 1 .. T_max, each
    sequence against its own fp64 attention; rows past cu[B] are never written, forward or backward."""
    o = ops()
    B, H, T = len(lens), 2, max(lens)
    D = H * 64
    R = sum(lens)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), device="cuda", dtype=torch.int32)
    g = G(R + causal)
    qkv = torch.randn(R + 5, 3 * D, device="cuda", generator=g).to(dt)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out = torch.full((R + 5, D), SENT, device="cuda", dtype=dt)
    out[:R] = float("nan")
    lse = torch.full((B, H, T), float("nan"), device="cuda")
    o.attention_fwd(q, k, v, out, B=B, T=T, H=H, causal=causal, lse=lse, cu=cu)
    dout = torch.randn(R + 5, D, device="cuda", generator=g).to(dt)
    dqkv = torch.full((R + 5, 3 * D), SENT, device="cuda", dtype=dt)
    dqkv[:R] = float("nan")
    o.attention_bwd(q, k, v, out, lse, dout, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=B, T=T, H=H, causal=causal, cu=cu)
    torch.cuda.synchronize()
    assert bool((out[R:] == SENT).all()) and bool((dqkv[R:] == SENT).all()), "rows past cu[B] were written"
    for b, L in enumerate(lens):
        r0 = int(cu[b])
        sl = slice(r0, r0 + L)
        sp = lambda x: _split_heads(x[sl], 1, L, H)
        ref = _attn64(sp(q), sp(k), sp(v), sp(dout), causal, None, 0.125)
        bnd = _attn_bounds(ref[5], 0.125, dt)
        within(f"packed seq {b} (len {L}) o", sp(out), ref[0], bnd["o"], dt=dt)
        within(f"packed seq {b} lse", lse[b, :, :L], ref[1][0], 1e-5 * (1 + ref[1][0].abs()))
        for nm, i, c0 in (("dq", 2, 0), ("dk", 3, D), ("dv", 4, 2 * D)):
            within(f"packed seq {b} (len {L}) {nm}", sp(dqkv[:, c0:c0 + D]), ref[i], bnd[nm], dt=dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,T,H,dh", [(2, 40, 8, 96), (3, 17, 4, 32)])
def test_attention_small_f64(B, T, H, dh, dt):
    """Generic-head_dim attention at the TransformerMapper geometry (8 heads x 96, 40 tokens) and one more head_dim."""
    o = ops()
    D = H * dh
    g = G(B * T * dh)
    qkv = torch.randn(B * T, 3 * D, device="cuda", generator=g).to(dt)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out = torch.full((B * T, D), float("nan"), device="cuda", dtype=dt)
    lse = torch.empty(B, H, T, device="cuda")
    o.attention_small_fwd(q, k, v, out, B=B, T=T, H=H, head_dim=dh, lse=lse)
    dout = torch.randn(B * T, D, device="cuda", generator=g).to(dt)
    dqkv = torch.full((B * T, 3 * D), float("nan"), device="cuda", dtype=dt)
    o.attention_small_bwd(q, k, v, out, lse, dout, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=B, T=T, H=H, head_dim=dh)
    torch.cuda.synchronize()
    sp = lambda x: _split_heads(x, B, T, H, dh)
    sc = dh ** -0.5
    ref = _attn64(sp(q), sp(k), sp(v), sp(dout), False, None, sc)
    bnd = _attn_bounds(ref[5], sc, dt)
    within("small o", sp(out), ref[0], bnd["o"], dt=dt)
    within("small lse", lse, ref[1], 1e-5 * (1 + ref[1].abs()))
    for nm, i, c0 in (("dq", 2, 0), ("dk", 3, D), ("dv", 4, 2 * D)):
        within(f"small {nm}", sp(dqkv[:, c0:c0 + D]), ref[i], bnd[nm], dt=dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S,B,H", [(1, 3, 4), (7, 8, 16), (64, 2, 12), (65, 5, 3), (1000, 2, 16), (2048, 8, 2)])
def test_attention_decode_f64(S, B, H, dt):
    """cclip_attention_decode (one query per sequence against its KV cache): padded position and sequence strides, a padded
    output row stride whose padding must survive; per (sequence, head) against fp64."""
    o = ops()
    D = H * 64
    Smax, pad = S + 3, 16
    g = G(S * 100 + B * 10 + H)
    kc = rnd((B, Smax, D + pad), dt, g)
    vc = rnd((B, Smax, D + pad), dt, g)
    kcache, vcache = kc[:, :, :D], vc[:, :, :D]
    q = rnd((B, D + pad), dt, g)[:, :D]
    obuf = torch.full((B + 1, D + pad), SENT, device="cuda", dtype=dt)
    obuf[:B, :D] = float("nan")
    o.attention_decode(q, kcache, vcache, obuf[:B, :D], H=H, S=S)
    torch.cuda.synchronize()
    pad_mask = torch.ones_like(obuf, dtype=torch.bool)
    pad_mask[:B, :D] = False
    assert bool((obuf[pad_mask] == SENT).all()), "write outside the output rows"
    qh = q.double().view(B, H, 1, 64)
    kh = kcache[:, :S].double().view(B, S, H, 64).permute(0, 2, 1, 3)
    vh = vcache[:, :S].double().view(B, S, H, 64).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * 0.125
    P = torch.softmax(s, -1)
    ref = (P @ vh).view(B, H * 64)
    bound = (4 * U(dt) * (P @ vh.abs()) + FLOOR(dt) * vh.abs().sum(-2, keepdim=True) + FLOOR(dt)).view(B, H * 64)
    within(f"decode S{S}", obuf[:B, :D], ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# smaller kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,D", [(7, 128), (513, 768), (64, 1024)])
def test_layernorm_16bit_io_f64(rows, D, dt):
    """LayerNorm forward with a 16-bit output, backward with a 16-bit upstream gradient and 16-bit dx, and the gathered
    (row_index) forms, against fp64 LayerNorm."""
    o = ops()
    g = G(rows + D)
    x = torch.randn(rows + 5, D, device="cuda", generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(D, device="cuda", generator=g)
    beta = 0.1 * torch.randn(D, device="cuda", generator=g)
    idx = torch.randperm(rows + 5, device="cuda", generator=g)[:rows].to(torch.int32)
    xs = x[idx.long()].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xs, (D,), gamma.double(), beta.double(), 1e-5)
    u = U(dt)
    buf, out = canvas(rows, D, dt)
    mean = torch.empty(rows, device="cuda"); rstd = torch.empty(rows, device="cuda")
    o.layernorm_fwd(x, gamma, beta, rows=rows, row_index=idx, out_bf16=out, mean=mean, rstd=rstd)
    torch.cuda.synchronize()
    check_canvas("ln out", buf, rows, D)
    within("ln 16-bit out", out, y.detach(), u * y.detach().abs() + 1e-5 * (1 + y.detach().abs()) + FLOOR(dt))
    dy = rnd((rows, D), dt, g)
    y.backward(dy.double())
    dxb = torch.full((rows + 5, D), SENT, device="cuda", dtype=dt)
    dxb[idx.long()] = float("nan")
    o.layernorm_bwd(dy, x, gamma, mean, rstd, rows=rows, row_index=idx, dx_out_bf16=dxb)
    torch.cuda.synchronize()
    left = torch.ones(rows + 5, dtype=torch.bool, device="cuda")
    left[idx.long()] = False
    assert bool((dxb[left] == SENT).all()), "dx rows outside row_index were written"
    ref = xs.grad
    # |dx| <= rstd * |gamma| * (|dy| + mean|dy| + |xhat| mean|dy xhat|): fp32 sums of D terms, one 16-bit rounding
    xh = (xs.detach() - xs.detach().mean(1, keepdim=True)) * torch.rsqrt(xs.detach().var(1, unbiased=False, keepdim=True) + 1e-5)
    dyg = dy.double().abs() * gamma.double().abs()
    mag = torch.rsqrt(xs.detach().var(1, unbiased=False, keepdim=True) + 1e-5) * (dyg + dyg.mean(1, keepdim=True) + xh.abs() * (dyg * xh.abs()).mean(1, keepdim=True))
    within("ln 16-bit dx", dxb[idx.long()], ref, u * ref.abs() + 1e-5 * mag + FLOOR(dt))


@pytest.mark.parametrize("dt", DTS)
def test_patchify_16bit_is_exact(dt):
    o = ops()
    P, grid, B = 14, 3, 2
    R = P * grid
    img = torch.randn(B, 3, R, R, device="cuda", generator=G(5)) * 3
    KP = 3 * P * P
    KPAD = (KP + 7) // 8 * 8
    out = torch.full((B * (grid * grid + 1), KPAD), float("nan"), device="cuda", dtype=dt)
    o.patchify(img, out, P)
    ref = torch.nn.functional.unfold(img, kernel_size=P, stride=P).transpose(1, 2)
    got = out.view(B, grid * grid + 1, KPAD)
    assert torch.equal(got[:, 1:, :KP], ref.to(dt))
    assert (got[:, 0] == 0).all() and (got[:, :, KP:] == 0).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("R,C", [(1000, 768), (4097, 104), (3, 2304)])
def test_colsum_16bit_input_f64(R, C, dt):
    o = ops()
    g = G(R + C)
    x = rnd((R, C + 8), dt, g)
    out = torch.ones(C, device="cuda")
    ws = torch.empty(o.colsum_ws_floats(R, C), device="cuda")
    o.colsum(x, out, ws, R=R, C=C, ld=C + 8, accumulate=True)
    torch.cuda.synchronize()
    xv = x[:, :C].double()
    ref = 1 + xv.sum(0)
    within("colsum", out, ref, C_ACC * 2.0 ** -24 * math.sqrt(R) * (1 + xv.abs().sum(0)) + 1e-30)


@pytest.mark.parametrize("dt", DTS)
def test_xent_rows_16bit_dlogits_at_caption_vocab(dt):
    """xent_rows writing 16-bit dlogits at the caption vocabulary width (21128 classes): softmax - onehot, scaled, one 16-bit
    rounding per element; ignored rows get zero gradient."""
    o = ops()
    R, C = 37, 21128
    g = G(C)
    lg = torch.randn(R, C, device="cuda", generator=g) * 4
    labels = torch.randint(0, C, (R,), device="cuda", generator=g, dtype=torch.int32)
    labels[5] = -100
    d = torch.full((R, C + 8), SENT, device="cuda", dtype=dt)
    d[:, :C] = float("nan")
    lrow = torch.empty(R, device="cuda")
    o.xent_rows(lg, labels, loss_row=lrow, dlogits=d[:, :C], grad_scale=0.5)
    torch.cuda.synchronize()
    assert bool((d[:, C:] == SENT).all())
    l64 = lg.double()
    p = torch.softmax(l64, 1)
    oh = torch.zeros_like(p)
    valid = labels >= 0
    oh[valid.nonzero().flatten(), labels[valid].long()] = 1
    ref = 0.5 * (p - oh) * valid[:, None].double()
    within("xent 16-bit dlogits", d[:, :C], ref, U(dt) * ref.abs() + 1e-6 * p + FLOOR(dt) + 1e-30)
    lref = (torch.logsumexp(l64, 1) - l64.gather(1, labels.clamp_min(0).long()[:, None])[:, 0]) * valid.double()
    within("xent loss", lrow, lref, 1e-5 * (1 + lref.abs()))


@pytest.mark.parametrize("dt", DTS)
def test_adamw_16bit_shadow_and_cast(dt):
    """AdamW with a 16-bit shadow: the shadow is the round-to-nearest 16-bit copy of the updated fp32 parameter, bit for bit; the
    fp32 update against fp64.  cast_f32_to_{bf16,f16}: bit for bit against torch's rounding, including ties, subnormals,
    overflow to inf, the largest finite values and signed zeros."""
    o = ops()
    g = G(9)
    n = 4096 + 64
    p = torch.randn(n, device="cuda", generator=g)
    p[:64] *= 1e-6                      # parameters whose 16-bit copies are small / subnormal in fp16
    gr = torch.randn(n, device="cuda", generator=g)
    m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    pr, mr, vr = p.double(), torch.zeros(n, device="cuda", dtype=torch.float64), torch.zeros(n, device="cuda", dtype=torch.float64)
    sh = torch.full((n,), float("nan"), device="cuda", dtype=dt)
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-6, 0.01
    for step in range(1, 4):
        o.adamw_step(p, gr, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step=step, bf16_shadow=sh)
        mr = b1 * mr + (1 - b1) * gr.double()
        vr = b2 * vr + (1 - b2) * gr.double() ** 2
        ss = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        pr = pr - ss * mr / (vr.sqrt() + eps)
        pr = pr - lr * wd * pr
    torch.cuda.synchronize()
    within("adamw p", p, pr, 1e-6 * (pr.abs() + lr))
    assert torch.equal(sh, p.to(dt)), "the shadow must be the rounded copy of the fp32 parameter"
    # casts
    vals = torch.cat([torch.randn(4096, device="cuda", generator=g) * s for s in (1.0, 1e-5, 1e-7, 3e4, 1e38)] + [
        torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26,
                      1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895e38, float("inf"),
                      -float("inf"), 1e-40, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25], device="cuda")])
    vals = vals[: vals.numel() // 4 * 4].contiguous()
    dst = torch.full(vals.shape, float("nan"), device="cuda", dtype=dt)
    o.cast_f32_to_bf16(vals, dst)
    torch.cuda.synchronize()
    want = vals.to(dt)
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), \
        f"cast differs at {(dst.view(torch.int16) != want.view(torch.int16)).nonzero()[:6].flatten().tolist()}"
