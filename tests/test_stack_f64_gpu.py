"""GPU: cclip_hip.stack.BlockStack constructed directly - hand-made BlockWeights at width 128, two blocks, NaN-prefilled fp32
gradient buffers, no model and no arena - against the float64 reference of tests/stack_ref_f64.py, in both 16-bit types.

A. Forward, launch by launch: every tensor the stack saves against float64 computed from THAT launch's saved inputs (the exact
   16-bit operands the kernel received), under the bound the kernel already has in the suite: kernel_refs_f64.ln_fwd (+ one
   16-bit rounding), gemm_refs_f64.epilogue_bounds, attn_refs_f64._attn_bounds and 1e-5 (1 + |lse|).  No error budget
   accumulates, so no new tolerance exists.  The compact tail (tail_rows) is judged the same way on its own operands; its
   attention rows are the full run's bit for bit, and its x_mid rows are within twice the GEMM bound of the full run's (both
   lie within one bound of the same float64 value: the two runs use different tile configurations).  The compact OUTPUT is
   judged against float64 of its own g / x_mid, not against the full run's rows: a 16-bit rounding of xn2 that falls the
   other way moves h by u |xn2| |w|, far more than the c_proj GEMM's bound.
B. Prefill: kv_out holds the k / v column blocks of the saved qkv bit for bit, the cache past T keeps its sentinel.
C. Backward against the float64 replay of the stack's own saved activations: per gradient tensor
       e_gpu = |got - g_exact| / |g_exact|  <=  2 e_round + C_ACC 2^-24 sqrt(K)
   with e_round the same figure of the reference's own 16-bit replay, computed here (stack_ref_f64.accepts).  Then every planted
   fault of stack_ref_f64.FAULTS: the device result must fall OUTSIDE the same region drawn around the faulty reference.
D. Exact invariants: side stream on / off / repeated, param_grads=False, a frozen block, the acc flags.

   decode_step: prefill of T-1 positions, then one step at pos = T-1.  x is updated in place, cache rows [0, pos) keep their
   bits and rows past pos their sentinel; block 0's new k / v row lies inside the per-element bound of the launches behind it
   (stack_ref_f64.row_chain64).  A worst-case per-element sum carried through |W| is useless past the first attention (bf16:
   0.07 on q, 4.5 on the attention output, inf after two blocks), so block 1's k / v row and the final x are judged the way
   section C judges gradients: relative L2 against the unrounded float64 forward <= 2 e_round + acc, e_round being the same
   figure of the 16-bit mimic of the forward; the last row of a T-position forward is held to the same, and the two device
   results to twice it.  A reference taken at pos - 1, and one with ln_2's affine used for ln_1 in block 1, are rejected.
   The compact-tail output is compared with the full run's rows in the same way.

Measured on an MI355X (58 tests, 5 s), largest e_gpu / e_round per geometry and tensor family (w matrices, b biases, ln LayerNorm
affines, dx = dx_in), fp16 / bf16 - the bound allows 2:
    vis    w 1.00 / 1.01   b 1.02 / 1.01   ln 1.07 / 1.25   dx 0.98 / 1.01
    txt    w 1.00 / 1.00   b 1.05 / 1.01   ln 1.09 / 1.01   dx 0.98 / 1.00
    pack   w 1.00 / 1.00   b 1.05 / 1.01   ln 1.04 / 1.01   dx 1.00 / 1.00
    pack64 w 1.02 / 1.01   b 1.06 / 1.00   ln 1.07 / 1.02   dx 1.00 / 1.01
    gpt    w 1.02 / 1.00   b 1.01 / 1.00   ln 1.01 / 1.01   dx 1.01 / 1.00
    map    w 1.00 / 1.00   b 1.00 / 1.00   ln 1.15 / 1.00   dx 0.95 / 0.94
  Forward, worst err / bound: LayerNorm 16-bit 0.99, mean 0.026, rstd 0.068; GEMM 16-bit 0.99 (one output rounding, tight by
  construction), fp32 0.029; attention o 0.36, lse 0.028; compact-tail x_mid against the full run 0.019.  Every exact invariant
  of D held bit for bit (side stream on / off / repeated at M % 64 == 0, param_grads=False, frozen block, unflagged tensors under
  acc; flagged tensors within 0.09 of the 2^-22 bound on g1 + g2).  decode_step: block 0's k / v row 0.27 of its per-element bound;
  e / e_round of block 1's k 1.00 / 1.01, v 1.00 / 0.97, final x 0.99 / 1.01, with decode against the forward's last row at 0.5 - 0.6
  of e_round.  No defect was found; stack.py, ops.py and the kernels are unchanged.
"""
import pytest
import torch

import kernel_refs_f64 as KR
import stack_ref_f64 as S
from attn_refs_f64 import _attn64, _attn_bounds, _split_heads
from gemm_refs_f64 import FLOOR, SENT, U, WORST, _acc_bound, _worst_report, epilogue_bounds, epilogue_ref, within  # noqa: F401

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
NAN = float("nan")


def dtn(dt):
    return str(dt).replace("torch.", "")


def cuda(t):
    return None if t is None else t.cuda()


class Rig:
    """one geometry on the device: the stack, its weights as dicts (for the reference) and the case's inputs"""

    def __init__(self, tag, dt, wt=False, frozen=()):
        from cclip_hip.stack import BlockStack, BlockWeights, Scratch, StackGeometry
        c = S.make_case(tag, dt)
        self.c, self.tag, self.dt, self.geo = c, tag, dt, c["geo"]
        geo = self.geo
        dev = torch.device("cuda")
        self.w = [{n: cuda(t) for n, t in w.items()} for w in c["weights"]]
        self.blocks = []
        for l, w in enumerate(self.w):
            grads = None if l in frozen else {n: torch.full(t.shape, NAN, device=dev) for n, t in w.items() if t is not None}
            wts = {n: w[n].t().contiguous() for n in S.MATS} if wt else None
            self.blocks.append(BlockWeights(**w, grads=grads, wt=wts))
        sg = StackGeometry(width=geo.D, heads=geo.H, tokens=0 if tag == "gpt" else c["T"], linear_layout=geo.linear, act=geo.act,
                           causal=geo.causal, head_dim=geo.dh, hidden=geo.Hd)
        self.stack = BlockStack(sg, self.blocks, Scratch(dev), dtype=dt)
        self.B, self.T, self.M = c["B"], c["T"], c["M"]
        self.keep, self.cu, self.rows = cuda(c["key_keep"]), cuda(c["cu"]), cuda(c["tail_rows"])
        self.dx_scale = 1.0

    def forward(self, tail=False, **kw):
        saved = self.stack.alloc_saved(self.B, torch.device("cuda"), T=self.T, M=self.M if self.cu is not None else None)
        saved["xs"][0, 0].copy_(self.c["x"])
        out = self.stack.forward(saved["xs"][0, 0], self.B, saved=saved, key_keep=self.keep, T=self.T, cu=self.cu,
                                 tail_rows=self.rows if tail else None, **kw)
        torch.cuda.synchronize()
        return out, saved

    def grad_inputs(self, tail):
        """(dx fp32, dxb: its 16-bit copy as the first rows of a taller NaN-filled buffer - a read past the last row shows)"""
        dx = cuda(self.c["dx_tail"] if tail else self.c["dx"]) * self.dx_scale
        n = dx.shape[0]
        big = torch.full((n + 7, self.geo.D), NAN, device="cuda", dtype=self.dt)
        big[:n] = dx.to(self.dt)
        return dx, big[:n]

    def poison(self, saved):
        """NaN-filled 16-bit buffers of the shapes backward() is about to torch.empty, freed again: the caching allocator hands
        the same blocks back, so a buffer read before it is written (dsm of the compact tail without its zero_()) gives NaN
        instead of whatever the allocator held."""
        L, Mp, M, D, Hd = len(self.blocks), saved["Mp"], saved["M"], self.geo.D, self.geo.Hd
        bufs = [torch.full(sh, NAN, device="cuda", dtype=self.dt)
                for sh in ((L, Mp, Hd), (L, Mp, 3 * D), (2 * L, Mp, D), (M, D), (Mp, 4 * D + Hd), (Mp, D))]
        torch.cuda.synchronize()
        del bufs

    def refill(self, keep_ids=()):
        for b in self.blocks:
            for t in (b.grads or {}).values():
                if id(t) not in keep_ids:
                    t.fill_(NAN)

    def backward(self, saved, tail=False, acc=None, **kw):
        """returns {key: gradient} (clones; 'dxb' = the returned 16-bit copy)"""
        dx, dxb = self.grad_inputs(tail)
        self.poison(saved)
        ret = self.stack.backward(dx, dxb, saved, {} if acc is None else acc, **kw)
        torch.cuda.synchronize()
        got = {"dx_in": saved["dx_in"].clone(), "dxb": ret.clone()}
        for l, b in enumerate(self.blocks):
            for n, t in (b.grads or {}).items():
                got[(l, n)] = t.clone()
        return got


def family(key):
    if key == "dx_in":
        return "dx"
    return "w" if key[1] in S.MATS else ("ln" if key[1].startswith("ln") else "b")


def compare_backward(r, saved, got, tail, label):
    """section C on one device result: every tensor inside 2 e_round + acc around the exact replay, outside it around every
    planted fault's replay"""
    geo, M, dt = r.geo, r.M, r.dt
    dx, dxb = r.grad_inputs(tail)
    frozen = tuple(l for l, b in enumerate(r.blocks) if b.grads is None)
    run = lambda **kw: S.flat(S.stack_backward64(saved, r.w, dx, geo, dxb=dxb, frozen=frozen, **kw))
    exact, rounded = run(), run(round_to=dt)
    assert set(exact) == set(got) - {"dxb"}
    for key, ref in exact.items():
        assert bool(torch.isfinite(got[key]).all()), f"{label} {key}: non-finite gradient"
        ok, e, er = S.accepts(got[key], ref, rounded[key], S.contraction(key, geo, M))
        print(f"{label} {dtn(dt)} {key}: e_gpu {e:.3g} e_round {er:.3g}")
        assert ok, f"{label} {key}: e_gpu {e:.3g} > 2 * e_round {er:.3g} + acc {S.acc_term(S.contraction(key, geo, M)):.3g}"
        if er > 0:
            k = (f"stackC {r.tag} {family(key)}", dtn(dt))
            WORST[k] = max(WORST.get(k, 0.0), e / er)
    # the 16-bit copy handed back: exactly M rows, one rounding of the fp32 gradient
    assert got["dxb"].shape == (M, geo.D) and got["dxb"].dtype == dt
    d = got["dx_in"].double()
    assert bool(((got["dxb"].double() - d).abs() <= U(dt) * d.abs() + FLOOR(dt)).all()), f"{label}: dxb is not the rounded dx_in"
    for fault in S.faults_of(r.tag, tail):
        key = S.fault_target(fault)
        if key not in exact:
            continue
        ok, e, er = S.accepts(got[key], run(fault=fault)[key], run(fault=fault, round_to=dt)[key], S.contraction(key, geo, M))
        assert not ok, f"{label}: the bound cannot see '{S.FAULTS[fault]}' in {key} (e {e:.3g}, e_round {er:.3g})"


# ---------------------------------------------------------------------------------------------------------------------------
# A. forward, launch by launch
# ---------------------------------------------------------------------------------------------------------------------------
def ln_check(name, x, gamma, beta, y16, mean, rstd, dt):
    ref, bnd = KR.ln_fwd(x, gamma, beta)
    within(f"stackA.ln {name}", y16, ref["y"], bnd["y"] + U(dt) * ref["y"].abs() + FLOOR(dt), dt=dt)
    within(f"stackA.ln.mean {name}", mean, ref["mean"], bnd["mean"] + 1e-300, dt=dt)
    within(f"stackA.ln.rstd {name}", rstd, ref["rstd"], bnd["rstd"], dt=dt)


def gemm_check(name, A, Wt, bias, act, res, geo, dt, out32=None, out16=None, pre=None):
    """one projection from the operands as stored; returns the fp32-output bound"""
    Am, Bm = A.double(), S._wm(Wt, geo)
    e = epilogue_ref(Am, Bm, 1.0, bias, act, res)
    bf, b16, bp = epilogue_bounds(_acc_bound(Am, Bm), e, dt)
    if out32 is not None:
        within(f"stackA.gemm {name} f32", out32, e["ref"], bf, dt=dt)
    if out16 is not None:
        within(f"stackA.gemm {name} 16", out16, e["ref"], b16, dt=dt)
    if pre is not None:
        within(f"stackA.gemm {name} pre", pre, e["pre"], bp, dt=dt)
    return bf, e["ref"]


def attn_check(name, qkv, a, lse, r):
    geo, D = r.geo, r.geo.D
    scale = geo.dh ** -0.5
    q, k, v = qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D]
    for b, (sl, nb, t, keep) in enumerate(S.seq_groups(r.B, r.T, r.keep, r.cu, r.M)):
        sp = lambda x: _split_heads(x[sl], nb, t, geo.H, geo.dh)
        o_r, lse_r, _, _, _, mag = _attn64(sp(q), sp(k), sp(v), torch.zeros_like(sp(q)), geo.causal, keep, scale)
        within(f"stackA.attn {name} seq{b}", sp(a), o_r, _attn_bounds(mag, scale, r.dt)["o"], dt=r.dt)
        got_lse = lse if r.cu is None else lse[b:b + 1, :, :t]
        within(f"stackA.lse {name} seq{b}", got_lse, lse_r, 1e-5 * (1 + lse_r.abs()), dt=r.dt)


def check_forward(r, out, saved, tail):
    geo, M, dt = r.geo, r.M, r.dt
    D, Hd, L = geo.D, geo.Hd, len(r.w)
    info = {}
    for l, w in enumerate(r.w):
        row = saved["bf"][l][:M]
        xn1, qkv, a = row[:, 0:D], row[:, D:4 * D], row[:, 4 * D:5 * D]
        xn2, h, g = row[:, 5 * D:6 * D], row[:, 6 * D:6 * D + Hd], row[:, 6 * D + Hd:6 * D + 2 * Hd]
        x_in, x_mid = saved["xs"][l, 0], saved["xs"][l, 1]
        m1, r1, m2, r2 = saved["st"][l]
        x_out = saved["xs"][l + 1, 0] if l + 1 < L else (out if tail else saved["out"])
        nm = f"{r.tag} l{l}"
        ln_check(nm + " ln1", x_in, w["ln1_w"], w["ln1_b"], xn1, m1, r1, dt)
        gemm_check(nm + " qkv", xn1, w["w_qkv"], w["b_qkv"], 0, None, geo, dt, out16=qkv)
        attn_check(nm, qkv, a, saved["lse"][l], r)
        if tail and l == L - 1:
            t = saved["tail"]
            assert torch.equal(t["rows"], r.rows) and torch.equal(t["a"], a.index_select(0, r.rows)), "compact attention rows"
            a, x_in, x_mid, xn2, h, g = t["a"], x_in.index_select(0, r.rows), t["xmid"], t["xn2"], t["h"], t["g"]
            m2, r2 = t["st"]
            nm += " tail"
        info["bound_mid"], info["ref_mid"] = gemm_check(nm + " o", a, w["w_o"], w["b_o"], 0, x_in, geo, dt, out32=x_mid)
        info["x_mid"] = x_mid
        ln_check(nm + " ln2", x_mid, w["ln2_w"], w["ln2_b"], xn2, m2, r2, dt)
        gemm_check(nm + " fc", xn2, w["w_fc"], w["b_fc"], geo.act, None, geo, dt, out16=g, pre=h)
        gemm_check(nm + " proj", g, w["w_proj"], w["b_proj"], 0, x_mid, geo, dt, out32=x_out)
    assert bool((saved["bf"][:, M:] == 0).all()), "rows [M, Mp) of the 16-bit slab are no longer zero"
    assert bool(torch.isfinite(saved["out"] if not tail else out).all())
    return info


FWD = [("vis", False), ("txt", False), ("txt", True), ("pack", False), ("pack", True), ("pack64", False), ("gpt", False), ("map", False)]


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag,tail", FWD)
def test_forward_launch_by_launch(tag, tail, dt):
    r = Rig(tag, dt)
    out, saved = r.forward(tail)
    assert saved["Mp"] == (r.M + 63) // 64 * 64 and saved["bf"].shape[1] == saved["Mp"]
    info = check_forward(r, out, saved, tail)
    if tail:
        assert out.shape == (r.rows.numel(), r.geo.D)
        out_f, saved_f = r.forward(False)
        full = check_forward(r, out_f, saved_f, False)
        assert torch.equal(saved_f["bf"][-1][:, :5 * r.geo.D], saved["bf"][-1][:, :5 * r.geo.D]), "xn1 | qkv | a differ with a compact tail"
        # both x_mid lie within one bound of the same float64 value (same operands bit for bit, other tile configuration)
        rows = r.rows
        within(f"stackA.tail x_mid-ref {tag}", info["x_mid"], full["ref_mid"].index_select(0, rows), info["bound_mid"], dt=dt)
        within(f"stackA.tail x_mid {tag}", info["x_mid"], full["x_mid"].index_select(0, rows).double(), 2 * info["bound_mid"], dt=dt)
        # the compact OUTPUT against the same rows of the full run: both against the unrounded float64 forward, in relative L2
        # like section C (a wrong row gather between the two paths is an O(1) error there)
        hw = [{n: (None if t is None else t.cpu()) for n, t in w.items()} for w in r.w]
        fwd = lambda rt: S.stack_forward64(r.c["x"].double(), hw, r.geo, r.B, r.T, r.c["key_keep"], r.c["cu"], round_to=rt)[0]
        exact = fwd(None).index_select(0, r.c["tail_rows"]).cuda()
        lim = 2 * S.rel_l2(fwd(dt).index_select(0, r.c["tail_rows"]).cuda(), exact) + S.acc_term(max(r.geo.Hd, 3 * r.geo.D))
        e_c, e_f = S.rel_l2(out, exact), S.rel_l2(out_f.index_select(0, rows), exact)
        e_cf = S.rel_l2(out, out_f.index_select(0, rows).double())
        print(f"tail out {tag} {dtn(dt)}: compact {e_c:.3g} full {e_f:.3g} compact-full {e_cf:.3g} limit {lim:.3g}")
        assert e_c <= lim and e_f <= lim and e_cf <= 2 * lim
    if tag in ("vis", "gpt"):
        x = cuda(r.c["x"]).clone()
        y = r.stack.forward(x, r.B, key_keep=r.keep, T=r.T)
        torch.cuda.synchronize()
        assert y.data_ptr() == x.data_ptr() and torch.equal(y, saved["out"]), "inference mode differs from the training forward"


# ---------------------------------------------------------------------------------------------------------------------------
# B. prefill
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=dtn)
def test_prefill_kv_cache(dt):
    r = Rig("gpt", dt)
    L, B, T, D = len(r.w), r.B, r.T, r.geo.D
    kc = torch.full((L, B, T + 3, D), SENT, device="cuda", dtype=dt)
    vc = torch.full((L, B, T + 3, D), SENT, device="cuda", dtype=dt)
    out, saved = r.forward(kv_out=(kc, vc))
    for l in range(L):
        qkv = saved["bf"][l][:r.M, D:4 * D]
        assert torch.equal(kc[l, :, :T].reshape(r.M, D), qkv[:, D:2 * D]) and torch.equal(vc[l, :, :T].reshape(r.M, D), qkv[:, 2 * D:3 * D])
    assert bool((kc[:, :, T:] == SENT).all() and (vc[:, :, T:] == SENT).all()), "the cache past T was written"
    _, saved0 = r.forward()
    assert torch.equal(saved0["out"], saved["out"]), "kv_out changed the pass"


@pytest.mark.parametrize("dt", DTS, ids=dtn)
def test_decode_step_after_prefill(dt):
    r = Rig("gpt", dt)
    geo, L, B, T, D = r.geo, len(r.w), r.B, r.T, r.geo.D
    pos = T - 1
    out_T, saved_T = r.forward()
    x3 = cuda(r.c["x"]).view(B, T, D)
    kc = torch.full((L, B, T + 2, D), SENT, device="cuda", dtype=dt)
    vc = torch.full((L, B, T + 2, D), SENT, device="cuda", dtype=dt)
    r.stack.forward(x3[:, :pos].reshape(B * pos, D).clone(), B, T=pos, kv_out=(kc, vc))
    torch.cuda.synchronize()
    assert bool((kc[:, :, pos:] == SENT).all() and (vc[:, :, pos:] == SENT).all())
    kc0, vc0 = kc.clone(), vc.clone()
    x = x3[:, pos].clone()
    y = r.stack.decode_step(x, kc, vc, pos)
    torch.cuda.synchronize()
    assert y.data_ptr() == x.data_ptr() and bool(torch.isfinite(y).all()), "decode_step: x is updated in place"
    assert torch.equal(kc[:, :, :pos], kc0[:, :, :pos]) and torch.equal(vc[:, :, :pos], vc0[:, :, :pos]), "cache rows [0, pos) changed"
    assert bool((kc[:, :, pos + 1:] == SENT).all() and (vc[:, :, pos + 1:] == SENT).all()), "a cache row past pos was written"
    # block 0's new row: per element, LayerNorm bound through |W| + the qkv GEMM's own
    _, _, per = S.row_chain64(x3[:, pos], r.w, geo, [kc[l, :, :T] for l in range(L)], [vc[l, :, :T] for l in range(L)], dt)
    k0, v0, dk0, dv0 = per[0]
    within("stackB.decode k0", kc[0, :, pos], k0, dk0, dt=dt)
    within("stackB.decode v0", vc[0, :, pos], v0, dv0, dt=dt)
    # deeper tensors: relative L2 against the unrounded float64 forward, 2 e_round + acc (e_round: the 16-bit mimic's own error)
    hw = [{n: (None if t is None else t.cpu()) for n, t in w.items()} for w in r.w]
    last = torch.arange(B) * T + pos

    def f64(ws, rt, rows=last):
        o, sv = S.stack_forward64(r.c["x"].double(), ws, geo, B, T, round_to=rt)
        return dict(x=o[rows].cuda(), k1=sv["bf"][1][rows, 2 * D:3 * D].cuda(), v1=sv["bf"][1][rows, 3 * D:4 * D].cuda())
    exact, mimic = f64(hw, None), f64(hw, dt)
    got = dict(x=y, k1=kc[1, :, pos], v1=vc[1, :, pos])
    fwd = dict(x=out_T[last.cuda()], k1=saved_T["bf"][1][last.cuda(), 2 * D:3 * D], v1=saved_T["bf"][1][last.cuda(), 3 * D:4 * D])
    acc = S.acc_term(max(geo.Hd, 3 * D))
    lims = {}
    for n in ("k1", "v1", "x"):
        er = S.rel_l2(mimic[n], exact[n])
        lims[n] = 2 * er + acc
        e_d, e_f, e_df = S.rel_l2(got[n], exact[n]), S.rel_l2(fwd[n], exact[n]), S.rel_l2(got[n], fwd[n].double())
        print(f"decode {dtn(dt)} {n}: decode {e_d:.3g} forward row {e_f:.3g} decode-forward {e_df:.3g} e_round {er:.3g}")
        assert e_d <= lims[n], f"decode_step {n}: {e_d:.3g} > 2 * {er:.3g} + {acc:.3g}"
        assert e_f <= lims[n] and e_df <= 2 * lims[n], (n, e_f, e_df)
        WORST[(f"stackB decode {n}", dtn(dt))] = max(WORST.get((f"stackB decode {n}", dtn(dt)), 0.0), e_d / er)
    # the same limits reject a reference taken one position early, and one with ln_2's affine used for ln_1 in block 1
    early = f64(hw, None, last - 1)
    swapped = [dict(w) for w in hw]
    swapped[1]["ln1_w"], swapped[1]["ln1_b"] = swapped[1]["ln2_w"], swapped[1]["ln2_b"]
    for wrong, what in ((early, "pos - 1"), (f64(swapped, None), "ln_2 for ln_1")):
        for n in ("k1", "x"):
            assert S.rel_l2(got[n], wrong[n]) > lims[n], f"the limit cannot see {what} in {n}"


# ---------------------------------------------------------------------------------------------------------------------------
# C. backward against the float64 replay
# ---------------------------------------------------------------------------------------------------------------------------
BWD = [("vis", False, True), ("vis", False, False), ("txt", False, True), ("txt", True, True), ("pack", False, True), ("pack", True, True),
       ("pack64", False, True), ("gpt", False, False), ("map", False, True)]


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag,tail,wt", BWD)
def test_backward_against_f64_replay(tag, tail, wt, dt):
    r = Rig(tag, dt, wt=wt)
    _, saved = r.forward(tail)
    got = r.backward(saved, tail)
    compare_backward(r, saved, got, tail, f"{tag}{' tail' if tail else ''}{'' if wt else ' no-wt'}")
    assert bool((saved["bf"][:, r.M:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# D. exact invariants
# ---------------------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag", ["txt16", "pack64"])
def test_side_stream_is_bit_identical(tag, dt, monkeypatch):
    """M % 64 == 0: both modes contract the same rows in the same order"""
    r = Rig(tag, dt, wt=True)
    assert r.M % 64 == 0
    _, saved = r.forward()
    runs = []
    for mode in ("1", "1", "0"):
        monkeypatch.setenv("CCLIP_WGRAD_STREAM", mode)
        r.refill()
        runs.append(r.backward(saved))
    same(runs[0], runs[1], "two side-stream runs")
    same(runs[0], runs[2], "side stream against one stream")


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag,tail", [("txt", False), ("txt", True), ("pack", True)])
def test_one_stream_ragged_rows_within_bound(tag, tail, dt, monkeypatch):
    """Ragged M (80 or 41 live slab rows): with the side stream the weight gradients contract over the zero-tailed slabs (Mk = Mp in
    BlockStack._wgrad: `pad` and both operands at least Mk rows tall), on one stream the caller's dxb has M rows only and Mk = M -
    other K-tile counts, so not bit-identical by construction: the one-stream result is held to the bound of section C instead.
    With tail_rows the one-stream pass also allocates its own zero-tailed dxb_in (the caller's dxb is compact) and fills dsm
    from the kept rows after zeroing it."""
    monkeypatch.setenv("CCLIP_WGRAD_STREAM", "0")
    r = Rig(tag, dt, wt=True)
    _, saved = r.forward(tail)
    compare_backward(r, saved, r.backward(saved, tail), tail, f"{tag}{' tail' if tail else ''} one-stream")


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag,tail", [("txt", True), ("vis", False)])
def test_param_grads_false(tag, tail, dt):
    """The dgrad chain alone: dx_in / dxb bit-identical (layernorm_bwd forms dx the same way with and without dgamma: the
    partial sums are separate accumulators of ln_bwd_kernel), no gradient buffer touched."""
    r = Rig(tag, dt, wt=True)
    _, saved = r.forward(tail)
    full = r.backward(saved, tail)
    r.refill()
    got = r.backward(saved, tail, param_grads=False)
    assert torch.equal(got["dx_in"], full["dx_in"]) and torch.equal(got["dxb"], full["dxb"])
    for k, t in got.items():
        if k not in ("dx_in", "dxb"):
            assert bool(t.isnan().all()), f"param_grads=False wrote {k}"


@pytest.mark.parametrize("dt", DTS, ids=dtn)
def test_frozen_block(dt):
    r = Rig("vis", dt, wt=True)
    _, saved = r.forward()
    full = r.backward(saved)
    f = Rig("vis", dt, wt=True, frozen=(0,))
    _, saved_f = f.forward()
    got = f.backward(saved_f)
    assert not any(k[0] == 0 for k in got if isinstance(k, tuple))
    for k, t in got.items():
        assert torch.equal(t, full[k]), f"frozen block 0: {k} differs"
    compare_backward(f, saved_f, got, False, "vis frozen0")


@pytest.mark.parametrize("dt", DTS, ids=dtn)
@pytest.mark.parametrize("tag", ["vis", "gpt"])
def test_acc_flags(tag, dt):
    """Two single backward passes over the same saved activations with different upstream gradients (dx and -0.5 dx rounded
    anew): g1 and g2.  Then the second again with one weight per block, one bias and one LayerNorm pair flagged in `acc`, their
    buffers holding g1, every other buffer NaN: a flagged tensor must hold g1 + g2 in float64 within 2^-22 (|g1| + |g2|) per
    element (so neither 2 g2 nor g2 alone passes), an unflagged one must equal the single run g2 bit for bit."""
    r = Rig(tag, dt, wt=(tag == "vis"))
    _, saved = r.forward()
    g1 = r.backward(saved)
    r.dx_scale = -0.5
    r.refill()
    g2 = r.backward(saved)
    flagged = [(0, "w_fc"), (1, "b_o"), (0, "ln1_w"), (0, "ln1_b"), (1, "w_qkv")]
    acc = {id(r.blocks[l].grads[n]): True for l, n in flagged}
    r.refill()
    for l, n in flagged:
        r.blocks[l].grads[n].copy_(g1[(l, n)])
    g3 = r.backward(saved, acc=acc)
    for k in g1:
        if k in flagged:
            a, b = g1[k].double(), g2[k].double()
            assert not torch.equal(g1[k], g2[k])
            within(f"stackD.acc {tag} {k[1]}", g3[k], a + b, 2.0 ** -22 * (a.abs() + b.abs()) + 1e-300, dt=dt)
        else:
            assert torch.equal(g3[k], g2[k]), f"unflagged {k} changed under acc"
