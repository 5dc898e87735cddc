"""Float64 reference of cclip_hip/stack.py: the forward of a pre-LN block stack and the hand-written backward of the whole stack,
in plain torch on whatever device the operands live on (no GPU needed to import it).

  block_forward64 / stack_forward64: LN1, qkv, attention, out-proj + residual, LN2, fc + activation, c_proj + residual, exactly
    as the docstring of stack.py lays a block out; returns every intermediate the stack saves, in the stack's own `saved`
    layout (bf = xn1|qkv|a|xn2|h|g, xs = x_in, x_mid, st = mean1 rstd1 mean2 rstd2, lse, out, tail).  Built from differentiable
    torch operators only, so torch.autograd through it is the independent check of the backward below
    (tests/test_stack_ref_cpu.py).  round_to = a 16-bit dtype rounds the six slab tensors where the stack stores them: the CPU
    mimic of a 16-bit forward.
  stack_backward64: the backward of the whole stack written out by hand, from the activations HANDED to it - a `saved` dict of
    stack_forward64 or BlockStack's own (tests/test_stack_f64_gpu.py), so that forward rounding is not part of a backward
    comparison.  Softmax probabilities are rebuilt from the saved q / k (the kernels rebuild them from q, k and the saved lse:
    the same numbers up to fp32 evaluation); delta = rowsum(dO * o) uses the saved attention output, as the kernels do.
    round_to = None is the exact result; a 16-bit dtype rounds exactly where BlockStack.backward stores a 16-bit tensor (dh, dsm
    in its three uses, dqkv, dxb_mid, dxb_in, and dh_c / ds_c / dxb_mid_c of a compact tail) and P / dS inside the attention
    (header of tests/test_kernels_f16_gpu.py).  The fp32 dx chain is never rounded.
    fault = one of FAULTS plants a deliberate error in the REFERENCE (never in the device code): the sensitivity checks show
    that the tolerance of the GPU comparison tells each of them from rounding.

Weights are dicts with BlockWeights' field names (tensors of any float dtype; b_qkv may be None); matrices are [out, in] for the
nn.Linear layout and [in, out] for GPT-2's Conv1D layout."""
import math
from collections import namedtuple

import torch

import kernel_refs_f64 as KR
from attn_refs_f64 import _attn64, _split_heads  # noqa: F401
from gemm_refs_f64 import C_ACC, FLOOR, U, _acc_bound, _act64, epilogue_bounds, epilogue_ref, skinny_bounds

Geo = namedtuple("Geo", "D H dh Hd linear act causal")
MATS = ("w_qkv", "w_o", "w_fc", "w_proj")
NAMES = ("ln1_w", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_w", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj")
# name -> (tensor it touches: (layer, grad name) or "dx_in", what it does)
FAULTS = {
    "wgrad_drop_row": "token row M-1 left out of layer 0's w_fc gradient contraction",
    "wgrad_drop_row_qkv": "token row M-1 left out of layer 0's w_qkv gradient contraction",
    "bgrad_drop_row": "row M-1 left out of layer 0's b_o gradient",
    "ignore_key_keep": "attention backward without the key padding mask",
    "pack_as_one": "attention backward treating a packed batch as one long sequence",
    "dgrad_wrong_weight": "w_fc read where w_proj belongs in layer 0's c_proj dgrad",
    "ln_no_res": "layer 0's LN2 backward without its dx_res residual add",
    "double": "layer 0's w_o gradient doubled, as if acc were set",
}


def fault_target(fault):
    """(layer, gradient name) or 'dx_in': the tensor the planted error must show in"""
    return {"wgrad_drop_row": (0, "w_fc"), "wgrad_drop_row_qkv": (0, "w_qkv"), "bgrad_drop_row": (0, "b_o"),
            "ignore_key_keep": (0, "w_qkv"), "pack_as_one": (0, "w_qkv"), "dgrad_wrong_weight": (0, "w_fc"), "ln_no_res": "dx_in",
            "double": (0, "w_o")}[fault]


def faults_of(tag, tail=False):
    """The planted errors a variant can show.  ignore_key_keep is left out of the compact-tail run only: the padding sits at the
    END of a causal sequence, so the mask only changes what the padded QUERY rows see, and with a compact tail those rows carry
    no gradient at all - the fault is then a mathematical no-op (it moves no tensor by a single bit), not a small effect."""
    common = ["wgrad_drop_row", "wgrad_drop_row_qkv", "bgrad_drop_row", "dgrad_wrong_weight", "ln_no_res", "double"]
    return common + (["ignore_key_keep"] if tag.startswith("txt") and not tail else []) + (["pack_as_one"] if tag.startswith("pack") else [])


def _R(t, dt):
    return t if dt is None else t.to(dt).double()


def _wm(w, geo):
    """a matrix as [out, in] in fp64"""
    return w.double() if geo.linear else w.double().t()


def _ln64(x, gamma, beta, eps=1e-5):
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / ((xc * xc).mean(1, keepdim=True) + eps).sqrt()
    return xc * rstd * gamma.double() + beta.double(), mean[:, 0], rstd[:, 0]


def seq_groups(B, T, key_keep, cu, M):
    """[(row slice, sequences, length, keep [sequences, length] or None)]: one group for a dense batch, one per sequence for a
    packed one"""
    if cu is None:
        return [(slice(0, B * T), B, T, key_keep)]
    c = [int(v) for v in cu.tolist()]
    return [(slice(c[b], c[b + 1]), 1, c[b + 1] - c[b], None) for b in range(B)]


def attention64(q, k, v, geo, B, T, key_keep=None, cu=None):
    """[M, D] q / k / v (fp64) -> a [M, D], lse [B, H, T] (a packed sequence fills [b, :, :len], the rest is 0)"""
    M = q.shape[0]
    scale = geo.dh ** -0.5
    outs, lse = [], torch.zeros(B, geo.H, T, dtype=torch.float64, device=q.device)
    for b, (sl, nb, t, keep) in enumerate(seq_groups(B, T, key_keep, cu, M)):
        sp = lambda x: _split_heads(x[sl], nb, t, geo.H, geo.dh)
        s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
        if geo.causal:
            s = s + torch.full((t, t), float("-inf"), device=q.device, dtype=torch.float64).triu_(1)
        if keep is not None:
            s = s.masked_fill(keep[:, None, None, :] == 0, float("-inf"))
        l_ = torch.logsumexp(s, -1)
        o = torch.exp(s - l_[..., None]) @ sp(v)
        outs.append(o.permute(0, 2, 1, 3).reshape(nb * t, geo.D))
        if cu is None:
            lse = l_
        else:
            lse[b, :, :t] = l_[0].detach()
    return torch.cat(outs, 0), lse


def attention_bwd64(q, k, v, o, dO, geo, B, T, key_keep=None, cu=None, round_to=None):
    """dq, dk, dv [M, D]; P and dS rounded to `round_to` before the three products, delta from the o handed in"""
    M = q.shape[0]
    scale = geo.dh ** -0.5
    dq, dk, dv = [], [], []
    for sl, nb, t, keep in seq_groups(B, T, key_keep, cu, M):
        sp = lambda x: _split_heads(x[sl], nb, t, geo.H, geo.dh)
        qh, kh, vh, oh, dOh = sp(q), sp(k), sp(v), sp(o), sp(dO)
        s = (qh @ kh.transpose(-1, -2)) * scale
        if geo.causal:
            s = s + torch.full((t, t), float("-inf"), device=q.device, dtype=torch.float64).triu_(1)
        if keep is not None:
            s = s.masked_fill(keep[:, None, None, :] == 0, float("-inf"))
        P = torch.softmax(s, -1)
        dS = P * (dOh @ vh.transpose(-1, -2) - (dOh * oh).sum(-1, keepdim=True))
        P, dS = _R(P, round_to), _R(dS, round_to)
        un = lambda x: x.permute(0, 2, 1, 3).reshape(nb * t, geo.D)
        dq.append(un(scale * dS @ kh)); dk.append(un(scale * dS.transpose(-1, -2) @ qh)); dv.append(un(P.transpose(-1, -2) @ dOh))
    return torch.cat(dq, 0), torch.cat(dk, 0), torch.cat(dv, 0)


def block_forward64(x, w, geo, B, T, key_keep=None, cu=None, round_to=None, rows=None):
    """One block on the fp64 stream x [M, D].  rows (int64 [R]): everything behind the attention runs on those rows only (the
    compact tail of the last block).  Returns a dict of every intermediate the stack saves."""
    D = geo.D
    xn1, m1, r1 = _ln64(x, w["ln1_w"], w["ln1_b"])
    xn1 = _R(xn1, round_to)
    qkv = xn1 @ _wm(w["w_qkv"], geo).t()
    if w.get("b_qkv") is not None:
        qkv = qkv + w["b_qkv"].double()
    qkv = _R(qkv, round_to)
    a, lse = attention64(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], geo, B, T, key_keep, cu)
    a = _R(a, round_to)
    a_t, x_t = (a, x) if rows is None else (a.index_select(0, rows), x.index_select(0, rows))
    x_mid = x_t + a_t @ _wm(w["w_o"], geo).t() + w["b_o"].double()
    xn2, m2, r2 = _ln64(x_mid, w["ln2_w"], w["ln2_b"])
    xn2 = _R(xn2, round_to)
    h = xn2 @ _wm(w["w_fc"], geo).t() + w["b_fc"].double()
    g = _R(_act64(h, geo.act, None)[0], round_to)
    h = _R(h, round_to)
    x_out = x_mid + g @ _wm(w["w_proj"], geo).t() + w["b_proj"].double()
    return dict(xn1=xn1, qkv=qkv, a=a, lse=lse, x_mid=x_mid, xn2=xn2, h=h, g=g, x_out=x_out, mean1=m1, rstd1=r1, mean2=m2, rstd2=r2,
                a_tail=a_t)


def stack_forward64(x, weights, geo, B, T, key_keep=None, cu=None, tail_rows=None, round_to=None):
    """The whole stack; returns (output [M, D] or the compact [R, D], saved) with `saved` in BlockStack's layout (fp64, Mp = M)."""
    L, M, D, Hd = len(weights), x.shape[0], geo.D, geo.Hd
    bf, xs, st, lse = [], [], [], []
    tail = None
    for l, w in enumerate(weights):
        rows = tail_rows if (tail_rows is not None and l == L - 1) else None
        r = block_forward64(x, w, geo, B, T, key_keep, cu, round_to, rows)
        lse.append(r["lse"])
        if rows is None:
            bf.append(torch.cat([r["xn1"], r["qkv"], r["a"], r["xn2"], r["h"], r["g"]], 1))
            xs.append(torch.stack([x, r["x_mid"]]))
            st.append(torch.stack([r["mean1"], r["rstd1"], r["mean2"], r["rstd2"]]))
        else:
            z = lambda c: torch.zeros(M, c, dtype=torch.float64, device=x.device)
            bf.append(torch.cat([r["xn1"], r["qkv"], r["a"], z(D), z(Hd), z(Hd)], 1))
            xs.append(torch.stack([x, z(D)]))
            st.append(torch.stack([r["mean1"], r["rstd1"], z(1)[:, 0], z(1)[:, 0]]))
            tail = dict(rows=rows, a=r["a_tail"], xmid=r["x_mid"], xn2=r["xn2"], h=r["h"], g=r["g"], st=torch.stack([r["mean2"], r["rstd2"]]))
        x = r["x_out"]
    saved = dict(T=T, M=M, Mp=M, B=B, cu=cu, key_keep=key_keep, bf=torch.stack(bf), xs=torch.stack(xs), st=torch.stack(st),
                 lse=torch.stack(lse), out=x, tail=tail)
    return x, saved


def _ln_bwd64(dy, x, gamma, mean, rstd, dx_res):
    """LayerNorm backward from the SAVED statistics; returns dx (+ dx_res), dgamma, dbeta"""
    xh = (x - mean[:, None]) * rstd[:, None]
    d = dy * gamma.double()
    dx = rstd[:, None] * (d - d.mean(1, keepdim=True) - xh * (d * xh).mean(1, keepdim=True))
    if dx_res is not None:
        dx = dx + dx_res
    return dx, (dy * xh).sum(0), dy.sum(0)


def stack_backward64(saved, weights, dx, geo, dxb=None, round_to=None, fault=None, frozen=()):
    """Backward of the whole stack.  dx (any float dtype, [M, D], or [R, D] when the forward kept a compact tail): gradient at the
    stack's output; dxb: its 16-bit copy as the device received it (default: dx rounded to round_to).  frozen: layers whose
    parameter gradients are not formed.  Returns dict(grads = [per layer dict, BlockWeights.grads' names], dx_in = fp64 [M, D],
    dxb = the 16-bit copy of dx_in, mid = [per layer dict of the 16-bit intermediates]), everything fp64."""
    assert fault is None or fault in FAULTS, fault
    D, Hd = geo.D, geo.Hd
    L, M, B, T = len(weights), saved["M"], saved["B"], saved["T"]
    key_keep, cu = saved.get("key_keep"), saved.get("cu")
    dact = {1: 16, 3: 18, 4: 19}[geo.act]
    rt = round_to
    dx = dx.double()
    dxb = _R(dx, rt) if dxb is None else dxb.double()
    grads, mids = [None] * L, [None] * L

    def wgrad(dy, xin, name, l):
        """(weight gradient in the weight's own layout, bias gradient)"""
        dyw, xw, dyb = dy, xin, dy
        if l == 0 and ((fault == "wgrad_drop_row" and name == "w_fc") or (fault == "wgrad_drop_row_qkv" and name == "w_qkv")):
            dyw, xw = dy[:-1], xin[:-1]
        if l == 0 and fault == "bgrad_drop_row" and name == "w_o":
            dyb = dy[:-1]
        gw = dyw.t() @ xw if geo.linear else xw.t() @ dyw
        if l == 0 and fault == "double" and name == "w_o":
            gw = 2 * gw
        return gw, dyb.sum(0)

    for l in range(L - 1, -1, -1):
        w = weights[l]
        row = saved["bf"][l][:M].double()
        xn1, qkv, a = row[:, 0:D], row[:, D:4 * D], row[:, 4 * D:5 * D]
        xn2, h, g = row[:, 5 * D:6 * D], row[:, 6 * D:6 * D + Hd], row[:, 6 * D + Hd:6 * D + 2 * Hd]
        x_in, x_mid = saved["xs"][l, 0].double(), saved["xs"][l, 1].double()
        m1, r1, m2, r2 = (saved["st"][l, i].double() for i in range(4))
        gr, mid = {}, {}
        tail = saved.get("tail") if l == L - 1 else None
        if tail is not None:
            rows = tail["rows"]
            a_t, x_mid, xn2, h, g = (tail[n].double() for n in ("a", "xmid", "xn2", "h", "g"))
            m2, r2 = tail["st"][0].double(), tail["st"][1].double()
        else:
            a_t = a
        # ---- MLP branch ----
        gr["w_proj"], gr["b_proj"] = wgrad(dxb, g, "w_proj", l)
        wp = _wm(w["w_fc"], geo).t() if (fault == "dgrad_wrong_weight" and l == 0) else _wm(w["w_proj"], geo)
        dh = _R(_act64(dxb @ wp, dact, h)[0], rt)
        gr["w_fc"], gr["b_fc"] = wgrad(dh, xn2, "w_fc", l)
        dsm = _R(dh @ _wm(w["w_fc"], geo), rt)
        res = None if (fault == "ln_no_res" and l == 0) else dx
        dx, gr["ln2_w"], gr["ln2_b"] = _ln_bwd64(dsm, x_mid, w["ln2_w"], m2, r2, res)
        dxb_mid = _R(dx, rt)
        mid.update(dh=dh, dsm_fc=dsm, dxb_mid=dxb_mid)
        # ---- attention branch ----
        gr["w_o"], gr["b_o"] = wgrad(dxb_mid, a_t, "w_o", l)
        da = _R(dxb_mid @ _wm(w["w_o"], geo), rt)
        if tail is not None:                  # the compact gradient re-enters the full-width stream
            da = torch.zeros(M, D, dtype=torch.float64, device=dx.device).index_copy_(0, rows, da)
            dx = torch.zeros(M, D, dtype=torch.float64, device=dx.device).index_copy_(0, rows, dx)
        kk, cc, TT, BB = key_keep, cu, T, B
        if fault == "ignore_key_keep":
            kk = None
        if fault == "pack_as_one" and cu is not None:
            cc = torch.tensor([0, M], dtype=torch.int32)
            BB = 1
        dq, dk, dv = attention_bwd64(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], a, da, geo, BB, TT, kk, cc, rt)
        dqkv = _R(torch.cat([dq, dk, dv], 1), rt)
        gr["w_qkv"], gb = wgrad(dqkv, xn1, "w_qkv", l)
        if w.get("b_qkv") is not None:
            gr["b_qkv"] = gb
        dsm = _R(dqkv @ _wm(w["w_qkv"], geo), rt)
        dx, gr["ln1_w"], gr["ln1_b"] = _ln_bwd64(dsm, x_in, w["ln1_w"], m1, r1, dx)
        dxb = _R(dx, rt)
        mid.update(da=da, dqkv=dqkv, dsm_qkv=dsm, dxb_in=dxb)
        grads[l] = None if l in frozen else gr
        mids[l] = mid
    return dict(grads=grads, dx_in=dx, dxb=dxb, mid=mids)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison of section C: e(t) <= 2 e_round(t) + acc(t)
# ---------------------------------------------------------------------------------------------------------------------------
def rel_l2(got, ref):
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def acc_term(K):
    """fp32 accumulation over a contraction of length K, relative"""
    return C_ACC * 2.0 ** -24 * math.sqrt(K)


def flat(res):
    """{(layer, name) | 'dx_in': tensor} of a stack_backward64 result"""
    out = {"dx_in": res["dx_in"]}
    for l, gr in enumerate(res["grads"]):
        if gr is not None:
            for n, t in gr.items():
                out[(l, n)] = t
    return out


def contraction(key, geo, M):
    """the contraction length behind a gradient tensor: the token count for parameter gradients, the longest dgrad K for dx"""
    return max(3 * geo.D, geo.Hd) if key == "dx_in" else M


def accepts(got, exact, rounded, K):
    """(inside?, e_gpu, e_round): the acceptance region of the GPU comparison around `exact`"""
    e, er = rel_l2(got, exact), rel_l2(rounded, exact)
    return e <= 2 * er + acc_term(K), e, er


# ---------------------------------------------------------------------------------------------------------------------------
# the cases both test modules run (host tensors; the GPU module moves them)
# ---------------------------------------------------------------------------------------------------------------------------
W = 128
GEOS = {
    #        geo                                                   batch
    "vis": (Geo(W, 2, 64, 512, True, 1, False), dict(B=3, T=50)),
    "txt": (Geo(W, 2, 64, 512, True, 1, True), dict(B=4, T=20, pad={0: 15, 2: 9})),
    "txt16": (Geo(W, 2, 64, 512, True, 1, True), dict(B=4, T=16, pad={0: 11, 2: 5})),
    "pack": (Geo(W, 2, 64, 512, True, 1, True), dict(lens=[1, 20, 7, 13])),
    "pack64": (Geo(W, 2, 64, 512, True, 1, True), dict(lens=[20, 16, 1, 27])),
    "gpt": (Geo(W, 2, 64, 512, False, 3, True), dict(B=2, T=24)),
    "map": (Geo(W, 4, 32, 256, True, 4, False), dict(B=3, T=17, no_bqkv=True)),
}


def make_case(tag, dt, L=2, seed=0):
    """weights (16-bit matrices, fp32 vectors), the stream entering block 0, the mask / packing and the kept rows of `tag`"""
    geo, bt = GEOS[tag]
    g = torch.Generator().manual_seed(1000 * seed + sum(ord(c) for c in tag))
    D, Hd = geo.D, geo.Hd
    rn = lambda *s: torch.randn(*s, generator=g)
    weights = []
    for _ in range(L):
        w = {}
        for name, (o, i) in (("w_qkv", (3 * D, D)), ("w_o", (D, D)), ("w_fc", (Hd, D)), ("w_proj", (D, Hd))):
            m = rn(o, i) * (1.5 / math.sqrt(i))
            w[name] = (m if geo.linear else m.t()).contiguous().to(dt)
        for name, n in (("b_qkv", 3 * D), ("b_o", D), ("b_fc", Hd), ("b_proj", D), ("ln1_b", D), ("ln2_b", D)):
            w[name] = 0.1 * rn(n)
        w["ln1_w"], w["ln2_w"] = 1 + 0.1 * rn(D), 1 + 0.1 * rn(D)
        if bt.get("no_bqkv"):
            w["b_qkv"] = None
        weights.append(w)
    key_keep = cu = None
    if "lens" in bt:
        lens = bt["lens"]
        B, T, M = len(lens), max(lens), sum(lens)
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
        tail_rows = cu[1:].long() - 1
    else:
        B, T = bt["B"], bt["T"]
        M = B * T
        last = torch.full((B,), T - 1, dtype=torch.int64)
        if "pad" in bt:
            key_keep = torch.ones(B, T)
            for b, n in bt["pad"].items():
                key_keep[b, n:] = 0
                last[b] = n - 1
        tail_rows = torch.arange(B) * T + last
    x = rn(M, D)
    return dict(tag=tag, geo=geo, B=B, T=T, M=M, weights=weights, key_keep=key_keep, cu=cu, tail_rows=tail_rows, x=x,
                dx=rn(M, D), dx_tail=rn(B, D))


# ---------------------------------------------------------------------------------------------------------------------------
# propagated bounds: how far one row's result may sit from its float64 chain after several launches
# ---------------------------------------------------------------------------------------------------------------------------
def act_lipschitz(act):
    """sup |act'| - the largest slope on a dense float64 grid (beyond +-12 every slope is within 1e-8 of 0 or 1)"""
    return _act64(torch.linspace(-12.0, 12.0, 240001, dtype=torch.float64), act, None)[1].max().item()


def ln_propagate(x, dx, gamma, eps=1e-5):
    """|LN(x') - LN(x)| per element for any x' with |x' - x| <= dx, without linearising: the centred value moves by at most
    dc = dx + mean(dx), the variance by at most mean(2 |xc| dc + dc^2), rstd stays between the values at var -+ that, and
    y = gamma xc rstd + beta gives |dy| <= |gamma| (dc rstd_hi + |xc| max(rstd_hi - rstd, rstd - rstd_lo))."""
    x, g = x.double(), gamma.double().abs()
    xc = x - x.mean(1, keepdim=True)
    var = (xc * xc).mean(1, keepdim=True)
    dc = dx + dx.mean(1, keepdim=True)
    dvar = (2 * xc.abs() * dc + dc * dc).mean(1, keepdim=True)
    r, r_hi, r_lo = (var + eps).rsqrt(), ((var - dvar).clamp_min(0.0) + eps).rsqrt(), (var + dvar + eps).rsqrt()
    return g * (dc * r_hi + xc.abs() * torch.maximum(r_hi - r, r - r_lo))


def _gemm_step(a, da, W, bias, act, res, dres, geo, dt, lip=1.0):
    """one projection on (value, bound) pairs: the float64 result of the reference operands and how far a device result fed
    operands within `da` (and a residual within `dres`) may sit from it: da |W|^T through the activation's largest slope, plus
    the launch's own bound (the tile kernels' or the skinny kernel's, whichever is larger; the stack may pick either).
    Returns (fp32-output pair, 16-bit-output pair)."""
    Bm = _wm(W, geo)
    e = epilogue_ref(a, Bm, 1.0, bias, act, res)
    bf, b16, _ = epilogue_bounds(_acc_bound(a, Bm), e, dt)
    sf, s16, _ = skinny_bounds(a, Bm, 1.0, e, act, dt)
    prop = lip * (da @ Bm.abs().t()) + (0.0 if dres is None else dres)
    return (e["ref"], prop + torch.maximum(bf, sf)), (e["ref"], prop + torch.maximum(b16, s16))


def row_chain64(x, weights, geo, K, V, dt):
    """One token per sequence through the whole stack (BlockStack.decode_step, or the last row of a causal forward): x [nb, D]
    is the stream entering block 0, K[l] / V[l] [nb, S, D] the 16-bit keys / values the attention of layer l READ, the token's own
    row (S - 1) included - operands observed on the device, so only the query carries a propagated bound.
    Returns (x_ref, d_x, [per layer (k_ref, v_ref, d_k, d_v)]): float64 values of the chain with nothing rounded, and per-element
    bounds on a device result built launch by launch from the kernels' own bounds (kernel_refs_f64.ln_fwd, epilogue_bounds /
    skinny_bounds, the 4u P|V| attention bound) - each launch's input bound is carried through |W|, through LayerNorm by
    ln_propagate, through the activation by its largest slope, and through the softmax by P' in P [e^-2m, e^2m] for scores moved
    by at most m."""
    D, H, dh = geo.D, geo.H, geo.dh
    u, fl, lip = U(dt), FLOOR(dt), act_lipschitz(geo.act)
    scale = dh ** -0.5
    x = x.double()
    dx = torch.zeros_like(x)
    per_layer = []
    for l, w in enumerate(weights):
        def ln(x, dx, gam, bet):
            ref, bnd = KR.ln_fwd(x, gam, bet)
            return ref["y"], ln_propagate(x, dx, gam) + bnd["y"] + u * ref["y"].abs() + fl
        xn, dxn = ln(x, dx, w["ln1_w"], w["ln1_b"])
        _, (qkv, dqkv) = _gemm_step(xn, dxn, w["w_qkv"], w.get("b_qkv"), 0, None, None, geo, dt)
        per_layer.append((qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], dqkv[:, D:2 * D], dqkv[:, 2 * D:3 * D]))
        nb, S = K[l].shape[0], K[l].shape[1]
        q, dq = qkv[:, 0:D].view(nb, H, 1, dh), dqkv[:, 0:D].view(nb, H, 1, dh)
        kh = K[l].double().view(nb, S, H, dh).permute(0, 2, 1, 3)
        vh = V[l].double().view(nb, S, H, dh).permute(0, 2, 1, 3)
        P = torch.softmax((q @ kh.transpose(-1, -2)) * scale, -1)
        m = (scale * (dq @ kh.abs().transpose(-1, -2))).amax(-1, keepdim=True)
        Pv = P @ vh.abs()
        a = (P @ vh).reshape(nb, D)
        da = (torch.expm1(2 * m) * Pv + 4 * u * Pv + fl * vh.abs().sum(-2, keepdim=True) + fl).reshape(nb, D)
        (x, dx), _ = _gemm_step(a, da, w["w_o"], w["b_o"], 0, x, dx, geo, dt)
        xn, dxn = ln(x, dx, w["ln2_w"], w["ln2_b"])
        _, (g, dg) = _gemm_step(xn, dxn, w["w_fc"], w["b_fc"], geo.act, None, None, geo, dt, lip)
        (x, dx), _ = _gemm_step(g, dg, w["w_proj"], w["b_proj"], 0, x, dx, geo, dt)
    return x, dx, per_layer
