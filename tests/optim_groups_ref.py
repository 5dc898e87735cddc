"""Float64 reference of the grouped AdamW step (csrc/optim.hip, adamw_groups_kernel; clip.optim.AdamW with parameter groups, norm
clipping and EMA weights) and of the sum of squares it clips by, each with the error bound an fp32 evaluation may reach.

`trajectory` composes kernel_refs_f64.adamw - which takes a gradient, a learning rate and a skip mask per step and carries its
bound - per group slice, and adds:
  * the clip coefficient c_t = gs * min(1, max_norm / (|gs| * sqrt(sum of g_t^2 over the live elements) + 1e-6)), formed in double
    from the gradients (never read back from the kernel under test) and multiplied into the gradient;
  * the EMA recurrence e' = d e + (1 - d) p_new, with the bound  b_e' = d b_e + (1 - d) b_p + the rounding of (1 - d), of the two
    products and of the sum:  E (d |e| + 2 (1 - d) |p_new| + |e'|);
  * the widening for the coefficient's own fp32 error.  The kernel's coefficient differs from c_t by a relative rho =
    COEF_ROUNDINGS * E + sumsq_rel / 2 (sqrtf, the product with |gs|, + 1e-6, the division, the product with gs: 5 roundings; a
    relative error r of the sum of squares is r / 2 of its root).  A relative perturbation rho_t of the gradient of step t,
    of either sign per step, moves
        m by   em' = b1 em + (1 - b1) |g c| rho,        v by   ev' = b2 ev + (1 - b2) (g c)^2 (2 rho + rho^2),
        p by   ep' = ep + step_size * (em' / den + |m| * min(ev' / (2 sqrt v), sqrt ev') / den^2)      (the form of adamw's d_upd),
    with den = sqrt(v) + eps (mode 0) or sqrt(v) / sqrt(bc2) + eps (mode 1) and the decay factors (<= 1) bounded by 1; the EMA
    takes (1 - d) ep' like any error of p.
`sumsq` is the double sum with the bound (chain + butterfly + partials) * E relative: every term is >= 0, so each of the
roundings on the longest path through ANY fixed tree costs at most E of the total.
FAULTS are planted errors the bounds must tell apart (tests/test_optim_groups_cpu.py)."""
import math

import torch

import kernel_refs_f64 as KR

E32 = KR.E32
COEF_ROUNDINGS = 5
FAULTS = ("table_shift", "decay_no_decay", "ema_p_old", "coef_after_moments")


def sumsq(x, out0=0.0, chain=1, butterfly=9, partials=1):
    """(ref, bound): out0 + sum x^2 in double; chain = fma roundings of one thread's chain, butterfly = levels of the block
    reduction (6 in the wave + the 3 adds over the 4 wave sums), partials = adds of the second stage (one per partial, the first onto 0 or out0)"""
    ref = out0 + (x.double() ** 2).sum()
    return ref, (chain + butterfly + partials) * E32 * ref


def sumsq_rel(n, grid_cap=1024, ranges=1):
    """the relative bound of `sumsq` for ops.sumsq over n elements (its launch: min(ceil(n / 1024), grid_cap) blocks of 256
    threads, one float4 per thread and trip), accumulated over `ranges` calls"""
    n4 = (n + 3) // 4
    blocks = min((n4 + 255) // 256, grid_cap)
    trips = (n4 + blocks * 256 - 1) // (blocks * 256)
    return (4 * trips + 9 + blocks) * E32 * ranges


def clip_coef(g_live, grad_scale, max_norm):
    """clip_grad_norm_'s coefficient on the gradients grad_scale * g, times grad_scale; in double"""
    if max_norm is None:
        return grad_scale
    return grad_scale * min(1.0, max_norm / (abs(grad_scale) * math.sqrt(float((g_live.double() ** 2).sum())) + 1e-6))


def trajectory(p0, grads, group_of, lrs, wds, *, steps, grad_scale=1.0, max_norm=None, skip=None, ema_decays=None, ema0=None,
               sumsq_rel=0.0, fault=None, beta1=0.9, beta2=0.999, eps=1e-6, correct_bias=True, mode=0, f32_hyper=True):
    """len(steps) grouped steps.  group_of: int64 [n], the group of every element; lrs: per step, one learning rate per group;
    wds: one weight decay per group; skip: per step None or the mask of the elements without a gradient (kept, and left out of the
    norm); ema_decays: per step the decay d (None: no EMA), ema0 the EMA before the first step (None: p0, as the optimiser starts
    it).  Plain torch on whatever device the operands live on.  Returns (dict p / m / v / ema after the last step, dict of bounds)."""
    assert fault is None or fault in FAULTS
    r = KR.f32 if f32_hyper else float
    T, n = len(steps), p0.numel()
    p0 = p0.double()
    skips = [None] * T if skip is None else list(skip)
    gs = r(grad_scale)
    if fault == "table_shift":
        group_of = torch.roll(group_of, 64)
    if fault == "decay_no_decay":
        wds = [max(wds) if w == 0 else w for w in wds]
    coefs, scaled = [], []
    for g_t, sk in zip(grads, skips):
        c = clip_coef(g_t if sk is None else g_t[~sk], gs, None if max_norm is None else r(max_norm))
        coefs.append(c)
        scaled.append(g_t.double() * (gs if fault == "coef_after_moments" else c))
    dev = p0.device
    z = torch.zeros(n, dtype=torch.float64, device=dev)
    kw = dict(beta1=beta1, beta2=beta2, eps=eps, correct_bias=correct_bias, mode=mode, f32_hyper=f32_hyper, grad_scale=1.0)
    states = []                                   # after every step: (values, bounds), so that the EMA can follow p
    for t in range(1, T + 1):
        val = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in "pmv"}
        bnd = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in "pmv"}
        for k in range(len(wds)):
            idx = (group_of == k).nonzero().flatten()
            if idx.numel() == 0:
                continue
            ref, b = KR.adamw(p0[idx], [g[idx] for g in scaled[:t]], z[idx], z[idx], lr=[lr[k] for lr in lrs[:t]], weight_decay=wds[k],
                              steps=tuple(steps[:t]), skip=[None if s is None else s[idx] for s in skips[:t]], **kw)
            for nm in "pmv":
                val[nm][idx], bnd[nm][idx] = ref[nm], b[nm]
        states.append((val, bnd))
    # the coefficient's own error, as a relative perturbation of the gradient
    b1, b2, ep_ = r(beta1), r(beta2), r(eps)
    em, ev, ex = z.clone(), z.clone(), z.clone()
    if max_norm is not None:
        rho = COEF_ROUNDINGS * E32 + sumsq_rel / 2
        for t in range(T):
            val = states[t][0]
            gr = scaled[t].abs()
            em_n = b1 * em + (1 - b1) * gr * rho
            ev_n = b2 * ev + (1 - b2) * gr * gr * (2 * rho + rho * rho)
            bc1 = 1.0 - b1 ** steps[t] if correct_bias else 1.0
            bc2 = 1.0 - b2 ** steps[t] if correct_bias else 1.0
            sq = val["v"].sqrt()
            lr_e = torch.tensor([float(x) for x in lrs[t]], dtype=torch.float64, device=dev)[group_of]
            if mode == 0:
                ss, den = lr_e * math.sqrt(bc2) / bc1, sq + ep_
                d_sq = torch.minimum(ev_n / (2 * sq).clamp_min(1e-300), ev_n.sqrt())
            else:
                ss, den = lr_e / bc1, sq / math.sqrt(bc2) + ep_
                d_sq = torch.minimum(ev_n / (2 * sq).clamp_min(1e-300), ev_n.sqrt()) / math.sqrt(bc2)
            ex_n = ex + ss * (em_n / den + val["m"].abs() * d_sq / (den * den))
            if skips[t] is not None:
                em_n, ev_n, ex_n = (torch.where(skips[t], o, nw) for o, nw in ((em, em_n), (ev, ev_n), (ex, ex_n)))
            em, ev, ex = em_n, ev_n, ex_n
            for nm, w in (("p", ex), ("m", em), ("v", ev)):
                states[t][1][nm] = states[t][1][nm] + w
    val, bnd = states[-1]
    if ema_decays is not None:
        e = p0.clone() if ema0 is None else ema0.double().clone()
        be = z.clone()
        prev = p0
        for t in range(T):
            d = r(ema_decays[t])
            src = prev if fault == "ema_p_old" else states[t][0]["p"]
            e_n = d * e + (1 - d) * src
            be_n = d * be + (1 - d) * states[t][1]["p"] + E32 * (d * e.abs() + 2 * (1 - d) * src.abs() + e_n.abs()) + KR.FLT_MIN
            if skips[t] is not None:
                e_n, be_n = torch.where(skips[t], e, e_n), torch.where(skips[t], be, be_n)
            e, be, prev = e_n, be_n, states[t][0]["p"]
        val, bnd = dict(val, ema=e), dict(bnd, ema=be)
    return val, bnd
