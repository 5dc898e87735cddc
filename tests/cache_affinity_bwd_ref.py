"""TEST-ONLY helper of test_cache_affinity_bwd_cpu.py, test_cache_affinity_bwd_gpu.py and test_fewshot_fit_gpu.py: a float64
closed form of the gradient of the class affinities with respect to the stored rows, its derived tolerance, and a torch
restatement of ops.cache_affinity_backward for host-logic tests.

Reference.  With w_ref[q, n] = dA[q, labels[n]] * exp(beta * (<q, g_n> - 1)) for n != exclude[q] and 0 otherwise,
    dG_ref[n, :] = beta * sum_q w_ref[q, n] * q[q, :]
in float64 on the SAME 16-bit operands, one stored row of the ORIGINAL order after the other: it shares no layout code with the
product (test_cache_affinity_bwd_cpu.py holds it against float64 autograd through cache_affinity_ref.reference).

Tolerance, per element, derived and not fitted.  With T[n, d] = |beta| * sum_q |w_ref[q, n]| |q[q, d]|:
    tol[n, d] = T[n, d] * ( |beta| * D * 2^-22 * max|q| * max|g|                        # (1)
                            + (8 * |beta| * (1 + max|s|) + 8) * 2^-24                   # (2)
                            + 4 * 2^-24                                                 # (3)
                            + u16^2                                                     # (4)
                            + 2 * Q * 2^-22 )                                           # (5)
                + [fp16 only]  |beta| * 2^e * 2^-25 * sum_q |q[q, d]|                   # (6)
(1), (2) the error of the recomputed weight exp(beta (s - 1)), relative: the score and exponent terms of
    cache_affinity_ref.tolerance (score: D - 1 fp32 additions with the factor 4 for the MFMA's internal order, times beta;
    exponent: five roundings and v_exp_f32's 1 ulp).  Every term of the sum carries it, so it multiplies T.
(3) dA * 2^-e is exact (a power of two); its product with the exponential rounds once, the accumulator times beta * 2^e rounds
    once and beta * 2^e is exact: two roundings, with room.
(4) the weight enters the second MFMA product as hi + lo, hi = round16(w), lo = round16(w - hi) with w - hi exact in fp32:
    what is lost is lo's rounding, at most u16 |w - hi| <= u16^2 |w| with u16 = 2^-8 for bf16 and 2^-11 for fp16 (unit
    roundoffs): 2^-16 and 2^-22.  Products of two 16-bit numbers are exact in fp32.
(5) the second product adds the 2 Q terms (hi and lo of every query; masked ones are exact zeros) of an element in fp32:
    at most 2 Q additions of 2^-24 relative to the running sum of absolute values, the same factor 4 for the MFMA's order.
(6) fp16 only: in the scaled units w 2^-e (e = the exponent frexp gives max|dA|, so |dA| 2^-e < 1) hi and lo may be
    subnormal; hi + lo is then off by at most half the smallest subnormal, 2^-25, per term whatever its size.  Scaled back
    by 2^e and beta and multiplied by |q[q, d]|.  bf16 shares fp32's exponent range: its term (2^-134) is dropped, and so is
    the underflow of dA * 2^-e itself (below 2^-149 in scaled units).
An element with T = 0 (a class with dA[:, c] = 0, a lone excluded row; padding rows have no reference row at all) has tol 0:
the kernel must give exactly 0.

Largest err / tol measured on the MI355X (every case prints its own `[cache-bwd] ... err/tol`): 0.32 (fp16, un-normalised rows of
small norm, D = 64); 7.0e-2 for bf16 on the same case; normalised rows stay below 0.25 (fp16, beta = 40) and 6e-2 (bf16).
"""
import math

import torch

import cache_affinity_ref as R

DTYPES = R.DTYPES


def weights(q16, g16, labels, beta, dA, exclude=None):
    """float64 w_ref [Q, N] and the scores s [Q, N]; exclude: ORIGINAL rows [Q] (or -1), or None"""
    q, g = q16.double().cpu(), g16.double().cpu()
    s = q @ g.t()
    w = dA.double().cpu()[:, labels] * torch.exp(beta * (s - 1.0))
    if exclude is not None:
        ex = torch.as_tensor(exclude).long()
        for i in range(q.shape[0]):
            if ex[i] >= 0:
                w[i, ex[i]] = 0.0
    return w, s


def reference(q16, g16, labels, beta, dA, exclude=None):
    """float64 (dG_ref [N, D], T [N, D], s [Q, N]) in the ORIGINAL row order, one stored row after the other"""
    w, s = weights(q16, g16, labels, beta, dA, exclude)
    q = q16.double().cpu()
    N, D = g16.shape
    dG, T = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64)
    for n in range(N):
        dG[n] = beta * (w[:, n, None] * q).sum(dim=0)
        T[n] = abs(beta) * (w[:, n, None].abs() * q.abs()).sum(dim=0)
    return dG, T, s


def scale_exponent(dA):
    """e with max|dA| = m * 2^e, 0.5 <= m < 1 (0 for a zero or non-finite maximum): the kernel's power-of-two scale"""
    m = dA.abs().max().item() if dA.numel() else 0.0
    return math.frexp(m)[1] if 0.0 < m < float("inf") else 0


def tolerance(T, beta, q16, g16, s, dA, exclude=None):
    Q, D = q16.shape
    qn = q16.double().norm(dim=1).max().item()
    gn = g16.double().norm(dim=1).max().item() if g16.shape[0] else 0.0
    smax = s.abs().max().item() if s.numel() else 0.0
    b = abs(beta)
    u16 = 2.0 ** -8 if q16.dtype == torch.bfloat16 else 2.0 ** -11
    rel = b * D * 2.0 ** -22 * qn * gn + (8.0 * b * (1.0 + smax) + 8.0) * 2.0 ** -24 + 4.0 * 2.0 ** -24 + u16 * u16 \
        + 2.0 * Q * 2.0 ** -22
    tol = T * rel
    if q16.dtype == torch.float16:
        absq = q16.double().cpu().abs().sum(dim=0)                              # [D]: an upper bound of the row's live queries
        tol = tol + torch.where(T > 0, b * 2.0 ** (scale_exponent(dA) - 25) * absq[None, :].expand_as(T), torch.zeros_like(T))
    return tol


def to_laid(x, gather, fill=0.0):
    """[N, D] in the ORIGINAL order -> [Np, D] in the product's layout, `fill` on the padding rows"""
    out = torch.full((gather.numel(), x.shape[1]), fill, dtype=x.dtype)
    out[gather >= 0] = x[gather[gather >= 0]]
    return out


def ratio(out, ref, tol):
    """largest err / tol over the elements (0 / 0 counts as 0, err > 0 at tol 0 as inf; a NaN counts as inf)"""
    err = (out.double().cpu() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def check(out, ref, tol, what):
    assert out.shape == ref.shape and out.dtype == torch.float32, what
    assert not torch.isnan(out).any(), f"{what}: NaN in the output"
    r = ratio(out, ref, tol)
    print(f"[cache-bwd] {what} err/tol {r:.3e}")
    assert r <= 1.0, f"{what}: err / tol = {r:.3e}"
    return r


def torch_cache_affinity_backward(q, g, class_off, class_len, beta, dA, *, exclude=None, out=None):
    """ops.cache_affinity_backward's contract restated with torch ops in fp32 on whatever device the operands live on: what
    the host logic of clip.fewshot is run on where there is no GPU."""
    assert q.dtype == g.dtype and q.dtype in DTYPES and class_off.dtype == torch.int32 and class_len.dtype == torch.int32
    Q, C = q.shape[0], class_len.numel()
    assert class_off.numel() == C + 1 and int(class_off[-1]) == g.shape[0]
    assert dA.dtype == torch.float32 and tuple(dA.shape) == (Q, C)
    rows = torch.arange(g.shape[0])
    cls = torch.zeros(g.shape[0], dtype=torch.long)
    live = torch.zeros(g.shape[0], dtype=torch.bool)
    for c in range(C):
        o, n = int(class_off[c]), int(class_len[c])
        cls[o:int(class_off[c + 1])] = c
        live[o:o + n] = True
    gz = torch.where(live[:, None], g.float(), torch.zeros((), dtype=torch.float32))
    w = dA[:, cls] * torch.exp(beta * (q.float() @ gz.t() - 1.0))
    take = live[None, :].expand(Q, -1)
    if exclude is not None:
        take = take & (rows[None, :] != exclude.long().cpu()[:, None])
    res = beta * (torch.where(take, w, torch.zeros_like(w)).t() @ q.float())
    if out is None:
        return res
    out.copy_(res)
    return out
