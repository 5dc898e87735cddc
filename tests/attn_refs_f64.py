"""Float64 attention reference and its per-element bounds, shared by tests/test_kernels_f16_gpu.py (where they were written; the
bound is derived in that module's header) and the BlockStack tests (tests/stack_ref_f64.py).  Plain torch on whatever device the
operands live on."""
import torch

from gemm_refs_f64 import FLOOR, U


def _split_heads(x, B, T, H, dh=64):
    return x.double().view(B, T, H, dh).permute(0, 2, 1, 3)


def _attn64(q, k, v, dO, causal, keep, scale):
    """fp64 attention fwd / bwd of [B,H,T,dh] operands; returns o, lse, dq, dk, dv and the per-element magnitude scales"""
    T = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        s = s + torch.full((T, T), float("-inf"), device=q.device, dtype=torch.float64).triu_(1)
    if keep is not None:
        s = s.masked_fill(keep[:, None, None, :] == 0, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = scale * dS @ k
    dk = scale * dS.transpose(-1, -2) @ q
    dv = P.transpose(-1, -2) @ dO
    Pv = P @ v.abs()
    dSm = P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * Pv).sum(-1, keepdim=True))
    mag = dict(o=Pv, dv=P.transpose(-1, -2) @ dO.abs(), dq=scale * dSm @ k.abs(), dk=scale * dSm.transpose(-1, -2) @ q.abs(),
               P=P, kabs=k.abs(), qabs=q.abs(), vabs=v.abs(), dOabs=dO.abs())
    return o, lse, dq, dk, dv, mag


def _attn_bounds(mag, scale, dt):
    """4u * magnitude + the subnormal floors of the rounded 16-bit P (o, dv) and dS (dq, dk)"""
    u, fl = U(dt), FLOOR(dt)
    return dict(o=4 * u * mag["o"] + fl * mag["vabs"].sum(-2, keepdim=True) + fl,
                dv=4 * u * mag["dv"] + fl * mag["dOabs"].sum(-2, keepdim=True) + fl,
                dq=4 * u * mag["dq"] + 2 * fl * scale * mag["kabs"].sum(-2, keepdim=True) + fl,
                dk=4 * u * mag["dk"] + 2 * fl * scale * mag["qabs"].sum(-2, keepdim=True) + fl)
