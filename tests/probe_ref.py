"""float64 restatement of the linear probe's objective of hi + lo (csrc/embed_probe.hip, clip/probe.py) on the same 16-bit
rows, and the tolerances its tests use.  Pure torch on the host; needs no library.

The function.  hi = round16(W), lo = round16(W - hi) in the rows' 16-bit type; z = b + x hi^T + x lo^T; lse, the per-row loss
rw (lse - z_y), the argmax (ties to the lower class, NaN lowest), g = rw (softmax(z) - onehot), dW = scale g^T x + l2 W,
db = scale sum g, objective = scale sum loss + l2 / 2 |W|^2.  A row whose label is outside [0, C) or whose clamped weight is 0
is ignored.  The reference is taken AT hi + lo, so the remainder W - (hi + lo) the split drops (below 2^-16 |W| in bf16, 2^-22 |W|
in fp16) does not enter a comparison with the kernel; it is the distance between the function the kernel declares and the
probe on W itself, and `split_remainder` reports it.

Tolerances (derived, none measured; u = 2^-24, the unit roundoff of fp32).

logits.  Products of two 16-bit operands are exact in fp32; a chain of D terms errs by at most D u sum_d |x| |w|, and a factor 4
  is left for the MFMA's internal summation order (the bound of the top-k and k-means tests).  Both chains, and the two adds
  (b + H) + L with one rounding each on numbers no larger than |b| + A, A = sum_d |x| (|hi| + |lo|):
      z_tol[n, c] = D 2^-22 A[n, c] + 2 u (|b_c| + A[n, c])
lse.  log-sum-exp is 1-Lipschitz in the maximum norm of z: max_c z_tol.  Computing it: a row's running sum passes through at
  most ceil(C / 16) tile steps and 4 butterfly steps; each multiplies by an exp (2 u for the function, R u for its rounded
  argument, R = max z - min z over the row) and rounds a product and a sum: (4 + R) u per step, one step of slack, then the
  logarithm (2 u |log s|, log s <= log 256 < 6) and the final add (u |lse|):
      lse_tol[n] = max_c z_tol[n, c] + (ceil(C / 16) + 5) (4 + R_n) u + u (|lse_n| + 12)
loss.  rw (lse - z_y): loss_tol = rw (lse_tol + z_tol[n, y]) + 2 u |loss|.
g.  The backward recomputes z (again within z_tol) and subtracts the forward's lse: the exponent is off by at most
  e = z_tol + lse_tol + u |z - lse|, so p = exp(z - lse) by p (expm1(e) + 2 u); then the subtraction and the weight:
      g_tol = rw (p (expm1(e) + 2 u) + u) + u |g|
  The 16-bit pair hi + lo of g drops at most  rem = r16 |g| + a16,  r16 = 2^-16, a16 = 0 for bf16;  r16 = 2^-22, a16 = 2^-25
  (half the smallest fp16 subnormal) for fp16.
dW.  The products of the second MFMA are exact; a term passes through at most h = 2 ceil(tpp / rs) + S + 8 additions (two
  MFMAs per tile of its stream, the S slots of the merge, slack for the 32-term sums inside an MFMA), again with the factor 4:
      dW_tol[c, d] = scale ( sum_n (g_tol + rem)[n, c] |x[n, d]| + 4 h u sum_n |g[n, c]| |x[n, d]| ) + 3 u |dW| + u l2 |W|
  db likewise with hb = 8 ceil(tpp / rs) + S + 2 sequential additions of the fp32 g:
      db_tol[c] = scale ( sum_n g_tol[n, c] + hb u sum_n |g[n, c]| ) + 2 u |db|
objective.  The loss tree adds a term through at most hl = N / 65536 + 24 additions, the W^2 tree through hw = C D / 65536 + 32:
      obj_tol = scale ( sum loss_tol + hl u sum |loss| ) + l2 / 2 (hw + 1) u sum W^2 + 4 u |objective|
"""
import math

import torch

U = 2.0 ** -24
SPLIT = {torch.bfloat16: (2.0 ** -16, 0.0), torch.float16: (2.0 ** -22, 2.0 ** -25)}


def geometry(N, C, D):
    """(rs, tpp, slots) of cclip_probe_parts' closed form (include/cclip_hip.h)"""
    cp = (C + 15) // 16 * 16
    rs = {16: 4, 32: 2}.get(cp, 1)
    T = (N + 31) // 32
    pmax = min(1024, max(1, (1 << 25) // (4 * rs * cp * D)))
    tpp = max(8, -(-T // pmax))
    return rs, tpp, rs * (-(-T // tpp))


def workspace_bytes(N, C, D):
    cp = (C + 15) // 16 * 16
    S = geometry(N, C, D)[2]
    return 4 * cp * D + 4 * S * cp * (D + 1) + 4 * (-(-C * D // 256) + 256)


def split16(W32, dtype):
    hi = W32.float().to(dtype)
    lo = (W32.float() - hi.float()).to(dtype)
    return hi, lo


def split_remainder(W32, dtype):
    hi, lo = split16(W32, dtype)
    return (W32.double() - hi.double() - lo.double()).abs().max().item()


def clamp_weights(rw, N):
    if rw is None:
        return torch.ones(N, dtype=torch.float64)
    rw = rw.double()
    return torch.where(rw > 0, rw.clamp(max=1.0), torch.zeros_like(rw))          # NaN fails the comparison


def argmax_ref(z):
    """ties to the lower class, NaN below every number"""
    zz = torch.where(torch.isnan(z), torch.full_like(z, -float("inf")), z)
    allnan = torch.isnan(z).all(dim=1)
    best = zz.max(dim=1, keepdim=True).values
    first = (zz == best).to(torch.uint8).argmax(dim=1)
    return torch.where(allnan, torch.zeros_like(first), first)


def reference(x16, W32, bias, labels, rw=None, scale=1.0, l2=0.0, fault=None):
    """Everything in float64 on the host.  `fault` plants one: "drop_lo", "bias_not_in_lse", "onehot_wrong_class",
    "ignored_row_leaks", "missing_part", "l2_on_bias".  Returns a dict of values and of tolerances (`*_tol`)."""
    dtype = x16.dtype
    x = x16.double().cpu()
    N, D = x.shape
    W32 = W32.float().cpu()
    C = W32.shape[0]
    b = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double().cpu()
    y = torch.full((N,), -1, dtype=torch.long) if labels is None else labels.long().cpu()
    w = clamp_weights(None if rw is None else rw.cpu(), N)
    hi, lo = split16(W32, dtype)
    hi, lo = hi.double(), lo.double()
    if fault == "drop_lo":
        lo = torch.zeros_like(lo)
    live = (y >= 0) & (y < C) & (w > 0)
    if fault == "ignored_row_leaks":
        live = (w > 0) | live
    yc = y.clamp(0, C - 1)
    xs = torch.where(live[:, None], x, torch.zeros_like(x))                     # an ignored row's content never enters
    H, L = x @ hi.t(), x @ lo.t()
    z = (b + H) + L
    zl = z - b if fault == "bias_not_in_lse" else z
    lse = torch.logsumexp(zl, dim=1)
    zy = z.gather(1, yc[:, None])[:, 0]
    loss = torch.where(live, w * (lse - zy), torch.zeros_like(lse))
    onehot = torch.zeros(N, C, dtype=torch.float64)
    onehot[torch.arange(N), (yc + 1) % C if fault == "onehot_wrong_class" else yc] = 1.0
    p = torch.exp(z - lse[:, None])
    g = torch.where(live[:, None], w[:, None] * (p - onehot), torch.zeros_like(p))
    gs = g
    rs, tpp, S = geometry(N, C, D)
    if fault == "missing_part":                                                 # the last row part never reaches the merge
        gs = g.clone()
        gs[(N - 1) // 32 // tpp * tpp * 32:] = 0
    Wd = W32.double()
    dW = scale * (gs.t() @ xs) + l2 * Wd
    db = scale * gs.sum(dim=0) + (l2 * b if fault == "l2_on_bias" else 0)
    obj = scale * loss.sum() + 0.5 * l2 * (Wd * Wd).sum()

    # ---- tolerances (module docstring) ----
    r16, a16 = SPLIT[dtype]
    A = x.abs() @ (hi.abs() + lo.abs()).t()
    z_tol = D * 2.0 ** -22 * A + 2 * U * (b.abs() + A)
    zf = torch.nan_to_num(z, nan=0.0, posinf=0.0, neginf=0.0)
    R = zf.max(dim=1).values - zf.min(dim=1).values
    lse_tol = z_tol.max(dim=1).values + (math.ceil(C / 16) + 5) * (4 + R) * U + U * (lse.abs() + 12)
    loss_tol = torch.where(live, w * (lse_tol + z_tol.gather(1, yc[:, None])[:, 0]) + 2 * U * loss.abs(), torch.zeros_like(lse))
    e = z_tol + lse_tol[:, None] + U * (z - lse[:, None]).abs()
    g_tol = torch.where(live[:, None], w[:, None] * (p * (torch.expm1(e) + 2 * U) + U) + U * g.abs(), torch.zeros_like(p))
    rem = torch.where(live[:, None], r16 * g.abs() + a16, torch.zeros_like(p))
    h = 2 * math.ceil(tpp / rs) + S + 8
    hb = 8 * math.ceil(tpp / rs) + S + 2
    ax = xs.abs()
    g_tol0, rem0, g0 = [torch.nan_to_num(t, nan=0.0) for t in (g_tol, rem, g.abs())]
    dW_tol = scale * ((g_tol0 + rem0).t() @ ax + 4 * h * U * (g0.t() @ ax)) + 3 * U * dW.abs() + U * l2 * Wd.abs()
    db_tol = scale * (g_tol0.sum(dim=0) + hb * U * g0.sum(dim=0)) + 2 * U * db.abs()
    hl, hw = N / 65536 + 24, C * D / 65536 + 32
    obj_tol = scale * (loss_tol.sum() + hl * U * loss.abs().sum()) + 0.5 * l2 * (hw + 1) * U * (Wd * Wd).sum() + 4 * U * obj.abs()
    return dict(z=z, lse=lse, loss=loss, pred=argmax_ref(z), g=g, dW=dW, db=db, objective=obj, live=live,
                z_tol=z_tol, lse_tol=lse_tol, loss_tol=loss_tol, dW_tol=dW_tol, db_tol=db_tol, obj_tol=obj_tol)


def objective64(x16, Weff, bias, labels, rw, scale, l2, W_l2=None):
    """The objective as a float64 function of the effective weights Weff (= hi + lo) and the bias - what a finite difference
    or autograd differentiates.  The penalty is taken on W_l2 (default Weff)."""
    x = x16.double().cpu()
    N, C = x.shape[0], Weff.shape[0]
    y = labels.long().cpu()
    w = clamp_weights(None if rw is None else rw.cpu(), N)
    live = (y >= 0) & (y < C) & (w > 0)
    x = torch.where(live[:, None], x, torch.zeros_like(x))
    z = x @ Weff.t() + bias
    per = torch.logsumexp(z, dim=1) - z.gather(1, y.clamp(0, C - 1)[:, None])[:, 0]
    Wp = Weff if W_l2 is None else W_l2
    return scale * torch.where(live, w * per, torch.zeros_like(per)).sum() + 0.5 * l2 * (Wp * Wp).sum()


def lbfgs_fit64(x16, labels, C, rw, scale, l2, max_iter, tol, W0=None, b0=None, history_size=10):
    """clip.probe's fit in float64 on the host: the same torch.optim.LBFGS settings on objective64 (Weff = W: no split)."""
    D = x16.shape[1]
    W = torch.nn.Parameter(torch.zeros(C, D, dtype=torch.float64) if W0 is None else W0.double().clone())
    b = torch.nn.Parameter(torch.zeros(C, dtype=torch.float64) if b0 is None else b0.double().clone())
    opt = torch.optim.LBFGS([W, b], lr=1.0, max_iter=max_iter, tolerance_grad=tol, tolerance_change=1e-9,
                            history_size=history_size, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        f = objective64(x16, W, b, labels, rw, scale, l2)
        f.backward()
        return f

    opt.step(closure)
    return W.detach(), b.detach()


def planted_rows(sizes, D, noise, seed, dtype):
    """len(sizes) random unit directions, sizes[j] unit rows around direction j, shuffled -> (x16 [N, D], labels int64 [N])"""
    gen = torch.Generator().manual_seed(seed)
    dirs = torch.randn(len(sizes), D, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    truth = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = dirs[truth] + noise / D ** 0.5 * torch.randn(truth.numel(), D, generator=gen)
    x = x / x.norm(dim=1, keepdim=True)
    perm = torch.randperm(truth.numel(), generator=gen)
    return x[perm].to(dtype), truth[perm], dirs
