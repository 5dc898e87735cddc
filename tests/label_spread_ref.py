"""float64 reference of the label-spreading kernels (csrc/label_spread.hip) and of the whole pipeline (clip/propagate.py) on
the same fp32 operands, and the tolerances its tests use.  Pure torch on the host; needs no library.  `fault=` plants one
known mistake (tests/test_label_spread_cpu.py shows that the tolerances see each of them).

Tolerances (derived, none measured; u = 2^-24, the unit roundoff of fp32; n_i = the entries of row i; first order in u, n u
< 1e-4 throughout).  The build has no fast-math flag: +, *, fma, / and sqrtf are correctly rounded (one u each).

CSR.  The kernels clamp offsets into [0, nnz], make a row's end no less than its start, and clamp cols into [0, N - 1]; `rows_of`
  restates that, so the reference is defined for any content.  Duplicate columns of a row add up.

normalize.  All weights are >= 0, a chain of n_i additions:      deg_tol[i] = (n_i + 1) u d_i
  r_i = 1 / sqrt(d_i) from the kernel's own d_i: half the relative error of d_i, then sqrtf and the division, u each:
  ((n_i + 1) / 2 + 2) u.  Two products follow:                     vals_tol[e] = ((n_i + n_j) / 2 + 7) u vals_out[e]
  (one more u than the count, kept for the second order).  A row with d_i = 0 gives r_i = 0 and exact zeros.

step.  Every term is >= 0.  A term of sum_j S_ij F_jc meets at most n_i roundings before the sum is complete, in any order
  whose chain depth is at most n_i: here the fma chain of edge group g (ceil(n_i / G) deep, the product not rounded) and the
  tree over the G groups, in which an addition of an exact 0 rounds nothing - at most min(log2 G, n_i - 1) more.  The label
  term (1 - alpha) w is fma(-alpha, w, w): one rounding.  The result is fma(alpha, sum, label term): one rounding.  With
  A = alpha sum_j S_ij F_jc and L the label term:  error <= n_i u A + u L + u (A + L), inside
      tol[i, c] = (n_i + 4) u A + 2 u out[i, c]
  delta_row = max_c |out - F_in|, the subtraction rounded once:    delta_tol[i] = max_c tol[i, c] + u delta[i]
  alpha is rounded to fp32 first, as the C ABI takes it.

T steps.  Componentwise, inside the reference (no norm argument: row sums of D^-1/2 W D^-1/2 may exceed 1).  With E_t >= the
  kernel's error on F_t, the kernel's step starts from a matrix within E_t of F_t:
      E_0 = u F_0 (the label term),    E_{t+1} = alpha (S E_t + dS (F_t + E_t)) + tol_step(F_t + E_t)
  tol_step is linear in its operand, so evaluating it at F_t + E_t covers the kernel's own operand.  dS_ij >= |S'_ij - S_ij|
  is the error of the operator the kernel is given: 0 in the kernel tests (the same vals), and in the pipeline
      dS = (2 w + (n_i + n_j) / 2 + 7) u S,    w = 2 beta max(1 - s) + 6
  from A = exp(-a), a = beta (1 - s): the subtraction and the product move a by 2 u a, expf is taken as <= 2 ulp (4 u), the sum
  of the two directions adds u: w u on every W_ij and on every d_i besides its (n_i + 1) u; then as under normalize.

finish.  z: a chain of at most ceil(C / CW) + log2 CW <= C additions of non-negative terms:   z_tol = (C + 1) u z
  p = F / z: (C + 3) u p, and conf = max p the same.  A term p log p, logf taken as <= 2 ulp (4 u) and the product u:
  u p ((C + 3) (|log p| + 1) + 5 |log p|); the sum of C terms adds C u sum |p log p|:
      H_tol = u sum_c p ((2 C + 8) |log p| + C + 3),    cert_tol = (H_tol + 5 u H) / log C + u
  (logf(C) 4 u, the division u, the final addition u of a value <= 1).  pred is compared only where the reference's top-two
  gap in F exceeds twice the bound on F (everywhere when F is the kernel's own operand: then ties go to the lowest class).
  z == 0: pred = -1, conf = cert = 0 and a zero dist row, all exact.
"""
import math

import torch

U = 2.0 ** -24
MAX_C = 1024
FAULTS = ("alpha_on_label", "row_norm", "drop_last", "in_place", "no_class_weight", "unlabelled_class0", "cert_log2", "tie_high",
          "zero_pred0")


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def spread_plan(C):
    """(class lanes CW, edge groups G, classes per lane NQ) of the step kernel: csrc/label_spread.hip's spread_plan"""
    cw = 2
    while cw < C and cw < 64:
        cw *= 2
    return cw, min(8, 64 // cw), 1 if C <= 64 else (2 if C <= 128 else 4)


def rows_of(offsets, cols, N):
    """The entries the kernels visit: (row [m], entry index [m], clamped col [m], n_i [N]) for any content of offsets / cols"""
    nnz = cols.numel()
    off = offsets.to(torch.int64)
    e0 = off[:-1].clamp(0, nnz)
    e1 = torch.minimum(torch.maximum(off[1:], e0), torch.tensor(nnz))
    n = e1 - e0
    row = torch.repeat_interleave(torch.arange(N), n)
    first = torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
    entry = torch.repeat_interleave(e0, n) + (torch.arange(int(n.sum())) - first)
    col = cols.to(torch.int64)[entry].clamp(0, N - 1)
    return row, entry, col, n


def sparse(row, col, val, N):
    return torch.sparse_coo_tensor(torch.stack([row, col]), val, (N, N)).coalesce()


# ---- normalize ----------------------------------------------------------------------------------------------------------
def normalize_ref(offsets, cols, vals32, N, fault=None, dtype=torch.float64):
    """deg [N], vals_out per visited entry [m] (with `entry`, their positions in vals), deg_tol, vals_tol"""
    row, entry, col, n = rows_of(offsets, cols, N)
    v = vals32[entry].to(dtype)
    d = torch.zeros(N, dtype=dtype).index_add_(0, row, v)
    r = torch.where(d > 0, 1.0 / torch.sqrt(d.clamp(min=1e-300)), torch.zeros_like(d))
    out = v * r[row] * (r[row] if fault == "row_norm" else r[col])
    nd = n.double()
    return dict(deg=d, vals=out, entry=entry, row=row, col=col, n=n, deg_tol=(nd + 1) * U * d.double(),
                vals_tol=((nd[row] + nd[col]) / 2 + 7) * U * out.double())


# ---- step ---------------------------------------------------------------------------------------------------------------
def one_hot(labels, class_weight, C, dtype, fault=None):
    lab = labels.to(torch.int64)
    if fault == "unlabelled_class0":
        lab = lab.clamp(min=0)
    ok = (lab >= 0) & (lab < C)
    w = torch.ones(C, dtype=dtype) if class_weight is None or fault == "no_class_weight" else class_weight.to(dtype)
    Y = torch.zeros(labels.numel(), C, dtype=dtype)
    Y[ok, lab[ok]] = w[lab[ok]]
    return Y


def step_tol(SF_alpha, out, n):
    return (n.double()[:, None] + 4) * U * SF_alpha + 2 * U * out


def step_ref(F32, labels, class_weight, offsets, cols, vals32, alpha, fault=None, dtype=torch.float64):
    """One iteration in `dtype` from fp32 operands: out [N, C], delta [N], tol, delta_tol"""
    N, C = F32.shape
    a = f32(alpha)
    row, entry, col, n = rows_of(offsets, cols, N)
    v = vals32[entry].to(dtype)
    if fault == "drop_last":
        last = torch.ones_like(row, dtype=torch.bool)
        last[:-1] = row[1:] != row[:-1]
        v = torch.where(last, torch.zeros_like(v), v)
    F = F32.to(dtype)
    Y = one_hot(labels, class_weight, C, dtype, fault)
    lab_term = (a if fault == "alpha_on_label" else 1.0 - a) * Y
    if fault == "in_place":
        out = F.clone()
        Sd = sparse(row, col, v, N).to_dense()
        for i in range(N):
            out[i] = a * (Sd[i] @ out) + lab_term[i]
        SF = a * (Sd @ F)
    else:
        SF = a * torch.sparse.mm(sparse(row, col, v, N), F)
        out = SF + lab_term
    tol = step_tol(SF.double(), out.double(), n)
    delta = (out - F).abs().max(dim=1).values
    return dict(out=out, delta=delta, tol=tol, delta_tol=tol.max(dim=1).values + U * delta.double(), n=n)


def spread_ref(labels, class_weight, offsets, cols, vals, alpha, n_iter, C, dS_rel=None):
    """n_iter steps in float64 from F_0 = (1 - alpha) Y with the propagated bound: F [N, C], E [N, C] (>= the kernels' error
    on F under the module's assumptions), delta [N] of the last step.  vals: the operator, fp32 (the kernels' own operand,
    dS_rel None) or float64 with dS_rel [m], the relative bound on every visited entry."""
    N = labels.numel()
    a = f32(alpha)
    row, entry, col, n = rows_of(offsets, cols, N)
    v = vals[entry].double()
    S = sparse(row, col, v, N)
    dS = None if dS_rel is None else sparse(row, col, v * dS_rel, N)
    lab_term = (1.0 - a) * one_hot(labels, class_weight, C, torch.float64)
    F, E = lab_term.clone(), U * lab_term
    delta = torch.zeros(N, dtype=torch.float64)
    for _ in range(n_iter):
        SF = a * torch.sparse.mm(S, F)
        out = SF + lab_term
        FE = F + E
        SFE = a * torch.sparse.mm(S, FE)
        E_new = a * torch.sparse.mm(S, E) + step_tol(SFE, SFE + lab_term, n)
        if dS is not None:
            E_new = E_new + a * torch.sparse.mm(dS, FE)
        delta = (out - F).abs().max(dim=1).values
        F, E = out, E_new
    return F, E, delta


def closed_form(labels, class_weight, offsets, cols, vals, alpha, C):
    """(1 - alpha) (I - alpha S)^-1 Y, dense float64"""
    N = labels.numel()
    a = f32(alpha)
    row, entry, col, n = rows_of(offsets, cols, N)
    Sd = sparse(row, col, vals[entry].double(), N).to_dense()
    Y = one_hot(labels, class_weight, C, torch.float64)
    return (1.0 - a) * torch.linalg.solve(torch.eye(N, dtype=torch.float64) - a * Sd, Y)


# ---- finish -------------------------------------------------------------------------------------------------------------
def finish_ref(F32, F_tol=None, fault=None, dtype=torch.float64):
    """dist, pred, conf, cert of the rows of F with their tolerances; `decided` [N]: where pred is compared; `zero`, `nan`
    [N]: the rows that sum to 0 / hold a NaN."""
    F = F32.to(dtype)
    N, C = F.shape
    z = F.sum(dim=1)
    nan = torch.isnan(z)
    zero = ~nan & ~(z > 0)
    zs = torch.where(z > 0, z, torch.ones_like(z))
    p = torch.where(zero[:, None], torch.zeros_like(F), F / zs[:, None])
    top = F.max(dim=1, keepdim=True).values
    ids = torch.arange(C)[None, :].expand(N, C)
    if fault == "tie_high":
        pred = torch.where(F == top, ids, torch.full_like(ids, -1)).max(dim=1).values
    else:
        pred = torch.where(F == top, ids, torch.full_like(ids, C)).min(dim=1).values
    pred = torch.where(zero | nan, torch.full_like(pred, 0 if fault == "zero_pred0" else -1), pred)
    logp = torch.where(p > 0, p, torch.ones_like(p)).log()
    H = -(p * logp).sum(dim=1)
    logC = math.log(2.0 if fault == "cert_log2" else C)
    cert = torch.where(zero, torch.zeros_like(z), 1.0 - H / logC)
    conf = p.max(dim=1).values
    pd, lp = p.double(), logp.double().abs()
    H_tol = U * (pd * ((2 * C + 8) * lp + C + 3)).sum(dim=1)
    if F_tol is None:
        decided = ~nan
    else:
        two = torch.topk(F.double(), 2, dim=1).values
        decided = ~nan & ((two[:, 0] - two[:, 1]) > 2 * F_tol.max(dim=1).values)
    return dict(z=z, dist=p, pred=pred, conf=conf, cert=cert, z_tol=(C + 1) * U * z.double().abs(), dist_tol=(C + 3) * U * pd,
                conf_tol=(C + 3) * U * conf.double(), cert_tol=(H_tol + 5 * U * H.double()) / math.log(C) + U, decided=decided,
                zero=zero, nan=nan)


# ---- the whole pipeline -------------------------------------------------------------------------------------------------
def affinity_dense(scores32, index, beta, dtype=torch.float64):
    """A + A^T, dense [N, N] in `dtype`, A_ij = exp(-beta (1 - s_ij)) on the directed edges"""
    N = scores32.shape[0]
    A = torch.zeros(N, N, dtype=dtype)
    A.scatter_(1, index.long(), torch.exp(-float(beta) * (1.0 - scores32.to(dtype))))
    return A + A.t()


def class_weights_ref(labels, C):
    """fp32, as clip/propagate.py: 1 / count_c (one correctly rounded division), 0 for a class without a labelled row"""
    lab = labels.to(torch.int64)
    counts = torch.bincount(lab[lab >= 0], minlength=C)[:C]
    return torch.where(counts > 0, 1.0 / counts.clamp(min=1).float(), torch.zeros(C))


def pipeline_ref(scores32, index, labels, C, beta, alpha, n_iter, class_balance=True):
    """clip.spread_labels in float64 from the kNN graph (scores fp32 [N, k], index [N, k]) the device found: F, its bound E,
    the last step's delta, and finish_ref of F under that bound."""
    N = scores32.shape[0]
    W = affinity_dense(scores32, index, beta)
    row, col = torch.nonzero(W, as_tuple=True)
    offsets = torch.searchsorted(row, torch.arange(N + 1))
    d = W.sum(dim=1)
    r = torch.where(d > 0, 1.0 / torch.sqrt(d.clamp(min=1e-300)), torch.zeros_like(d))
    vals = W[row, col] * r[row] * r[col]
    n = offsets.diff().double()
    w = 2.0 * float(beta) * float((1.0 - scores32.double()).max().clamp(min=0)) + 6
    dS_rel = (2 * w + (n[row] + n[col]) / 2 + 7) * U
    cw = class_weights_ref(labels, C) if class_balance else None
    F, E, delta = spread_ref(labels, cw, offsets, col.to(torch.int32), vals, alpha, n_iter, C, dS_rel=dS_rel)
    fin = finish_ref(F, F_tol=E)
    z = F.sum(dim=1, keepdim=True)
    # p = F / z with F and z both moved: |dp| <= (E + p sum_c E) / (z - sum_c E), plus the kernel's own (C + 3) u p
    Es = E.sum(dim=1, keepdim=True)
    dist_tol = torch.where(z > Es, (E + fin["dist"] * Es) / (z - Es).clamp(min=1e-300), torch.zeros_like(E)) + fin["dist_tol"]
    return dict(F=F, E=E, delta=delta, finish=fin, dist_tol=dist_tol, offsets=offsets, cols=col.to(torch.int32), vals=vals, class_weight=cw)


def planted(N, Cn, noise, per_class, seed, D=64, dtype=torch.bfloat16):
    """The planted clusters of the end-to-end tests: unit centres normalize(randn(Cn, D)), rows normalize(centre[i mod Cn] +
    noise randn(D) / 8) rounded to `dtype`; the first per_class rows of every class carry their label.  Returns (rows 16-bit
    [N, D], truth int64 [N], labels int64 [N] with -1 for an unlabelled row)."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.nn.functional.normalize(torch.randn(Cn, D, generator=g), dim=1)
    truth = torch.arange(N) % Cn
    rows = torch.nn.functional.normalize(centre[truth] + noise * torch.randn(N, D, generator=g) / 8.0, dim=1).to(dtype)
    labels = torch.where(torch.arange(N) < per_class * Cn, truth, torch.full_like(truth, -1))
    return rows, truth, labels
