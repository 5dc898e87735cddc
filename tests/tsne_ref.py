"""float64 reference of the t-SNE steps (csrc/tsne.hip, clip/tsne.py) on the same fp32 operands, and the tolerances its tests
use.  Pure torch on the host; needs no library.  `fault=` plants one known mistake (tests/test_tsne_cpu.py shows that the
tolerances see each of them).

Tolerances (derived, none measured; u = 2^-24, the unit roundoff of fp32; "N u a" stands for gamma_N a, N u < 0.01 throughout).

repulsion.  One pair: dx, dy round once each (u), d2 = fma(dx, dx, dy dy) <= 4 u relative, 1 + d2 one more, v_rcp_f32 is
  1 ulp = 2 u: w carries <= 8 u, w^2 <= 17 u, and the fma of w^2 with dx <= 19 u with dx's own rounding.
  A term then passes through a chain of additions of depth at most
      h(N) = tps(N) (J / 4 + 3) + 2 + S(N)
  - the four chains of a split take a quarter of each of its tps tiles of J = 512 points (chain 0 up to 3 more of a short
  tile), two additions join the chains, S - 1 join the splits; S and tps are the kernel's split plan, restated in split_plan.
      zrow_tol[i]   = (h + 8)  u zrow[i]                               (all terms are >= 0: a multiple of N u zrow / (4 S))
      rep_tol[i, d] = (h + 20) u sum_j w_ij^2 |y_id - y_jd|            (on the sum of magnitudes, not on |rep|, which cancels)
      Z_tol         = sum_i zrow_tol[i] + (ceil(B / 256) + 24) u Z,    B = ceil(N / 256) block sums: a thread adds at most
                      ceil(B / 256) of them, the two trees add 2 (6 + 3) levels, and zrow's own tree is counted in the 24.

affinities.  The reference takes diff_j = d2_j - min d2 in fp32 exactly as the kernel does (2 - 2 s, a negative value to 0,
  the minimum, the subtraction: each correctly rounded, the same bits on any IEEE machine), so the comparison starts at diff.
  With a_j = beta diff_j, e_j = exp(-a_j), p_j = e_j / S, A1 = sum p_j a_j, A2 = sum p_j a_j^2:  the product rounds (a_j u on
  e_j), expf is taken as <= 2 ulp (4 u): delta_j <= (a_j + 5) u on e_j.  H = log S + beta T / S moves by
  sum_j p_j delta_j (1 + a_j + A1) <= u (A2 + A1^2 + 11 A1 + 5); the two sums of k terms add k u (1 + 2 A1), logf (2 ulp),
  the product, the quotient and the last addition 4 u (log k + A1) more, the fp32 target u log(perplexity):
      eps_H    = u (A2 + A1^2 + 11 A1 + 5 + k (1 + 2 A1) + 8 (log k + A1) + log perplexity)
  The kernel's bisection ends between two adjacent floats whose computed entropies straddle the target, so the entropy of
  its beta is within eps_H of the target, plus one spacing of beta; dH / dbeta = -beta Var_p(diff), both in float64 per row:
      beta_tol = 2 eps_H / (beta Var_p(diff)) + 4 u beta          (the 2 covers the second order)
      P_tol[j] = p_j |diff_j - mean_p diff| beta_tol + p_j (a_j + k + 7) u + 2^-125
                 (d p_j / d beta; then e_j, S and the quotient; and fp32's underflow: an e_j or a quotient below the smallest
                 normal 2^-126 may lose all its bits or be flushed to zero, and S >= 1)
  A row with Var_p(diff) = 0 (all distances equal; or the target out of reach because >= perplexity distances tie at the
  minimum) is `degenerate`: beta is not compared there, P only with the second term.

step.  Per entry q = 1 + (dx^2 + dy^2) <= 5 u, ex p / q two roundings more, times dx (its own u and one more): <= 9 u a term,
  a chain of n_i entries:     att_tol = (n_i + 9) u sum_j |ex P_ij w_ij (y_id - y_jd)|
      grad_tol  = 4 (att_tol + u |rep_d / Z| + rep_tol / Z + |rep_d| Z_tol / Z^2) + u |grad|      (rep_tol, Z_tol: 0 when the
                  kernel and the reference are given the same rep and Z)
      gains_tol = 3 u max(gains', 1)     where both take the same branch (0.2f and 0.8f are within u of 0.2 and 0.8)
      vel_tol   = lr (gains' grad_tol + |grad| gains_tol) + 4 u (|m vel| + |lr gains' grad|)
      y_tol     = vel_tol + u |y'|
      kl_tol[i] = (n_i + 12) u sum_j P_ij (|log P_ij| + log q_ij + |log Z| + 1) + sum_j P_ij Z_tol / Z
  An element whose |grad| <= grad_tol, or whose vel is exactly 0, may take either branch of the gains rule: `decided` is
  False there and gains, vel and y are not compared.  The scalar arguments are rounded to fp32 first, as the C ABI takes them.
"""
import math

import torch

U = 2.0 ** -24
TILE, ROWS, SPLIT_MAX, TARGET_BLOCKS, BISECT_STEPS, MAX_K = 512, 256, 16, 1024, 100, 63


def split_plan(N):
    """(tiles per split, splits) of the repulsion kernel: csrc/tsne.hip's split_plan"""
    ntiles, rb = -(-N // TILE), -(-N // ROWS)
    want = min(-(-TARGET_BLOCKS // rb), SPLIT_MAX, ntiles)
    tps = -(-ntiles // want)
    return tps, -(-ntiles // tps)


def chain_depth(N):
    tps, splits = split_plan(N)
    return tps * (TILE // 4 + 3) + 2 + splits


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---- affinities ---------------------------------------------------------------------------------------------------------
def diffs32(scores32):
    """fp32, operation by operation as the kernel: d2 = 2 - 2 s with a negative value taken as 0 (NaN stays), minus the row minimum"""
    s = scores32.float()
    v = 2.0 - 2.0 * s
    d2 = torch.where(v < 0, torch.zeros_like(v), v)
    return d2 - d2.min(dim=1, keepdim=True).values


def entropy(beta, diff, bits=False):
    e = torch.exp(-beta[:, None] * diff)
    S = e.sum(dim=1)
    H = torch.log(S) + beta * (diff * e).sum(dim=1) / S
    return H / math.log(2.0) if bits else H


def affinities_ref(scores32, perplexity, fault=None, dtype=torch.float64):
    """(P [N, k], beta [N], info) by the kernel's bisection rule and step count in `dtype`.  A row with a NaN score gets NaN.
    info: H (the entropy at beta), eps_H, beta_tol, P_tol, degenerate."""
    if fault == "no_shift":
        v = 2.0 - 2.0 * scores32.float()
        diff = torch.where(v < 0, torch.zeros_like(v), v).to(dtype)
    else:
        diff = diffs32(scores32).to(dtype)
    if fault == "drop_last":
        diff = diff[:, :-1]
    N, k = diff.shape
    bits = fault == "bits"
    target = math.log(perplexity)
    beta = torch.ones(N, dtype=dtype)
    lo, hi = torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=dtype)
    have_hi = torch.zeros(N, dtype=torch.bool)
    for _ in range(BISECT_STEPS):
        up = entropy(beta, diff, bits) > target
        lo = torch.where(up, beta, lo)
        hi = torch.where(up, hi, beta)
        have_hi = have_hi | ~up
        beta = torch.where(have_hi, 0.5 * (lo + hi), beta * 2.0)
    e = torch.exp(-beta[:, None] * diff)
    P = e / e.sum(dim=1, keepdim=True)
    bad = torch.isnan(diff).any(dim=1)
    P[bad] = float("nan")
    beta = torch.where(bad, torch.full_like(beta, float("nan")), beta)
    if fault == "drop_last":
        P = torch.cat([P, torch.zeros(N, 1, dtype=dtype)], dim=1)
        return P, beta, None
    a = beta[:, None] * diff
    A1, A2 = (P * a).sum(dim=1), (P * a * a).sum(dim=1)
    eps_H = U * (A2 + A1 * A1 + 11 * A1 + 5 + k * (1 + 2 * A1) + 8 * (math.log(k) + A1) + target)
    mean = (P * diff).sum(dim=1, keepdim=True)
    var = (P * (diff - mean) ** 2).sum(dim=1)
    degenerate = ~(var * beta * beta > 1e-12) | ~(beta < 2.0 ** 90)
    beta_tol = 2 * eps_H / (beta * var) + 4 * U * beta
    eval_tol = P * (a + k + 7) * U + 2.0 ** -125
    P_tol = torch.where(degenerate[:, None], eval_tol, P * (diff - mean).abs() * beta_tol[:, None] + eval_tol)
    return P, beta, dict(H=entropy(beta, diff), eps_H=eps_H, beta_tol=beta_tol, P_tol=P_tol, degenerate=degenerate)


def knn_ref(x16, k):
    """float64 top-k of every row against the others, equal scores by the lower index: (scores [N, k], index [N, k])"""
    x = x16.double()
    s = x @ x.t()
    s.fill_diagonal_(-float("inf"))
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), order


def joint_dense(P, index):
    """(P_cond + P_cond^T) / (2 N) as a dense float64 [N, N]"""
    N = P.shape[0]
    C = torch.zeros(N, N, dtype=torch.float64)
    C.scatter_(1, index.long(), P.double())
    return (C + C.t()) / (2.0 * N)


def csr_dense(offsets, cols, vals, N):
    D = torch.zeros(N, N, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(N), offsets.diff())
    D.index_put_((rows, cols.long()), vals.double(), accumulate=True)
    return D


# ---- repulsion ----------------------------------------------------------------------------------------------------------
def repulsion_ref(y32, fault=None, chunk=1024):
    """zrow [N], rep [N, 2], Z of the fp32 map in float64, with zrow_tol, rep_tol, Z_tol.  Rows in chunks: no N x N matrix."""
    y = y32.double()
    N = y.shape[0]
    zrow, rep, mag = torch.empty(N, dtype=torch.float64), torch.empty(N, 2, dtype=torch.float64), torch.empty(N, 2, dtype=torch.float64)
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        d = y[r0:r1, None, :] - y[None, :, :]                                  # [c, N, 2]
        w = 1.0 / (1.0 + (d * d).sum(dim=2))
        if fault != "diag":
            w[torch.arange(r1 - r0), torch.arange(r0, r1)] = 0.0
        ww = w if fault == "w1" else w * w
        zrow[r0:r1] = w.sum(dim=1)
        rep[r0:r1] = (ww[:, :, None] * d).sum(dim=1)
        mag[r0:r1] = (ww[:, :, None] * d.abs()).sum(dim=1)
    h = chain_depth(N)
    Z = zrow.sum()
    zrow_tol = (h + 8) * U * zrow
    B = -(-N // 256)
    return dict(zrow=zrow, rep=rep, Z=Z, zrow_tol=zrow_tol, rep_tol=(h + 20) * U * mag,
                Z_tol=zrow_tol.sum() + (-(-B // 256) + 24) * U * Z)


# ---- step ---------------------------------------------------------------------------------------------------------------
def step_ref(y32, vel32, gains32, Pd, rep, Z, exaggeration, momentum, learning_rate, min_gain, rep_tol=None, Z_tol=0.0, fault=None):
    """One update in float64 from fp32 state.  Pd: the joint P, dense float64 [N, N] (zero where the CSR has no entry); rep
    [N, 2] and Z as the kernel is given them (then rep_tol = None, Z_tol = 0) or from repulsion_ref with its bounds.
    Returns y, vel, gains, grad, kl_row and their tolerances, and `decided` [N, 2]."""
    ex, m, lr, mg = f32(exaggeration), f32(momentum), f32(learning_rate), f32(min_gain)
    y, vel, gains = y32.double(), vel32.double(), gains32.double()
    rep = rep.double()
    Z = float(Z)
    N = y.shape[0]
    d = y[:, None, :] - y[None, :, :]
    q = 1.0 + (d * d).sum(dim=2)
    live = Pd > 0
    n_i = (Pd != 0).sum(dim=1).double()
    term = (ex * Pd / q)[:, :, None] * d
    att = term.sum(dim=1)
    att_tol = ((n_i + 9) * U)[:, None] * term.abs().sum(dim=1)
    r = rep / Z if fault != "ex_on_rep" else ex * rep / Z
    grad = (1.0 if fault == "no_4" else 4.0) * (att - r)
    rt = torch.zeros_like(rep) if rep_tol is None else rep_tol.double()
    grad_tol = 4 * (att_tol + U * (rep / Z).abs() + rt / Z + rep.abs() * Z_tol / Z ** 2) + U * grad.abs()
    differ = (vel > 0) != (grad > 0)
    if fault == "gains_inverted":
        differ = ~differ
    g_new = torch.where(differ, gains + 0.2, gains * 0.8).clamp(min=mg)
    v_new = m * vel - lr * g_new * grad
    y_new = y + v_new
    gains_tol = 3 * U * g_new.clamp(min=1.0)
    vel_tol = lr * (g_new * grad_tol + grad.abs() * gains_tol) + 4 * U * ((m * vel).abs() + (lr * g_new * grad).abs())
    logP = torch.where(live, Pd, torch.ones_like(Pd)).log()
    kl_row = (Pd * (logP + q.log() + math.log(Z))).sum(dim=1)
    kl_tol = (n_i + 12) * U * (Pd * (logP.abs() + q.log() + abs(math.log(Z)) + 1)).sum(dim=1) + Pd.sum(dim=1) * Z_tol / Z
    decided = (grad.abs() > grad_tol) & (vel != 0)
    return dict(y=y_new, vel=v_new, gains=g_new, grad=grad, kl_row=kl_row, grad_tol=grad_tol, gains_tol=gains_tol, vel_tol=vel_tol,
                y_tol=vel_tol + U * y_new.abs(), kl_tol=kl_tol, decided=decided)


def kl_ref(Pd, y):
    """KL(P || Q) of the dense joint P and the map y, float64: Q_ij = w_ij / sum_{k != l} w_kl"""
    y = y.double()
    d = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (d * d).sum(dim=2))
    w = w - torch.diag(torch.diag(w))
    Q = w / w.sum()
    live = Pd > 0
    return (Pd[live] * (Pd[live].log() - Q[live].log())).sum()


def grad_ref(Pd, y):
    """the closed form of d KL / d y: 4 sum_j (P_ij - Q_ij) w_ij (y_i - y_j)"""
    y = y.double()
    d = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (d * d).sum(dim=2))
    w = w - torch.diag(torch.diag(w))
    Z = w.sum()
    return 4.0 * (((Pd - w / Z) * w)[:, :, None] * d).sum(dim=1)


def loop_ref(Pd, y0, n_iter, exaggeration=12.0, exaggeration_iters=250, learning_rate=None, kl_at=(), dtype=torch.float64):
    """clip.tsne's loop in `dtype`, dense: returns (the centred map, {it: KL of the map entering iteration it, for it in
    kl_at}, the final KL)"""
    N = Pd.shape[0]
    lr = max(N / exaggeration / 4.0, 50.0) if learning_rate is None else learning_rate
    Pd = Pd.to(dtype)
    y = y0.to(dtype).clone()
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    kls = {}
    for it in range(n_iter):
        ex, m = (exaggeration, 0.5) if it < exaggeration_iters else (1.0, 0.8)
        d = y[:, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (d * d).sum(dim=2))
        w = w - torch.diag(torch.diag(w))
        Z = w.sum()
        if it in kl_at:
            kls[it] = float(kl_ref(Pd.double(), y))
        grad = 4.0 * (((ex * Pd - w / Z) * w)[:, :, None] * d).sum(dim=1)
        differ = (vel > 0) != (grad > 0)
        gains = torch.where(differ, gains + 0.2, gains * 0.8).clamp(min=0.01)
        vel = m * vel - lr * gains * grad
        y = y + vel
    return y - y.mean(dim=0, keepdim=True), kls, float(kl_ref(Pd.double(), y))


def one_nn_agreement(y, labels):
    """the share of points whose nearest other point in the plane carries their label"""
    y = y.double().cpu()
    d = torch.cdist(y, y)
    d.fill_diagonal_(float("inf"))
    return (labels[d.argmin(dim=1)] == labels).double().mean().item()


def planted_map_case(dtype_seed=0):
    """The planted set of the map tests: N = 600 rows around C = 3 random unit directions in D = 64, noise 0.5 / sqrt(D) per
    coordinate, shuffled.  Returns (features fp32 [600, 64], labels int64 [600])."""
    import kmeans_ref
    feats, truth, _ = kmeans_ref.planted([200, 200, 200], 64, 0.5, 77 + dtype_seed)
    return feats, truth
