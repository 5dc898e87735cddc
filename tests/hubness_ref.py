"""The float64 reference of the hubness correction (clip/hubness.py, csrc/embed_hub.hip, cclip_similarity_topk_biased) and the
planted-hub fixture its tests share.  Plain torch on the CPU; everything takes the 16-bit rows the kernels take, as float64.

  * `scores`, `bank_lse`: s[b, j] = <bank[b], g[j]> and lse[j] = log sum_b exp(beta s[b, j]).
  * `topk_biased`: the top-k of t = scale s + bias[n], keyed as the kernel keys - higher t first, equal t by the lower index,
    NaN last (-inf before NaN).
  * `fit` / `search`: the composition of the three methods ("is", "dis", "csls") as clip.fit_querybank / EmbeddingIndex.search
    compose them, with the gate of "dis".
  * `planted_hubs`: unit rows in D = 64, 256 query / gallery pairs that share one direction h on the query side only, a bank
    of 256 typical queries, and 4 hub rows near h appended to the gallery.  Raw cosine ranks a hub first for about 40 % of the
    queries; each of the three methods removes them.
"""
import math

import torch

F64 = torch.float64
BETA, CSLS_K = 20.0, 10          # the defaults of clip.fit_querybank


def round16(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float rows -> rounded once to the 16-bit `dtype` -> float64 (what the kernel's operands hold)"""
    return x.to(torch.float32).to(dtype).to(F64)


def scores(a: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    return a.to(F64) @ g.to(F64).T


def bank_lse(g: torch.Tensor, bank: torch.Tensor, beta: float) -> torch.Tensor:
    """[N]: log sum_b exp(beta <bank[b], g[j]>) with beta rounded to fp32, as the entry takes it"""
    beta = float(torch.tensor(beta, dtype=torch.float32))
    return torch.logsumexp(beta * scores(bank, g), dim=0)


def order_keys(t: torch.Tensor) -> torch.Tensor:
    """[Q, N] permutation per row: higher t first, equal t by the lower index, NaN last (behind -inf).  Two stable sorts, the
    less significant first: numbers before NaN (each in index order), then descending by t with NaN counted as -inf - among
    equal values a stable sort keeps the earlier, so a genuine -inf stays ahead of every NaN."""
    nan = torch.isnan(t)
    first = torch.argsort(nan.to(torch.int8), dim=1, stable=True)
    key = torch.gather(torch.where(nan, torch.full_like(t, -math.inf), t), 1, first)
    return torch.gather(first, 1, torch.argsort(key, dim=1, descending=True, stable=True))


def topk_biased(q: torch.Tensor, g: torch.Tensor, k: int, bias: torch.Tensor, scale: float = 1.0):
    """(t [Q, k] float64, index [Q, k] int64, full t [Q, N]) of t = scale s + bias[n]"""
    t = float(scale) * scores(q, g) + bias.to(F64)[None, :]
    order = order_keys(t)[:, :k]
    return torch.gather(t, 1, order), order, t


def kth_gap(t: torch.Tensor, k: int) -> torch.Tensor:
    """[Q]: the reference's own gap between its k-th and (k+1)-th t (inf where there is no (k+1)-th)"""
    if k >= t.shape[1]:
        return torch.full((t.shape[0],), math.inf, dtype=F64)
    s = torch.gather(t, 1, order_keys(t)[:, :k + 1])
    return s[:, k - 1] - s[:, k]


class RefBank:
    def __init__(self, method, scale, bias, active):
        self.method, self.scale, self.bias, self.active = method, scale, bias, active


def fit(g: torch.Tensor, bank: torch.Tensor, method: str = "dis", beta: float = BETA, k: int = CSLS_K, activation_k: int = 1) -> RefBank:
    N, B = g.shape[0], bank.shape[0]
    active = torch.ones(N, dtype=torch.bool)
    if method in ("is", "dis"):
        bias = -bank_lse(g, bank, beta)
        scale = float(torch.tensor(beta, dtype=torch.float32))
        if method == "dis":
            idx = order_keys(scores(bank, g))[:, :min(activation_k, N)]
            active = torch.zeros(N, dtype=torch.bool)
            active[idx.reshape(-1)] = True
    elif method == "csls":
        kk = min(k, B)
        s = scores(g, bank)                                          # [N, B]
        bias = -torch.gather(s, 1, order_keys(s)[:, :kk]).mean(dim=1)
        scale = 2.0
    else:
        raise ValueError(method)
    return RefBank(method, scale, bias, active)


def search(q: torch.Tensor, g: torch.Tensor, k: int, qb: RefBank = None, mask: torch.Tensor = None):
    """(t [Q, k], index [Q, k], gate [Q], raw full scores [Q, N], adjusted full t [Q, N]) - mask True = the row is left out"""
    N = g.shape[0]
    drop = torch.zeros(N, dtype=F64) if mask is None else torch.where(mask, torch.tensor(-math.inf, dtype=F64), torch.tensor(0.0, dtype=F64))
    raw_s, raw_i, raw_t = topk_biased(q, g, k, drop, 1.0)
    if qb is None:
        return raw_s, raw_i, torch.zeros(q.shape[0], dtype=torch.bool), raw_t, raw_t
    adj_s, adj_i, adj_t = topk_biased(q, g, k, qb.bias + drop, qb.scale)
    gate = qb.active[raw_i[:, 0]]
    return (torch.where(gate[:, None], adj_s, raw_s), torch.where(gate[:, None], adj_i, raw_i), gate, raw_t, adj_t)


def hubness_counts(indices: torch.Tensor, n: int):
    """(counts [n] int64, skewness, share of never-retrieved rows)"""
    c = torch.bincount(indices.reshape(-1).long(), minlength=n).to(F64)
    mu, sd = c.mean(), c.std(unbiased=False)
    skew = float(((c - mu) ** 3).mean() / sd ** 3) if sd > 0 else 0.0
    return c.long(), skew, float((c == 0).to(F64).mean())


# ---- the planted-hub fixture ------------------------------------------------------------------------------------------
HUB_D, HUB_PAIRS, HUB_BANK, HUB_HUBS = 64, 256, 256, 4


def _norm(x):
    return x / x.norm(dim=1, keepdim=True)


def planted_hubs(seed: int):
    """(queries [256, 64], gallery [260, 64], bank [256, 64]) float64 unit rows; query i pairs with gallery row i, the gallery
    rows 256 .. 259 are the hubs."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=F64)
    D, P = HUB_D, HUB_PAIRS
    u = _norm(rn(P, D))
    h = _norm(rn(1, D))
    gallery = _norm(u + 0.05 * rn(P, D))
    queries = _norm(u + 0.9 * h + 0.05 * rn(P, D))
    bank = _norm(_norm(rn(HUB_BANK, D)) + 0.9 * h + 0.05 * rn(HUB_BANK, D))
    hubs = _norm(h + 0.3 * _norm(rn(HUB_HUBS, D)))
    return queries, torch.cat([gallery, hubs]), bank


def score_tol(D: int) -> float:
    """What the fp32 MFMA chain can move the score of two unit rows by: D 2^-24 sum_d |a_d b_d| <= D 2^-24"""
    return D * 2.0 ** -24


def adjusted_tol(method: str, D: int, B: int, beta: float = BETA) -> float:
    """The same for the adjusted value t = scale s + bias: the scaled score, plus the bias' own error - for the log-sum-exp the
    kernel's ceiling beta D 2^-24 + (B + 64) 2^-23 (csrc/embed_hub.hip), for CSLS one score's error and the fp32 mean's rounding"""
    if method == "csls":
        return 3 * score_tol(D) + 2.0 ** -22
    return 2 * beta * score_tol(D) + (B + 64) * 2.0 ** -23


def recall_at_1(index: torch.Tensor) -> float:
    return float((index[:, 0].cpu() == torch.arange(index.shape[0])).to(F64).mean())


# ---- the random cases of the biased top-k tests (CPU and GPU share them) -----------------------------------------------
TOPK_TWO_SPLIT_N = 257           # the smallest gallery cclip_similarity_topk cuts in two (a split keeps at least 256 rows)
# (Q, N, k, D): Q in {1, 17, 65}, N in {k, 63, 65, two splits}, k in {1, 7, 64}, D in {32, 160, 1024}, each value in three cases
TOPK_CASES = [(1, 1, 1, 32), (1, 7, 7, 160), (17, 64, 64, 1024), (17, 63, 7, 32), (65, 65, 64, 160), (65, TOPK_TWO_SPLIT_N, 7, 1024),
              (1, TOPK_TWO_SPLIT_N, 64, 32), (17, TOPK_TWO_SPLIT_N, 1, 160), (65, 63, 1, 1024), (17, 65, 7, 32)]
TOPK_SCALE = 1.5
# seeds are chosen so that the reference's own k-th / (k+1)-th gap stays above 2 x topk_tol for every query (test_hubness_cpu
# checks it): the case whose plain seed left queries out draws from another one
TOPK_SEED_SALT = {(65, TOPK_TWO_SPLIT_N, 7, 1024): 4}


def topk_case(Q: int, N: int, k: int, D: int, dtype: torch.dtype):
    """(q16 [Q, D], g16 [N, D], bias fp32 [N]) of a random case: unit rows rounded to `dtype`, a bias of the size of the scores"""
    gen = torch.Generator().manual_seed(7919 * D + 31 * N + 7 * Q + k + 1000003 * TOPK_SEED_SALT.get((Q, N, k, D), 0))
    q = _norm(torch.randn(Q, D, generator=gen, dtype=F64)).to(torch.float32).to(dtype)
    g = _norm(torch.randn(N, D, generator=gen, dtype=F64)).to(torch.float32).to(dtype)
    bias = (0.1 * torch.randn(N, generator=gen, dtype=F64)).to(torch.float32)
    return q, g, bias


def topk_tol(q16: torch.Tensor, g16: torch.Tensor, bias: torch.Tensor, scale: float) -> float:
    """What t = fmaf(scale, s, bias) can differ from float64 by: the chain's D 2^-24 sum_d |q_d g_d| on s, scaled, and the one
    rounding of the fma, 2^-24 of the largest |t|"""
    D = q16.shape[1]
    mag = float((q16.to(F64).abs() @ g16.to(F64).abs().T).max())
    tmax = abs(scale) * mag + float(bias.abs().max())
    return abs(scale) * D * 2.0 ** -24 * mag + 2.0 ** -24 * tmax
