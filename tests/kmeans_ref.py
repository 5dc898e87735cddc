"""float64 reference of spherical k-means on the same 16-bit operands (csrc/embed_kmeans.hip, clip/cluster.py), and the
tolerances its tests use.  Pure torch on the host; needs no library.

Tolerances (derived, none measured; u = 2^-24, the unit roundoff of fp32):

assign.  Products of two 16-bit operands are exact in fp32, so only the D - 1 additions round: sequentially D u |x| |c|, and
  assign_tol = D 2^-22 max|x| max|c| leaves a factor 4 for the MFMA's internal summation order (test_retrieval_gpu.py's bound).

update, three parts.
  1. The fp32 sum.  Converting a 16-bit value to fp32 is exact.  Any order of adding n numbers in fp32 errs by at most
     gamma_h sum|x| with h the longest chain of additions a term passes through; h <= n - 1 always, and the kernel's order
     (<= 64 sequential per stream, <= 63 streams, n / 256 + 1 slabs) keeps h far below n for the large clusters, so
         delta_d <= n_k u sum_n |x_nd|                                       per column d
     (for n <= 4096, gamma_{n-1} <= n u holds as it stands; above, h <= 128 + n / 256 < n / 2).
  2. Norm, scale, divide in fp32.  |S^| differs from |S| by at most |delta|_2.  Its computed value carries one rounding per
     square, at most 12 per column chain of the fixed tree (3 in the thread, 6 in the butterfly, 3 across waves) and the
     square root's: relative (13 u) / 2 + u < 8 u to first order; 16 u is used.  So
         norm_tol = |delta|_2 + 16 u (|S| + |delta|_2)
     and with eta = norm_tol / |S| (the reference asserts eta < 1/2) and one more rounding u for the division
         f32_tol_d = ( delta_d / |S| + |c_d| (eta + u) ) / (1 - eta)
     bounds the distance of the kernel's fp32 quotient from the float64 c_d = S_d / |S|.
  3. One rounding to the 16-bit type: round-to-nearest-even is monotone, so the kernel's output lies between
     round16(c_d - f32_tol_d) and round16(c_d + f32_tol_d).  Where the two agree the output is decided exactly; where they
     differ ("the band": c_d lies within f32_tol_d of a rounding boundary) they are at most neighbours as long as
     2 f32_tol_d is below the spacing, and either may come out.
"""
import torch

U = 2.0 ** -24
P16 = {torch.bfloat16: (8, -125), torch.float16: (11, -13)}     # significand bits; torch.frexp exponent of the smallest normal


def round16(v64, dtype):
    """float64 -> the 16-bit type, rounded ONCE to nearest-even (a cast through fp32 would round twice)"""
    p, emin = P16[dtype]
    _, e = torch.frexp(v64)
    ulp = torch.ldexp(torch.ones_like(v64), e.clamp(min=emin) - p)
    return (torch.round(v64 / ulp) * ulp).to(dtype)


def assign_tol(D, x16, c16):
    return D * 2.0 ** -22 * x16.double().norm(dim=1).max().item() * c16.double().norm(dim=1).max().item()


def scores64(x16, c16):
    return x16.double() @ c16.double().t()


def assign_ref(x16, c16):
    """(assign int64 [N], best, second float64 [N]) under the kernel's order: NaN below every number, equal scores to the
    lower centroid; second = the second-largest score (NaN if K == 1)"""
    s = scores64(x16, c16)
    K = s.shape[1]
    nan = torch.isnan(s)
    by_score = torch.sort(torch.where(nan, torch.full_like(s, -float("inf")), s), dim=1, descending=True, stable=True).indices
    numbers_first = torch.sort(torch.gather(nan, 1, by_score).to(torch.uint8), dim=1, stable=True).indices   # -inf stays above NaN
    idx = torch.gather(by_score, 1, numbers_first)[:, :2]
    best = torch.gather(s, 1, idx[:, :1])[:, 0]
    second = torch.gather(s, 1, idx[:, 1:2])[:, 0] if K > 1 else torch.full_like(best, float("nan"))
    return idx[:, 0].clone(), best, second


def update_ref(x16, assign, K, prev16):
    """float64 centroid step.  Returns a dict: S [K, D] sums, norm [K], c [K, D] float64 unit rows (prev for the kept ones),
    keep bool [K] (empty, or |S| == 0), counts int64 [K], and the bounds delta [K, D], norm_tol [K], f32_tol [K, D]."""
    x = x16.double()
    N, D = x.shape
    assign = assign.long()
    counts = torch.bincount(assign, minlength=K)
    S = torch.zeros(K, D, dtype=torch.float64).index_add_(0, assign, x)
    A = torch.zeros(K, D, dtype=torch.float64).index_add_(0, assign, x.abs())
    norm = S.norm(dim=1)
    keep = (counts == 0) | (norm == 0)
    delta = counts[:, None].double() * U * A
    dn = delta.norm(dim=1)
    norm_tol = dn + 16 * U * (norm + dn)
    safe = torch.where(keep, torch.ones_like(norm), norm)
    eta = norm_tol / safe
    c = torch.where(keep[:, None], prev16.double(), S / safe[:, None])
    f32_tol = (delta / safe[:, None] + c.abs() * (eta + U)[:, None]) / (1 - eta.clamp(max=0.5))[:, None]
    return dict(S=S, norm=torch.where(keep, torch.zeros_like(norm), norm), c=c, keep=keep, counts=counts, delta=delta,
                norm_tol=norm_tol, f32_tol=f32_tol, eta=eta)


def update_ref16(x16, assign, K, prev16):
    """the float64 centroid step with its unit rows rounded once to the operands' type (what a next iteration sees)"""
    r = update_ref(x16, assign, K, prev16)
    c16 = round16(r["c"], x16.dtype)
    c16[r["keep"]] = prev16[r["keep"]]
    return c16, r


def lloyd_ref(x16, c16, max_iter=50, tol=0.0, reseed_empty=True):
    """clip.cluster's loop in float64 (centroids rounded to the 16-bit type between iterations, as the device's are).  Returns
    a dict with the final fields and `history`: per iteration (assign, best, second, counts, objective)."""
    N, K = x16.shape[0], c16.shape[0]
    prev, n_iter, converged, history = None, 0, False, []
    c = c16.clone()
    while True:
        assign, best, second = assign_ref(x16, c)
        n_iter += 1
        c_new, r = update_ref16(x16, assign, K, c)
        history.append(dict(assign=assign, best=best, second=second, counts=r["counts"], objective=best.mean().item(), centroids=c))
        changed = int((assign != prev).sum()) if prev is not None else N
        if prev is not None and changed <= tol * N:
            converged = True
            break
        if n_iter >= max_iter:
            break
        empty = torch.nonzero(r["counts"] == 0).flatten()
        if empty.numel() and reseed_empty:
            worst = torch.sort(best, stable=True).indices[:empty.numel()]
            c_new[empty] = x16[worst]
        c, prev = c_new, assign
    counts = r["counts"]
    conc = torch.where(counts > 0, r["norm"] / counts.clamp(min=1).double(), torch.zeros_like(r["norm"]))
    return dict(centroids=c, labels=assign, scores=best, margin=best - second, counts=counts, concentration=conc,
                objective=best.mean().item(), n_iter=n_iter, converged=converged, history=history)


def planted(sizes, D, noise, seed):
    """Planted clusters: len(sizes) random unit directions in D dimensions, sizes[j] rows around direction j (direction +
    noise / sqrt(D) randn, re-normalised), shuffled.  Returns (features fp32 [N, D], truth int64 [N], directions [k, D])."""
    gen = torch.Generator().manual_seed(seed)
    dirs = torch.randn(len(sizes), D, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    truth = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = dirs[truth] + noise / D ** 0.5 * torch.randn(truth.numel(), D, generator=gen)
    x = x / x.norm(dim=1, keepdim=True)
    perm = torch.randperm(truth.numel(), generator=gen)
    return x[perm], truth[perm], dirs


def same_partition(a, b):
    """two labelings describe one partition (up to renaming)"""
    a, b = torch.as_tensor(a).long(), torch.as_tensor(b).long()
    pairs = torch.unique(torch.stack([a, b], dim=1), dim=0)
    return pairs.shape[0] == torch.unique(a).numel() == torch.unique(b).numel()
