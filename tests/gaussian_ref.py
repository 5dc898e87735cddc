"""float64 numpy reference of the Gaussian class models (clip/gaussian.py, csrc/embed_moments.hip, csrc/gauss_scores.hip):
moments of 16-bit rows, both shrinkage rules, the whitening, the hi + lo pair of an fp32 matrix as include/cclip_hip.h defines
it, z / d2 / score / lse / argmax / argmin, and pca.  No GPU, no product code."""
import numpy as np
import torch


def rows16(N, D, seed, dtype, unit=True):
    """N x D rows rounded to the 16-bit dtype (torch CPU tensor)"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, D))
    if unit:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return torch.from_numpy(x).to(dtype)


def rows64(x16):
    return x16.detach().cpu().double().numpy()


def round16(a, dtype):
    """float64 array -> the values of its round-to-nearest-even 16-bit image, through fp32 as the kernel rounds"""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype).double().numpy()


def pair16(T32, dtype):
    """hi = round16(T), lo = round16(T - hi) with T - hi taken in fp32: the header's pair.  Returns (hi, lo) as float64."""
    T32 = np.asarray(T32, dtype=np.float32)
    hi = round16(T32, dtype)
    lo = round16((T32 - hi.astype(np.float32)).astype(np.float32), dtype)
    return hi, lo


def moments64(X, labels, C):
    """(count int64 [C], sum [C, D], gram [D, D]) of the float64 rows; a label outside [0, C) drops the row"""
    X = np.asarray(X, dtype=np.float64)
    y = np.zeros(len(X), dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    live = (y >= 0) & (y < C)
    Xl, yl = X[live], y[live]
    count = np.bincount(yl, minlength=C).astype(np.int64)
    s = np.zeros((C, X.shape[1]))
    np.add.at(s, yl, Xl)
    return count, s, Xl.T @ Xl


def scatter64(count, s, gram):
    mean = s / np.maximum(count, 1)[:, None]
    return gram - (mean * count[:, None]).T @ mean


def covariance64(count, s, gram, shrinkage):
    """the shrunk covariance: "auto" (Wang et al.: precision = D ((N - 1) S + tr S I)^-1) or a float lam"""
    N, C, D = float(count.sum()), len(count), gram.shape[0]
    S = scatter64(count, s, gram) / (N - C if N > C else max(N, 1.0))
    S = (S + S.T) / 2
    tr = np.trace(S)
    if isinstance(shrinkage, str):
        assert shrinkage == "auto"
        return ((N - 1.0) * S + tr * np.eye(D)) / D
    lam = float(shrinkage)
    if lam == 0.0 and np.linalg.eigvalsh(S)[0] <= np.linalg.eigvalsh(S)[-1] * D * 2.3e-16:
        raise ValueError(f"singular covariance at N = {int(N)}, C = {C}, D = {D}")
    return (1.0 - lam) * S + lam * tr / D * np.eye(D)


def whitening64(sigma):
    """T = Lambda^(-1/2) U^T, log det sigma, the condition number"""
    ev, U = np.linalg.eigh(sigma)
    return U.T / np.sqrt(ev)[:, None], float(np.log(ev).sum()), float(ev[-1] / ev[0])


def fit64(X, labels, C, shrinkage="auto", priors="empirical"):
    """what GaussianClassifier keeps, float64 and its fp32 casts: dict(T, t0, centres, offset, log_det, cond, sigma, mean)"""
    count, s, gram = moments64(X, labels, C)
    sigma = covariance64(count, s, gram, shrinkage)
    T, log_det, cond = whitening64(sigma)
    mean = s.sum(0) / max(count.sum(), 1)
    cm = s / np.maximum(count, 1)[:, None]
    with np.errstate(divide="ignore"):
        prior = np.log(count / count.sum()) if priors == "empirical" else np.full(C, -np.log(C))
    return dict(T=T, t0=T @ mean, centres=(cm - mean) @ T.T, offset=prior, log_det=log_det, cond=cond, sigma=sigma, mean=mean,
                class_mean=cm, count=count,
                T32=T.astype(np.float32), t032=(T @ mean).astype(np.float32), centres32=((cm - mean) @ T.T).astype(np.float32),
                offset32=prior.astype(np.float32))


def scores64(X, T32, dtype, t0=None, centres=None, offset=None):
    """float64 arithmetic on the kernel's operands: the 16-bit rows X (float64 values), the hi + lo pair of the fp32 T, the
    fp32 t0 / centres / offset.  dict(z, zmag, d2, score, lse, pred, nearest, dmin)"""
    hi, lo = pair16(T32, dtype)
    Tp = hi + lo
    z = X @ Tp.T
    zmag = np.abs(X) @ np.abs(Tp).T
    if t0 is not None:
        t0 = np.asarray(t0, dtype=np.float64)
        z = z - t0
        zmag = zmag + np.abs(t0)
    out = dict(z=z, zmag=zmag)
    if centres is None:
        return out
    m = np.asarray(centres, dtype=np.float64)
    d2 = np.stack([((z - mc) ** 2).sum(1) for mc in m], axis=1)
    off = np.zeros(len(m)) if offset is None else np.asarray(offset, dtype=np.float64)
    score = -0.5 * d2 + off
    mx = score.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(score - mx).sum(1, keepdims=True)))[:, 0]
    out.update(d2=d2, score=score, lse=lse, pred=score.argmax(1), nearest=d2.argmin(1), dmin=d2.min(1))
    return out


def top_two_gap(a, largest=True):
    """per row: the gap between the best and the second best entry (inf with one column)"""
    if a.shape[1] < 2:
        return np.full(len(a), np.inf)
    s = np.sort(a, axis=1)
    return s[:, -1] - s[:, -2] if largest else s[:, 1] - s[:, 0]


def outside_margin(ref, tol):
    """(keep_pred, keep_nearest): the rows whose float64 top-two gap exceeds twice the tolerance of the quantity, the tolerance
    of a d2 being tol * d2 and of a score half that.  nearest: the two smallest d2, s0 <= s1, differ by more than 2 tol s1;
    pred: the two best scores differ by more than 2 * 0.5 tol * the larger d2 of those two classes."""
    d2, score = ref["d2"], ref["score"]
    if d2.shape[1] < 2:
        return np.ones(len(d2), dtype=bool), np.ones(len(d2), dtype=bool)
    s = np.sort(d2, axis=1)
    keep_n = s[:, 1] - s[:, 0] > 2 * tol * s[:, 1]
    order = np.argsort(-score, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(d2))
    gap = score[rows, order[:, 0]] - score[rows, order[:, 1]]
    keep_p = gap > 2 * 0.5 * tol * np.maximum(d2[rows, order[:, 0]], d2[rows, order[:, 1]])
    return keep_p, keep_n


def pca64(X, k, center=True):
    """dict(mean, components [k, D], explained_variance, explained_variance_ratio) from the Gram matrix, float64 eigh,
    descending, each component's largest-magnitude entry positive"""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    mean = X.mean(0) if center else np.zeros(D)
    cov = (X.T @ X - N * np.outer(mean, mean)) / (N - 1)
    ev, U = np.linalg.eigh((cov + cov.T) / 2)
    var = np.maximum(ev[::-1][:k], 0.0)
    comp = U[:, ::-1].T[:k].copy()
    big = np.abs(comp).argmax(1)
    sign = np.sign(comp[np.arange(k), big])
    comp *= np.where(sign == 0, 1.0, sign)[:, None]
    return dict(mean=mean, components=comp, explained_variance=var, explained_variance_ratio=var / np.trace(cov))


def planted(N, C, D, seed, dtype, sep=4.0, cone=3.0, scale=0.05):
    """Planted Gaussian classes with a shared anisotropic covariance around a dominant common direction (the embedding cone):
    class means `sep` whitened units apart.  Returns (x16 torch CPU [N, D] unit rows of `dtype`, labels int64 [N])."""
    g = np.random.default_rng(seed)
    A = g.standard_normal((D, D)) / np.sqrt(D) * np.geomspace(1.0, 0.2, D)[None, :]         # the shared covariance's root
    mus = g.standard_normal((C, D)) @ A.T * sep / np.sqrt(2.0)
    y = np.arange(N) % C
    x = cone * np.ones(D) / np.sqrt(D) + scale * (mus[y] + g.standard_normal((N, D)) @ A.T)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return torch.from_numpy(x).to(dtype), y.astype(np.int64)
