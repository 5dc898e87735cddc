"""Float64 restatement of the caption-selection contract (include/cclip_hip.h, cclip_caption_select; csrc/caption_select.hip's
header): numpy only, no device.  `caption_select_ref` gives what tests/test_caption_select_gpu.py and
tests/test_captioner_best_of_gpu.py compare the device against, `cos_bound` and `bounds` the derived error bounds, and
`check_outputs` applies the comparison rule (values within their bounds; the order equal wherever two scores are further apart
than twice the bound, exact ties lower index first)."""
import numpy as np

U = 2.0 ** -24                                    # unit roundoff of fp32


def _cos(a, b):
    """cosine of every row of a [.., E] with the matching row of b, 0 when either norm is 0"""
    na, nb = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1))
    den = na * nb
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((na == 0) | (nb == 0), 0.0, (a * b).sum(-1) / np.where(den == 0, 1.0, den))


class SelectRef:
    """cos, clip_score, rmax, ref_score (None without references), score: float64 [N, K]; order [N, K], best [N]."""

    def __init__(self, cos, clip_score, rmax, ref_score, score, order):
        self.cos, self.clip_score, self.rmax, self.ref_score, self.score, self.order = cos, clip_score, rmax, ref_score, score, order
        self.best = order[:, 0]


def order_ref(score):
    """[N, K] scores -> the candidates of every row by (score descending, k ascending); -0 == +0"""
    score = np.asarray(score, dtype=np.float64) + 0.0
    K = score.shape[1]
    return np.stack([np.lexsort((np.arange(K), -row)) for row in score]).astype(np.int64)


def caption_select_ref(img, txt, K, lm_mean=None, ref=None, ref_off=None, w=2.5, lm_weight=0.0):
    """img [N, E], txt [N * K, E], ref [Rtot, E]: arrays of fp32 values; w and lm_weight are taken as the fp32 numbers the
    kernel receives.  Everything else in float64."""
    img = np.asarray(img, dtype=np.float32).astype(np.float64)
    txt = np.asarray(txt, dtype=np.float32).astype(np.float64)
    N, E = img.shape
    assert txt.shape == (N * K, E)
    w, lm_weight = float(np.float32(w)), float(np.float32(lm_weight))
    t = txt.reshape(N, K, E)
    cos = _cos(img[:, None, :], t)
    cs = w * np.maximum(cos, 0.0)
    rmax, rs = np.zeros((N, K)), None
    if ref is not None:
        ref = np.asarray(ref, dtype=np.float32).astype(np.float64)
        assert len(ref_off) == N + 1
        for n in range(N):
            rows = ref[ref_off[n]:ref_off[n + 1]]
            if len(rows):
                rmax[n] = np.maximum(0.0, _cos(t[n][:, None, :], rows[None, :, :]).max(axis=1))
        den = cs + rmax
        rs = np.where(den == 0, 0.0, 2.0 * cs * rmax / np.where(den == 0, 1.0, den))
    score = cos.copy()
    if lm_mean is not None:
        score = cos + lm_weight * np.asarray(lm_mean, dtype=np.float32).astype(np.float64).reshape(N, K)
    return SelectRef(cos, cs, rmax, rs, score, order_ref(score))


def cos_bound(E):
    """|cos_device - cos_exact|: a lane adds E / 256 float4 products (at most E / 64 terms) one after the other and six
    butterfly levels follow, so each of the dot and the two squared norms errs by at most (E / 64 + 6) u of sum |a_i b_i| <=
    |a| |b|.  The dot contributes (E / 64 + 6) u; each norm enters as a square root (half its relative error) and there are
    two, another (E / 64 + 6) u on |cos| <= 1; the two square roots, their product and the division round four more times.
    2 (E / 64 + 6) u + 4 u <= 4 (E / 64 + 8) u, the bound the kernel's header and DESIGN.md section 6.14 state."""
    return 4.0 * (E / 64.0 + 8.0) * U


def bounds(ref: SelectRef, E, w=2.5, lm_mean=None, lm_weight=0.0):
    """per-element bounds (cos, clip_score, ref_score, score) propagated from cos_bound through the formulas:
    clip_score = w max(cos, 0): |w| b plus one rounding of the product.
    ref_score = h(a, m) = 2 a m / (a + m), a = clip_score within da, m = rmax within b: both partial derivatives of h lie in
      [0, 2], so |dh| <= 2 (da + b); the sum, two products and the division round four more times (relative to h).
    score = cos + lm_weight lm_mean: b, plus one rounding of the product and one of the sum."""
    b = cos_bound(E)
    w = abs(float(np.float32(w)))
    d_cs = w * b + U * (np.abs(ref.clip_score) + w * b)
    d_rs = None
    if ref.ref_score is not None:
        d_rs = 2.0 * (d_cs + b) + 4.0 * U * (np.abs(ref.ref_score) + 2.0 * (d_cs + b))
    d_sc = np.full_like(ref.cos, b)
    if lm_mean is not None:
        term = np.abs(float(np.float32(lm_weight)) * np.asarray(lm_mean, dtype=np.float64).reshape(ref.cos.shape))
        d_sc = b + U * term + U * (np.abs(ref.score) + b)
    return np.full_like(ref.cos, b), d_cs, d_rs, d_sc


def close_pairs(ref: SelectRef, d_sc):
    """the pairs (n, j, k), j < k, whose float64 scores differ by no more than the sum of their bounds (<= twice the larger):
    their device order is not determined by the float64 order.  Exact float64 ties (duplicated rows) are listed too."""
    out = []
    N, K = ref.score.shape
    for n in range(N):
        for j in range(K):
            for k in range(j + 1, K):
                if abs(ref.score[n, j] - ref.score[n, k]) <= 2.0 * max(d_sc[n, j], d_sc[n, k]):
                    out.append((n, j, k))
    return out


def check_outputs(ref: SelectRef, E, got, w=2.5, lm_mean=None, lm_weight=0.0, ties=()):
    """got = (cos, clip_score, ref_score or None, score, order, best) as numpy arrays.  Every value within its bound; `order` a
    permutation that puts j ahead of k wherever the float64 score of j exceeds k's by more than twice the bound; the pairs of
    `ties` [(n, j, k), j < k: duplicated rows] in index order.  Returns (max error / bound per output, pairs left undetermined)."""
    cos, cs, rs, sc, order, best = [None if g is None else np.asarray(g) for g in got]
    b_cos, b_cs, b_rs, b_sc = bounds(ref, E, w, lm_mean, lm_weight)
    ratios = {}
    for name, g, r, b in (("cos", cos, ref.cos, b_cos), ("clip_score", cs, ref.clip_score, b_cs),
                          ("ref_score", rs, ref.ref_score, b_rs), ("score", sc, ref.score, b_sc)):
        assert (g is None) == (r is None), name
        if r is None:
            continue
        err = np.abs(g.astype(np.float64) - r)
        ratios[name] = float((err / b).max())
        assert (err <= b).all(), (name, float(err.max()), float(np.min(b)), ratios[name])
    N, K = ref.score.shape
    assert order.shape == (N, K) and best.shape == (N,)
    assert (np.sort(order, axis=1) == np.arange(K)[None]).all(), "order is not a permutation"
    assert (best == order[:, 0]).all()
    rank = np.argsort(order, axis=1)                                     # rank[n, k] = place of candidate k
    loose = 0
    ties = {tuple(t) for t in ties}
    for n in range(N):
        for j in range(K):
            for k in range(j + 1, K):
                gap = ref.score[n, j] - ref.score[n, k]
                if (n, j, k) in ties:
                    assert sc[n, j] == sc[n, k] and rank[n, j] < rank[n, k], ("tie not in index order", n, j, k)
                elif abs(gap) > 2.0 * max(b_sc[n, j], b_sc[n, k]):
                    assert (rank[n, j] < rank[n, k]) == (gap > 0), ("order", n, j, k, gap)
                else:
                    loose += 1
    return ratios, loose
