"""Float64 restatement of the row-sampling contract (include/cclip_hip.h, cclip_sample_rows; csrc/sample_rows.hip's header):
numpy only, no device.  `sample_rows_ref` gives, per row, what the acceptance checks of tests/test_sample_rows_gpu.py are
written against - the exact order, the float64 probabilities and the float64 mass ahead of every token of that order - and
`draw_ref` applies the draw rule to it."""
import numpy as np


class RowRef:
    """One row: order (token ids by (logit descending, id ascending)), p (float64 softmax(logits * inv_t), indexed by id),
    ahead (float64, indexed by rank: the mass of the tokens strictly ahead of the token at that rank), k (min(top_k or V, V))."""

    def __init__(self, order, p, ahead, k, top_p):
        self.order, self.p, self.ahead, self.k, self.top_p = order, p, ahead, k, top_p

    def n_kept(self, top_p=None):
        """size of the kept set: ranks r < k with ahead[r] <= top_p (a prefix: ahead never decreases; rank 0 has ahead 0)"""
        top_p = self.top_p if top_p is None else top_p
        return max(1, int(min(self.k, np.searchsorted(self.ahead, top_p, side="right"))))

    def kept(self, n=None):
        """ids of the first n (default: n_kept()) tokens of the order, ascending"""
        return np.sort(self.order[:self.n_kept() if n is None else n])


def sample_rows_ref(logits, inv_t, top_k, top_p):
    """logits: [n, V] array of fp32 values.  inv_t is taken as the fp32 number the kernel receives."""
    logits = np.asarray(logits, dtype=np.float32)
    inv_t = float(np.float32(inv_t))
    out = []
    for row in logits:
        V = row.shape[0]
        order = np.lexsort((np.arange(V), -row.astype(np.float64)))      # primary: logit descending (-0 == +0); then id ascending
        z = row.astype(np.float64) * inv_t
        z = z - z[np.isfinite(z)].max()
        e = np.exp(z)                                                     # exp(-inf) = 0
        p = e / e.sum()
        inc = np.cumsum(p[order])
        ahead = np.concatenate(([0.0], inc[:-1]))
        out.append(RowRef(order, p, ahead, V if top_k <= 0 or top_k >= V else int(top_k), float(top_p)))
    return out


def draw_ref(ref: RowRef, u: float, n=None):
    """(token, Z, C_excl, C_incl): walk the kept ids ascending; the first whose running kept mass exceeds u * Z, else the last"""
    ids = ref.kept(n)
    c = np.cumsum(ref.p[ids])
    Z = c[-1]
    at = int(np.searchsorted(c, u * Z, side="right"))
    at = min(at, len(ids) - 1)
    return int(ids[at]), Z, (c[at - 1] if at else 0.0), c[at]


FREQ_ROWS, FREQ_SEED = 8192, 2024


def frequency_case():
    """The frequency test's inputs: one seeded 64-token distribution (logits N(0, 1.5^2)) and FREQ_ROWS uniforms from a CPU
    generator (so the same numbers exist without a device).  Returns (logits fp32 [64], u fp32 [FREQ_ROWS], p float64 [64])."""
    import torch
    g = torch.Generator().manual_seed(FREQ_SEED)
    logits = (torch.randn(64, generator=g) * 1.5).numpy()
    u = torch.rand(FREQ_ROWS, generator=g).numpy()
    return logits, u, sample_rows_ref(logits[None], 1.0, 0, 1.0)[0].p


def frequency_bound_ok(counts, p, rows=FREQ_ROWS, sigmas=5.0):
    """every token's count within `sigmas` binomial standard deviations of rows * p"""
    dev = np.abs(np.asarray(counts, dtype=np.float64) - rows * p) / np.sqrt(rows * p * (1 - p))
    return bool((dev <= sigmas).all()), float(dev.max())
