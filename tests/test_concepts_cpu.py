"""CPU: the float64 reference of the concept codes (tests/concepts_ref.py) pinned by facts that do not depend on it - the KKT
conditions, closed forms, planted recovery -, its fp32 restatement against it, and the host logic of clip.decompose through a
CPU stand-in for the ops it calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concepts_ref as R  # noqa: E402

# the correlated dictionary of the planted test: normalise(SHARED * s + noise).  The issue's 0.8 was checked with the float64
# reference first: with both sides centred it recovers 16 of 16 rows at (V, D) = (200, 64), l1 = 0.1, so 0.8 is used as stated
# (at l1 = 0.05 it does not, at any correlation from 0.3 to 0.8: a centred row is no longer an exact pair of centred concepts,
# and the weaker penalty lets a third concept take up the difference).
SHARED = 0.8


def _problem(N, V, D, seed, dtype=torch.bfloat16):
    X, C = R.rows64(R.unit_rows16(N, D, seed, dtype)), R.rows64(R.unit_rows16(V, D, seed + 1000, dtype))
    return X, C, 1.0 / R.lipschitz(C)


def test_kkt_conditions_hold_at_the_reference_solution():
    X, C, eta = _problem(8, 75, 32, 0)
    l1 = 0.1
    o = R.fista64(X, C, l1, eta, 1000)
    w, g = o["w"], o["g"]
    active = w > 0
    assert active.any() and (~active).any()
    worst = np.abs(g - l1)[active].max()
    print(f"[concepts] KKT active |g - l1| max {worst:.3e}; inactive max g - l1 {(g - l1)[~active].max():.3e}")
    # what the reference is used for sets the bound: it judges fp32 kernels (unit round-off 2^-24 = 6e-8), so its own distance
    # from the optimum has to lie well below that - 2^-30 = 9.3e-10, 64 times finer
    assert worst < 2.0 ** -30
    assert (g[~active] <= l1).all()
    assert o["kkt"].max() == max(worst, 0.0)


def test_closed_forms():
    X, C, eta = _problem(6, 40, 32, 1)
    bound = float((X @ C.T).max())
    for l1 in (bound, bound + 0.5):
        o = R.fista64(X, C, l1, eta, 50)
        assert (o["w"] == 0).all() and (o["nnz"] == 0).all()
        assert np.allclose(o["resid2"], (X * X).sum(1), rtol=0, atol=1e-15)
    c = C[:1]
    l1 = 0.05
    o = R.fista64(X, c, l1, 1.0 / R.lipschitz(c), 400)
    want = np.maximum(0.0, X @ c[0] - l1) / (c[0] @ c[0])
    assert np.abs(o["w"][:, 0] - want).max() < 1e-13
    z = R.fista64(X, C, 0.1, eta, 0)
    assert (z["w"] == 0).all() and (z["delta"] == 0).all() and np.array_equal(z["resid2"], (X * X).sum(1))


@pytest.mark.parametrize("l1", [0.05, 0.1])
@pytest.mark.parametrize("V,D", [(75, 32), (200, 64), (1000, 512)])
def test_planted_pairs_are_recovered(V, D, l1):
    x16, c16, pairs = R.planted(V, D, 16, seed=V + D)
    X, C = R.rows64(x16), R.rows64(c16)
    o = R.fista64(X, C, l1, 1.0 / R.lipschitz(C), 200)
    for i in range(16):
        assert set(np.nonzero(o["w"][i] > 1e-3)[0]) == set(pairs[i]), (i, np.nonzero(o["w"][i] > 1e-3)[0], pairs[i])


def test_planted_pairs_in_a_correlated_dictionary_with_centring():
    x16, c16, pairs = R.planted(200, 64, 16, seed=5, shared=SHARED)
    X, C = R.rows64(x16), R.rows64(c16)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)   # noqa: E731
    Cc = unit(C - C.mean(0))
    Xc = unit(X - C.mean(0))                               # the planted rows share the dictionary's cone: its mean centres both
    o = R.fista64(Xc, Cc, 0.1, 1.0 / R.lipschitz(Cc), 200)
    for i in range(16):
        assert set(np.nonzero(o["w"][i] > 1e-3)[0]) == set(pairs[i]), (i, np.nonzero(o["w"][i] > 1e-3)[0], pairs[i])


def test_fp32_restatement_stays_with_float64_and_the_gap_does_not_grow():
    """The iteration is non-expansive (eta = 1 / L), so rounding errors do not accumulate: 20 times the iterations leave the
    gap where it was.  Seen here: 1.34e-7, 1.69e-7, 1.79e-7 at 50, 200, 1000 iterations.
    The bounds, in units of u = 2^-24, the spacing of fp32 weights in [0.5, 1) and so the most one rounding moves a weight < 1:
    - the gap itself: 8 u = 4.8e-7.  A 32-term fp32 dot product of g carries about sqrt(32) = 5.7 roundings, eta < 1 scales it,
      and the prox adds one more; no count of iterations enters.
    - growth: a longer run may exceed a shorter one by one u, the granularity of the gap itself (the largest of 16 x 75
      differences of fp32 numbers moves in such steps), and by nothing that scales with the iterations - linear accumulation
      from 50 to 1000 would be a factor of 20.
    l1 = 0.1: there the active set is smaller than D = 32 and the minimiser is unique (at 0.05 the 75 concepts leave flat
    directions in which any two arithmetics drift apart)."""
    X, C, eta = _problem(16, 75, 32, 3)
    u = 2.0 ** -24
    gaps = []
    for iters in (50, 200, 1000):
        a, b = R.fista64(X, C, 0.1, eta, iters), R.fista32(X, C, 0.1, eta, iters)
        assert a["w"].max() < 1.0
        gaps.append(float(np.abs(a["w"] - b["w"]).max()))
    print(f"[concepts] fp32 vs float64 at 50 / 200 / 1000 iterations: {gaps}")
    assert max(gaps) < 8 * u
    assert gaps[1] <= gaps[0] + u and gaps[2] <= gaps[1] + u and gaps[2] <= gaps[0] + u


# ---- the host logic through the shim -----------------------------------------------------------------------------------
@pytest.fixture
def cc(monkeypatch):
    import importlib
    mod = importlib.import_module("clip.concepts")
    import concepts_ops_shim as shim
    shim.CALLS.clear()
    norm = lambda f, dtype, device=None: torch.nn.functional.normalize(f.double(), dim=1).to(dtype)   # noqa: E731
    monkeypatch.setattr(mod, "ops", shim)
    monkeypatch.setattr(mod, "_unit_rows", lambda f, dtype: f if f.dtype == dtype else norm(f, dtype))
    monkeypatch.setattr(mod, "normalize_rows", norm)
    mod.shim = shim
    return mod


def _same(a, b):
    for k in ("indices", "weights", "nnz", "cosine", "kkt", "delta", "l1norm", "resid2", "truncated"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_decompose_chunks_give_the_one_chunk_result(cc):
    x16, c16, _ = R.planted(75, 32, 16, seed=2)
    d = cc.ConceptDictionary(c16, dtype=torch.bfloat16)
    assert abs(d.L - R.lipschitz(R.rows64(c16))) < 1e-9
    one = cc.decompose(x16, d, l1=0.05, iters=60)
    assert cc.shim.CALLS == [(16, 75)]
    cc.shim.CALLS.clear()
    many = cc.decompose(x16, d, l1=0.05, iters=60, chunk_bytes=8 * 76 * 5)      # 5 rows of two [rows, 76] fp32 buffers
    assert cc.shim.CALLS == [(5, 75), (5, 75), (5, 75), (1, 75)]
    _same(one, many)
    tiny = cc.decompose(x16, d, l1=0.05, iters=60, chunk_bytes=1)               # never less than a row
    assert len(cc.shim.CALLS) == 4 + 16
    _same(one, tiny)


def test_truncation_and_the_truncated_flag(cc):
    x16 = R.unit_rows16(12, 32, 7, torch.bfloat16)
    c16 = R.unit_rows16(75, 32, 8, torch.bfloat16)
    d = cc.ConceptDictionary(c16, names=[f"w{v}" for v in range(75)], dtype=torch.bfloat16)
    full = cc.decompose(x16, d, l1=0.01, iters=100, max_terms=75)
    cut = cc.decompose(x16, d, l1=0.01, iters=100, max_terms=3)
    assert not full.truncated.any() and (full.nnz > 3).any()
    assert torch.equal(cut.truncated, full.nnz > 3) and torch.equal(cut.nnz, full.nnz)
    assert torch.equal(cut.indices, full.indices[:, :3]) and torch.equal(cut.weights, full.weights[:, :3])
    assert ((full.indices >= 0).sum(1) == full.nnz).all() and (full.weights[full.indices < 0] == 0).all()
    assert (full.weights[:, :-1] >= full.weights[:, 1:]).all()
    terms = cut.terms(0)
    assert [n for n, _ in terms] == [f"w{v}" for v in cut.indices[0].tolist()] and len(terms) == 3
    crow, col, val = full.to_csr()
    assert crow.tolist() == [0] + full.nnz.cumsum(0).tolist() and col.numel() == int(full.nnz.sum()) and (val > 0).all()
    # the cosine of a full row is the cosine with the dense reconstruction
    o = R.fista32(x16.float().numpy(), c16.float().numpy(), 0.01, 1.0 / d.L, 100)
    s = torch.from_numpy(o["w"]) @ c16.float()
    want = torch.nn.functional.cosine_similarity(s, x16.float(), dim=1)
    assert (full.cosine - want).abs().max() < 1e-5
    assert (cut.cosine <= full.cosine + 1e-6).all()


def test_centring_round_trip_in_recompose(cc):
    """Rows built as mean + a positive combination of two centred concepts: after centring the code finds the pair, and
    recompose (scale * sum w c + mean, normalised) returns to the row."""
    g = torch.Generator().manual_seed(11)
    texts = torch.nn.functional.normalize(0.8 * torch.randn(1, 64, generator=g, dtype=torch.float64) +
                                          torch.nn.functional.normalize(torch.randn(120, 64, generator=g, dtype=torch.float64), dim=1), dim=1)
    d = cc.ConceptDictionary(texts, dtype=torch.float16, center="mean")
    assert d.mean is not None and torch.allclose(d.mean.double(), texts.float().mean(0).double(), atol=1e-6)
    mean = torch.nn.functional.normalize(torch.randn(64, generator=g, dtype=torch.float64), dim=0) * 0.6
    c = d.rows.double()
    s = 0.5 * c[3] + 0.3 * c[40]
    x = torch.nn.functional.normalize(mean + s, dim=0)[None].repeat(3, 1)
    dec = cc.decompose(x.float(), d, l1=0.001, iters=400, center=(mean / (mean + s).norm()).float())   # the unit row minus this is s / |mean + s|
    assert set(dec.indices[0][dec.weights[0] > 1e-2].tolist()) == {3, 40}
    back = dec.recompose()
    assert back.shape == (3, 64)
    assert torch.nn.functional.cosine_similarity(back.double(), x, dim=1).min() > 0.999
    assert dec.cosine.min() > 0.999
    own = cc.decompose(torch.randn(5, 64, generator=g), d, l1=0.05, iters=20, center="mean")
    assert own.mean is not None and own.scale.shape == (5,)
    plain = cc.decompose(torch.randn(5, 64, generator=g), d, l1=0.05, iters=20)
    assert plain.mean is None and plain.scale is None and plain.recompose().shape == (5, 64)


def test_profile_and_distinctive_on_a_hand_made_case(cc):
    d = cc.ConceptDictionary(torch.eye(4, 32), names=["a", "b", "c", "d"], dtype=torch.bfloat16)
    z = torch.zeros(4)
    dec = cc.ConceptDecomposition(indices=torch.tensor([[0, 1], [0, -1], [2, 3], [3, -1]]),
                                  weights=torch.tensor([[0.5, 0.25], [1.0, 0.0], [0.75, 0.25], [0.5, 0.0]]),
                                  nnz=torch.tensor([2, 1, 2, 1]), cosine=z, kkt=z, delta=z, l1norm=z, resid2=z,
                                  truncated=torch.zeros(4, dtype=torch.bool), dictionary=d)
    p = cc.concept_profile(dec, [7, 7, 2, -1])
    import clip
    assert type(p) is clip.ConceptProfile
    assert p.groups.tolist() == [2, 7] and p.counts.tolist() == [1, 2]
    assert torch.equal(p.mean, torch.tensor([[0.0, 0.0, 0.75, 0.25], [0.75, 0.125, 0.0, 0.0]]))
    assert torch.allclose(p.overall, torch.tensor([1.5, 0.25, 0.75, 0.25]) / 3)
    top = cc.distinctive(p, 2)
    assert [n for n, _ in top[2]] == ["c", "d"] and [n for n, _ in top[7]] == ["a", "b"]
    assert top[7][0][1] == pytest.approx(0.25)
    with pytest.raises(ValueError):
        cc.concept_profile(dec, [0, 1])
    with pytest.raises(ValueError):
        cc.distinctive(p, 0)


def test_argument_errors(cc):
    c16 = R.unit_rows16(10, 32, 0, torch.bfloat16)
    x16 = R.unit_rows16(4, 32, 1, torch.bfloat16)
    d = cc.ConceptDictionary(c16, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        cc.ConceptDictionary(c16, names=["x"], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        cc.ConceptDictionary(c16[0], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        cc.ConceptDictionary(c16, dtype=torch.bfloat16, center="median")
    with pytest.raises(TypeError):
        cc.decompose(x16, c16)
    for kw in (dict(l1=-1.0), dict(l1=float("nan")), dict(iters=-1), dict(iters=1.5), dict(max_terms=0), dict(chunk_bytes=0),
               dict(center=torch.zeros(5))):
        with pytest.raises(ValueError):
            cc.decompose(x16, d, **kw)
    with pytest.raises(ValueError):
        cc.decompose(R.unit_rows16(4, 64, 1, torch.bfloat16), d)
