"""CPU: the float64 reference of the Gaussian class models (tests/gaussian_ref.py) pinned against independent statements, and
the host-side contract of the new ops wrappers.  Every float64 tolerance is derived from the condition number of the covariance
in play: solving with a matrix of condition kappa loses about kappa * 2^-52 relative, and the test prints kappa."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussian_ref as R  # noqa: E402

EPS = 2.0 ** -52


@pytest.fixture(scope="module", autouse=True)
def _the_product_is_there():
    """the reference is pinned for the sake of the product it is compared with: no test of this file runs without it"""
    import __graft_entry__ as ge
    ge.build()
    import clip.gaussian  # noqa: F401


def _data(N, C, D, seed=0):
    x16, y = R.planted(N, C, D, seed, torch.bfloat16)
    return R.rows64(x16), y


def _tol(cond, scale, tag):
    tol = 64 * cond * EPS * scale
    print(f"[gaussian cpu] {tag}: condition number {cond:.3e}, tolerance {tol:.3e}")
    return tol


def test_scatter_is_the_weighted_mean_of_class_covariances():
    X, y = _data(120, 3, 64)
    count, s, gram = R.moments64(X, y, 3)
    S = R.scatter64(count, s, gram) / (120 - 3)
    want = sum((count[c] - 1) * np.cov(X[y == c].T) for c in range(3)) / (120 - 3)
    # gram - N mean mean^T cancels |mean|^2 against the spread: condition |gram| / |S|
    tol = _tol(np.abs(gram).max() / np.abs(S).max(), np.abs(S).max(), "scatter")
    assert np.abs(S - want).max() <= tol


@pytest.mark.parametrize("shrinkage", (0.5, "auto"))
def test_d2_and_scores_against_the_direct_forms(shrinkage):
    C, D = 3, 64
    X, y = _data(300, C, D)
    f = R.fit64(X, y, C, shrinkage)
    Q, _ = _data(50, C, D, seed=7)
    P = np.linalg.inv(f["sigma"])
    z = Q @ f["T"].T - f["t0"]
    d2 = np.stack([((z - m) ** 2).sum(1) for m in f["centres"]], axis=1)
    want = np.stack([np.einsum("qd,de,qe->q", Q - mu, P, Q - mu) for mu in f["class_mean"]], axis=1)
    tol = _tol(f["cond"], np.abs(want).max(), f"d2 {shrinkage}")
    assert np.abs(d2 - want).max() <= tol
    # the paper's linear form W x + b differs by the class-independent -1/2 x^T P x: compare after subtracting the row maximum
    score = -0.5 * d2 + f["offset"]
    W = f["class_mean"] @ P
    lin = Q @ W.T + f["offset"] - 0.5 * np.einsum("cd,cd->c", W, f["class_mean"])
    xPx = np.einsum("qd,de,qe->q", Q, P, Q)
    tol = _tol(f["cond"], np.abs(xPx).max(), f"linear form {shrinkage}")
    assert np.abs((score - score.max(1, keepdims=True)) - (lin - lin.max(1, keepdims=True))).max() <= tol
    assert np.array_equal(score.argmax(1), lin.argmax(1))


def test_auto_is_the_closed_formula_at_n_below_d():
    N, C, D = 18, 9, 64
    X, y = _data(N, C, D)
    count, s, gram = R.moments64(X, y, C)
    S = R.scatter64(count, s, gram) / (N - C)
    sigma = R.covariance64(count, s, gram, "auto")
    precision = D * np.linalg.inv((N - 1) * S + np.trace(S) * np.eye(D))
    T, _, cond = R.whitening64(sigma)
    tol = _tol(cond, np.abs(precision).max(), "auto")
    assert np.abs(T.T @ T - precision).max() <= tol
    assert cond <= (N - 1) * D + 1.0001                     # (N - 1) lambda_max + tr over tr: bounded whatever the rank


def test_lam_zero_with_singular_covariance_is_an_error():
    X, y = _data(18, 9, 64)
    count, s, gram = R.moments64(X, y, 9)
    with pytest.raises(ValueError, match="N = 18, C = 9, D = 64"):
        R.covariance64(count, s, gram, 0.0)
    assert R.covariance64(*R.moments64(*_data(300, 3, 64), 3), 0.0).shape == (64, 64)


def test_pca_against_the_svd_of_the_centred_rows():
    X, _ = _data(90, 3, 64)
    k = 5
    p = R.pca64(X, k)
    Xc = X - X.mean(0)
    _, sv, Vt = np.linalg.svd(Xc, full_matrices=False)
    var = sv ** 2 / (len(X) - 1)
    cond = np.abs(X.T @ X).max() / var[k - 1]
    tol = _tol(cond, var[0], "pca")
    assert np.abs(p["explained_variance"] - var[:k]).max() <= tol
    assert abs(p["explained_variance_ratio"].sum() - var[:k].sum() / var.sum()) <= tol / var[0]
    gap = np.min(var[:k] - var[1:k + 1])
    assert np.abs(np.abs(p["components"] @ Vt[:k].T) - np.eye(k)).max() <= tol / gap        # the same subspace, axis by axis
    big = np.abs(p["components"]).argmax(1)
    assert (p["components"][np.arange(k), big] > 0).all()
    assert np.abs(np.linalg.norm(p["components"], axis=1) - 1).max() <= 1e-12


def test_class_moments_addition_is_the_joint_fit():
    X, y = _data(100, 3, 64)
    a, b, c = R.moments64(X[:37], y[:37], 3), R.moments64(X[37:], y[37:], 3), R.moments64(X, y, 3)
    for u, v, w in zip(a, b, c):
        assert np.abs((u + v) - w).max() <= 100 * EPS * max(1.0, np.abs(w).max())


@pytest.mark.parametrize("N,C,shrinkage", [(300, 3, 0.5), (300, 9, "auto"), (18, 9, "auto"), (8, 9, 0.5), (300, 9, 0.0)])
def test_product_algebra_from_exact_moments(N, C, shrinkage):
    """clip.GaussianClassifier's float64 algebra (the divisor, both shrinkage rules, the whitening, centres, offsets, log det)
    on the reference's exact float64 moments, through from_state_dict on the host: no kernel runs.  d2 is independent of the
    eigenvectors' signs, so T is compared through T^T T and the centres through their distances."""
    import __graft_entry__ as ge
    ge.build()
    import clip
    X, y = R.planted(N, min(C, 4) if N <= C else C, 64, 1, torch.bfloat16, sep=0.6)
    X = R.rows64(X)
    count, s, gram = R.moments64(X, y, C)
    f = R.fit64(X, y, C, shrinkage)
    state = dict(count=torch.from_numpy(count.astype(np.float64)), sum=torch.from_numpy(s), gram=torch.from_numpy(gram),
                 class_names=None, shrinkage=shrinkage, priors="empirical", text_features=None, logit_scale=100.0, alpha=1.0,
                 dtype="bfloat16")
    gc = clip.GaussianClassifier.from_state_dict(state, "cpu")
    sigma = gc.covariance().numpy()
    assert np.abs(sigma - f["sigma"]).max() <= 64 * EPS * np.abs(gram).max()          # the cancellation of the mean term
    tol = _tol(f["cond"], 1.0, f"product algebra N={N} C={C} {shrinkage}")
    P = np.linalg.inv(f["sigma"])
    T = gc.T.double().numpy()
    assert np.abs(T.T @ T - P).max() <= (tol + 4 * 2.0 ** -24) * np.abs(P).max()       # T is kept in fp32
    assert abs(gc.log_det - f["log_det"]) <= tol * 64
    m, m64 = gc.centres.double().numpy(), f["centres"]
    have = count > 0
    dist = lambda a: ((a[have][:, None, :] - a[have][None, :, :]) ** 2).sum(-1)
    assert np.abs(dist(m) - dist(m64)).max() <= (tol + 8 * 2.0 ** -24) * max(1.0, dist(m64).max())
    assert np.array_equal(gc.offset.numpy(), f["offset32"])
    if shrinkage == 0.0:
        with pytest.raises(ValueError, match="N = 18, C = 9, D = 64"):
            x2, y2 = R.planted(18, 9, 64, 1, torch.bfloat16)
            c2, s2, g2 = R.moments64(R.rows64(x2), y2, 9)
            clip.GaussianClassifier.from_state_dict(dict(state, count=torch.from_numpy(c2.astype(np.float64)),
                                                         sum=torch.from_numpy(s2), gram=torch.from_numpy(g2)), "cpu")


def test_pair16_is_the_headers_pair():
    g = np.random.default_rng(0)
    T = (g.standard_normal((7, 32)) * np.geomspace(1e-3, 1e3, 32)).astype(np.float32)
    for dtype, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        hi, lo = R.pair16(T, dtype)
        assert np.array_equal(hi, torch.from_numpy(T).to(dtype).double().numpy())
        assert np.abs(hi + lo - T).max() <= np.abs(T).max() * 2.0 ** (-2 * bits) * 1.01 + 2.0 ** -25


@pytest.mark.parametrize("call", ("class_moments", "gauss_scores"))
def test_new_wrappers_refuse_host_tensors(call):
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip import ops
    x = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match=rf"{call}.*cuda"):
        if call == "class_moments":
            ops.class_moments(x, torch.zeros(8, dtype=torch.int32), 2)
        else:
            ops.gauss_scores(x, torch.zeros(4, 64))
    assert ops.moments_parts(612, 9, 64) == 3 and ops.moments_workspace(0, 9, 64) == 0
    assert ops.gauss_scores_workspace(33, 64) == 4 * 48 * 64


def test_gpu_pred_inputs_keep_the_reference_inside_the_cap():
    """the inputs of tests/test_gaussian_kernels_gpu.py: the float64 reference alone leaves at most 2 % of a case's rows out of
    the argmax / argmin comparison"""
    import test_gaussian_kernels_gpu as G
    worst = 0.0
    for Q, D, Rr, C, kind in G.GAUSS_CASES:
        if C < 2 or D > 512 or Q < 33:                     # (one class has no gap; the largest shapes are left to the GPU run)
            continue
        for dtype in G.BOTH:
            x16, T, t0, centres, offset, _ = G._gauss_inputs(Q, D, Rr, C, kind, dtype)
            ref = R.scores64(R.rows64(x16), T, dtype, t0, centres, offset)
            keep_p, keep_n = R.outside_margin(ref, G.d2_tol(Rr))
            worst = max(worst, (~keep_p).mean(), (~keep_n).mean())
    print(f"[gaussian cpu] worst skipped share {worst:.4f}")
    assert worst <= 0.02
