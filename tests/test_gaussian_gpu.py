"""GPU: the public surface of clip/gaussian.py at toy sizes (D = 64, C = 3 and 9, N from 18 to 300) against the float64
reference (tests/gaussian_ref.py): GaussianClassifier, mahalanobis / calibrate / outliers / suspects, add, the state_dict round
trip, from_index, EmbeddingIndex.gaussian / pca, pca, and scripts/flag_outliers.py --synthetic as a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussian_ref as R  # noqa: E402
from test_gaussian_kernels_gpu import D2_TOL  # noqa: E402  (the kernel's asserted tolerance: the margin of the comparisons)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (torch.bfloat16, torch.float16)
D = 64


def _clip():
    import clip
    return clip


def _ref_scores(f, q16):
    return R.scores64(R.rows64(q16), f["T32"], q16.dtype, f["t032"], f["centres32"], f["offset32"])


def _agree(pred, ref, what="score"):
    """predictions against the float64 reference on every row outside the margin; at most 2 % of the rows inside it"""
    keep = R.outside_margin(ref, D2_TOL)[0 if what == "score" else 1]
    assert (~keep).mean() <= 0.02
    want = ref["pred"] if what == "score" else ref["nearest"]
    assert np.array_equal(pred.cpu().numpy()[keep], want[keep])


def _sigma_bound(X, y, C, shrinkage):
    """Entrywise bound of |covariance from the kernel's fp32 moments - covariance from exact moments|, derived: gram and sum
    are within n 2^-24 sum |terms| of the exact sums (the bound test_gaussian_kernels_gpu.py asserts), and the float64 algebra
    carries that through scatter = gram - sum_c s_c s_c^T / count_c, the divisor and the shrinkage rule."""
    live = (y >= 0) & (y < C)
    A, yl = np.abs(X[live]), y[live]
    N, Dd = len(A), X.shape[1]
    ne = (N + 16) * 2.0 ** -24
    count = np.bincount(yl, minlength=C)
    s, mag = np.zeros((C, Dd)), np.zeros((C, Dd))
    np.add.at(s, yl, X[live])
    np.add.at(mag, yl, A)
    B = ne * (A.T @ A)
    for c in range(C):
        if count[c]:
            ds = ne * mag[c]
            B += (np.outer(np.abs(s[c]), ds) + np.outer(ds, np.abs(s[c])) + np.outer(ds, ds)) / count[c]
    div = N - C if N > C else N
    trB = np.trace(B)
    if shrinkage == "auto":
        return ((N - 1) * B + trB * np.eye(Dd)) / (Dd * div)
    return (1 - shrinkage) * B / div + shrinkage * trB / (Dd * div) * np.eye(Dd)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N,C,shrinkage", [(300, 3, 0.5), (300, 9, "auto"), (18, 9, "auto"), (40, 3, "auto"), (300, 9, 0.1), (8, 9, 0.5)])
def test_covariance_is_the_reference_covariance(N, C, shrinkage, dtype):
    """the product's divisor (N - C, or N when N <= C), both shrinkage rules and the kernel's moments against fit64's sigma"""
    clip = _clip()
    x16, y = R.planted(N, min(C, 4) if N <= C else C, D, 1, dtype, sep=0.6)      # N = 8 <= C = 9: four classes with rows, five without
    X = R.rows64(x16)
    gc = clip.GaussianClassifier(x16.cuda(), y, num_classes=C, shrinkage=shrinkage)
    f = R.fit64(X, y, C, shrinkage)
    bound = _sigma_bound(X, y, C, shrinkage) + 1e-12 * np.abs(f["sigma"]).max()
    got = gc.covariance().cpu().numpy()
    ratio = float((np.abs(got - f["sigma"]) / bound).max())
    print(f"[gaussian] covariance N={N} C={C} {shrinkage}: worst ratio to the derived bound {ratio:.3e}; the bound is at most "
          f"{bound.max() / np.abs(f['sigma']).max():.3e} of |sigma|, condition number {f['cond']:.3e}")
    assert ratio <= 1.0
    # the bound is sharp enough to tell a wrong rule apart: at most 1 % of |sigma| (computed: 0.07 - 0.91 %), where dividing by
    # N instead of N - C moves sigma by 8 % at (40, 3), 3 % at (300, 9) and a factor 2 at (18, 9), and a dropped 1 / D by 64 x
    assert bound.max() <= 1e-2 * np.abs(f["sigma"]).max()
    assert np.array_equal(gc.moments.count.cpu().numpy(), f["count"])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N,C,shrinkage", [(300, 3, 0.5), (300, 9, "auto"), (18, 9, "auto"), (40, 3, "auto")])
def test_classifier_matches_the_reference(N, C, shrinkage, dtype):
    clip = _clip()
    # classes that overlap (0.6 whitened units apart): predictions and accuracy depend on the covariance - with the identity
    # in its place the float64 accuracy of the N = 300 cases drops from 0.92 / 0.89 to 0.85 / 0.71
    x16, y = R.planted(N, C, D, 1, dtype, sep=0.6)
    q16, yq = R.planted(400, C, D, 1, dtype, sep=0.6)             # the same classes (same seed), 400 rows
    gc = clip.GaussianClassifier(x16.cuda(), y, num_classes=C, shrinkage=shrinkage)
    f = R.fit64(R.rows64(x16), y, C, shrinkage)
    # the kept fp32 T whitens the classifier's own float64 covariance: rows u_i / sqrt(lambda_i) rounded to fp32 move an entry
    # of T Sigma T^T by at most 2 * 2^-24 * sqrt(D lambda_max / lambda_min); 4 D instead of 2 sqrt(D) leaves room for eigh
    sigma = gc.covariance().cpu().numpy()
    T64 = gc.T.double().cpu().numpy()
    print(f"[gaussian] N={N} C={C} {shrinkage}: condition number {f['cond']:.3e}")
    assert np.abs(T64 @ sigma @ T64.T - np.eye(D)).max() <= 4 * D * 2.0 ** -24 * np.sqrt(f["cond"])
    assert abs(gc.log_det - np.linalg.slogdet(sigma)[1]) <= 1e-9 * max(1.0, abs(gc.log_det))
    # predictions: reference arithmetic on the classifier's OWN fp32 operands (eigenvector signs are free)
    own = dict(T32=gc.T.cpu().numpy(), t032=gc.t0.cpu().numpy(), centres32=gc.centres.cpu().numpy(), offset32=gc.offset.cpu().numpy())
    ref = _ref_scores(own, q16)
    _agree(gc.predict(q16.cuda()), ref)
    logits = gc.logits(q16.cuda()).cpu().double().numpy()
    assert np.abs(logits - ref["score"]).max() <= D2_TOL * ref["d2"].max()
    # and the planted labels are recovered at the rate the float64 fit recovers them
    ref64 = R.scores64(R.rows64(q16), f["T32"], dtype, f["t032"], f["centres32"], f["offset32"])
    acc, acc64 = gc.score(q16.cuda(), yq), float((ref64["pred"] == yq).mean())
    print(f"[gaussian] accuracy {acc:.3f}, float64 fit {acc64:.3f}")
    assert abs(acc - acc64) <= 0.02
    proba = gc.predict_proba(q16.cuda())
    assert torch.allclose(proba.sum(1), torch.ones(400, device="cuda"), atol=1e-5)
    probs, idx, names = gc(image_features=q16.cuda())
    assert torch.equal(idx, probs.argmax(1)) and names == idx.tolist()


def test_text_features_alpha_priors_and_errors():
    clip = _clip()
    C = 3
    x16, y = R.planted(90, C, D, 2, torch.bfloat16)
    y[:50] = 0                                                    # unbalanced: the priors matter
    text = torch.nn.functional.normalize(torch.randn(C, D, generator=torch.Generator().manual_seed(0)), dim=1)
    plain = clip.GaussianClassifier(x16.cuda(), y, num_classes=C, shrinkage=0.5)
    uni = clip.GaussianClassifier(x16.cuda(), y, num_classes=C, shrinkage=0.5, priors="uniform")
    withtext = clip.GaussianClassifier(x16.cuda(), y, shrinkage=0.5, text_features=text, alpha=0.25, logit_scale=50.0,
                                       class_names=["a", "b", "c"])
    q = x16[:20].cuda()
    count = np.bincount(y, minlength=C)
    assert torch.allclose(plain.offset.cpu(), torch.from_numpy(np.log(count / count.sum())).float())
    assert torch.allclose(uni.offset.cpu(), torch.full((C,), -np.log(C)))
    assert torch.allclose(plain.logits(q) - uni.logits(q), (plain.offset - uni.offset).expand(20, C), atol=1e-3)
    zs = 50.0 * torch.nn.functional.normalize(q.float(), dim=1) @ text.cuda().T
    assert torch.allclose(withtext.logits(q), zs + 0.25 * plain.logits(q), atol=2e-3)
    assert withtext(image_features=q)[2][0] in ("a", "b", "c")
    with pytest.raises(ValueError, match="N = 18, C = 9, D = 64"):
        xs, ys = R.planted(18, 9, D, 3, torch.bfloat16)
        clip.GaussianClassifier(xs.cuda(), ys, shrinkage=0.0)
    with pytest.raises(TypeError, match="cuda"):
        clip.GaussianClassifier(x16, y)
    with pytest.raises(ValueError, match="shrinkage"):
        clip.GaussianClassifier(x16.cuda(), y, shrinkage="ledoit")


@pytest.mark.parametrize("dtype", BOTH)
def test_mahalanobis_outliers_and_suspects(dtype):
    clip = _clip()
    N, C = 300, 9
    x16, y = R.planted(N + 200, C, D, 4, dtype)
    fit_x, fit_y, held, held_y = x16[:N], y[:N].copy(), x16[N:N + 100], y[N:N + 100]
    inl = x16[N + 100:]
    swapped = np.arange(0, N, 37)                                 # planted label swaps
    fit_y[swapped] = (fit_y[swapped] + 1) % C
    gc = clip.GaussianClassifier(fit_x.cuda(), fit_y, num_classes=C, shrinkage="auto")
    far = torch.nn.functional.normalize(torch.randn(20, D, generator=torch.Generator().manual_seed(5)), dim=1).to(dtype)
    m_in, m_far = gc.mahalanobis(inl.cuda()), gc.mahalanobis(far.cuda())
    assert float(m_far.dmin.min()) > float(m_in.dmin.max())
    assert float(m_far.log_density.max()) < float(m_in.log_density.min())
    own = dict(T32=gc.T.cpu().numpy(), t032=gc.t0.cpu().numpy(), centres32=gc.centres.cpu().numpy(), offset32=gc.offset.cpu().numpy())
    ref = _ref_scores(own, inl)
    assert np.abs(m_in.dmin.cpu().double().numpy() - ref["dmin"]).max() <= D2_TOL * ref["d2"].max()
    _agree(m_in.nearest, ref, "d2")
    const = 0.5 * gc.log_det + 0.5 * D * np.log(2 * np.pi)
    assert np.abs(m_in.log_density.cpu().double().numpy() - (ref["lse"] - const)).max() <= 1e-4 * max(1.0, abs(const))
    # calibrate: the empirical quantile on held-out rows; fitted rows would sit lower
    thr = gc.calibrate(held.cuda(), 0.95)
    ref_h = _ref_scores(own, held)
    assert abs(thr - np.quantile(ref_h["dmin"], 0.95)) <= 4 * D2_TOL * ref_h["d2"].max()
    assert gc.calibrate(fit_x.cuda(), 0.95) < thr
    assert bool(gc.outliers(far.cuda(), thr).all())
    assert float(gc.outliers(inl.cuda(), thr).float().mean()) <= 0.15
    # suspects: the planted swaps lead the ranking at the rate the float64 reference puts them there
    rows, margin = gc.suspects(fit_x.cuda(), fit_y, top=len(swapped))
    ref_f = _ref_scores(own, fit_x)
    ref_margin = ref_f["d2"][np.arange(N), fit_y] - ref_f["dmin"]
    ref_rows = np.argsort(-ref_margin, kind="stable")[: len(swapped)]
    found, found64 = len(set(rows.tolist()) & set(swapped.tolist())), len(set(ref_rows.tolist()) & set(swapped.tolist()))
    print(f"[gaussian] suspects: {found} of {len(swapped)} swaps in the top {len(swapped)}, float64 reference {found64}")
    assert found == found64 and found >= len(swapped) - 1
    assert bool((margin[:-1] >= margin[1:]).all())


def test_add_state_dict_and_index():
    clip = _clip()
    N, C = 120, 3
    x16, y = R.planted(N, C, D, 6, torch.bfloat16)
    xd = x16.cuda()
    whole = clip.GaussianClassifier(xd, y, num_classes=C)
    parts = clip.GaussianClassifier(xd[:50], y[:50], num_classes=C).add(xd[50:], y[50:])
    m, p = whole.moments, parts.moments
    assert torch.equal(m.count, p.count)
    n_tol = N * 2.0 ** -24                                        # two orders of fp32 sums of the same exact products
    assert float((m.sum - p.sum).abs().max()) <= n_tol * float(m.sum.abs().max())
    assert float((m.gram - p.gram).abs().max()) <= n_tol * float(m.gram.abs().max())
    q = xd[:40]
    assert float((whole.logits(q) - parts.logits(q)).abs().max()) <= 1e-3 * float(whole.logits(q).abs().max())
    mm = clip.class_moments(xd[:50], y[:50], C) + clip.class_moments(xd[50:], y[50:], C)
    assert torch.equal(mm.gram, p.gram) and isinstance(mm, clip.ClassMoments)
    # state_dict: bitwise on the kept fp32 operands
    state = parts.state_dict()
    assert state["gram"].dtype == torch.float64 and not state["gram"].is_cuda
    back = clip.GaussianClassifier.from_state_dict(state, "cuda:0")
    for a, b in ((back.T, parts.T), (back.t0, parts.t0), (back.centres, parts.centres), (back.offset, parts.offset)):
        assert torch.equal(a, b)
    assert torch.equal(back.predict(q), parts.predict(q))
    with pytest.raises(KeyError):
        clip.GaussianClassifier.from_state_dict({k: v for k, v in state.items() if k != "gram"})
    # from_index and the thin methods of EmbeddingIndex
    names = ["x", "y", "z"]
    index = clip.EmbeddingIndex(xd.float(), metadata=[{"kind": names[int(c)]} for c in y])
    gi = index.gaussian("kind", class_names=names)
    assert gi.class_names == names and torch.equal(gi.moments.count, whole.moments.count)
    assert gi(image_features=index.features[:5])[2] == [names[int(c)] for c in gi.predict(index.features[:5])]
    pr = index.pca(4)
    assert tuple(pr.components.shape) == (4, D) and tuple(pr.transform(index.features).shape) == (N, 4)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("k,whiten", [(1, False), (5, False), (5, True), (D, False)])
def test_pca_against_the_reference(k, whiten, dtype):
    clip = _clip()
    x16, _ = R.planted(200, 3, D, 7, dtype)
    X = R.rows64(x16)
    p = clip.pca(x16.cuda(), k, whiten=whiten)
    ref = R.pca64(X, k)
    var0 = ref["explained_variance"][0]
    # the kernel's fp32 Gram matrix: N 2^-24 of |gram| per entry, seen through the cancellation of the mean term
    tol = 64 * 200 * 2.0 ** -24 * np.abs(X.T @ X).max()
    assert np.abs(p.explained_variance.cpu().numpy() - ref["explained_variance"]).max() <= tol
    assert abs(float(p.explained_variance_ratio.sum()) - ref["explained_variance_ratio"].sum()) <= tol / var0
    comp = p.components.cpu().numpy()
    big = np.abs(comp).argmax(1)
    assert (comp[np.arange(k), big] > 0).all()
    assert np.abs(comp @ comp.T - np.eye(k)).max() <= 1e-9
    # transform: against float64 on the result's own components (the kernel's hi + lo pair of T is exact to 2^-16 |T|)
    z = p.transform(x16.cuda()).cpu().double().numpy()
    T = p.T.cpu().numpy()
    ref_z = R.scores64(X, T, dtype, p.t0.cpu().numpy())
    assert np.abs(z - ref_z["z"]).max() <= ((2 * D + 2) * 2.0 ** -24 * ref_z["zmag"]).max()
    want = (X - X.mean(0)) @ (comp / np.sqrt(p.explained_variance.cpu().numpy())[:, None] if whiten else comp).T
    assert np.abs(z - want).max() <= 1e-3 * max(1.0, np.abs(want).max())
    if whiten and k < D:
        assert np.abs(z.var(0, ddof=1) - 1).max() <= 1e-2
    if k <= 5:                                                    # the leading axes of the reference, where the spectrum has gaps
        gap = np.min(-np.diff(R.pca64(X, k + 1)["explained_variance"]))
        assert np.abs(np.abs(comp @ ref["components"].T) - np.eye(k)).max() <= 4 * tol / gap


def test_flag_outliers_script_synthetic():
    env = dict(os.environ)
    for extra in ([], ["--suspects", "3"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "flag_outliers.py"), "--synthetic", *extra],
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        if extra:
            assert len(rows) == 3 and rows[0]["row"] == 0 and rows[0]["nearest"] == "fall"
        else:
            assert len(rows) == 21 and all(set(r_) == {"file_name", "class", "probability", "mahalanobis", "outlier"} for r_ in rows)
            assert all(r_["outlier"] for r_ in rows[-3:]) and sum(r_["outlier"] for r_ in rows[:-3]) <= 3
