"""Without a GPU: the float64 closed form of cache_affinity_bwd_ref.py against float64 autograd, planted errors against its
bound, and the host logic of CacheClassifier.fit / state_dict / load_state_dict and of the script's new flags on torch
restatements of the two ops."""
import math

import pytest
import torch

import cache_affinity_bwd_ref as B
import cache_affinity_ref as R

pytestmark = pytest.mark.filterwarnings("ignore::UserWarning")
SIZES = (0, 1, 16, 17, 3, 40)


def _problem(dtype, Q=17, D=64, seed=7):
    q16, g16, labels = R.make_problem(seed, Q, SIZES, D, dtype)
    dA = (torch.randn(Q, len(SIZES), generator=torch.Generator().manual_seed(seed + 1)) / Q).float()
    return q16, g16, labels, dA


@pytest.mark.parametrize("dtype", B.DTYPES, ids=["bf16", "fp16"])
def test_reference_agrees_with_float64_autograd(dtype):
    q16, g16, labels, dA = _problem(dtype)
    C, beta = len(SIZES), 5.5
    dG, T, s = B.reference(q16, g16, labels, beta, dA)
    g = g16.double().requires_grad_(True)
    A, _ = R.reference(q16.double(), g, labels, C, beta)                      # the forward reference, float64, differentiated
    (A * dA.double()).sum().backward()
    assert (g.grad - dG).abs().max().item() <= 1e-14 * max(1.0, T.max().item() * 1e3)
    assert (dG.abs() <= T * (1 + 1e-12)).all()
    # with exclude (the forward reference masks in place, which autograd refuses): the same composition with a where-mask
    ex = torch.arange(q16.shape[0]) % labels.numel()
    ex[::5] = -1
    dGx, _, _ = B.reference(q16, g16, labels, beta, dA, ex)
    g = g16.double().requires_grad_(True)
    e = torch.exp(beta * (q16.double() @ g.t() - 1.0))
    keep = torch.arange(labels.numel())[None, :] != ex[:, None]
    onehot = torch.nn.functional.one_hot(labels, C).double()
    ((torch.where(keep, e, torch.zeros_like(e)) @ onehot) * dA.double()).sum().backward()
    assert (g.grad - dGx).abs().max().item() <= 1e-14
    assert (dGx - dG).abs().max().item() > 0


@pytest.mark.parametrize("dtype", B.DTYPES, ids=["bf16", "fp16"])
def test_bound_passes_fp32_and_catches_planted_errors(dtype):
    """the fp32 torch restatement lies inside the bound; each planted error leaves it on at least one element"""
    q16, g16, labels, dA = _problem(dtype, Q=17, D=64)
    C, beta = len(SIZES), 5.5
    Q, N = q16.shape[0], labels.numel()
    ex = torch.arange(Q) % N
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    exl = R.to_laid(ex, gather)
    dG, T, s = B.reference(q16, g16, labels, beta, dA, ex)
    ref, tol = B.to_laid(dG, gather), B.to_laid(B.tolerance(T, beta, q16, g16, s, dA, ex), gather)
    good = B.torch_cache_affinity_backward(q16, laid, off, ln, beta, dA, exclude=exl)
    assert not torch.isnan(good).any() and (good[gather < 0] == 0).all()
    assert B.ratio(good, ref, tol) <= 1.0

    def planted(what):
        if what == "query dropped":
            d, _, _ = B.reference(q16[:-1], g16, labels, beta, dA[:-1], ex[:-1])
        elif what == "neighbouring class":
            d = dG.clone()
            n = int((labels == 3).nonzero()[0, 0])
            w, _ = B.weights(q16, g16, labels, beta, dA.roll(1, dims=1), ex)                 # row n reads column labels[n] - 1
            d[n] = beta * (w[:, n, None] * q16.double()).sum(dim=0)
        elif what == "exclude ignored":
            d, _, _ = B.reference(q16, g16, labels, beta, dA, None)
        elif what == "beta missing":
            d = dG / beta
        return B.to_laid(d, gather)
    for what in ("query dropped", "neighbouring class", "exclude ignored", "beta missing"):
        r = B.ratio(planted(what).float(), ref, tol)
        print(f"[cache-bwd planted] {what} {dtype}: err/tol {r:.3e}")
        assert r > 1.0, what
    # a padding row treated as a zero vector that receives a gradient: s = 0 there, the weight dA * exp(-beta)
    pad = good.clone()
    j = int((gather < 0).nonzero()[0, 0])
    c = int((off[1:] > j).nonzero()[0, 0])
    pad[j] = beta * ((dA[:, c] * math.exp(-beta))[:, None] * q16.float()).sum(dim=0)
    assert B.ratio(pad, ref, tol) == math.inf


def test_zero_reference_has_zero_tolerance():
    q16, g16, labels, dA = _problem(torch.float16)
    dA[:, 5] = 0.0
    only = int((labels == 1).nonzero()[0, 0])
    ex = torch.full((q16.shape[0],), only)
    dG, T, s = B.reference(q16, g16, labels, 5.5, dA, ex)
    tol = B.tolerance(T, 5.5, q16, g16, s, dA, ex)
    assert (tol[labels == 5] == 0).all() and (tol[only] == 0).all() and (dG[only] == 0).all()
    assert (tol[labels == 3] > 0).all()
    assert B.scale_exponent(torch.tensor([0.3, -0.6])) == 0 and B.scale_exponent(torch.tensor([1.0])) == 1
    assert B.scale_exponent(torch.zeros(3)) == 0


# ---- the host logic of fit / state_dict ---------------------------------------------------------------------------------
@pytest.fixture
def host_fewshot(monkeypatch):
    """clip.fewshot with its device entry points replaced by host restatements; records the backward op's `exclude`"""
    import clip.fewshot as F
    monkeypatch.setattr(F, "normalize_rows", lambda x, dtype, device=None: R.round_rows(x, dtype) if x.dtype != dtype else x)
    monkeypatch.setattr(F.ops, "cache_affinity", R.torch_cache_affinity)
    seen = []

    def backward(q, g, off, ln, beta, dA, *, exclude=None, out=None):
        seen.append(None if exclude is None else exclude.clone())
        return B.torch_cache_affinity_backward(q, g, off, ln, beta, dA, exclude=exclude, out=out)
    monkeypatch.setattr(F.ops, "cache_affinity_backward", backward, raising=False)

    def host_logits(fi, ft, log_scale):
        fi, ft = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
        return (log_scale.exp() * (fi @ ft.t()),)
    monkeypatch.setattr(F, "normalized_logits", host_logits)
    F.seen_excludes = seen
    return F


FIT_EVERY, FIT_ALPHA = 2, 5.0


def _classifier(F, dtype=torch.bfloat16, every=1, alpha=R.FIX_ALPHA, **kw):
    """the fixture's classifier.  At every = 1, alpha = 20 its leave-one-out loss is 0 to fp32: nothing to train.  The fit tests
    lower the signal: every other stored row (6 per class) and alpha = 5 give a loss of 1.11 that five epochs bring to 0.47."""
    fx = R.fewshot_fixture()
    return F.CacheClassifier(fx["features"][::every], fx["labels"][::every], num_classes=R.FIX_C, text_features=fx["text"],
                             alpha=alpha, beta=R.FIX_BETA, dtype=dtype, **kw), fx


def _loo_loss(clf):
    return torch.nn.functional.cross_entropy(clf.leave_one_out(), clf.labels).item()


def test_fit_history_exclude_and_loss_drop(host_fewshot):
    F = host_fewshot
    clf, fx = _classifier(F, every=FIT_EVERY, alpha=FIT_ALPHA)
    before, start = _loo_loss(clf), clf.features.clone()
    hist = clf.fit(epochs=5, lr=1e-3)
    assert isinstance(hist, list) and len(hist) == 5 and all(isinstance(v, float) and math.isfinite(v) for v in hist)
    assert abs(hist[0] - before) <= 1e-4 * max(1.0, before), "the first epoch's loss is the leave-one-out loss of the start"
    after = _loo_loss(clf)
    print(f"[fit] leave-one-out loss {before:.4f} -> {after:.4f}; history {hist}")
    assert after < 0.8 * before and hist[-1] < hist[0], "the fixture shows a clear drop"
    assert len(F.seen_excludes) == 5 and all(torch.equal(e, clf._pos.to(torch.int32)) for e in F.seen_excludes)
    assert clf.features.dtype == torch.bfloat16 and not torch.equal(clf.features, start)
    assert torch.equal(clf._laid[clf._pos], clf.features) and torch.isnan(clf._laid.float()).any()
    norms = clf.features.float().norm(dim=1)
    assert (norms - 1).abs().max() > 1e-3, "the trained keys are not renormalised"
    # add() still works: the new rows are appended normalised
    clf.add(fx["queries"][:3], fx["query_labels"][:3])
    assert len(clf) == 9 * 6 + 3 and (clf.features[-3:].float().norm(dim=1) - 1).abs().max() < 1e-2
    assert torch.isfinite(clf.logits(fx["queries"])).all()


def test_fit_with_train_features_and_batches(host_fewshot):
    F = host_fewshot
    clf, fx = _classifier(F, dtype=torch.float16, per_class="mean")
    hist = clf.fit(fx["queries"], fx["query_labels"], epochs=2, batch_size=32, seed=3)
    assert len(hist) == 2 and len(F.seen_excludes) == 2 * 3 and all(e is None for e in F.seen_excludes)
    a = [i.tolist() for _, i in F.fit_batches(90, 32, 2, 3)]
    b = [i.tolist() for _, i in F.fit_batches(90, 32, 2, 3)]
    assert a == b and [len(x) for x in a] == [32, 32, 26] * 2 and sorted(a[0] + a[1] + a[2]) == list(range(90)) and a[:3] != a[3:]
    assert [i.tolist() for _, i in F.fit_batches(5, None, 2, 0)] == [list(range(5))] * 2
    with pytest.raises(ValueError, match="both"):
        clf.fit(fx["queries"])
    with pytest.raises(ValueError, match="train_labels"):
        clf.fit(fx["queries"], fx["query_labels"][:5])
    with pytest.raises(ValueError, match="epochs"):
        clf.fit(epochs=0)
    with pytest.raises(ValueError, match="batch_size"):
        clf.fit(batch_size=0)
    with pytest.raises(TypeError):
        clf.fit(epochs=1, momentum=0.9)                                       # unknown arguments raise
    with pytest.raises(TypeError):
        clf.fit(None, None, 3)                                                # epochs is keyword-only


def test_queries_get_no_gradient(host_fewshot):
    F = host_fewshot
    clf, fx = _classifier(F)
    laid32 = clf._laid.float().requires_grad_(True)
    q = clf.features[:4].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="towers are frozen"):
        F.CacheAffinityFunction.apply(laid32, q, clf.class_off, clf.class_len, clf.beta, None)
    A = F.CacheAffinityFunction.apply(laid32, q.detach(), clf.class_off, clf.class_len, clf.beta, None)
    A.sum().backward()
    assert laid32.grad.shape == laid32.shape and (laid32.grad[clf._pos].abs().sum(dim=1) > 0).all()


def test_state_dict_round_trip(host_fewshot, tmp_path):
    F = host_fewshot
    clf, fx = _classifier(F, class_names=[f"k{i}" for i in range(R.FIX_C)])
    clf.fit(epochs=2)
    clf.alpha, clf.beta = 7.0, 3.0
    sd = clf.state_dict()
    assert set(sd) == set(F.CacheClassifier._STATE_KEYS)
    for v in sd.values():
        assert v is None or isinstance(v, (torch.Tensor, list, float, int, str))
    path = tmp_path / "cache.pt"
    torch.save(sd, path)
    back = F.CacheClassifier.from_state_dict(torch.load(path, weights_only=True), device="cpu")
    assert torch.equal(back.logits(fx["queries"]), clf.logits(fx["queries"])), "logits after a round trip are not bit-equal"
    assert torch.equal(back.leave_one_out(), clf.leave_one_out())
    assert (back.alpha, back.beta, back.per_class, back.class_names, back.logit_scale) == (7.0, 3.0, "sum", clf.class_names, 100.0)
    other, _ = _classifier(F, dtype=torch.float16)
    assert other.load_state_dict(sd) is other and other.dtype == torch.bfloat16
    assert torch.equal(other.logits(fx["queries"]), clf.logits(fx["queries"]))
    with pytest.raises(KeyError, match="unexpected"):
        other.load_state_dict(dict(sd, momentum=1))
    with pytest.raises(KeyError, match="missing"):
        other.load_state_dict({k: v for k, v in sd.items() if k != "labels"})
    with pytest.raises(ValueError, match="keys"):
        other.load_state_dict(dict(sd, keys=sd["keys"].float()))


def test_script_flags():
    """the new flags parse, and without them the defaults leave the old path alone (fit 0, no cache file)"""
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("fewshot_classify_flags", os.path.join(root, "scripts", "fewshot_classify.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    for argv in (["--fit"], ["--fit", "x"], ["--lr", "fast"], ["--seed", "1.5"], ["--save-cache"], ["--no-such-flag"],
                 ["--fit", "2"]):                                             # the last: neither --support nor --synthetic
        with pytest.raises(SystemExit):
            mod.main(argv)
