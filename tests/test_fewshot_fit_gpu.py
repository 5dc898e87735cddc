"""CacheClassifier.fit / state_dict on the MI355X, on the seeded fixture of cache_affinity_ref.py with its signal lowered (every
other stored row, alpha = 5: at 12 rows per class and alpha = 20 the leave-one-out loss is 0 to fp32 and there is nothing to
train): the gradient of the leave-one-out cross-entropy through CacheAffinityFunction against float64 autograd, the loss drop,
the loss history against a torch run of the same trajectory, save and reload, the refusal of a query gradient, the script.

Measured on the MI355X: the loss history differs from the torch run's by at most 9.537e-07 (bf16) and 5.960e-07 (fp16), see
HISTORY_DIFF below; the gradient's largest err / tol is 3.3e-3 (bf16) and 5.1e-3 (fp16)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import cache_affinity_bwd_ref as B
import cache_affinity_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["bf16", "fp16"]
EVERY, ALPHA = 2, 5.0

# largest |loss history (HIP kernels) - loss history (torch composition + autograd on the host)| over 5 epochs, measured on
# the MI355X: 9.537e-07 for bf16, 5.960e-07 for fp16 (8 and 5 fp32 ulps of losses between 1.1 and 0.45).  Both sides are
# deterministic; the test allows 4 x the measured value for rounding-path differences of the host side.
HISTORY_DIFF = {torch.bfloat16: 9.537e-07, torch.float16: 5.960e-07}


def classifier(dtype, **kw):
    import clip
    fx = R.fewshot_fixture()
    clf = clip.CacheClassifier(fx["features"][::EVERY], fx["labels"][::EVERY], num_classes=R.FIX_C, text_features=fx["text"],
                               alpha=ALPHA, beta=R.FIX_BETA, dtype=dtype, **kw)
    return clf, fx


def loo_loss(clf):
    return torch.nn.functional.cross_entropy(clf.leave_one_out(), clf._labels_dev).item()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_gradient_against_float64_autograd(dtype):
    """d(mean leave-one-out cross-entropy)/d(keys).  The reference differentiates the float64 logits of cache_affinity_ref
    with autograd; its dA = alpha / Q * (softmax - onehot) goes through the closed form for the bound, so tol carries the
    factor alpha / Q.  On top of the kernel's bound: the product's dA is taken from ITS logits, off by at most ltol (the
    forward bound of reference_logits), which moves a softmax entry p by at most p (exp(2 max ltol) - 1), and from an fp32
    softmax and cross-entropy gradient (16 roundings of 2^-24 on p + onehot, with room); both enter as a weight of their own."""
    from clip.fewshot import CacheAffinityFunction
    clf, fx = classifier(dtype)
    g16, labels = clf.features.cpu(), clf.labels
    N, C, beta = g16.shape[0], R.FIX_C, R.FIX_BETA
    own = torch.arange(N)
    # the product: keys fp32 [N, E] -> laid-out -> A -> logits -> loss
    keys = clf.features.float().requires_grad_(True)
    laid32 = torch.full((clf._laid.shape[0], clf.dim), float("nan"), device="cuda").index_put((clf._pos,), keys)
    A = CacheAffinityFunction.apply(laid32, clf.features, clf.class_off, clf.class_len, beta, clf._pos.to(torch.int32))
    logits = clf._zero_shot16(clf.features) + ALPHA * A
    torch.nn.functional.cross_entropy(logits, clf._labels_dev).backward()
    got = keys.grad.cpu()
    # float64 autograd through the forward reference's formula
    g = g16.double().requires_grad_(True)
    e = torch.exp(beta * (g16.double() @ g.t() - 1.0))
    Aref = torch.where(torch.eye(N, dtype=torch.bool), torch.zeros_like(e), e) @ torch.nn.functional.one_hot(labels, C).double()
    qd, td = g16.double(), fx["text"].double()
    zs = 100.0 * ((qd / qd.norm(dim=1, keepdim=True)) @ (td / td.norm(dim=1, keepdim=True)).t())
    ref_logits = zs + ALPHA * Aref
    torch.nn.functional.cross_entropy(ref_logits, labels).backward()
    want = g.grad
    chk, ltol = R.reference_logits(g16, g16, labels, C, ALPHA, beta, text=fx["text"], exclude=own)
    assert (chk - ref_logits.detach()).abs().max().item() < 1e-9
    # the bound
    p = ref_logits.detach().softmax(dim=1)
    onehot = torch.nn.functional.one_hot(labels, C).double()
    dA = (ALPHA / N) * (p - onehot)
    ddA = (ALPHA / N) * (p * torch.expm1(2.0 * ltol.max(dim=1, keepdim=True).values) + 16 * 2.0 ** -24 * (p + onehot))
    dG, T, s = B.reference(g16, g16, labels, beta, dA.float(), own)
    assert (dG - want).abs().max().item() <= 1e-6 * T.max().item(), "closed form on the fp32 dA and autograd disagree"
    _, T2, _ = B.reference(g16, g16, labels, beta, ddA, own)
    tol = B.tolerance(T, beta, g16, g16, s, dA.float(), own) + T2 + T * 2.0 ** -23     # (dA rounded to fp32 for the closed form)
    r = B.ratio(got, want, tol)
    print(f"[fit-grad] {dtype} err/tol {r:.3e}; largest |grad| {want.abs().max().item():.3e}")
    assert not torch.isnan(got).any() and r <= 1.0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_fit_drops_the_loss_and_follows_the_torch_trajectory(dtype, monkeypatch):
    import clip.fewshot as F
    clf, fx = classifier(dtype)
    start = clf.state_dict()
    before = loo_loss(clf)
    hist = clf.fit(epochs=5, lr=1e-3, seed=0)
    after = loo_loss(clf)
    print(f"[fit] {dtype} leave-one-out loss {before:.5f} -> {after:.5f}; history {hist}")
    assert len(hist) == 5 and all(math.isfinite(v) for v in hist)
    assert after < 0.8 * before and hist[-1] < 0.8 * hist[0]
    assert abs(hist[0] - before) < 1e-4
    # tune() and the other methods use the trained keys
    a, b, acc, grid = clf.tune((1.0, 5.0, 20.0), (1.0, 5.5))
    assert 0.0 <= acc <= 1.0 and torch.equal(clf._laid[clf._pos], clf.features)
    # the same trajectory with torch ops on the host: the same fit() on the same start, its two ops replaced by the
    # composition matmul, exp, one-hot matmul (cache_affinity_ref.torch_cache_affinity) and autograd through it
    def autograd_backward(q, g, off, ln, beta, dA, *, exclude=None, out=None):
        Np, C = g.shape[0], ln.numel()
        rows = torch.arange(Np)
        cls = torch.bucketize(rows, off[1:].long(), right=True).clamp(max=C - 1)
        live = rows < (off[:-1].long() + ln.long())[cls]
        g32 = torch.where(live[:, None], g.float(), torch.zeros(())).requires_grad_(True)
        with torch.enable_grad():
            e = torch.exp(beta * (q.float() @ g32.t() - 1.0))
            take = live[None, :] if exclude is None else live[None, :] & (rows[None, :] != exclude.long()[:, None])
            A = torch.where(take, e, torch.zeros_like(e)) @ torch.nn.functional.one_hot(cls, C).float()
            return torch.autograd.grad(A, g32, dA)[0]

    def host_logits(fi, ft, log_scale):
        fi, ft = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
        return (log_scale.exp() * (fi @ ft.t()),)
    monkeypatch.setattr(F.ops, "cache_affinity", R.torch_cache_affinity)
    monkeypatch.setattr(F.ops, "cache_affinity_backward", autograd_backward)
    monkeypatch.setattr(F, "normalized_logits", host_logits)
    host = F.CacheClassifier.from_state_dict(start, device="cpu")
    assert torch.equal(host.features, start["keys"])
    host_hist = host.fit(epochs=5, lr=1e-3, seed=0)
    diff = max(abs(x - y) for x, y in zip(hist, host_hist))
    print(f"[fit-trajectory] {dtype} largest history difference {diff:.3e}; torch run {host_hist}")
    assert diff <= 4.0 * HISTORY_DIFF[dtype]


def test_state_dict_round_trip_and_query_gradient(tmp_path):
    import clip
    from clip.fewshot import CacheAffinityFunction
    clf, fx = classifier(torch.bfloat16, class_names=[f"k{i}" for i in range(R.FIX_C)])
    clf.fit(fx["queries"], fx["query_labels"], epochs=2, batch_size=32, seed=1)           # augmented-view style: nothing excluded
    path = tmp_path / "cache.pt"
    torch.save(clf.state_dict(), path)
    back = clip.CacheClassifier.from_state_dict(torch.load(path, weights_only=True), device="cuda")
    want, got = clf.logits(fx["queries"]), back.logits(fx["queries"])
    assert torch.equal(want.view(torch.int32), got.view(torch.int32)), "logits after save and reload are not bit-equal"
    assert back.class_names == clf.class_names and (back.alpha, back.beta) == (clf.alpha, clf.beta)
    q = clf.features[:5].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="towers are frozen"):
        CacheAffinityFunction.apply(clf._laid.float().requires_grad_(True), q, clf.class_off, clf.class_len, clf.beta, None)


def test_fewshot_script_fit_save_load(tmp_path):
    script, path = os.path.join(ROOT, "scripts", "fewshot_classify.py"), str(tmp_path / "cache.pt")

    def run(*flags):
        r = subprocess.run([sys.executable, script, "--synthetic", *flags], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    first = run("--fit", "2", "--seed", "3", "--save-cache", path)
    assert first[0]["fit"] is True and first[0]["epochs"] == 2 and math.isfinite(first[0]["last_loss"]) and len(first) == 1 + 27
    second = run("--load-cache", path)
    assert second[0]["loaded"] == path and second[0]["support"] == 81 and len(second) == 1 + 27
    assert [r["predicted"] for r in second[1:]] == [r["predicted"] for r in first[1:]]
    assert [r["probabilities"] for r in second[1:]] == [r["probabilities"] for r in first[1:]]
