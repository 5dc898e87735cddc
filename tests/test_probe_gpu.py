"""clip.LinearProbe on the MI355X: L-BFGS on the probe kernels against the float64 reference (tests/probe_ref.py) - two fresh
fits bitwise equal, descent and the stopping rule in float64, balanced weights, the zero-shot start, the inference entries,
from_index, sweep_l2, persistence, and the memory of one objective evaluation."""
import functools

import pytest
import torch

import probe_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
L2, TOL, ITERS = 1e-3, 1e-4, 200


@functools.lru_cache(maxsize=None)
def data(dtype):
    """5 classes, 400 unit rows around 5 random directions in D = 64, plus 12 rows of label -1; shared, never written to"""
    x16, y, dirs = R.planted_rows([80] * 5, 64, 0.5, 21, dtype)
    extra = R.planted_rows([12], 64, 0.5, 22, dtype)[0]
    return torch.cat([x16, extra]), torch.cat([y, torch.full((12,), -1)]), dirs


@functools.lru_cache(maxsize=None)
def fitted(dtype):
    import clip
    x16, y, _ = data(dtype)
    p = clip.LinearProbe(64, 5, dtype=dtype)
    res = p.fit(x16.cuda(), y, l2=L2, tol=TOL, max_iter=ITERS)
    return p, res


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fit_is_bitwise_reproducible_descends_and_stops(dtype):
    import clip
    x16, y, _ = data(dtype)
    p1, r1 = fitted(dtype)
    p2 = clip.LinearProbe(64, 5, dtype=dtype)
    r2 = p2.fit(x16.cuda(), y, l2=L2, tol=TOL, max_iter=ITERS)
    assert torch.equal(p1.W.view(torch.int32), p2.W.view(torch.int32)) and torch.equal(p1.bias.view(torch.int32), p2.bias.view(torch.int32))
    assert r1.as_dict() == r2.as_dict(), (r1, r2)
    scale = 1.0 / 400
    assert r1.scale == scale and r1.n_iter >= 1 and r1.n_eval > r1.n_iter
    W, b = p1.W.cpu(), p1.bias.cpu()
    ref = R.reference(x16, W, b, y, None, scale, L2)
    ref0 = R.reference(x16, torch.zeros_like(W), torch.zeros_like(b), y, None, scale, L2)
    print(f"[probe-fit] {dtype}: {r1} objective64 {ref['objective'].item():.6f} from {ref0['objective'].item():.6f}")
    assert ref["objective"].item() < ref0["objective"].item()
    assert abs(r1.objective - ref["objective"].item()) <= ref["obj_tol"].item()
    # the stopping rule in float64: max |gradient| within tol plus the derived gradient bound
    gnorm = max(ref["dW"].abs().max().item(), ref["db"].abs().max().item())
    gbound = max(ref["dW_tol"].max().item(), ref["db_tol"].max().item())
    print(f"[probe-fit] {dtype}: float64 max |grad| {gnorm:.3e} tol {TOL:.1e} bound {gbound:.3e} converged {r1.converged}")
    assert r1.converged and gnorm <= TOL + gbound
    # accuracy: where the float64 fit reaches 100 %, so does the device's
    W64, b64 = R.lbfgs_fit64(x16, y, 5, None, scale, L2, ITERS, TOL)
    live = y >= 0
    z64 = x16.double() @ W64.t() + b64
    assert (z64.argmax(dim=1)[live] == y[live]).all(), "the float64 reference fit does not separate the data"
    assert p1.score(x16.cuda(), y) == 1.0


def test_balanced_weights_reach_the_kernel(monkeypatch):
    import clip
    from cclip_hip import ops
    x16, y, _ = R.planted_rows([200, 20], 64, 0.5, 31, torch.bfloat16)
    seen = []
    real = ops.probe_backward

    def spy(x, W, bias, labels, lse, scale, l2, row_weight=None, **kw):
        seen.append((scale, None if row_weight is None else row_weight.clone()))
        return real(x, W, bias, labels, lse, scale, l2, row_weight, **kw)

    monkeypatch.setattr(ops, "probe_backward", spy)
    p = clip.LinearProbe(64, 2)
    p.fit(x16.cuda(), y, l2=1e-2, max_iter=5, class_weight="balanced")
    scale, rw = seen[0]
    raw = torch.where(y == 0, torch.tensor(220 / (2 * 200.0), dtype=torch.float64), torch.tensor(220 / (2 * 20.0), dtype=torch.float64))
    assert torch.equal(rw.cpu(), (raw / raw.max()).float()) and abs(scale - raw.max().item() / 220) < 1e-12
    assert all(s == scale for s, _ in seen)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_zero_shot_start(dtype):
    import clip
    x16, y, dirs = data(dtype)
    p = clip.LinearProbe(64, 5, dtype=dtype)
    res = p.fit(x16.cuda(), y, l2=0.0, max_iter=3, init="zero_shot", text_features=dirs, logit_scale=100.0)
    ref = R.reference(x16, (dirs * 100.0).float(), None, y, None, 1.0 / 400, 0.0)
    print(f"[probe-fit] zero-shot start {p.initial_objective:.6f} float64 {ref['objective'].item():.6f} tol {ref['obj_tol'].item():.2e}")
    assert abs(p.initial_objective - ref["objective"].item()) <= ref["obj_tol"].item()
    assert res.objective <= p.initial_objective
    with pytest.raises(ValueError):
        p.fit(x16.cuda(), y, init="zero_shot")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_inference_entries_agree(dtype):
    import clip
    x16, y, _ = data(dtype)
    p, _ = fitted(dtype)
    xd = x16.cuda()
    pred, proba = p.predict(xd), p.predict_proba(xd)
    probs, idx, names = p(image_features=xd)
    assert torch.equal(pred, idx) and torch.equal(proba, probs) and names == idx.tolist()
    assert torch.equal(proba.argmax(dim=1), pred) and (proba.sum(dim=1) - 1).abs().max().item() < 1e-5
    ref = R.reference(x16, p.W.cpu(), p.bias.cpu(), None)
    top2 = ref["z"].topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * ref["z_tol"].max(dim=1).values
    assert sure.sum() > 300 and torch.equal(pred.cpu()[sure], ref["pred"][sure])
    live = y >= 0
    assert abs(p.score(xd, y) - (pred.cpu()[live] == y[live]).double().mean().item()) < 1e-12
    with pytest.raises(TypeError):
        p.predict(x16)                                                      # a CPU tensor raises: no eager fallback
    q = clip.LinearProbe.from_state_dict(p.state_dict(), "cuda")
    assert torch.equal(q.predict(xd), pred) and torch.equal(q.predict_proba(xd).view(torch.int32), proba.view(torch.int32))


def test_from_index_and_sweep():
    import clip
    x16, y, _ = R.planted_rows([60] * 4, 64, 0.9, 41, torch.bfloat16)
    names = ["a", "b", "c", "d"]
    index = clip.EmbeddingIndex(x16.float(), metadata=[dict(kind=names[i]) for i in y.tolist()])
    p = clip.LinearProbe.from_index(index, "kind", names, l2=1e-2, max_iter=30)
    q = clip.LinearProbe(64, class_names=names)
    q.fit(index.features, y, l2=1e-2, max_iter=30)
    assert torch.equal(p.W.view(torch.int32), q.W.view(torch.int32)) and p.class_names == names
    rows = index.features
    tr, va = rows[:180].contiguous(), rows[180:].contiguous()
    s = clip.LinearProbe(64, class_names=names)
    table = s.sweep_l2(tr, y[:180], va, y[180:], [1.0, 1e-2, 1e-4], max_iter=30)
    accs = [r["val_accuracy"] for r in table]
    k = accs.index(max(accs))
    assert [r["best"] for r in table] == [i == k for i in range(3)] and s.l2 == table[k]["l2"]
    assert s.score(va, y[180:]) == accs[k]


def test_memory_of_one_evaluation():
    """N = 262144, C = 256, D = 64: workspace + outputs + 1 MB stays under a quarter of the fp32 N x C matrix (256 MB)."""
    from cclip_hip import ops
    N, C, D = 262144, 256, 64
    bound = ops.probe_workspace(N, C, D) + 3 * 4 * N + 4 * (C * D + C + 1) + (1 << 20)
    assert bound < N * C * 4 // 4
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, D, generator=gen).bfloat16().cuda()
    W, b = torch.randn(C, D, generator=gen).cuda(), torch.zeros(C).cuda()
    y = torch.randint(0, C, (N,), generator=gen).to(torch.int32).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    lse, loss, _, _ = ops.probe_forward(x, W, b, y)
    dW, db, obj = ops.probe_backward(x, W, b, y, lse, 1.0 / N, 1e-3, loss=loss)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[probe-memory] N {N} C {C} D {D}: peak rise {rise} bytes, bound {bound}, fp32 N x C {N * C * 4}")
    assert rise <= bound and torch.isfinite(obj).all()
