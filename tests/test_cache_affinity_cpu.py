"""CPU: ops.cache_layout's properties; the float64 reference and derived bound of cache_affinity_ref.py (an fp32 evaluation in
another summation order passes, each planted error exceeds the bound by at least 2x); the classification fixture's margins;
and the host logic of clip.CacheClassifier on a torch restatement of ops.cache_affinity (cache_affinity_ref.torch_cache_affinity)."""
import pytest
import torch

import cache_affinity_ref as R

SIZES = [0, 1, 15, 16, 17, 63, 65, 0, 33]


# ---- cache_layout ------------------------------------------------------------------------------------------------------
def test_layout_properties():
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(3)
    labels = torch.cat([torch.full((n,), c, dtype=torch.long) for c, n in enumerate(SIZES)])
    labels = labels[torch.randperm(labels.numel(), generator=gen)]
    C, N = len(SIZES), labels.numel()
    gather, off, ln = ops.cache_layout(labels, C)
    assert gather.dtype == torch.int64 and off.dtype == torch.int32 and ln.dtype == torch.int32
    assert off.shape == (C + 1,) and ln.shape == (C,) and not gather.is_cuda
    assert ln.tolist() == SIZES and off[0] == 0 and gather.numel() == off[-1]
    assert (off % 16 == 0).all() and (off[1:] >= off[:-1]).all()
    assert (off[1:] - off[:-1]).tolist() == [(n + 15) // 16 * 16 for n in SIZES]          # no row more than needed; empty: none
    live = gather[gather >= 0]
    assert sorted(live.tolist()) == list(range(N)), "gather is not a permutation of the rows plus -1 entries"
    for c in range(C):
        seg = gather[off[c]:off[c + 1]]
        assert (seg[:ln[c]] >= 0).all() and (seg[ln[c]:] == -1).all()
        assert seg[:ln[c]].tolist() == (labels == c).nonzero()[:, 0].tolist(), "a class's rows left their original order"


def test_layout_edge_cases():
    from cclip_hip import ops
    gather, off, ln = ops.cache_layout([], 3)
    assert gather.numel() == 0 and off.tolist() == [0, 0, 0, 0] and ln.tolist() == [0, 0, 0]
    gather, off, ln = ops.cache_layout([2, 2, 0], 4)                                          # a list; trailing empty class
    assert off.tolist() == [0, 16, 16, 32, 32] and ln.tolist() == [1, 0, 2, 0]
    assert gather[0] == 2 and gather[16:18].tolist() == [0, 1] and (gather >= 0).sum() == 3
    gather, off, ln = ops.cache_layout(torch.tensor([1, 0, 1], dtype=torch.int32), 2)
    assert gather[16:18].tolist() == [0, 2]
    for bad in ([0, 3], [-1, 0], [5]):
        with pytest.raises(ValueError, match="labels outside"):
            ops.cache_layout(bad, 3)
    with pytest.raises(ValueError):
        ops.cache_layout(torch.tensor([0.0, 1.0]), 2)
    with pytest.raises(ValueError):
        ops.cache_layout(torch.zeros(2, 2, dtype=torch.long), 2)
    with pytest.raises(ValueError):
        ops.cache_layout([0], 0)


def test_segment_checks_precede_the_library():
    """the content contract of class_off / class_len is decided on the host, before any device tensor is touched"""
    from cclip_hip import ops
    good_off, good_len = torch.tensor([0, 16, 48], dtype=torch.int32), torch.tensor([3, 20], dtype=torch.int32)
    assert ops._check_cache_segments(good_off, good_len, 48) == 2
    I = lambda *v: torch.tensor(v, dtype=torch.int32)
    for off, ln, np_ in ((I(0, 8, 48), good_len, 48), (I(0, 32, 16), I(3, 0), 16), (I(16, 32, 48), good_len, 48),
                         (good_off, good_len, 64), (good_off, I(17, 20), 48), (good_off, I(3, -1), 48), (good_off, I(3, 33), 48)):
        with pytest.raises(ValueError):
            ops._check_cache_segments(off, ln, np_)
    with pytest.raises(ValueError):
        ops._check_cache_segments(good_off, I(3), 48)
    with pytest.raises(TypeError):
        ops._check_cache_segments(good_off.long(), good_len, 48)
    with pytest.raises(NotImplementedError):
        ops._check_cache_segments(torch.zeros(258, dtype=torch.int32), torch.zeros(257, dtype=torch.int32), 0)


# ---- the bound ---------------------------------------------------------------------------------------------------------
def _fp32_other_order(q16, g16, labels, C, beta, exclude=None):
    """fp32, rows of a class in DESCENDING original order, one after the other"""
    s = q16.float() @ g16.float().t()
    e = torch.exp(torch.tensor(beta, dtype=torch.float32) * (s - 1.0))
    A = torch.zeros(q16.shape[0], C, dtype=torch.float32)
    for c in range(C):
        for n in reversed((labels == c).nonzero()[:, 0].tolist()):
            keep = torch.ones(q16.shape[0], dtype=torch.bool) if exclude is None else torch.as_tensor(exclude) != n
            A[:, c] += torch.where(keep, e[:, n], torch.zeros(()))
    return A


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,beta,normalise", [(512, 5.5, True), (96, 1.0, True), (1024, 20.0, True), (64, 5.5, False)])
def test_bound_passes_fp32_and_catches_planted_errors(D, beta, normalise, dtype):
    Q, C = 7, len(SIZES)
    q16, g16, labels = R.make_problem(11 + D, Q, SIZES, D, dtype, normalise=normalise, scale=0.05)
    N = labels.numel()
    # as in leave-one-out, the excluded row is the query's nearest stored row (two queries exclude nothing)
    exclude = (q16.double() @ g16.double().t()).argmax(dim=1)
    exclude[[1, 4]] = -1
    A, s = R.reference(q16, g16, labels, C, beta, exclude)
    tol = R.tolerance(A, beta, q16, g16, labels, s)
    assert (A[:, [0, 7]] == 0).all() and (tol[:, [0, 7]] == 0).all()
    honest = _fp32_other_order(q16, g16, labels, C, beta, exclude)
    r = R.check(honest, A, tol, f"fp32 other order D{D} beta{beta} {dtype}")
    assert r < 1.0

    e = torch.exp(beta * (s - 1.0))
    planted = {}
    n = int((labels == 5).nonzero()[3, 0])                                   # one row of class 5 (63 rows) dropped
    planted["row dropped"] = A.clone(); planted["row dropped"][:, 5] -= torch.where(exclude == n, 0.0, 1.0) * e[:, n]
    m = A.clone(); m[:, 5] -= torch.where(exclude == n, 0.0, 1.0) * e[:, n]; m[:, 6] += torch.where(exclude == n, 0.0, 1.0) * e[:, n]
    planted["row in the neighbouring class"] = m
    planted["exclude ignored"] = R.reference(q16, g16, labels, C, beta, None)[0]
    m = A.clone(); m[:, 2] += torch.exp(torch.tensor(-beta, dtype=torch.float64))          # a zero vector scores s = 0
    planted["padding row counted as a zero vector"] = m
    for what, wrong in planted.items():
        bad = R.ratio(wrong.float(), A, tol)
        print(f"[cache-planted] {what} D{D} beta{beta} {dtype}: err/tol {bad:.3e}")
        assert bad >= 2.0, f"{what}: the bound lets it through (err / tol = {bad:.3e})"


def test_reference_in_original_order_agrees_with_the_layout():
    """the reference (original order) and the restatement (laid-out order, NaN padding) describe the same sums"""
    q16, g16, labels = R.make_problem(5, 4, SIZES, 64, torch.bfloat16)
    C = len(SIZES)
    exclude = torch.tensor([0, -1, 100, 7])
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    assert torch.isnan(laid[gather < 0].float()).all() and not torch.isnan(laid[gather >= 0].float()).any()
    out = R.torch_cache_affinity(q16, laid, off, ln, 5.5, exclude=R.to_laid(exclude, gather))
    A, s = R.reference(q16, g16, labels, C, 5.5, exclude)
    R.check(out, A, R.tolerance(A, 5.5, q16, g16, labels, s), "restatement")


# ---- the classification fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
def test_fixture_margins(dtype):
    """the float64 reference alone leaves at most 1 % of the rows undecided, queries and leave-one-out rows alike, and the
    cache model is far better than the zero-shot term alone"""
    fx = R.fewshot_fixture()
    g16, q16 = R.round_rows(fx["features"], dtype), R.round_rows(fx["queries"], dtype)
    logits, tol = R.reference_logits(q16, g16, fx["labels"], R.FIX_C, R.FIX_ALPHA, R.FIX_BETA, text=fx["text"])
    ok, top = R.decided(logits, tol)
    assert (~ok).double().mean().item() <= 0.01
    acc = (top == fx["query_labels"]).double().mean().item()
    zs = R.reference_logits(q16, g16, fx["labels"], R.FIX_C, 0.0, R.FIX_BETA, text=fx["text"])[0]
    acc_zs = (zs.argmax(1) == fx["query_labels"]).double().mean().item()
    print(f"[fixture] {dtype} cache accuracy {acc:.3f}, zero-shot alone {acc_zs:.3f}")
    assert acc >= 0.95 and acc_zs <= 0.4
    loo, ltol = R.reference_logits(g16, g16, fx["labels"], R.FIX_C, R.FIX_ALPHA, R.FIX_BETA, text=fx["text"],
                                   exclude=torch.arange(g16.shape[0]))
    assert (~R.decided(loo, ltol)[0]).double().mean().item() <= 0.01


# ---- the host logic of CacheClassifier ---------------------------------------------------------------------------------
class _FakeIndex:
    def __init__(self, features, metadata, dtype):
        self.features, self.metadata, self.dtype = features, metadata, dtype


@pytest.fixture
def host_fewshot(monkeypatch):
    """clip.fewshot with its three device entry points replaced by host restatements"""
    import clip.fewshot as F
    monkeypatch.setattr(F, "normalize_rows", lambda x, dtype, device=None: R.round_rows(x, dtype) if x.dtype != dtype else x)
    monkeypatch.setattr(F.ops, "cache_affinity", R.torch_cache_affinity)

    def host_logits(fi, ft, log_scale):
        fi, ft = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
        return (log_scale.exp() * (fi @ ft.t()),)
    monkeypatch.setattr(F, "normalized_logits", host_logits)
    return F


def test_classifier_label_and_name_resolution(host_fewshot):
    F = host_fewshot
    kinds = ["gear", "fall", "gear", "site", "fall", "gear"]
    meta = [{"file_name": f"{i}.png", "violation_type": k} for i, k in enumerate(kinds)]
    rows = R.round_rows(torch.randn(6, 64, generator=torch.Generator().manual_seed(0)), torch.bfloat16)
    clf = F.CacheClassifier.from_index(_FakeIndex(rows, meta, torch.bfloat16), "violation_type")
    assert clf.class_names == ["gear", "fall", "site"] and clf.labels.tolist() == [0, 1, 0, 2, 1, 0]       # first appearance
    assert clf.num_classes == 3 and len(clf) == 6 and clf.dim == 64 and torch.equal(clf.features, rows)
    clf = F.CacheClassifier.from_index(_FakeIndex(rows, meta, torch.bfloat16), "violation_type",
                                       class_names=["fall", "blast", "site", "gear"], beta=2.0)
    assert clf.labels.tolist() == [3, 0, 3, 2, 0, 3] and clf.class_len.tolist() == [2, 0, 1, 3] and clf.beta == 2.0
    probs, idx, names = clf(image_features=rows.float())
    assert probs.shape == (6, 4) and names == [clf.class_names[i] for i in idx.tolist()]
    assert (probs[:, 1] < probs.max(dim=1).values).all()                                                  # the empty class never wins
    with pytest.raises(ValueError, match="not among class_names"):
        F.CacheClassifier.from_index(_FakeIndex(rows, meta, torch.bfloat16), "violation_type", class_names=["fall", "gear"])
    with pytest.raises(ValueError, match="has no 'caption_type'"):
        F.CacheClassifier.from_index(_FakeIndex(rows, meta, torch.bfloat16), "caption_type")
    with pytest.raises(ValueError, match="no metadata"):
        F.CacheClassifier.from_index(_FakeIndex(rows, None, torch.bfloat16), "violation_type")
    with pytest.raises(TypeError, match="unexpected"):
        F.CacheClassifier.from_index(_FakeIndex(rows, meta, torch.bfloat16), "violation_type", gamma=1)
    # the padding rows are NaN, the live ones are the class's rows in their original order
    assert torch.isnan(clf._laid.float()).all(dim=1).sum() == clf._laid.shape[0] - 6
    assert torch.equal(clf._laid[clf._pos], rows)


def test_classifier_exclude_mean_and_errors(host_fewshot):
    F = host_fewshot
    q16, g16, labels = R.make_problem(8, 5, [3, 0, 20, 1], 64, torch.bfloat16)
    clf = F.CacheClassifier(g16.float(), labels, num_classes=4, beta=3.0)
    A, s = R.reference(q16, g16, labels, 4, 3.0)
    tol = R.tolerance(A, 3.0, q16, g16, labels, s)
    R.check(clf.affinity(q16.float()), A, tol, "host affinity")
    only = int((labels == 3).nonzero()[0, 0])
    exclude = [only, -1, int((labels == 2).nonzero()[5, 0]), int((labels == 0).nonzero()[0, 0]), -1]      # ORIGINAL rows
    Ae = R.reference(q16, g16, labels, 4, 3.0, exclude)[0]
    out = clf.affinity(q16.float(), exclude=exclude)
    R.check(out, Ae, tol, "host affinity, exclude")
    assert out[0, 3] == 0 and (out[:, 1] == 0).all() and out[1, 3] > 0
    assert torch.equal(clf.affinity(q16.float(), exclude=[-1] * 5), clf.affinity(q16.float()))
    mean = F.CacheClassifier(g16.float(), labels, num_classes=4, beta=3.0, per_class="mean").affinity(q16.float())
    count = torch.tensor([3.0, 1.0, 20.0, 1.0])
    assert torch.equal(mean, clf.affinity(q16.float()) / count) and (mean[:, 1] == 0).all()
    assert torch.equal(clf.logits(q16.float(), alpha=2.0), 2.0 * clf.affinity(q16.float()))              # no text: the cache term alone
    assert torch.equal(clf.affinity(q16.float(), beta=1.0), F.CacheClassifier(g16.float(), labels, num_classes=4, beta=1.0).affinity(q16.float()))
    loo = clf.leave_one_out()
    for i in (0, only, 11):
        assert torch.equal(loo[i], clf.logits(g16[i:i + 1].float(), exclude=[i])[0])
    for bad in ([0, 1], [24, 0, 0, 0, 0], [-2, 0, 0, 0, 0], [0.0] * 5):
        with pytest.raises(ValueError, match="exclude"):
            clf.affinity(q16.float(), exclude=bad)
    with pytest.raises(ValueError, match="queries"):
        clf.affinity(torch.zeros(2, 32))
    with pytest.raises(ValueError, match="per_class"):
        F.CacheClassifier(g16.float(), labels, per_class="max")
    with pytest.raises(ValueError, match="labels"):
        F.CacheClassifier(g16.float(), labels[:-1])
    with pytest.raises(ValueError, match="labels outside"):
        F.CacheClassifier(g16.float(), labels, num_classes=3)
    with pytest.raises(ValueError, match="text_features"):
        F.CacheClassifier(g16.float(), labels, num_classes=4, text_features=torch.zeros(3, 64))
    with pytest.raises(NotImplementedError):
        F.CacheClassifier(torch.randn(4, 40), [0, 1, 0, 1])
    grown = F.CacheClassifier(g16[:10].float(), labels[:10], num_classes=4, beta=3.0).add(g16[10:].float(), labels[10:])
    assert torch.equal(grown._laid.view(torch.int16), clf._laid.view(torch.int16)) and torch.equal(grown.class_off, clf.class_off)
    assert torch.equal(grown.affinity(q16.float()), clf.affinity(q16.float()))


def test_tune_grid_and_argmax(host_fewshot):
    F = host_fewshot
    fx = R.fewshot_fixture()
    clf = F.CacheClassifier(fx["features"], fx["labels"], text_features=fx["text"], alpha=R.FIX_ALPHA, beta=R.FIX_BETA)
    assert clf.num_classes == R.FIX_C
    alphas, betas = [0.0, 1.0, 20.0, 50.0], [1.0, 5.5]
    a, b, acc, grid = clf.tune(alphas, betas)                                # leave-one-out
    assert grid.shape == (4, 2) and grid.dtype == torch.float64 and not grid.is_cuda
    want = torch.empty(4, 2, dtype=torch.float64)
    for i, al in enumerate(alphas):
        for j, be in enumerate(betas):
            want[i, j] = (clf.leave_one_out(alpha=al, beta=be).argmax(1) == fx["labels"]).double().mean()
    assert torch.equal(grid, want)
    first = int(want.reshape(-1).argmax())                                   # ties: the first grid point
    assert (a, b) == (alphas[first // 2], betas[first % 2]) and acc == want.reshape(-1)[first].item()
    assert grid[0, 0] == grid[0, 1] and grid[0, 0] < 0.5 and acc >= 0.95     # alpha = 0: the zero-shot term alone, whatever beta
    a, b, acc, grid = clf.tune(alphas, betas, fx["queries"], fx["query_labels"])
    want = torch.tensor([[(clf.logits(fx["queries"], alpha=al, beta=be).argmax(1) == fx["query_labels"]).double().mean()
                          for be in betas] for al in alphas], dtype=torch.float64)
    assert torch.equal(grid, want) and acc == want.max().item()
    with pytest.raises(ValueError, match="both"):
        clf.tune(alphas, betas, fx["queries"])
    with pytest.raises(ValueError, match="empty grid"):
        clf.tune([], betas)


def test_confusion_matrix_and_public_names():
    import clip
    from clip.fewshot import confusion_matrix
    cm = confusion_matrix(torch.tensor([0, 2, 2, 1, 0]), torch.tensor([0, 2, 1, 1, 2]), 3)
    assert cm.dtype == torch.int64 and cm.tolist() == [[1, 0, 0], [0, 1, 1], [1, 0, 1]]
    assert callable(clip.CacheClassifier) and callable(clip.confusion_matrix)
    for name in ("affinity", "logits", "leave_one_out", "tune", "add", "from_index", "from_pickle"):
        assert hasattr(clip.CacheClassifier, name)
