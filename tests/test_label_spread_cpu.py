"""CPU: the float64 label-spreading reference (tests/label_spread_ref.py) - its tolerances against planted faults and against
an fp32 restatement, its fixed point against the closed form and against scikit-learn's LabelSpreading, the planted recipe of
the end-to-end tests - and the host logic of clip/propagate.py (the affinity CSR, the argument errors) and
scripts/propagate_labels.py's argument parsing.  No case needs a device."""
import functools
import importlib
import os
import sys

import pytest
import torch

import label_spread_ref as R
import tsne_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

CONFIGS = [(600, 6, 1.0, 3), (257, 2, 0.6, 2), (300, 9, 0.8, 1)]                  # N, classes, noise, labelled per class


def P():
    return importlib.import_module("clip.propagate")


def worst(got, ref, tol):
    err = (got.double() - ref.double()).abs()
    return float("inf") if torch.isnan(err).any() else (err / tol.clamp(min=1e-300)).max().item()


@functools.lru_cache(maxsize=None)
def graph_case(N=40, C=5, seed=0):
    """A random symmetric graph with an empty row, labels on a third of the rows (class 0 twice as often), a state F"""
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(N, N, generator=g) * (torch.rand(N, N, generator=g) < 0.2)
    A.fill_diagonal_(0)
    W = (A + A.t()).float()
    W[1] = 0
    W[:, 1] = 0
    row, col = torch.nonzero(W, as_tuple=True)
    offsets = torch.searchsorted(row, torch.arange(N + 1))
    labels = torch.full((N,), -1, dtype=torch.int32)
    labels[::3] = (torch.arange(N)[::3] % (C + 1) % C).to(torch.int32)
    cw = R.class_weights_ref(labels, C)
    F = torch.rand(N, C, generator=g).float()
    return offsets, col.to(torch.int32), W[row, col], labels, cw, F


def test_exports_and_plan():
    import clip
    assert callable(clip.spread_labels) and clip.LabelSpreadResult.__name__ == "LabelSpreadResult" and callable(clip.affinity_csr)
    assert hasattr(clip.EmbeddingIndex, "spread_labels")
    from cclip_hip import load_library, ops
    lib = load_library()
    for sym in ("cclip_label_graph_normalize", "cclip_label_spread_step", "cclip_label_spread_finish", "cclip_label_spread_groups"):
        assert hasattr(lib, sym)
    assert ops.LABEL_SPREAD_MAX_C == R.MAX_C
    for C in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024):  # the reference restates the kernel's plan
        assert ops.label_spread_groups(C) == R.spread_plan(C)[1]
    assert ops.label_spread_groups(1) == 0 and ops.label_spread_groups(1025) == 0
    assert [R.spread_plan(C) for C in (2, 9, 64, 65, 129)] == [(2, 8, 1), (16, 4, 1), (64, 1, 1), (64, 1, 2), (64, 1, 4)]
    cpu = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="no CPU path"):
        ops.label_spread_finish(cpu)
    with pytest.raises(TypeError, match="no CPU path"):
        ops.label_spread_step(cpu, None, None, None, None, 0.5)
    with pytest.raises(TypeError, match="no CPU path"):
        ops.label_graph_normalize(torch.zeros(5, dtype=torch.int64), None, None)


def test_tolerances_see_the_planted_faults():
    offsets, cols, vals, labels, cw, F = graph_case()
    N, C = F.shape
    norm = R.normalize_ref(offsets, cols, vals, N)
    S = norm["vals"].float()
    seen = {}
    bad = R.normalize_ref(offsets, cols, vals, N, fault="row_norm")
    seen["row_norm"] = worst(bad["vals"], norm["vals"], norm["vals_tol"])
    step = R.step_ref(F, labels, cw, offsets, cols, S, 0.9)
    for fault in ("alpha_on_label", "drop_last", "in_place", "no_class_weight", "unlabelled_class0"):
        seen[fault] = worst(R.step_ref(F, labels, cw, offsets, cols, S, 0.9, fault=fault)["out"], step["out"], step["tol"])
    Ft = F.clone()
    Ft[3] = 0
    Ft[5, 1] = Ft[5, 4] = Ft[5].max() + 1.0                                       # an exact tie of classes 1 and 4
    fin = R.finish_ref(Ft)
    assert fin["pred"][5].item() == 1 and fin["pred"][3].item() == -1 and fin["decided"].all()
    seen["cert_log2"] = worst(R.finish_ref(Ft, fault="cert_log2")["cert"], fin["cert"], fin["cert_tol"])
    seen["tie_high"] = float((R.finish_ref(Ft, fault="tie_high")["pred"] != fin["pred"]).sum())
    seen["zero_pred0"] = float((R.finish_ref(Ft, fault="zero_pred0")["pred"] != fin["pred"]).sum())
    print("[label spread] planted faults, err / tol (or rows of pred that differ):", {k: round(v, 1) for k, v in seen.items()})
    assert set(seen) == set(R.FAULTS)
    assert all(v > 1.0 for k, v in seen.items() if k not in ("tie_high", "zero_pred0")), seen
    assert seen["tie_high"] == 1 and seen["zero_pred0"] == 1
    # the unplanted reference against itself
    assert worst(R.step_ref(F, labels, cw, offsets, cols, S, 0.9)["out"], step["out"], step["tol"]) == 0.0


def test_fp32_restatement_stays_inside_the_bounds():
    """the same formulas in fp32 torch (another summation order of depth <= n_i) must pass where the kernels must"""
    offsets, cols, vals, labels, cw, F = graph_case(N=200, C=9, seed=4)
    N, C = F.shape
    norm = R.normalize_ref(offsets, cols, vals, N)
    n32 = R.normalize_ref(offsets, cols, vals, N, dtype=torch.float32)
    r = [worst(n32["deg"], norm["deg"], norm["deg_tol"]), worst(n32["vals"], norm["vals"], norm["vals_tol"])]
    S = n32["vals"]
    step = R.step_ref(F, labels, cw, offsets, cols, S, 0.9)
    s32 = R.step_ref(F, labels, cw, offsets, cols, S, 0.9, dtype=torch.float32)
    r += [worst(s32["out"], step["out"], step["tol"]), worst(s32["delta"], step["delta"], step["delta_tol"])]
    fin, f32 = R.finish_ref(F), R.finish_ref(F, dtype=torch.float32)
    r += [worst(f32[k], fin[k], fin[k + "_tol"]) for k in ("z", "dist", "conf", "cert")]
    print("[label spread] fp32 restatement, err / tol:", [round(v, 3) for v in r])
    assert max(r) <= 1.0 and torch.equal(f32["pred"], fin["pred"])


def fake_topk(q, x, k):
    s = q.double() @ x.double().t()
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order).float(), order.to(torch.int32)


def test_affinity_csr_is_the_dense_symmetrisation():
    g = torch.Generator().manual_seed(5)
    x = torch.nn.functional.normalize(torch.randn(50, 16, generator=g), dim=1).to(torch.bfloat16)
    x[7] = x[2]
    x[9] = x[2]                                                                   # duplicate rows: similarity and affinity next to 1
    from clip.tsne import knn_graph
    s, idx = knn_graph(x, 4, topk=fake_topk)
    one_sided = sum(1 for i in range(50) for j in idx[i].tolist() if i not in idx[j].tolist())
    assert one_sided > 0                                                          # asymmetric edges are in the case
    offsets, cols, vals = P().affinity_csr(s, idx, 5.5)
    assert offsets.dtype == torch.int64 and cols.dtype == torch.int32 and vals.dtype == torch.float32
    A = torch.zeros(50, 50, dtype=torch.float64)
    A.scatter_(1, idx.long(), torch.exp(-5.5 * (1.0 - s.float())).double())
    Wd = A + A.t()
    assert offsets[-1].item() == cols.numel() == int((Wd > 0).sum())
    rows = torch.repeat_interleave(torch.arange(50), offsets.diff())
    key = rows * 50 + cols.long()
    assert (key[1:] > key[:-1]).all()
    got = tsne_ref.csr_dense(offsets, cols, vals, 50)
    assert ((got - Wd).abs() <= R.U * Wd).all()                                   # one rounding: the sum of the two directions
    assert got[2, 7].item() > 1.9 and torch.equal(got, got.t())                   # the twins name each other
    with pytest.raises(ValueError):
        P().affinity_csr(s, idx, -1.0)
    with pytest.raises(ValueError):
        P().affinity_csr(s, idx, float("nan"))


def test_fixed_point_is_the_closed_form():
    offsets, cols, vals, labels, cw, _ = graph_case(N=60, C=4, seed=2)
    S = R.normalize_ref(offsets, cols, vals, 60)["vals"].float()
    F, E, delta = R.spread_ref(labels, cw, offsets, cols, S, 0.9, 400, 4)
    want = R.closed_form(labels, cw, offsets, cols, S, 0.9, 4)
    assert (F - want).abs().max().item() <= 1e-12 and delta.max().item() <= 1e-12
    assert (F >= 0).all() and (F[1] == 0).all() and R.finish_ref(F)["pred"][1].item() == -1      # the empty row is unreachable
    assert (E >= 0).all() and E.max().item() < 1e-4


def test_reference_matches_sklearn_label_spreading():
    sk = pytest.importorskip("sklearn.semi_supervised")
    import numpy as np
    rows, truth, labels = R.planted(120, 3, 0.8, 2, seed=11)
    s, idx = tsne_ref.knn_ref(rows, 8)
    W = R.affinity_dense(s.float(), idx, 5.5)
    assert (W.sum(dim=1) > 0).all()
    model = sk.LabelSpreading(kernel=lambda X, Y: W.numpy(), alpha=0.9, max_iter=2000, tol=1e-14)
    model.fit(np.zeros((120, 1)), labels.numpy())
    row, col = torch.nonzero(W, as_tuple=True)
    offsets = torch.searchsorted(row, torch.arange(121))
    d = W.sum(dim=1)
    vals = W[row, col] / torch.sqrt(d[row] * d[col])
    # sklearn iterates F <- alpha S F + (1 - alpha) Y with a zero diagonal and normalises the rows at the end: the same
    # fixed point up to the row scale, so the normalised distributions are compared
    F, _, _ = R.spread_ref(labels, None, offsets, col.to(torch.int32), vals, 0.9, 2000, 3)
    fin = R.finish_ref(F)
    assert (fin["dist"] - torch.from_numpy(model.label_distributions_)).abs().max().item() <= 1e-9
    assert torch.equal(fin["pred"], torch.from_numpy(model.transduction_).long())


@pytest.mark.parametrize("N,Cn,noise,per", CONFIGS)
def test_planted_recipe(N, Cn, noise, per):
    """what the end-to-end tests rely on, in float64 with the exact kNN graph: every unlabelled row takes its cluster's label,
    by a wide margin, and the change of the 50th step is what alpha = 0.9 allows"""
    rows, truth, labels = R.planted(N, Cn, noise, per, seed=100 + N)
    s, idx = tsne_ref.knn_ref(rows, 10)
    ref = R.pipeline_ref(s.float(), idx, labels, max(2, Cn), 5.5, 0.9, 50)
    fin = ref["finish"]
    un = labels < 0
    two = torch.topk(fin["dist"], 2, dim=1).values
    print(f"[label spread] planted N{N}: accuracy {(fin['pred'][un] == truth[un]).double().mean().item():.4f}, smallest margin "
          f"{(two[:, 0] - two[:, 1]).min().item():.3f}, last change {ref['delta'].max().item():.2e}, largest bound on F "
          f"{(ref['E'] / ref['F'].clamp(min=1e-300)).max().item():.2e} relative")
    assert torch.equal(fin["pred"][un], truth[un]) and fin["decided"].all()
    assert (two[:, 0] - two[:, 1]).min().item() >= 0.84
    assert ref["delta"].max().item() <= 0.9 ** 50 * 0.1                           # alpha^t times the first change, itself below 1 - alpha


def test_spread_labels_argument_errors():
    p = P()
    x = torch.randn(20, 8)
    lab = [-1] * 20
    lab[0], lab[1] = 0, 1
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float("nan")), dict(beta=-1.0), dict(beta=float("inf")),
               dict(beta=float("nan")), dict(k=0), dict(k=64), dict(k=20), dict(n_classes=1), dict(n_classes=1025),
               dict(n_iter=-1), dict(check_every=-1), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            p.spread_labels(x, lab, **{**dict(k=5), **kw})
    with pytest.raises(ValueError, match="labels must be 20"):
        p.spread_labels(x, lab[:19], k=5)
    with pytest.raises(ValueError, match="labels must be"):
        p.spread_labels(x, torch.zeros(20), k=5)
    with pytest.raises(ValueError, match="no labelled row"):
        p.spread_labels(x, [-1] * 20, k=5)
    with pytest.raises(ValueError, match="label 2 with n_classes"):
        p.spread_labels(x, [0, 1, 2] + [-1] * 17, n_classes=2, k=5)
    w = p.class_weights(torch.tensor([0, 0, 2, -1, -5, 2, 2, 0]), 4)
    third = float(torch.tensor(1.0) / 3)
    assert w.tolist() == [third, 0.0, third, 0.0]
    assert torch.equal(w, R.class_weights_ref(torch.tensor([0, 0, 2, -1, -5, 2, 2, 0]), 4))


def test_propagate_labels_arguments():
    import propagate_labels as M
    a = M.parse_args(["--index", "e.pkl", "--label-key", "violation_type"])
    assert (a.k, a.beta, a.alpha, a.iters, a.min_confidence, a.suspects, a.write_labels) == (15, 5.5, 0.9, 50, 0.0, False, None)
    a = M.parse_args(["--index", "e.pkl", "--label-key", "kind", "--k", "10", "--beta", "4", "--alpha", "0.8", "--iters", "20",
                      "--min-confidence", "0.6", "--suspects", "--write-labels", "o.json", "--dtype", "fp16"])
    assert (a.k, a.beta, a.alpha, a.iters, a.min_confidence, a.suspects, a.write_labels, a.dtype) == \
        (10, 4.0, 0.8, 20, 0.6, True, "o.json", "fp16")
    for bad in ([], ["--index", "e.pkl"], ["--label-key", "kind"], ["--index", "e.pkl", "--label-key", "k", "--alpha", "1"],
                ["--index", "e.pkl", "--label-key", "k", "--beta", "-1"], ["--index", "e.pkl", "--label-key", "k", "--k", "64"],
                ["--index", "e.pkl", "--label-key", "k", "--iters", "-1"],
                ["--index", "e.pkl", "--label-key", "k", "--min-confidence", "1.5"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
    names, given = M.encode_labels(["fall", "", None, "blast", "fall"])
    assert names == ["blast", "fall"] and given == [1, -1, -1, 0, 1]
