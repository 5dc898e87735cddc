"""CPU: the float64 t-SNE reference (tests/tsne_ref.py) against autograd, its calibration, its tolerances against planted
faults, the host logic of clip/tsne.py (self-removal in the kNN graph, the CSR symmetrisation, the argument errors) and
scripts/map_images.py's argument parsing.  No case needs a device."""
import functools
import importlib
import math
import os
import sys

import pytest
import torch

import kmeans_ref
import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)


def T():
    return importlib.import_module("clip.tsne")


@functools.lru_cache(maxsize=None)
def planted():
    """the planted set in bf16, its float64 kNN graph at k = 30 and the reference's conditional and joint P at perplexity 10"""
    feats, labels = R.planted_map_case()
    x = feats / feats.norm(dim=1, keepdim=True)
    x16 = x.to(torch.bfloat16)
    s, idx = R.knn_ref(x16, 30)
    P, beta, info = R.affinities_ref(s.float(), 10.0)
    return x16, labels, s.float(), idx, P, beta, info, R.joint_dense(P, idx)


def random_state(N, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    y = (scale * torch.randn(N, 2, generator=g)).float()
    vel = (0.1 * torch.randn(N, 2, generator=g)).float()
    gains = (0.5 + torch.rand(N, 2, generator=g)).float()
    A = torch.rand(N, N, generator=g, dtype=torch.float64) * (torch.rand(N, N, generator=g) < 0.3)
    A.fill_diagonal_(0)
    Pd = A + A.t()
    return y, vel, gains, Pd / Pd.sum()


def test_exports():
    import clip
    assert callable(clip.tsne) and clip.TSNEResult.__name__ == "TSNEResult"
    assert hasattr(clip.EmbeddingIndex, "knn_graph") and hasattr(clip.EmbeddingIndex, "tsne")
    from cclip_hip import ops
    for name in ("tsne_affinities", "tsne_repulsion", "tsne_repulsion_workspace", "tsne_step"):
        assert callable(getattr(ops, name))
    from cclip_hip import load_library
    lib = load_library()
    for sym in ("cclip_tsne_affinities", "cclip_tsne_repulsion", "cclip_tsne_repulsion_workspace", "cclip_tsne_step"):
        assert hasattr(lib, sym)
    for N in (1, 2, 511, 512, 513, 4099, 8192, 8193, 20000, 200000):            # the reference restates the kernel's plan
        assert ops.tsne_repulsion_splits(N) == R.split_plan(N)[1]
        assert ops.tsne_repulsion_workspace(N) == (3 * N * R.split_plan(N)[1] + -(-N // 256)) * 4
    assert (ops.TSNE_TILE, ops.TSNE_SPLIT_MAX, ops.TSNE_BISECT_STEPS, ops.TSNE_MAX_K) == (R.TILE, R.SPLIT_MAX, R.BISECT_STEPS, R.MAX_K)
    assert ops.tsne_repulsion_splits(20000) * -(-20000 // 256) >= 512             # N = 20 000 fills 256 CUs at least twice


def test_reference_gradient_is_autograd_of_the_dense_kl():
    y32, vel, gains, Pd = random_state(40, 1)
    y = y32.double().requires_grad_(True)
    R.kl_ref(Pd, y).backward()
    closed = R.grad_ref(Pd, y.detach())
    assert (closed - y.grad).abs().max().item() <= 1e-10
    rep = R.repulsion_ref(y32)
    st = R.step_ref(y32, vel, gains, Pd, rep["rep"], rep["Z"], 1.0, 0.8, 100.0, 0.01)
    assert (st["grad"] - y.grad).abs().max().item() <= 1e-10
    assert abs(st["kl_row"].sum().item() - R.kl_ref(Pd, y32).item()) <= 1e-10


def test_every_calibrated_row_meets_the_perplexity():
    _, _, s, _, P, beta, info, _ = planted()
    assert not info["degenerate"].any()
    assert (info["H"] - math.log(10.0)).abs().max().item() <= 1e-9
    assert (P.sum(dim=1) - 1).abs().max().item() <= 1e-12
    for k, perp in ((2, 1.5), (5, 1.5), (33, 20.0), (63, 20.0), (63, 5.0)):
        g = torch.Generator().manual_seed(k)
        sc = (0.2 + 0.6 * torch.rand(50, k, generator=g)).float()
        sc[3] = 0.5                                                               # all equal: uniform
        sc[5, 0] = 1.0                                                            # an exact duplicate among far ones
        sc[5, 1:] = 0.1 * torch.rand(k - 1, generator=g)
        sc[7, 0] = float("nan")
        P, beta, info = R.affinities_ref(sc, perp)
        good = ~info["degenerate"]
        good[7] = False
        assert info["degenerate"][3] and not info["degenerate"][5] and int(good.sum()) >= 47
        assert (info["H"][good] - math.log(perp)).abs().max().item() <= 1e-9
        assert torch.equal(P[3], torch.full((k,), 1.0 / k, dtype=torch.float64)) and beta[3].item() == 2.0 ** 100
        assert torch.isnan(P[7]).all() and torch.isnan(beta[7]) and not torch.isnan(P[[6, 8]]).any()


def worst(err, tol):
    return (err / tol.clamp(min=1e-300)).max().item()


def test_tolerances_see_the_planted_faults():
    x16, _, s, idx, P, beta, info, Pd = planted()
    # repulsion: a mid-run map
    y32, vel, gains, Pr = random_state(257, 5)
    good = R.repulsion_ref(y32)
    diag = R.repulsion_ref(y32, fault="diag")
    assert abs(diag["Z"] - good["Z"]) > good["Z_tol"] and worst((diag["zrow"] - good["zrow"]).abs(), good["zrow_tol"]) > 1
    w1 = R.repulsion_ref(y32, fault="w1")
    assert worst((w1["rep"] - good["rep"]).abs(), good["rep_tol"]) > 1
    # step
    args = (y32, vel, gains, Pr, good["rep"], good["Z"], 12.0, 0.5, 200.0, 0.01)
    st = R.step_ref(*args)
    assert st["decided"].double().mean().item() >= 0.99
    for fault in ("no_4", "ex_on_rep"):
        bad = R.step_ref(*args, fault=fault)
        assert worst((bad["grad"] - st["grad"]).abs(), st["grad_tol"]) > 1, fault
        assert worst((bad["y"] - st["y"]).abs(), st["y_tol"]) > 1, fault
    bad = R.step_ref(*args, fault="gains_inverted")
    assert worst((bad["gains"] - st["gains"]).abs()[st["decided"]], st["gains_tol"][st["decided"]]) > 1
    # affinities
    for fault in ("bits", "drop_last"):
        Pb, bb, _ = R.affinities_ref(s, 10.0, fault=fault)
        assert worst((Pb - P).abs(), info["P_tol"]) > 1, fault
    assert worst((R.affinities_ref(s, 10.0, fault="bits")[1] - beta).abs(), info["beta_tol"]) > 1
    # d2 not shifted by its minimum is the same function in exact arithmetic; in the kernel's fp32 every exp(-beta d2) of a
    # row of far neighbours (d2 near 2, differences of 1e-3) underflows before beta is found
    g = torch.Generator().manual_seed(9)
    far = (0.02 + 1e-3 * torch.rand(20, 30, generator=g)).float()
    Pf, bf, inf_f = R.affinities_ref(far, 10.0)
    assert not inf_f["degenerate"].any() and bf.min().item() > 200
    P32, b32, _ = R.affinities_ref(far, 10.0, dtype=torch.float32)
    assert worst((P32.double() - Pf).abs(), inf_f["P_tol"]) <= 1 and worst((b32.double() - bf).abs(), inf_f["beta_tol"]) <= 1
    Pn, bn, _ = R.affinities_ref(far, 10.0, fault="no_shift", dtype=torch.float32)
    err = (Pn.double() - Pf).abs()
    assert torch.isnan(err).any() or worst(err, inf_f["P_tol"]) > 1


def test_fp32_restatement_stays_inside_the_bounds():
    """the bounds are not vacuous the other way: the same arithmetic in fp32 on the host meets them"""
    _, _, s, _, P, beta, info, _ = planted()
    P32, b32, _ = R.affinities_ref(s, 10.0, dtype=torch.float32)
    assert worst((b32.double() - beta).abs(), info["beta_tol"]) <= 1
    assert worst((P32.double() - P).abs(), info["P_tol"]) <= 1


def fake_topk(x, g, k):
    """similarity_topk's contract on the host: float64 scores, descending, equal scores by the lower index"""
    s = x.double() @ g.double().t()
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order).float(), order.to(torch.int32)


def test_knn_graph_drops_the_row_itself_among_exact_duplicates():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 32, generator=g)
    x = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    x[7] = x[2]
    x[9] = x[2]                                                                   # rows 2, 7, 9 are one row
    x[11] = x[4]
    for k in (1, 2, 5, 11):
        s, idx = T().knn_graph(x, k, topk=fake_topk)
        assert s.shape == (12, k) and idx.dtype == torch.int32
        assert not (idx == torch.arange(12)[:, None]).any()
        rs, ri = R.knn_ref(x, k)
        assert torch.equal(idx.long(), ri) and torch.equal(s.double(), rs.float().double())
    s, idx = T().knn_graph(x, 1, topk=fake_topk)                                  # row 9: both twins rank ahead of it
    assert idx[9, 0].item() == 2 and idx[7, 0].item() == 2 and idx[2, 0].item() == 7
    # where the row itself is not among the k + 1 (more than k copies ahead), the last entry goes
    y = x[2:3].repeat(5, 1)
    s, idx = T().knn_graph(y, 2, topk=fake_topk)
    assert idx.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1], [0, 1]]
    with pytest.raises(ValueError, match="top-k kernel"):
        T().knn_graph(x.repeat(8, 1), 64, topk=fake_topk)
    with pytest.raises(ValueError):
        T().knn_graph(x, 12, topk=fake_topk)
    with pytest.raises(ValueError):
        T().knn_graph(x, 0, topk=fake_topk)


def test_joint_csr_is_the_dense_symmetrisation():
    _, _, _, idx, P, _, _, Pd = planted()
    offsets, cols, vals = T().joint_csr(P.float(), idx.to(torch.int32))
    N = P.shape[0]
    assert offsets.dtype == torch.int64 and cols.dtype == torch.int32 and vals.dtype == torch.float32
    assert offsets[0].item() == 0 and offsets[-1].item() == cols.numel() == int((Pd > 0).sum())
    rows = torch.repeat_interleave(torch.arange(N), offsets.diff())
    key = rows * N + cols.long()
    assert (key[1:] > key[:-1]).all()                                             # ascending columns inside ascending rows
    assert (R.csr_dense(offsets, cols, vals, N) - Pd).abs().max().item() <= 3 * R.U * Pd.max().item()
    assert abs(vals.double().sum().item() - 1.0) <= 1e-5
    # a row nobody names and that names nobody cannot exist, but a row with one-sided edges only keeps them
    P2 = torch.tensor([[1.0], [1.0], [1.0]])
    off, c, v = T().joint_csr(P2, torch.tensor([[1], [0], [0]], dtype=torch.int32))
    assert off.tolist() == [0, 2, 3, 4] and c.tolist() == [1, 2, 0, 0]
    assert torch.allclose(v, torch.tensor([2.0, 1.0, 2.0, 1.0]) / 6.0)


def test_learning_rate_and_argument_errors():
    t = T()
    assert t.auto_learning_rate(600, 12.0) == 50.0 and t.auto_learning_rate(20000, 12.0) == 20000 / 12.0 / 4.0
    assert t.neighbour_count(600, 10.0) == 30 and t.neighbour_count(4, 2.0) == 3 and t.neighbour_count(1000, 21.0) == 63
    with pytest.raises(ValueError, match="top-k kernel"):
        t.neighbour_count(1000, 21.5)
    with pytest.raises(ValueError, match="below k"):
        t.neighbour_count(4, 3.0)
    with pytest.raises(ValueError, match="above 1"):
        t.neighbour_count(100, 1.0)
    with pytest.raises(ValueError):
        t.neighbour_count(1, 2.0)
    from cclip_hip import ops
    cpu = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="no CPU path"):
        ops.tsne_affinities(cpu, 2.0)
    with pytest.raises(TypeError, match="no CPU path"):
        ops.tsne_repulsion(torch.zeros(4, 2))
    with pytest.raises(TypeError, match="no CPU path"):
        ops.tsne_step(torch.zeros(4, 2), None, None, None, None, None, None, None)


def test_map_images_arguments():
    import map_images as M
    a = M.parse_args(["--synthetic"])
    assert a.synthetic and a.label_key == "violation_type" and a.learning_rate == "auto" and a.clusters is None and a.png is None
    a = M.parse_args(["--index", "e.pkl", "--label-key", "kind", "--clusters", "8", "--png", "m.png", "--learning-rate", "150",
                      "--perplexity", "12", "--n-iter", "300"])
    assert (a.index, a.label_key, a.clusters, a.png, a.learning_rate, a.perplexity, a.n_iter) == ("e.pkl", "kind", 8, "m.png", 150.0, 12.0, 300)
    for bad in ([], ["--index", "e.pkl", "--clusters", "0"], ["--index", "e.pkl", "--learning-rate", "fast"],
                ["--index", "e.pkl", "--learning-rate", "-1"], ["--index", "e.pkl", "--n-iter", "-1"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
    feats, caps = M.synthetic_embeddings()
    assert feats.shape == (540, 64) and len(caps) == 540 and caps[0]["clip_embedding"] == 0 and caps[0]["violation_type"]
    assert len(set(M.palette(9))) == 9


def test_the_float64_loop_separates_the_planted_set():
    """pins the condition of tests/test_tsne_gpu.py: on this set the loop itself, in float64 and in fp32, gives 1-NN agreement 1.0"""
    _, labels, _, _, _, _, _, Pd = planted()
    y0 = 1e-4 * torch.randn(600, 2, generator=torch.Generator().manual_seed(0))
    for dtype in (torch.float64, torch.float32):
        y, kls, kl = R.loop_ref(Pd, y0, 500, kl_at=(249,), dtype=dtype)
        assert torch.isfinite(y).all() and y.mean(dim=0).abs().max().item() <= 1e-4 * y.std().item()
        assert R.one_nn_agreement(y, labels) == 1.0
        assert kl < kls[249]


def test_joint_p_matches_sklearn():
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    import numpy as np
    feats, _ = R.planted_map_case()
    x16 = (feats[:120] / feats[:120].norm(dim=1, keepdim=True)).to(torch.bfloat16)
    N = x16.shape[0]
    s, idx = R.knn_ref(x16, N - 1)
    P, beta, info = R.affinities_ref(s.float(), 10.0)
    ours = R.joint_dense(P, idx)
    d2 = torch.zeros(N, N).scatter_(1, idx, (2.0 - 2.0 * s.float()).clamp(min=0))
    from scipy.spatial.distance import squareform
    theirs = torch.from_numpy(squareform(sk._joint_probabilities(d2.numpy().astype(np.float32), 10.0, 0))).double()
    # sklearn stops its bisection at |H - log perplexity| <= 1e-5: beta moves by 1e-5 / (beta Var), P by p |diff - mean| times that
    diff = R.diffs32(s.float()).double()
    mean = (P * diff).sum(dim=1, keepdim=True)
    var = (P * (diff - mean) ** 2).sum(dim=1)
    cond_tol = P * (diff - mean).abs() * (2e-5 / (beta * var))[:, None] + 1e-6 * P + 1e-12
    tol = R.joint_dense(cond_tol, idx)
    assert ((ours - theirs).abs() <= tol).all()
