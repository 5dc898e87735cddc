"""clip.tsne on the MI355X through the public surface, for bf16 and fp16: a planted set must come apart in the plane, maps are
bitwise repeatable, `init=` is honoured, the loop agrees with the float64 reference step by step inside a real run (each
step from the GPU's own state: trajectories are chaotic, single steps are not), the kNN graph never names a row its own
neighbour, the memory stays N O(k), and scripts/map_images.py runs end to end."""
import functools
import importlib
import json
import os
import sys

import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def planted_run(dtype):
    import clip
    feats, labels = R.planted_map_case()
    return feats, labels, clip.tsne(feats, perplexity=10, n_iter=500, log_every=50, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planted_set_comes_apart(dtype):
    feats, labels, res = planted_run(dtype)
    y = res.embedding
    assert y.shape == (600, 2) and y.dtype == torch.float32 and res.n_iter == 500
    assert torch.isfinite(y).all() and torch.isfinite(res.beta).all() and res.kl_divergence == res.kl_divergence
    agree = R.one_nn_agreement(y, labels)
    hist = dict(res.kl_history)
    print(f"[tsne] planted {dtype}: 1-NN agreement {agree:.4f}, KL entering iteration 249 {hist[249]:.4f}, final KL {res.kl_divergence:.4f}")
    assert agree >= 0.95
    assert sorted(hist) == list(range(49, 500, 50)) and res.kl_divergence < hist[249]
    assert y.mean(dim=0).abs().max().item() <= 1e-4 * y.std().item()
    assert res.knn_index.shape == (600, 30) and res.knn_index.dtype == torch.int32 and res.beta.shape == (600,)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_repeatable_and_seeded(dtype):
    import clip
    feats, _, res = planted_run(dtype)
    again = clip.tsne(feats, perplexity=10, n_iter=500, log_every=50, dtype=dtype)
    assert same_bits(res.embedding, again.embedding) and res.kl_divergence == again.kl_divergence and res.kl_history == again.kl_history
    other = clip.tsne(feats, perplexity=10, n_iter=60, seed=1, dtype=dtype)
    base = clip.tsne(feats, perplexity=10, n_iter=60, seed=0, dtype=dtype)
    assert not same_bits(other.embedding, base.embedding)
    index = clip.EmbeddingIndex(feats, dtype=dtype)
    assert same_bits(index.tsne(perplexity=10, n_iter=60).embedding, base.embedding)


def test_init_is_honoured():
    import clip
    feats, _ = R.planted_map_case()
    init = torch.randn(600, 2, generator=torch.Generator().manual_seed(5)) + 3.0
    res = clip.tsne(feats, perplexity=10, n_iter=0, init=init)
    want = init.to("cuda") - init.to("cuda").mean(dim=0, keepdim=True)
    assert same_bits(res.embedding, want) and res.n_iter == 0 and res.kl_divergence > 0
    with pytest.raises(ValueError):
        clip.tsne(feats, perplexity=10, init=init[:10])
    with pytest.raises(ValueError, match="top-k kernel"):
        clip.tsne(feats, perplexity=30)
    with pytest.raises(ValueError):
        clip.tsne(feats, perplexity=10, learning_rate="fast")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_steps_match_the_reference_inside_a_real_run(dtype):
    """drive clip.tsne's loop with the ops; at six iterations apply the float64 reference to the GPU's own state"""
    from cclip_hip import ops
    T = importlib.import_module("clip.tsne")
    from clip.retrieval import normalize_rows
    feats, _ = R.planted_map_case()
    N = 600
    x = normalize_rows(feats, dtype)
    scores, index = T.knn_graph(x, 30)
    P, beta = ops.tsne_affinities(scores, 10.0)
    offsets, cols, vals = T.joint_csr(P, index)
    Pd = R.csr_dense(offsets.cpu(), cols.cpu(), vals.cpu(), N)
    lr = T.auto_learning_rate(N, 12.0)
    y = (1e-4 * torch.randn(N, 2, generator=torch.Generator().manual_seed(0))).to("cuda")
    y2, vel, gains = torch.empty_like(y), torch.zeros_like(y), torch.ones_like(y)
    worst = 0.0
    for it in range(500):
        ex, mom = (12.0, 0.5) if it < 250 else (1.0, 0.8)
        check = it in (0, 1, 50, 249, 250, 499)
        if check:
            before = (y.cpu(), vel.cpu(), gains.cpu())
        zrow, rep, z = ops.tsne_repulsion(y)
        _, kl = ops.tsne_step(y, vel, gains, offsets, cols, vals, rep, z, exaggeration=ex, momentum=mom, learning_rate=lr,
                              min_gain=0.01, out_y=y2)
        if check:
            rr = R.repulsion_ref(before[0])
            st = R.step_ref(*before, Pd, rr["rep"], rr["Z"], ex, mom, lr, 0.01, rep_tol=rr["rep_tol"], Z_tol=rr["Z_tol"])
            d = st["decided"]
            if it > 0:                                                            # at iteration 0 every velocity is exactly zero
                assert d.double().mean().item() >= 0.99
            pairs = [("zrow", zrow, rr["zrow"], rr["zrow_tol"]), ("rep", rep, rr["rep"], rr["rep_tol"]),
                     ("Z", z[0], rr["Z"], rr["Z_tol"]), ("kl_row", kl, st["kl_row"], st["kl_tol"]),
                     ("gains", gains.cpu()[d], st["gains"][d], st["gains_tol"][d]), ("vel", vel.cpu()[d], st["vel"][d], st["vel_tol"][d]),
                     ("y", y2.cpu()[d], st["y"][d], st["y_tol"][d])]
            for name, got, ref, tol in pairs:
                err = (got.double().cpu() - ref).abs()
                r = (err / tol.clamp(min=1e-300)).max().item() if err.numel() else 0.0
                print(f"[tsne] loop {dtype} iteration {it} {name}: largest err / tol {r:.3f}")
                assert r <= 1.0 and not torch.isnan(err).any(), (it, name)
                worst = max(worst, r)
        y, y2 = y2, y
    print(f"[tsne] loop {dtype}: largest err / tol over the six iterations {worst:.3f}")


def test_four_rows():
    import clip
    g = torch.Generator().manual_seed(2)
    res = clip.tsne(torch.randn(4, 64, generator=g), perplexity=2, n_iter=50)
    assert res.embedding.shape == (4, 2) and torch.isfinite(res.embedding).all() and res.knn_index.shape == (4, 3)
    assert res.kl_divergence == res.kl_divergence


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_knn_graph_with_exact_copies(dtype):
    import clip
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(200, 64, generator=g)
    feats[150] = feats[20]
    feats[77] = feats[20]                                                         # rows 20, 77, 150 are one row
    index = clip.EmbeddingIndex(feats, dtype=dtype)
    x16 = index.features.cpu()
    # equal to the float64 top-k (ties by the lower index) wherever float64 decides the order: with tol the score kernel's
    # bound (D 2^-22 for unit rows, kmeans_ref.assign_tol), a run of neighbours whose consecutive float64 scores lie within
    # 2 tol may come in any order, unless all of them tie exactly (copies of one row: the same bits on the device too)
    tol = 64 * 2.0 ** -22
    full, fi = R.knn_ref(x16, 199)
    gaps = full[:, :-1] - full[:, 1:]
    near = gaps <= 2 * tol
    run = torch.cat([torch.zeros(200, 1, dtype=torch.long), torch.cumsum((~near).long(), dim=1)], dim=1)     # the run of every position
    impure = torch.zeros(200, 199).scatter_add_(1, run[:, :-1], (near & (gaps != 0)).float())
    decided = torch.gather(impure, 1, run) == 0
    assert decided.double().mean().item() > 0.9
    for k in (1, 2, 10, 63):
        s, idx = index.knn_graph(k)
        assert s.shape == (200, k) and idx.dtype == torch.int32 and s.dtype == torch.float32
        assert not (idx.cpu() == torch.arange(200)[:, None]).any()
        assert (s.cpu().double() - full[:, :k]).abs().max().item() <= tol
        assert torch.equal(idx.cpu().long()[decided[:, :k]], fi[:, :k][decided[:, :k]])
    assert set(index.knn_graph(2)[1][20].tolist()) == {77, 150} and index.knn_graph(2)[1][150].tolist() == [20, 77]
    with pytest.raises(ValueError):
        index.knn_graph(64)


def test_memory_stays_linear_in_n():
    import clip
    N = 20000
    g = torch.Generator().manual_seed(8)
    feats = torch.randn(N, 64, generator=g)
    x = clip.EmbeddingIndex(feats).features
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = clip.tsne(x, perplexity=10, n_iter=5)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    dense = 4 * N * N
    print(f"[tsne] N = {N}: peak {peak / 2 ** 20:.1f} MiB above the rows; one dense N x N fp32 matrix is {dense / 2 ** 20:.0f} MiB")
    assert torch.isfinite(res.embedding).all()
    assert peak < dense / 4


def test_map_images_script(capsys, tmp_path):
    import map_images as M
    png = tmp_path / "map.png"
    lines, summary = M.main(["--synthetic", "--n-iter", "250", "--clusters", "4", "--png", str(png)])
    out = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 540 and len(out) == 541 and "summary" in out[-1]
    for ln in out[:-1]:
        assert ln["x"] == ln["x"] and ln["y"] == ln["y"] and abs(ln["x"]) < float("inf") and abs(ln["y"]) < float("inf")
        assert ln["label"] and 0 <= ln["cluster"] < 4 and ln["file_name"]
    try:
        import PIL  # noqa: F401
        assert png.exists() and summary["png"] == str(png)
    except ImportError:
        assert "png" not in summary
