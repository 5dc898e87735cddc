"""CPU: the float64 k-means reference (tests/kmeans_ref.py) against a naive loop, its Lloyd loop on planted data, and the
host-side pieces of clip/cluster.py and scripts/cluster_images.py.  No kernel runs here."""
import math
import os
import sys

import pytest
import torch

import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_round16_rounds_once(dtype):
    p, _ = R.P16[dtype]
    one = torch.tensor([1.0], dtype=torch.float64)
    ulp = 2.0 ** (1 - p)                                                    # spacing in [1, 2)
    # just above the midpoint of 1 and 1 + ulp: one rounding goes up; a cast through fp32 first lands ON the midpoint, then to even
    v = one + ulp / 2 + 2.0 ** -40
    assert R.round16(v, dtype).double().item() == 1.0 + ulp
    assert v.float().to(dtype).double().item() == 1.0
    assert R.round16(one + ulp / 2, dtype).double().item() == 1.0           # the exact midpoint: to even
    assert R.round16(one + 3 * ulp / 2, dtype).double().item() == 1.0 + 2 * ulp
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).to(dtype)
    assert torch.equal(R.round16(x.double(), dtype), x)                     # representable values stay
    tiny = torch.tensor([2.0 ** -20, -2.0 ** -24 * 1.5, 0.0], dtype=torch.float64)
    assert torch.equal(R.round16(tiny, torch.float16).double(), torch.tensor([2.0 ** -20, -2.0 ** -23, 0.0], dtype=torch.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_assign_ref_against_naive_loop(dtype):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(40, 32, generator=gen).to(dtype)
    c = torch.randn(7, 32, generator=gen).to(dtype)
    c[3] = c[1]                                                             # an exact tie for every row
    c[5, 0] = float("nan")
    x[9] = 0
    a, b, s2 = R.assign_ref(x, c)
    for n in range(40):
        sc = [sum(float(x[n, d]) * float(c[k, d]) for d in range(32)) for k in range(7)]
        rank = sorted(range(7), key=lambda k: (math.isnan(sc[k]), -sc[k] if not math.isnan(sc[k]) else 0.0, k))
        assert a[n].item() == rank[0] and rank[0] != 5 and rank[0] != 3
        assert abs(b[n].item() - sc[rank[0]]) <= 1e-12 and abs(s2[n].item() - sc[rank[1]]) <= 1e-12
    a1, b1, s1 = R.assign_ref(x, c[:1])
    assert a1.tolist() == [0] * 40 and torch.isnan(s1).all()
    inf = torch.zeros(1, 32).to(dtype)
    inf[0, 0] = 1
    cc = torch.zeros(3, 32).to(dtype)
    cc[0, 0], cc[1, 0], cc[2, 0] = float("nan"), float("-inf"), float("nan")
    a2, b2, s2 = R.assign_ref(inf, cc)
    assert a2.item() == 1 and b2.item() == -float("inf") and math.isnan(s2.item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_update_ref_against_naive_loop(dtype):
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(50, 32, generator=gen).to(dtype)
    x[11] = -x[10]
    assign = torch.randint(0, 5, (50,), generator=gen)
    assign[assign == 2] = 1                                                 # cluster 2 empty
    assign[assign == 4] = 0
    assign[10] = assign[11] = 4                                             # cluster 4 cancels to zero
    prev = torch.randn(5, 32, generator=gen).to(dtype)
    r = R.update_ref(x, assign, 5, prev)
    for k in range(5):
        rows = [n for n in range(50) if assign[n] == k]
        assert r["counts"][k].item() == len(rows)
        s = [sum(float(x[n, d]) for n in rows) for d in range(32)]
        nrm = math.sqrt(sum(v * v for v in s))
        if k in (2, 4):
            assert r["keep"][k] and r["norm"][k].item() == 0 and torch.equal(r["c"][k], prev[k].double())
        else:
            assert not r["keep"][k] and abs(r["norm"][k].item() - nrm) <= 1e-12 * nrm
            assert max(abs(r["c"][k, d].item() - s[d] / nrm) for d in range(32)) <= 1e-12
            assert (r["f32_tol"][k] > 0).all() and r["eta"][k] < 1e-4
    c16, _ = R.update_ref16(x, assign, 5, prev)
    assert torch.equal(c16[2], prev[2]) and torch.equal(c16[4], prev[4]) and c16.dtype == dtype


@pytest.mark.parametrize("D", [64, 128])
def test_reference_lloyd_recovers_the_planted_partition_from_random_init(D):
    sizes = [60, 80, 100, 120]
    feats, truth, _ = R.planted(sizes, D, 0.3, 17 + D)
    x16 = feats.to(torch.bfloat16)
    found = None
    for seed in range(8):                                                   # a random start may put two rows of one group first
        pick = torch.randperm(x16.shape[0], generator=torch.Generator().manual_seed(seed))[:4]
        out = R.lloyd_ref(x16, x16[pick])
        objs = [h["objective"] for h in out["history"]]
        # Lloyd's steps never lower the mean score for exact centroids; the centroids here are rounded to bf16 as the device's
        # are, which moves a unit row by at most 2^-9 of its length and so every score, before and after, by at most 2^-9
        assert all(b >= a - 2 * 2.0 ** -9 for a, b in zip(objs, objs[1:])), f"seed {seed}: the objective decreased: {objs}"
        assert out["n_iter"] == len(out["history"]) <= 50
        assert out["counts"].sum().item() == x16.shape[0]
        if R.same_partition(out["labels"], truth):
            found = seed
            assert out["converged"]
            assert sorted(out["counts"].tolist()) == sorted(sizes)
            assert (out["concentration"] > 0.8).all() and (out["concentration"] <= 1.0 + 1e-3).all()
            break
    assert found is not None, "no random start of 8 recovered the planted partition"


def reseed_case(dtype=torch.bfloat16):
    """three planted groups and an init whose second centroid, far from every row, appears twice: both copies win no row"""
    feats, truth, dirs = R.planted([60, 50, 70], 64, 0.3, 3)
    away = -dirs.sum(dim=0, keepdim=True)
    init = torch.cat([dirs[:1], away, away])
    return feats.to(dtype), truth, (init / init.norm(dim=1, keepdim=True)).to(dtype)


def test_reference_lloyd_reseeds_empty_clusters():
    x16, truth, init = reseed_case()
    kept = R.lloyd_ref(x16, init, reseed_empty=False)
    assert kept["history"][0]["counts"].tolist() == [180, 0, 0] and kept["counts"].tolist() == [180, 0, 0]
    assert torch.equal(kept["centroids"][1:], init[1:]) and kept["converged"] and kept["n_iter"] == 2
    assert kept["concentration"][1:].tolist() == [0.0, 0.0]
    reseeded = R.lloyd_ref(x16, init, reseed_empty=True)
    assert reseeded["history"][0]["counts"].tolist() == [180, 0, 0]
    assert (reseeded["counts"] > 0).all() and reseeded["converged"]
    assert reseeded["objective"] > kept["objective"]


def test_cluster_purity_on_hand_made_input():
    import clip
    labels = [0, 0, 0, 1, 1, 2, 2, 2, 2, 4]
    classes = [5, 5, 7, 7, -1, 3, 1, 1, 3, -1]
    purity, major = clip.cluster_purity(labels, classes)
    assert major.tolist() == [5, 7, 1, -1, -1]                              # 2: a tie of 1 and 3 goes to the lower; 3 empty; 4 unlabelled
    assert purity == pytest.approx((2 + 1 + 2) / 8)
    purity, major = clip.cluster_purity(torch.tensor([1, 1]), torch.tensor([-1, -1]))
    assert purity == 0.0 and major.tolist() == [-1, -1]
    with pytest.raises(ValueError):
        clip.cluster_purity([0, 1], [0])


def test_representatives_padding_and_ties():
    from clip.cluster import KMeansResult, representatives
    labels = torch.tensor([2, 0, 2, 2, 0, 3, 2])
    scores = torch.tensor([0.5, 0.9, 0.7, 0.7, 0.9, 0.1, 0.2])
    rep = representatives(labels, scores, 5, 3)
    assert rep.dtype == torch.int64 and rep.tolist() == [[1, 4, -1], [-1, -1, -1], [2, 3, 0], [5, -1, -1], [-1, -1, -1]]
    assert representatives(labels, scores, 5, 1).tolist() == [[1], [-1], [2], [5], [-1]]
    res = KMeansResult(centroids=torch.zeros(5, 32), labels=labels, scores=scores, margin=scores, counts=torch.bincount(labels, minlength=5),
                       concentration=torch.zeros(5), objective=0.0, n_iter=1, converged=True)
    assert res.representatives(2).tolist() == [[1, 4], [-1, -1], [2, 3], [5, -1], [-1, -1]]
    with pytest.raises(ValueError):
        representatives(labels, scores, 5, 0)


def test_n_init_tie_rule():
    from clip.cluster import pick_best_run
    assert pick_best_run([0.5]) == 0
    assert pick_best_run([0.5, 0.7, 0.6]) == 1
    assert pick_best_run([0.7, 0.7, 0.7]) == 0                              # equal objectives: the lower seed
    assert pick_best_run([0.1, 0.7, 0.7]) == 1


def test_kmeans_argument_errors_need_no_kernel():
    import clip
    with pytest.raises(ValueError, match="2-D float"):
        clip.kmeans(torch.zeros(4, dtype=torch.float32), 2)
    with pytest.raises(ValueError, match="2-D float"):
        clip.kmeans(torch.zeros(4, 32, dtype=torch.int64), 2)


def test_script_argument_parsing_and_majority_labels(capsys):
    import cluster_images
    a = cluster_images.parse_args(["--index", "e.pkl", "--k", "8"])
    assert (a.k, a.show, a.dtype, a.init, a.n_init, a.seed, a.label_key, a.write_labels) == (8, 3, "bf16", "kmeans++", 1, 0, None, None)
    a = cluster_images.parse_args(["--index", "e.pkl", "--k", "4", "--show", "2", "--label-key", "violation_type", "--dtype", "fp16",
                                   "--init", "random", "--write-labels", "o.json", "--tol", "0.01", "--max-iter", "7"])
    assert (a.show, a.label_key, a.dtype, a.init, a.write_labels, a.tol, a.max_iter) == (2, "violation_type", "fp16", "random", "o.json", 0.01, 7)
    for bad in (["--k", "8"], ["--index", "e.pkl"], ["--index", "e.pkl", "--k", "0"], ["--index", "e.pkl", "--k", "2", "--show", "0"],
                ["--index", "e.pkl", "--k", "2", "--checkpoint", "w.pt"], ["--index", "e.pkl", "--k", "2", "--init", "pca"]):
        with pytest.raises(SystemExit):
            cluster_images.parse_args(bad)
    capsys.readouterr()
    got = cluster_images.majority_labels([0, 0, 0, 0, 1, 1, 2, 2, 2], ["a", "b", "b", "", "", None, "z", "y", ""], 4)
    assert got == [("b", 2 / 3, 1), (None, 0.0, 2), ("y", 0.5, 1), (None, 0.0, 0)]


def test_analysis_wrappers_refuse_host_tensors_before_the_library(monkeypatch):
    """every wrapper of the embedding-analysis family (k-means and what was built beside it): well-formed host tensors are a
    TypeError raised by the argument checks, before the library is loaded - there is no host path"""
    import cclip_hip._lib as L
    from cclip_hip import ops

    def boom():
        raise AssertionError("the library must not be touched")
    monkeypatch.setattr(L, "load_library", boom)
    x, c = torch.zeros(3, 32).bfloat16(), torch.zeros(2, 32).bfloat16()
    f, i = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    _, class_off, class_len = ops.cache_layout([0, 1, 0], 2)
    off, cols, vals = torch.tensor([0, 2, 3, 4]), i(4), f(4)
    calls = {
        "similarity_topk": lambda: ops.similarity_topk(x, c, 2),
        "similarity_range": lambda: ops.similarity_range(x, c, 0.5),
        "lm_head_score": lambda: ops.lm_head_score(x, c, i(3)),
        "cache_affinity": lambda: ops.cache_affinity(x, torch.zeros(32, 32).bfloat16(), class_off, class_len, 5.5),
        "cache_affinity_backward": lambda: ops.cache_affinity_backward(x, torch.zeros(32, 32).bfloat16(), class_off, class_len, 5.5, f(3, 2)),
        "kmeans_assign": lambda: ops.kmeans_assign(x, c),
        "kmeans_update": lambda: ops.kmeans_update(x, i(3), 2, c),
        "coreset_step": lambda: ops.coreset_step(x, f(3), i(3), torch.zeros(1, dtype=torch.int64), centre=0),
        "coreset_greedy": lambda: ops.coreset_greedy(x, f(3), i(3), 2, first=0),
        "mreach_nearest": lambda: ops.mreach_nearest(x, f(3), i(3)),
        "mst_boruvka": lambda: ops.mst_boruvka(x, f(3)),
        "probe_forward": lambda: ops.probe_forward(x, f(2, 32), f(2), i(3)),
        "probe_backward": lambda: ops.probe_backward(x, f(2, 32), f(2), i(3), f(3), 0.5, 0.0),
        "tsne_affinities": lambda: ops.tsne_affinities(f(3, 3), 2.0),
        "tsne_repulsion": lambda: ops.tsne_repulsion(f(3, 2)),
        "tsne_step": lambda: ops.tsne_step(f(3, 2), f(3, 2), f(3, 2), off, cols, vals, f(3, 2), f(1)),
        "label_graph_normalize": lambda: ops.label_graph_normalize(off, cols, vals),
        "label_spread_step": lambda: ops.label_spread_step(f(3, 2), i(3), off, cols, vals, 0.9),
        "label_spread_finish": lambda: ops.label_spread_finish(f(3, 2)),
        "concept_codes": lambda: ops.concept_codes(x, c, 0.1, 0.5, 2),
    }
    for name, call in calls.items():
        with pytest.raises(TypeError, match="cuda") as info:
            call()
        assert name in str(info.value), f"{name}: {info.value}"
