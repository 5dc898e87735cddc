"""CPU: the references of tests/hdbscan_ref.py against each other and against brute force, the planted faults, the host tree
code of clip/hdbscan.py against the independent condensed tree and against scikit-learn, and the argument errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdbscan_ref as R  # noqa: E402

from clip.hdbscan import hdbscan, mutual_reachability_mst, tree_clusters  # noqa: E402

DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]


def host_bits(x16):
    """some fp32 score bits for the rows (any symmetric fp32 matrix serves the exact checks)"""
    x = x16.float().numpy()
    s = (x @ x.T).astype(np.float32)
    return np.maximum(s, s.T)


def core_of(S, min_samples):
    if min_samples == 1:
        return np.full(S.shape[0], np.inf, dtype=np.float32)
    return (-np.sort(-S, axis=1)[:, min_samples - 1]).astype(np.float32)


def values64(S, core):
    return R.key_values(R.mreach_keys(S, core)).astype(np.float64)


def ultrametric(levels=4):
    """N = 2^levels rows whose similarity falls with the highest bit in which two rows differ: Boruvka halves the components
    exactly once a round, so it needs every one of its ceil(log2 N) rounds"""
    N = 1 << levels
    i = np.arange(N)
    top = np.floor(np.log2(np.maximum(i[:, None] ^ i[None, :], 1))).astype(np.int64)
    S = (0.9 - 0.1 * top).astype(np.float32)
    np.fill_diagonal(S, 1.0)
    return S


def fault_cases():
    out = []
    for seed in range(10):
        for ms in (1, 2, 3):
            S = host_bits(R.random_rows(24 + 3 * seed, 32, seed, torch.bfloat16, dup_fraction=0.3))
            out.append((S, core_of(S, ms)))
    S = ultrametric()
    out.append((S, core_of(S, 1)))
    return out


@pytest.fixture(scope="module")
def cases():
    return fault_cases()


def test_exact_mst_weights_equal_prim():
    for seed in range(20):
        N = 5 + (seed * 7) % 36                                      # 5 .. 40
        S = host_bits(R.random_rows(N, 32, 100 + seed, DTYPES[seed % 2], dup_fraction=0.25 if seed % 3 == 0 else 0.0))
        core = core_of(S, 1 + seed % 5)
        tree = R.exact_mst(S, core)
        assert R.is_spanning_tree(N, [e[0] for e in tree], [e[1] for e in tree])
        M = values64(S, core)
        edges, total = R.prim(M)
        mine = np.sort(R.key_values(np.array([e[2] for e in tree], dtype=np.uint64)).astype(np.float64))
        assert np.array_equal(mine, np.sort([M[a, b] for a, b in edges]))      # every maximum spanning tree has these weights
        assert abs(mine.sum() - total) <= 1e-12 * N


def test_exact_mst_equals_enumeration_with_duplicates():
    for seed in range(12):
        N = 4 + seed % 4                                             # 4 .. 7
        x = R.random_rows(N, 32, 200 + seed, DTYPES[seed % 2])
        x[N - 1] = x[0]
        x[N - 2] = x[1 if seed % 2 else 0]                           # bitwise copies: exact ties
        S = host_bits(x)
        for ms in (1, 2, 3):
            core = core_of(S, ms)
            assert R.exact_mst(S, core) == R.brute_force_mst(S, core), (seed, ms)


def test_boruvka_restatement_is_exact_without_fault(cases):
    for S, core in cases:
        u, v, m = R.boruvka_np(S, core)
        assert (u >= 0).sum() == len(core) - 1
        assert R.edge_set(u, v, m) == R.exact_mst(S, core)
        ok, ratio = R.check_mst(u[u >= 0], v[u >= 0], values64(S, core), 1e-12)
        assert ok and ratio == 0.0


def three_pairs():
    """Six rows in three close pairs {0, 5}, {1, 4}, {2, 3} (0.9) with every other similarity tied at 0.5.  After round 0
    the components are named 0, 1, 2 and every outgoing edge ties, so only the total order keeps their choices apart."""
    S = np.full((6, 6), 0.5, dtype=np.float32)
    for a, b in ((0, 5), (1, 4), (2, 3)):
        S[a, b] = S[b, a] = 0.9
    np.fill_diagonal(S, 1.0)
    return S, core_of(S, 1)


def one_sparse_row():
    """Three rows, row 1 with a low core: the true tree is {0, 2} (0.8) and {0, 1} (0.6 = core_1)."""
    S = np.array([[1.0, 0.9, 0.8], [0.9, 1.0, 0.5], [0.8, 0.5, 1.0]], dtype=np.float32)
    return S, np.array([np.inf, 0.6, np.inf], dtype=np.float32)


# For every planted fault a case on which it provably breaks the tree, so that BOTH checks must see it on EVERY case listed:
#   mask, stale  the ultrametric set needs all four rounds.  A search that ignores comp returns, from round 1 on, every row's
#                partner of round 0 (inside its component: no hook): 8 of 15 edges.  Labels one round old do the same in
#                rounds 1 and 3: 12 of 15 edges.
#   tie_high     three_pairs, round 1: the rows of component 0 = {0, 5} name row 4, the highest outside, and the reduction
#                keeps {0, 4}; the rows of component 1 = {1, 4} name row 5 and it keeps {1, 5}.  Two different edges between
#                the same two components: neither sees a mutual choice, both hang and record - 6 edges on 6 rows, a cycle.
#   m_only       three_pairs, round 1: a reduction by m alone lets the last row met win, {1, 5} for component 0 and {0, 4} for
#                component 1 - the same cycle.
#   no_core_j    one_sparse_row: row 0 sees its edge to row 1 at 0.9, row 1 sees it at 0.6; the two keys differ, no mutual
#                choice is seen and both rows hang under each other: 3 recorded edges on 3 rows, one with m = 0.9, which no pair has.
def all_rounds():
    S = ultrametric()
    return S, core_of(S, 1)


PROVABLE = {"mask": [all_rounds], "stale": [all_rounds], "tie_high": [three_pairs], "m_only": [three_pairs],
            "no_core_j": [one_sparse_row]}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_round_faults_are_caught(fault):
    assert PROVABLE[fault]
    for make in PROVABLE[fault]:
        S, core = make()
        want, M = R.exact_mst(S, core), values64(S, core)
        u, v, m = R.boruvka_np(S, core)                              # the restatement itself is right on the case
        assert R.edge_set(u, v, m) == want and R.check_mst(u[u >= 0], v[u >= 0], M, 1e-12) == (True, 0.0)
        u, v, m = R.boruvka_np(S, core, fault)
        live = u >= 0
        assert R.edge_set(u, v, m) != want or live.sum() != len(core) - 1, (fault, make.__name__)
        assert not R.check_mst(u[live], v[live], M, 1e-12)[0], (fault, make.__name__)


def test_edge_list_faults_are_caught(cases):
    S, core = cases[1]
    mk, M = R.mreach_keys(S, core), values64(S, core)
    want = R.exact_mst(S, core)
    heavier = R.swap_heavier(want, mk)
    assert heavier is not None and heavier != want
    assert not R.check_mst([e[0] for e in heavier], [e[1] for e in heavier], M, 1e-12)[0]
    u, v, m = R.sort_edges(want)
    u2, v2 = u.copy(), v.copy()
    u2[-1], v2[-1] = u2[0], v2[0]                                    # an edge emitted twice
    assert R.edge_set(u2, v2, m) != want
    assert not R.check_mst(u2, v2, M, 1e-12)[0]
    assert R.check_mst(u, v, M, 1e-12) == (True, 0.0)


def float64_tree(x16, min_samples):
    """sorted float64 tree edges of the rows: (u, v, chord length)"""
    S = R.scores64(x16)
    M = R.mreach64(S, R.core64(S, min_samples))
    edges, _ = R.prim(M)
    w = np.array([M[a, b] for a, b in edges])
    order = np.argsort(-w, kind="stable")
    return (np.array([edges[k][0] for k in order]), np.array([edges[k][1] for k in order]), R.chord64(w[order]))


@pytest.mark.parametrize("method", ["eom", "leaf"])
def test_host_tree_equals_plain_loop_reference(method):
    sets = [R.planted_recipe(torch.bfloat16)[0]]
    sets += [R.random_rows(30 + 11 * s, 32, 300 + s, DTYPES[s % 2], dup_fraction=0.3 * (s % 2)) for s in range(6)]
    for x in sets:
        for ms, mcs, single in ((1, 2, False), (2, 3, True), (5, 5, False), (5, 10, True)):
            u, v, d = float64_tree(x, ms)
            labels, prob, pers = tree_clusters(len(x), u, v, d, mcs, method, single)
            rl, rp = R.ref_clusters(len(x), u, v, d, mcs, method, single)
            assert np.array_equal(labels, rl)
            assert np.abs(prob - rp).max() <= 1e-12
            assert len(pers) == labels.max() + 1
    u, v, d = np.array([0, 2, 0]), np.array([1, 3, 2]), np.array([0.5, 0.5, 0.5])       # tied weights: merges in edge order
    for single in (False, True):
        labels, prob, _ = tree_clusters(4, u, v, d, 2, method, single)
        rl, rp = R.ref_clusters(4, u, v, d, 2, method, single)
        assert np.array_equal(labels, rl) and np.abs(prob - rp).max() <= 1e-12


def test_lambda_from_similarity_is_caught():
    x, _ = R.planted_recipe(torch.bfloat16)
    u, v, d = float64_tree(x, 5)
    labels, prob, _ = tree_clusters(len(x), u, v, d, 10)
    _, wrong = R.ref_clusters(len(x), u, v, d, 10, lam_of=lambda dist: 1.0 / max(dist * dist / 2.0, 1e-6))   # 1 - m, not the chord
    assert np.abs(prob - wrong).max() > 1e-3


def test_small_sets():
    for single, want in ((False, -1), (True, 0)):
        labels, prob, pers = tree_clusters(1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), 5, "eom", single)
        assert labels.tolist() == [want] and len(pers) == (want + 1)
        labels, prob, pers = tree_clusters(2, np.array([0]), np.array([1]), np.array([0.3]), 5, "eom", single)
        assert labels.tolist() == [want, want] and len(pers) == (want + 1)
        assert prob.tolist() == ([1.0, 1.0] if single else [0.0, 0.0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("min_samples", [5, 10])
def test_against_scikit_learn(dtype, min_samples):
    """sklearn.cluster.HDBSCAN(metric="precomputed") on the float64 chord matrix of the planted recipe: four clusters of 40,
    the 12 noise rows -1, ARI 1 against the planted labels; our labels equal up to renaming.  Largest probability difference
    measured: 0.0 in all four cases (bound 1e-6)."""
    from sklearn.cluster import HDBSCAN
    x, planted = R.planted_recipe(dtype)
    dist = R.chord64(R.scores64(x))
    np.fill_diagonal(dist, 0.0)
    sk = HDBSCAN(min_cluster_size=10, min_samples=min_samples, metric="precomputed").fit(dist)
    assert sorted(np.bincount(sk.labels_[sk.labels_ >= 0]).tolist()) == [40, 40, 40, 40]
    assert np.all(sk.labels_[planted < 0] == -1) and R.adjusted_rand(sk.labels_, planted) == 1.0
    u, v, d = float64_tree(x, min_samples)
    labels, prob, pers = tree_clusters(len(x), u, v, d, 10)
    assert R.same_partition(labels, sk.labels_) and np.array_equal(labels < 0, sk.labels_ < 0)
    assert labels[0] == 0 and labels[40] == 1 and labels[80] == 2 and labels[120] == 3        # numbered by the lowest row
    diff = float(np.abs(prob - sk.probabilities_).max())
    print(f"[hdbscan] sklearn {IDS[DTYPES.index(dtype)]} min_samples={min_samples}: largest probability difference {diff:.3g}")
    assert diff <= 1e-6
    assert len(pers) == 4 and np.all(pers > 0)


def test_argument_errors_before_any_device():
    x = torch.randn(20, 32)
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan(x, min_samples=0)
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan(x, min_samples=21)                                   # above N
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan(torch.randn(100, 32), min_samples=65)                # above the top-k kernel's 64
    with pytest.raises(ValueError, match="min_samples"):
        mutual_reachability_mst(x, min_samples=0)
    with pytest.raises(ValueError, match="min_cluster_size"):
        hdbscan(x, min_cluster_size=1)
    with pytest.raises(ValueError, match="cluster_selection"):
        hdbscan(x, cluster_selection="dbscan")
    with pytest.raises(ValueError, match="float"):
        hdbscan(torch.zeros(20, 32, dtype=torch.int64))
    with pytest.raises(ValueError, match="float"):
        mutual_reachability_mst(torch.zeros(20, 32, dtype=torch.int64))


def test_ops_refuse_cpu_tensors():
    from cclip_hip import ops
    x = torch.zeros(4, 32, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="cuda"):
        ops.mreach_nearest(x, torch.zeros(4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="cuda"):
        ops.mst_boruvka(x, torch.zeros(4))
