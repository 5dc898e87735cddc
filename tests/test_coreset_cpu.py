"""CPU: the float64 reference of k-centre greedy selection (tests/coreset_ref.py) against a plain numpy loop and the brute-force
optimum, the kernel's fp32 order against the derived bounds, every planted fault against the checks the GPU tests apply, and
the host logic of clip.select_coreset through a CPU stand-in for the ops it calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as R  # noqa: E402

DTYPES = (torch.bfloat16, torch.float16)


def test_reference_equals_plain_numpy_loop():
    for seed in range(5):
        X = R.rows64(R.unit_rows16(150, 64, seed, torch.bfloat16))
        g = R.greedy(X, None, 20, first=seed)
        chosen, mind = R.numpy_greedy(X, 20, seed)
        assert np.array_equal(g["picks"], chosen)
        assert np.array_equal(g["mind"], mind)
        assert (g["owner"][chosen] == chosen).all()
        assert np.array_equal(1.0 - np.einsum("ij,ij->i", X, X[g["owner"]])[g["owner"] != np.arange(150)],
                              g["mind"][g["owner"] != np.arange(150)])


def test_two_approximation_against_brute_force():
    """N = 12, m = 3, 20 seeds, float64.  The theorem (Gonzalez 1985) needs a metric: the chord length sqrt(2 (1 - cos)) of unit
    rows is one, and greedy picks are the same under it (a monotone map of the distance), so the chord radius is at most twice
    the optimal chord radius.  The cosine distance itself, half a squared chord, is asserted within the factor 2 as well on
    these 20 sets."""
    worst_chord, worst_cos = 0.0, 0.0
    for seed in range(20):
        g = np.random.RandomState(seed)
        X = g.standard_normal((12, 8))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Dm = np.maximum(1.0 - X @ X.T, 0.0)
        np.fill_diagonal(Dm, 0.0)
        got = R.greedy(X, None, 3, first=int(g.randint(12)))
        owner = got["owner"]
        radius = np.max(Dm[np.arange(12), owner])
        opt = R.optimal_radius(Dm, 3)
        opt_chord = R.optimal_radius(np.sqrt(2.0 * Dm), 3)
        worst_chord = max(worst_chord, np.sqrt(2.0 * radius) / opt_chord)
        worst_cos = max(worst_cos, radius / opt)
        assert np.sqrt(2.0 * radius) <= 2.0 * opt_chord * (1 + 1e-12)
        assert radius <= 2.0 * opt * (1 + 1e-12)
    print(f"[coreset] greedy / optimum: chord {worst_chord:.4f}, cosine {worst_cos:.4f}")


def test_unweighted_radius_never_grows():
    for seed in range(4):
        X = R.rows64(R.unit_rows16(300, 32, seed, torch.float16))
        r = R.greedy(X, None, 60, first=0)["radius"]
        assert r[0] == np.inf and (np.diff(r[1:]) <= 0).all()            # exact: a maximum of minima cannot grow
        seeds = [3, 77, 150]
        r = R.greedy(X, None, 40, seeds=seeds)["radius"]
        assert (np.diff(r) <= 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 96, 512, 544, 1024])
def test_fp32_kernel_order_stays_inside_the_bounds(dtype, D):
    x16 = R.unit_rows16(257, D, D, dtype)
    X, X32 = R.rows64(x16), x16.float().numpy()
    g = np.random.RandomState(D)
    w = g.uniform(0.1, 2.0, 257).astype(np.float32)
    worst = 0.0
    for c in (0, 100, 256):
        d32 = np.float32(1.0) - R.dot32(X32, X32[c])
        ratio = np.abs(d32.astype(np.float64) - R.dist64(X, c)) / R.tol_d(X, c)
        worst = max(worst, ratio.max())
    print(f"[coreset] fp32 order D={D} {dtype}: largest distance err / tol = {worst:.4f}")
    assert worst <= 1.0
    for wt in (None, w):
        got = R.greedy32(X32, wt, 40, first=5)
        bad, ratio = R.check_selection(X, None if wt is None else wt.astype(np.float64), got["picks"], got["radius"],
                                       got["mind"].astype(np.float64), got["owner"], first=5)
        print(f"[coreset] fp32 selection D={D} {dtype} weights={wt is not None}: largest err / tol = {ratio:.4f}")
        assert not bad, bad


def _fault_case(fault):
    """rows, weights, seeds, m on which the fault shows: duplicates for the exact rules, weights where they matter"""
    x16 = R.unit_rows16(140, 64, 11, torch.bfloat16)
    x16[40] = (x16[40].double() * 1.02).to(torch.bfloat16)             # a little longer than 1: its copy sits at a distance below 0,
    x16[41] = x16[40]                                   # under the 0 of a centre.  Equal rows: equal keys, and equal centres once
    x16[120] = x16[7]                                   # both are chosen
    w = None
    if fault in ("weight_ignored", "nan_weight"):
        g = np.random.RandomState(2)
        w = g.uniform(0.05, 3.0, 140).astype(np.float32)
        w[:30] = 0.0
        if fault == "nan_weight":
            w[50] = np.nan
    if fault == "owner_le":                             # both copies become centres early, while rows are left to take sides
        x16[7] = (x16[7].double() * 0.98).to(torch.bfloat16)
        x16[120] = x16[7]
        w = np.ones(140, dtype=np.float32)
        w[[7, 120]] = 1e6
    m = 140 if fault in ("centre_eligible", "tie_high") else 30
    return x16, w, m


@pytest.mark.parametrize("fault", (None,) + R.FAULTS)
def test_every_planted_fault_is_seen(fault):
    x16, w, m = _fault_case(fault)
    X, X32 = R.rows64(x16), x16.float().numpy()
    if w is not None:
        m = min(m, int(np.sum(w > 0)))
    w64 = None if w is None else w.astype(np.float64)
    for planted in (None, fault):                       # the same rows pass without the fault
        got = R.greedy32(X32, w, m, first=None, fault=planted, skip_from=131)
        bad, _ = R.check_selection(X, w64, got["picks"], got["radius"], got["mind"].astype(np.float64), got["owner"])
        if planted is None:
            assert not bad, bad
        else:
            assert bad, f"the checks do not see the planted fault {fault}"


def test_step_check_sees_faults_too():
    x16 = R.unit_rows16(100, 32, 5, torch.float16)
    X, X32 = R.rows64(x16), x16.float().numpy()
    mind0, owner0, _ = R.step32(X32, None, np.full(100, np.inf, dtype=np.float32), np.full(100, -1, dtype=np.int64), 3)
    good = R.step32(X32, None, mind0, owner0, 60)
    assert not R.check_step(X, None, mind0, owner0, 60, *good)[0]
    for fault in ("overwrite", "radius_after", "rows_skipped"):
        got = R.step32(X32, None, mind0, owner0, 60, fault=fault, skip_from=90)
        assert R.check_step(X, None, mind0, owner0, 60, *got)[0], fault


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_planted_clusters_are_separated_by_100_tolerances(dtype):
    """the premise of tests/test_coreset_gpu.py's exact comparison: at every pick of the K the best key leads the second best by
    at least 100 x the tolerance the two keys carry, so the device's picks must equal the reference's"""
    P = R.PLANTED
    x16, cls = R.planted_clusters16(dtype=dtype, **P)
    X = R.rows64(x16)
    mean = X.sum(0)
    first = R.argmax_key(X @ (mean / np.linalg.norm(mean)), np.ones(len(X), dtype=bool))
    # replay with the tolerance of the two leading keys at every pick
    st = R.new_state(len(X))
    mind, owner, tol = st["mind"], st["owner"], st["tol"]
    mind, owner, _, tol = R.step(X, None, mind, owner, first, tol)
    smallest = np.inf
    picks = [first]
    for _ in range(P["K"] - 1):
        el = R.eligible(owner, None)
        c = R.argmax_key(mind, el)
        rest = el.copy(); rest[c] = False
        second = R.argmax_key(mind, rest)
        smallest = min(smallest, (mind[c] - mind[second]) / (tol[c] + tol[second]))
        mind, owner, _, tol = R.step(X, None, mind, owner, c, tol)
        picks.append(c)
    print(f"[coreset] planted {dtype}: smallest gap / tol = {smallest:.1f}")
    assert smallest >= 100.0
    assert sorted(cls[picks]) == list(range(P["K"]))               # one pick per cluster
    assert np.array_equal(R.greedy(X, None, P["K"], first=first)["picks"], picks)


# ---------------------------------------------------------------------------------------------------------------------------
# host logic of clip.select_coreset


@pytest.fixture
def cs(monkeypatch):
    import importlib
    mod = importlib.import_module("clip.coreset")
    import coreset_ops_shim as shim
    monkeypatch.setattr(mod, "ops", shim)
    monkeypatch.setattr(mod, "_unit_rows", lambda f, dtype: f)
    monkeypatch.setattr(mod, "normalize_rows", lambda f, dtype, device=None: torch.nn.functional.normalize(f.double(), dim=1).to(dtype))
    return mod


def _x():
    return R.unit_rows16(90, 32, 21, torch.bfloat16)


def test_labelled_in_its_three_forms(cs):
    x = _x()
    rows = [4, 17, 60]
    mask = torch.zeros(90, dtype=torch.bool); mask[rows] = True
    labels = torch.full((90,), -1); labels[rows] = torch.tensor([2, 0, 2])
    res = [cs.select_coreset(x, 12, labelled=lab) for lab in (rows, torch.tensor(rows[::-1]), mask, labels, labels.tolist())]
    for r in res:
        assert r.seeds.tolist() == rows
        assert not set(r.picks.tolist()) & set(rows) and len(set(r.picks.tolist())) == 12
        assert torch.equal(r.picks, res[0].picks) and torch.equal(r.distance, res[0].distance) and torch.equal(r.owner, res[0].owner)
        assert r.picks.dtype == torch.int64 and r.owner.dtype == torch.int64 and r.radius.dtype == torch.float32
        centres, counts = r.cover_counts()
        assert centres.tolist() == rows + r.picks.tolist() and int(counts.sum()) == 90
        assert torch.equal(counts, torch.bincount(r.owner, minlength=90)[centres])
        assert float(r.cover_radius) == float(r.distance.max()) and float(r.covered(2.0)) == 1.0
        assert abs(float(r.covered(0.5)) - float((r.distance <= 0.5).float().mean())) == 0
    X = R.rows64(x)
    ref = R.greedy(X, None, 12, seeds=rows)
    bad, _ = R.check_selection(X, None, res[0].picks.numpy(), res[0].radius.numpy(), res[0].distance.double().numpy(),
                               res[0].owner.numpy(), seeds=rows)
    assert not bad, bad
    assert (res[0].radius.numpy()[1:] <= res[0].radius.numpy()[:-1]).all() and len(ref["picks"]) == 12


def test_labelled_errors(cs):
    x = _x()
    for lab in ([0, 0, 3], [-1, 2], [90], torch.zeros(89, dtype=torch.bool), torch.zeros(90), torch.zeros(3, 3, dtype=torch.long)):
        with pytest.raises(ValueError):
            cs.select_coreset(x, 2, labelled=lab)


def test_m_limits(cs):
    x = _x()
    with pytest.raises(ValueError, match="m = 91"):
        cs.select_coreset(x, 91)
    with pytest.raises(ValueError, match="m = 88"):
        cs.select_coreset(x, 88, labelled=[1, 2, 3])
    with pytest.raises(ValueError):
        cs.select_coreset(x, -1)
    with pytest.raises(ValueError):
        cs.select_coreset(x, 2.5)
    r = cs.select_coreset(x, 0, labelled=[1, 2, 3])
    assert r.picks.numel() == 0 and r.radius.numel() == 0 and set(r.owner.tolist()) == {1, 2, 3}
    r = cs.select_coreset(x, 0)
    assert r.picks.numel() == 0 and (r.owner == -1).all() and torch.isinf(r.distance).all()
    full = cs.select_coreset(x, 87, labelled=[1, 2, 3])
    assert sorted(full.picks.tolist() + [1, 2, 3]) == list(range(90)) and (full.distance == 0).all()


def test_weights(cs):
    x = _x()
    for bad in (torch.ones(89), torch.ones(90, dtype=torch.long), torch.ones(90, 1), [True] * 90):
        with pytest.raises(ValueError, match="weights"):
            cs.select_coreset(x, 2, weights=bad)
    w = torch.ones(90, dtype=torch.float64); w[:45] = 0; w[50] = float("nan")
    r = cs.select_coreset(x, 44, weights=w)
    assert min(r.picks.tolist()) >= 45 and 50 not in r.picks.tolist() and len(set(r.picks.tolist())) == 44


def test_first(cs):
    x = _x()
    for bad in ("median", 90, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="first"):
            cs.select_coreset(x, 2, first=bad)
    assert cs.select_coreset(x, 3, first=7).picks[0].item() == 7
    X = R.rows64(x)
    mean = X.sum(0)
    assert cs.select_coreset(x, 3).picks[0].item() == int(np.argmax(X @ (mean / np.linalg.norm(mean))))
    assert cs.select_coreset(x, 3, first=7, labelled=[7]).picks.tolist().count(7) == 0      # first is unused with seeds


def test_cpu_tensors_have_no_path():
    from cclip_hip import ops
    x = _x()
    mind, owner = torch.full((90,), float("inf")), torch.full((90,), -1, dtype=torch.int32)
    keys = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.coreset_step(x, mind, owner, keys, centre=0)
    with pytest.raises(TypeError):
        ops.coreset_greedy(x, mind, owner, 2, first=0)
