"""GPU: csrc/mst.hip through cclip_hip.ops and clip/hdbscan.py on top of it.  The device's own fp32 score bits come from
ops.similarity_range(x, x, -inf), which returns every pair with the bits the score kernels share, so what the kernels decide
is compared EXACTLY with tests/hdbscan_ref.py: key for key for the nearest kernel, edge set for edge set for the tree (the
tree under the strict total order is unique).  One float64 check of the cycle property, at the pair tolerance of
tests/kmeans_ref.py, prints `[hdbscan] name: largest err / tol`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdbscan_ref as R  # noqa: E402
import kmeans_ref as KR  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    from cclip_hip import ops as o
    return o


def on_device(x16, pad=0):
    """the rows on the device with row stride D + pad"""
    N, D = x16.shape
    buf = torch.zeros(N, D + pad, dtype=x16.dtype, device="cuda")
    buf[:, :D] = x16.cuda()
    return buf[:, :D]


def device_bits(ops, x):
    """fp32 [N, N]: the score bits of every pair, as the kernels compute them"""
    N = x.shape[0]
    offsets, index, scores = ops.similarity_range(x, x, -INF)
    assert index.numel() == N * N and bool((offsets.diff() == N).all())
    return scores.cpu().numpy().reshape(N, N)


def device_core(ops, x, min_samples):
    N = x.shape[0]
    if min_samples == 1:
        return torch.full((N,), INF, device="cuda")
    return ops.similarity_topk(x, x, min_samples)[0][:, min_samples - 1].contiguous()


def as_u64(keys):
    return keys.cpu().numpy().view(np.uint64)


def comp_variants(N, seed):
    rng = np.random.default_rng(seed)
    odd = np.array([-2 ** 31, -5, 7, 2 ** 31 - 1], dtype=np.int64)
    return {"singletons": np.arange(N), "two": rng.integers(0, 2, N), "one": np.zeros(N, dtype=np.int64),
            "any int32": odd[rng.integers(0, 4, N)]}


def core_variants(ops, x, seed):
    N = x.shape[0]
    rng = np.random.default_rng(seed)
    out = {"inf": torch.full((N,), INF, device="cuda"), "topk": device_core(ops, x, min(5, N))}
    nan = out["topk"].clone()
    nan[torch.from_numpy(rng.integers(0, N, max(1, N // 8))).cuda()] = float("nan")
    out["nan"] = nan
    return out


def check_nearest(ops, x16, pad, seed):
    x = on_device(x16, pad)
    N = x.shape[0]
    S = device_bits(ops, x)
    for cname, core in core_variants(ops, x, seed).items():
        for vname, comp in comp_variants(N, seed).items():
            got = as_u64(ops.mreach_nearest(x, core, torch.from_numpy(comp).to(torch.int32).cuda()))
            want = R.nearest_keys(S, core.cpu().numpy(), comp)
            assert np.array_equal(got, want), (N, x.shape[1], pad, cname, vname, int(np.argmax(got != want)))
            if vname == "one":
                assert not got.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [2, 63, 64, 65, 257])
def test_mreach_nearest_sizes(ops, dtype, N):
    check_nearest(ops, R.random_rows(N, 32, N, dtype, dup_fraction=1 / 3), 0, N)      # a third of the rows are bitwise copies


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("D", [32, 64, 96, 512, 544, 1024])
def test_mreach_nearest_widths_and_strides(ops, dtype, D, pad):
    check_nearest(ops, R.random_rows(257, D, D + pad, dtype, dup_fraction=1 / 3), pad, D)


@pytest.fixture(scope="module", params=DTYPES, ids=IDS)
def big(ops, request):
    """N = 4 099, D = 32: several row blocks, several gallery splits, a partial last tile.  Bits and core computed once per
    16-bit type."""
    x = on_device(R.random_rows(4099, 32, 4099, request.param, dup_fraction=0.05))
    assert ops.mreach_nearest_splits(4099) > 1
    return x, device_bits(ops, x), device_core(ops, x, 5)


def test_mreach_nearest_split_gallery(ops, big):
    x, S, core = big
    comp = np.random.default_rng(1).integers(0, 700, 4099)
    got = as_u64(ops.mreach_nearest(x, core, torch.from_numpy(comp).to(torch.int32).cuda()))
    assert np.array_equal(got, R.nearest_keys(S, core.cpu().numpy(), comp))
    again = as_u64(ops.mreach_nearest(x, core, torch.from_numpy(comp).to(torch.int32).cuda()))
    assert np.array_equal(got, again)


def check_tree(ops, x, S, core):
    N = x.shape[0]
    u, v, m = ops.mst_boruvka(x, core)
    u2, v2, m2 = ops.mst_boruvka(x, core)
    un, vn, mn = u.cpu().numpy(), v.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(un, u2.cpu().numpy()) and np.array_equal(vn, v2.cpu().numpy())
    assert np.array_equal(mn.view(np.uint32), m2.cpu().numpy().view(np.uint32))                  # two calls: bitwise equal
    empty = un < 0
    assert empty.sum() == 1 and np.array_equal(empty, vn < 0) and np.isnan(mn[empty]).all()       # one empty slot
    live = ~empty
    assert live.sum() == N - 1 and np.all(un[live] != vn[live])
    assert un[live].max(initial=0) < N and vn[live].max(initial=0) < N and vn[live].min(initial=0) >= 0
    got = R.edge_set(un, vn, mn)
    assert len(got) == N - 1
    assert got == R.exact_mst(S, core.cpu().numpy())
    return un[live], vn[live]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [2, 3, 64, 65, 257])
def test_mst_boruvka_is_the_exact_tree(ops, dtype, N):
    for kind, dup in (("random", 0.0), ("duplicates", 1 / 3)):
        x = on_device(R.random_rows(N, 32, 7 * N + 1, dtype, dup_fraction=dup))
        S = device_bits(ops, x)
        for ms in (1, 2, 5, 64):
            if ms <= N:
                check_tree(ops, x, S, device_core(ops, x, ms))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mst_boruvka_planted(ops, dtype):
    x = on_device(R.planted_recipe(dtype)[0])
    S = device_bits(ops, x)
    for ms in (1, 2, 5, 64):
        check_tree(ops, x, S, device_core(ops, x, ms))


def test_mst_boruvka_many_blocks(ops, big):
    x, S, core = big
    check_tree(ops, x, S, core)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cycle_property_in_float64(ops, dtype):
    """Largest err / tol measured on an MI355X: 0.00 in all four cases (the float64 tree and the device's agree on every
    decision that is not an exact tie)."""
    for name, x16 in (("planted", R.planted_recipe(dtype)[0]), ("random D=512", R.random_rows(257, 512, 5, dtype))):
        x = on_device(x16)
        core = device_core(ops, x, 5)
        u, v, m = ops.mst_boruvka(x, core)
        live = (u >= 0).cpu().numpy()
        S64 = R.scores64(x16)
        M = R.mreach64(S64, R.core64(S64, 5))
        tol = KR.assign_tol(x16.shape[1], x16, x16)
        ok, ratio = R.check_mst(u.cpu().numpy()[live], v.cpu().numpy()[live], M, tol)
        print(f"[hdbscan] cycle property {IDS[DTYPES.index(dtype)]} {name}: largest err / tol = {ratio:.2f}")      # tol itself, not 2 tol
        assert ok
        got = np.abs(m.cpu().numpy()[live].astype(np.float64) - M[u.cpu().numpy()[live], v.cpu().numpy()[live]]).max()
        assert got <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cut_equals_duplicate_groups(dtype):
    from clip import EmbeddingIndex
    index = EmbeddingIndex(R.random_rows(300, 64, 11, dtype, dup_fraction=0.5).float(), dtype=dtype)
    tree = index.mst(min_samples=1)
    assert tree.u.shape == (299,) and tree.u.dtype == torch.int64 and tree.u.is_cuda
    sim = tree.similarity.cpu().numpy()
    assert np.all(np.diff(sim) <= 0)                                  # sorted by the total order
    for t in (0.5, 0.9, 0.99):
        assert torch.equal(tree.cut(t), index.duplicate_groups(t)), t


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hdbscan_end_to_end(ops, dtype):
    import clip
    from clip.hdbscan import tree_clusters
    x16, planted = R.planted_recipe(dtype)
    x = on_device(x16)
    for ms in (5, 10):
        res = clip.hdbscan(x, min_cluster_size=10, min_samples=ms)
        labels = res.labels.cpu().numpy()
        assert res.n_clusters == 4 and R.adjusted_rand(labels, planted) == 1.0 and np.all(labels[planted < 0] == -1)
        assert res.labels.dtype == torch.int64 and res.probabilities.dtype == torch.float32
        prob = res.probabilities.cpu().numpy()
        assert np.all(prob[labels < 0] == 0) and np.all(prob[labels >= 0] > 0) and prob.max() == 1.0
        u, v, m = R.sort_edges(R.exact_mst(device_bits(ops, x), device_core(ops, x, ms).cpu().numpy()))
        assert np.array_equal(res.mst.u.cpu().numpy(), u) and np.array_equal(res.mst.v.cpu().numpy(), v)
        want, wprob, wpers = tree_clusters(len(x16), u, v, R.chord64(m), 10)
        assert np.array_equal(labels, want) and np.abs(prob - wprob).max() <= 1e-6
        assert np.allclose(res.persistence.cpu().numpy(), wpers, rtol=1e-6)
    leaf = clip.hdbscan(x, min_cluster_size=10, cluster_selection="leaf")
    assert leaf.n_clusters >= 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hdbscan_tiny_sets(dtype):
    import clip
    for N in (1, 2):
        x = on_device(R.random_rows(N, 32, N, dtype))
        res = clip.hdbscan(x, min_cluster_size=5, min_samples=1)
        assert res.labels.tolist() == [-1] * N and res.n_clusters == 0 and res.mst.u.numel() == N - 1
        res = clip.hdbscan(x, min_cluster_size=5, allow_single_cluster=True)
        assert res.labels.tolist() == [0] * N and res.n_clusters == 1 and res.probabilities.tolist() == [1.0] * N
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", IDS)
def test_script_synthetic(capsys, dtype):
    import json
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import density_clusters as M
    clusters, noise, summary = M.main(["--synthetic", "--min-cluster-size", "10", "--show", "2", "--dtype", dtype])
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert printed == clusters + [noise, dict(summary=summary)]
    assert summary["clusters"] == len(clusters) == 9 and summary["rows"] == 360          # nine planted classes of 40
    assert sum(c["size"] for c in clusters) + noise["size"] == 360 and noise["cluster"] == -1
    assert all(set(c) >= {"cluster", "size", "persistence", "central", "majority_label"} and len(c["central"]) == 2
               and c["persistence"] > 0 for c in clusters)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_c_abi_refusals(ops, dtype):
    from cclip_hip._lib import lib
    f_nearest, f_tree = ((lib.cclip_mreach_nearest, lib.cclip_mst_boruvka) if dtype == torch.bfloat16 else
                         (lib.cclip_mreach_nearest_f16, lib.cclip_mst_boruvka_f16))
    N, D = 40, 64
    x = on_device(R.random_rows(N, D, 3, dtype))
    core = torch.full((N,), INF, device="cuda")
    comp = torch.arange(N, dtype=torch.int32, device="cuda")
    keys = torch.full((N,), 77, dtype=torch.int64, device="cuda")
    u = torch.full((N,), 77, dtype=torch.int32, device="cuda")
    v, m = u.clone(), torch.full((N,), 77.0, device="cuda")
    nbytes = ops.mst_workspace(N)
    assert nbytes == 32 * N + 256 and ops.mst_workspace(0) == 0 and ops.mst_workspace(2 ** 31) == 0
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    def nearest(**kw):
        a = dict(x=x.data_ptr(), ldx=D, N=N, D=D, core=core.data_ptr(), comp=comp.data_ptr(), keys=keys.data_ptr())
        a.update(kw)
        return f_nearest(vp(a["x"]), i64(a["ldx"]), i64(a["N"]), i32(a["D"]), vp(a["core"]), vp(a["comp"]), vp(a["keys"]), stream)

    def tree(**kw):
        a = dict(x=x.data_ptr(), ldx=D, N=N, D=D, core=core.data_ptr(), u=u.data_ptr(), v=v.data_ptr(), m=m.data_ptr(),
                 ws=ws.data_ptr(), nbytes=nbytes)
        a.update(kw)
        return f_tree(vp(a["x"]), i64(a["ldx"]), i64(a["N"]), i32(a["D"]), vp(a["core"]), vp(a["u"]), vp(a["v"]), vp(a["m"]),
                      vp(a["ws"]), i64(a["nbytes"]), stream)

    bad = [dict(x=0), dict(core=0), dict(D=48, ldx=48), dict(D=0), dict(x=x.data_ptr() + 2), dict(ldx=D + 4), dict(N=0),
           dict(N=2 ** 31)]
    for kw in bad + [dict(comp=0), dict(keys=0), dict(keys=keys.data_ptr() + 4)]:
        assert nearest(**kw) == 1, kw
    for kw in bad + [dict(u=0), dict(v=0), dict(m=0), dict(ws=0), dict(nbytes=nbytes - 1), dict(ws=ws.data_ptr() + 4)]:
        assert tree(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((keys == 77).all()) and bool((u == 77).all()) and bool((v == 77).all()) and bool((m == 77.0).all())
    assert nearest() == 0 and tree() == 0
    torch.cuda.synchronize()
    assert int((u < 0).sum()) == 1
