"""The three t-SNE kernels (csrc/tsne.hip) on the MI355X against the float64 reference of tests/tsne_ref.py, under its derived
bounds, at the kernels' own edges: the tile width J = 512 (N = J - 1, J, J + 1), the split cap S = 16 (N = S J + 1 = 8193: the
first N whose splits take two tiles each), 64-wide waves and the 256-row work-group.  Every case prints its largest
err / tol before it asserts."""
import functools
import math

import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
J, S = R.TILE, R.SPLIT_MAX
REP_N = [2, 3, 63, 64, 65, 257, 1025, 4099, J - 1, J, J + 1, S * J + 1]


def ratio(name, got, ref, tol):
    err = (got.double().cpu() - ref).abs()
    r = (err / tol.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    r = float("inf") if torch.isnan(err).any() else r
    print(f"[tsne] {name}: largest err / tol {r:.3f}")
    return r


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def map_case(N, scale):
    g = torch.Generator().manual_seed(1000 + N)
    y = torch.randn(N, 2, generator=g)
    if scale == "init":
        y = 1e-4 * y
    elif scale == "mid":
        y = 10.0 * y
    else:
        y = 1e3 * y
        y[0] = torch.tensor([4e4, -3e4])                                          # two far outliers
        y[N - 1] = torch.tensor([-5e4, 2e4])
    y = y.float()
    return y, R.repulsion_ref(y)


@pytest.mark.parametrize("scale", ["init", "mid", "far"])
@pytest.mark.parametrize("N", REP_N)
def test_repulsion(N, scale):
    from cclip_hip import ops
    y, ref = map_case(N, scale)
    yd = y.to(DEV)
    zrow, rep, z = ops.tsne_repulsion(yd)
    zrow2, rep2, z2 = ops.tsne_repulsion(yd.clone())
    r = max(ratio(f"repulsion N{N} {scale} zrow", zrow, ref["zrow"], ref["zrow_tol"]),
            ratio(f"repulsion N{N} {scale} rep", rep, ref["rep"], ref["rep_tol"]),
            ratio(f"repulsion N{N} {scale} Z", z[0], ref["Z"], ref["Z_tol"]))
    assert r <= 1.0
    assert same_bits(zrow, zrow2) and same_bits(rep, rep2) and same_bits(z, z2)
    assert ops.tsne_repulsion_workspace(N) == (3 * N * R.split_plan(N)[1] + -(-N // 256)) * 4


def test_repulsion_two_points_by_hand():
    from cclip_hip import ops
    y = torch.tensor([[0.0, 0.0], [1.0, 2.0]])
    zrow, rep, z = ops.tsne_repulsion(y.to(DEV))
    w = 1.0 / 6.0
    assert (zrow.cpu().double() - w).abs().max().item() <= 9 * R.U * w
    assert abs(z.item() - 2 * w) <= 20 * R.U * w
    want = torch.tensor([[-w * w, -2 * w * w], [w * w, 2 * w * w]], dtype=torch.float64)
    assert (rep.cpu().double() - want).abs().max().item() <= 20 * R.U * 2 * w * w


def test_repulsion_coincident_points():
    from cclip_hip import ops
    y, _ = map_case(257, "mid")
    y = y.clone()
    y[[3, 64, 65, 200, 256]] = y[3].clone()                                       # five points in one place
    ref = R.repulsion_ref(y)
    zrow, rep, z = ops.tsne_repulsion(y.to(DEV))
    r = max(ratio("coincident zrow", zrow, ref["zrow"], ref["zrow_tol"]), ratio("coincident rep", rep, ref["rep"], ref["rep_tol"]),
            ratio("coincident Z", z[0], ref["Z"], ref["Z_tol"]))
    assert r <= 1.0
    alone = torch.zeros(5, 2) + y[3]                                              # only coincident points: each meets 4 others at w = 1
    zrow, rep, z = ops.tsne_repulsion(alone.to(DEV))
    assert zrow.tolist() == [4.0] * 5 and z.item() == 20.0 and rep.abs().max().item() == 0.0


# ---- affinities ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_case(k):
    g = torch.Generator().manual_seed(50 + k)
    s = (0.1 + 0.8 * torch.rand(300, k, generator=g)).float()
    s = torch.sort(s, dim=1, descending=True).values
    s[3] = 0.5                                                                    # all equal
    s[5, 0] = 1.0                                                                 # an exact duplicate among far ones
    s[5, 1:] = torch.sort(0.1 * torch.rand(k - 1, generator=g), descending=True).values
    s[7, k // 2] = float("nan")                                                   # a NaN row between two good rows
    return s


@pytest.mark.parametrize("k,perplexity", [(k, p) for k in (2, 5, 31, 32, 33, 63) for p in (1.5, 5.0, 20.0) if p < k])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_affinities(k, perplexity, strided):
    from cclip_hip import ops
    s = score_case(k)
    P_ref, beta_ref, info = R.affinities_ref(s, perplexity)
    if strided:
        wide = torch.full((300, k + 5), 7.0, device=DEV)
        wide[:, 2:2 + k] = s.to(DEV)
        sd = wide[:, 2:2 + k]
    else:
        sd = s.to(DEV)
    P, beta = ops.tsne_affinities(sd, perplexity)
    P, beta = P.cpu(), beta.cpu()
    assert torch.isnan(P[7]).all() and torch.isnan(beta[7])
    good = torch.ones(300, dtype=torch.bool)
    good[7] = False
    assert torch.isfinite(P[good]).all() and torch.isfinite(beta[good]).all()
    sums = (P[good].double().sum(dim=1) - 1).abs().max().item()
    print(f"[tsne] affinities k{k} perplexity {perplexity}: largest |row sum - 1| / (k 2^-23) {sums / (k * 2.0 ** -23):.3f}")
    assert sums <= k * 2.0 ** -23
    assert (P[3].double() - 1.0 / k).abs().max().item() <= (k + 7) * R.U / k and info["degenerate"][3]
    cal = good & ~info["degenerate"]
    assert int(cal.sum()) >= 290 and cal[5]
    rb = ratio(f"affinities k{k} perplexity {perplexity} beta", beta[cal], beta_ref[cal], info["beta_tol"][cal])
    rp = ratio(f"affinities k{k} perplexity {perplexity} P", P[good], P_ref[good], info["P_tol"][good])
    assert rb <= 1.0 and rp <= 1.0


# ---- step ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(N):
    """A seeded Gaussian state away from iteration 0, a CSR with an empty row and (N > 126) a row of 126 entries"""
    g = torch.Generator().manual_seed(7 + N)
    y = (5.0 * torch.randn(N, 2, generator=g)).float()
    vel = (0.3 * torch.randn(N, 2, generator=g)).float()
    gains = (0.2 + 2.0 * torch.rand(N, 2, generator=g)).float()
    A = torch.rand(N, N, generator=g) * (torch.rand(N, N, generator=g) < min(0.5, 20.0 / N))
    A.fill_diagonal_(0)
    A[1] = 0                                                                      # the empty row
    A[0, N - 1], A[N - 1, 0] = 0.7, 0.4                                           # (N = 3 keeps entries whatever the draw)
    if N > 126:
        A[2] = 0
        A[2, 3:129] = torch.rand(126, generator=g) + 0.1                          # the row of 126 entries
    vals_dense = (A / A.sum()).float()
    rows, cols = torch.nonzero(vals_dense, as_tuple=True)
    offsets = torch.searchsorted(rows, torch.arange(N + 1))
    vals = vals_dense[rows, cols]
    rep = R.repulsion_ref(y)
    return y, vel, gains, offsets, cols.to(torch.int32), vals, rep["rep"].float(), torch.tensor([float(rep["Z"])]), vals_dense.double()


@pytest.mark.parametrize("phase", ["exaggerated", "plain"])
@pytest.mark.parametrize("N", [3, 65, 1025])
def test_step(N, phase):
    from cclip_hip import ops
    y, vel, gains, offsets, cols, vals, rep, z, Pd = step_case(N)
    ex, mom = (12.0, 0.5) if phase == "exaggerated" else (1.0, 0.8)
    lr, mg = 200.0, 0.01
    assert offsets[2].item() == offsets[1].item() and (N <= 126 or int(offsets[3] - offsets[2]) == 126)
    ref = R.step_ref(y, vel, gains, Pd, rep, z.item(), ex, mom, lr, mg)
    undecided = 1.0 - ref["decided"].double().mean().item()
    print(f"[tsne] step N{N} {phase}: share of elements left out of the gains comparison {undecided:.4f}")
    assert undecided <= 0.01                                                      # a condition on the inputs, before the kernel runs
    yd, veld, gainsd = y.to(DEV), vel.to(DEV), gains.to(DEV)
    y_in = yd.clone()
    out_y, kl = ops.tsne_step(yd, veld, gainsd, offsets.to(DEV), cols.to(DEV), vals.to(DEV), rep.to(DEV), z.to(DEV),
                              exaggeration=ex, momentum=mom, learning_rate=lr, min_gain=mg)
    assert out_y.data_ptr() != yd.data_ptr() and same_bits(yd, y_in)
    d = ref["decided"]
    r = max(ratio(f"step N{N} {phase} kl_row", kl, ref["kl_row"], ref["kl_tol"]),
            ratio(f"step N{N} {phase} gains", gainsd.cpu()[d], ref["gains"][d], ref["gains_tol"][d]),
            ratio(f"step N{N} {phase} vel", veld.cpu()[d], ref["vel"][d], ref["vel_tol"][d]),
            ratio(f"step N{N} {phase} y", out_y.cpu()[d], ref["y"][d], ref["y_tol"][d]))
    assert r <= 1.0
    assert kl[1].item() == 0.0 and (gainsd.cpu() >= mg).all()
    # an undecided element took one of the two branches
    g_new = gainsd.cpu().double()
    plus, times = (gains.double() + 0.2).clamp(min=mg), (gains.double() * 0.8).clamp(min=mg)
    assert (((g_new - plus).abs() <= ref["gains_tol"]) | ((g_new - times).abs() <= ref["gains_tol"])).all()
    # evaluation only: the same kl rows, nothing else touched
    kl2 = ops.tsne_step(y_in, None, None, offsets.to(DEV), cols.to(DEV), vals.to(DEV), None, z.to(DEV), update=False)[1]
    assert same_bits(kl, kl2)


def test_argument_errors():
    from cclip_hip import ops
    s = torch.rand(8, 5, device=DEV)
    for bad, exc in ((s.cpu(), TypeError), (s.double(), TypeError), (s.t(), ValueError), (torch.rand(8, 64, device=DEV), ValueError),
                     (s[:0], ValueError), (s[0], ValueError)):
        with pytest.raises(exc):
            ops.tsne_affinities(bad, 2.0)
    for perp in (1.0, 5.0, 7.0, float("nan")):
        with pytest.raises(ValueError):
            ops.tsne_affinities(s, perp)
    with pytest.raises(ValueError):
        ops.tsne_affinities(s, 2.0, out_P=torch.empty(8, 4, device=DEV))
    P, beta = torch.empty(8, 5, device=DEV), torch.empty(8, device=DEV)
    assert ops.tsne_affinities(s, 2.0, out_P=P, out_beta=beta)[0] is P

    y = torch.randn(9, 2, device=DEV)
    for bad, exc in ((y.cpu(), TypeError), (y.half(), TypeError), (y[:, :1], ValueError), (torch.randn(2, 9, device=DEV).t(), ValueError),
                     (y[:0], ValueError)):
        with pytest.raises(exc):
            ops.tsne_repulsion(bad)
    with pytest.raises(ValueError):
        ops.tsne_repulsion(y, workspace=torch.empty(4, device=DEV))
    with pytest.raises(ValueError):
        ops.tsne_repulsion(y, out_zrow=torch.empty(8, device=DEV))
    zrow, rep, z = ops.tsne_repulsion(y)

    off = torch.tensor([0, 1, 1, 2, 2, 2, 2, 2, 2, 2], device=DEV)
    cols, vals = torch.tensor([1, 0], device=DEV, dtype=torch.int32), torch.tensor([0.5, 0.5], device=DEV)
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    ok = (y, vel, gains, off, cols, vals, rep, z)
    assert ops.tsne_step(*ok)[0].shape == (9, 2)
    swaps = [(0, y.cpu(), TypeError), (1, vel.double(), TypeError), (2, gains[:8], ValueError), (3, off.int(), TypeError),
             (3, off[:9], ValueError), (4, cols.long(), TypeError), (5, vals[:1], ValueError), (6, rep.cpu(), TypeError),
             (7, z[:0], ValueError), (4, cols.cpu(), TypeError)]
    for pos, bad, exc in swaps:
        args = list(ok)
        args[pos] = bad
        with pytest.raises(exc):
            ops.tsne_step(*args)
    with pytest.raises(ValueError):
        ops.tsne_step(*ok, out_y=y)
    with pytest.raises(ValueError):
        ops.tsne_step(*ok, learning_rate=float("nan"))
    with pytest.raises(ValueError):
        ops.tsne_step(*ok, update=False, out_y=torch.empty_like(y))
