"""GPU: cclip_concept_codes through the ops binding against the float64 reference (tests/concepts_ref.py) on the same 16-bit
inputs, at the smallest shapes at which the kernel can go wrong: tile edges in V, row-block edges in N, every D rung, the
iterations at which the momentum starts, strides with poisoned gaps, a NaN row, the bitwise properties and the error paths.

The tolerances are 4 x the largest deviation measured on an MI355X at exactly these shapes; the margin is
there because the conditioning of the active-set Gram matrix varies with the draw.  Every element and every row is compared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concepts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# measured over this file's cases: max |w - w64| 2.06e-6 (bf16), 1.67e-7 (fp16); the read-outs 3.87e-6 (bf16), 4.12e-7 (fp16),
# both at l1norm.  The hi + lo pair keeps 2^-17 = 7.6e-6 of a residual of norm <= 1 in bf16 and 2^-23 in fp16: the measured
# values lie inside what the split explains.  Asserted: 4 x.
W_TOL = {torch.bfloat16: 4 * 2.06e-6, torch.float16: 4 * 1.67e-7}
READ_TOL = {torch.bfloat16: 4 * 3.87e-6, torch.float16: 4 * 4.12e-7}
# kkt alone (bf16): at most 2.6e-6 from the reference's over this file's cases; and, at V = 75, D = 32, 1000 iterations, the
# kernel's kkt against the float64 violation recomputed at the kernel's own w: at most 1.004e-6 apart (measured)
KKT_TOL = 4 * 2.6e-6
KKT_SEEN = 1.004e-6
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_deviation():
    yield
    print(f"[concepts] worst deviations of this run: {WORST}")


def _ops():
    from cclip_hip import ops
    return ops


def _inputs(N, V, D, seed, dtype):
    return R.unit_rows16(N, D, seed, dtype), R.unit_rows16(V, D, seed + 1000, dtype)


def _check(x16, c16, l1, iters, got, tag):
    """every w and every read-out against float64; returns the deviations"""
    X, C = R.rows64(x16), R.rows64(c16)
    eta = 1.0 / R.lipschitz(C)
    ref = R.fista64(X, C, l1, np.float32(eta), iters)
    w, resid2, l1norm, nnz, delta, kkt = [t.cpu().double().numpy() for t in got]
    dt = x16.dtype
    dev_w = float(np.abs(w - ref["w"]).max())
    devs = {k: float(np.abs(v - ref[k]).max()) for k, v in (("resid2", resid2), ("l1norm", l1norm), ("delta", delta), ("kkt", kkt))}
    print(f"[concepts] {tag}: max |w - w64| {dev_w:.3e}; " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()))
    key = str(dt)
    WORST[key] = max(WORST.get(key, 0.0), dev_w)
    WORST[key + " read-outs"] = max(WORST.get(key + " read-outs", 0.0), *devs.values())
    assert dev_w <= W_TOL[dt], (tag, dev_w)
    for k in ("resid2", "l1norm", "delta", "kkt"):
        assert devs[k] <= READ_TOL[dt], (tag, k, devs)
    # nnz, on every row: exactly the positive entries of the returned w (no tolerance; this also keeps padding concepts out of
    # the count), and between the reference weights that are clearly positive and those that are not clearly negative
    assert np.array_equal(nnz, (w > 0).sum(1)), tag
    assert ((ref["w"] > W_TOL[dt]).sum(1) <= nnz).all() and (nnz <= (ref["w"] > -W_TOL[dt]).sum(1)).all(), tag
    assert (w >= 0).all(), tag
    # l1norm against the returned w itself: any fixed order of fp32 additions of nnz positive terms (adding a zero is exact)
    # is within nnz roundings of 2^-24 of the sum
    exact = w.sum(1)
    assert (np.abs(l1norm - exact) <= nnz * 2.0 ** -24 * exact).all(), (tag, float(np.abs(l1norm - exact).max()))
    return eta


def _run(x16, c16, l1, iters, **kw):
    eta = 1.0 / R.lipschitz(R.rows64(c16))
    return _ops().concept_codes(x16.cuda(), c16.cuda(), l1, eta, iters, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 75])
def test_tile_edges_in_v(V, dtype):
    x16, c16 = _inputs(65, V, 64, V, dtype)
    got = _run(x16, c16, 0.05, 50)
    _check(x16, c16, 0.05, 50, got, f"V={V} {dtype}")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("D", [32, 64, 512, 1024])
def test_row_block_edges_and_every_d(N, D):
    dtype = torch.bfloat16 if (N + D) % 3 else torch.float16
    x16, c16 = _inputs(N, 75, D, N + D, dtype)
    got = _run(x16, c16, 0.1, 50)
    _check(x16, c16, 0.1, 50, got, f"N={N} D={D} {dtype}")


@pytest.mark.parametrize("iters", [0, 1, 2, 50])
def test_where_the_momentum_starts(iters):
    x16, c16 = _inputs(33, 75, 32, 9, torch.bfloat16)
    got = _run(x16, c16, 0.05, iters)
    _check(x16, c16, 0.05, iters, got, f"iters={iters}")
    if iters == 0:
        assert (got[0] == 0).all() and (got[4] == 0).all() and (got[3] == 0).all()
        assert torch.allclose(got[1].cpu().double(), (x16.double() ** 2).sum(1), rtol=0, atol=2.0 ** -20)


def test_l1_zero_and_l1_above_the_closed_form_bound():
    x16, c16 = _inputs(40, 75, 64, 3, torch.bfloat16)
    _check(x16, c16, 0.0, 50, _run(x16, c16, 0.0, 50), "l1=0")
    bound = float((x16.double() @ c16.double().t()).max())
    got = _run(x16, c16, bound + 2.0 ** -10, 50)               # above the bound by far more than the operand split's 2^-16
    assert (got[0] == 0).all() and (got[3] == 0).all() and (got[2] == 0).all() and (got[5] == 0).all()


def test_strides_with_poisoned_gaps():
    N, V, D = 37, 45, 64
    x16, c16 = _inputs(N, V, D, 21, torch.bfloat16)
    xs = torch.full((N, D + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    cs = torch.full((V, D + 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    xs[:, :D] = x16.cuda()
    cs[:, :D] = c16.cuda()
    wbuf = torch.full((N, 52), -7.0, dtype=torch.float32, device="cuda")
    eta = 1.0 / R.lipschitz(R.rows64(c16))
    got = _ops().concept_codes(xs[:, :D], cs[:, :D], 0.05, eta, 50, out_w=wbuf[:, :V])
    dense = _run(x16, c16, 0.05, 50)
    for a, b in zip(got, dense):
        assert torch.equal(a, b)
    assert (wbuf[:, V:] == -7.0).all()
    assert torch.isnan(xs[:, D:]).all() and torch.isnan(cs[:, D:]).all()
    _check(x16, c16, 0.05, 50, got, "strided")


def test_realistic_case():
    x16, c16 = _inputs(130, 1000, 512, 77, torch.bfloat16)
    _check(x16, c16, 0.1, 50, _run(x16, c16, 0.1, 50), "N=130 V=1000 D=512")


@pytest.mark.parametrize("D", [64, 1024])
def test_bitwise_repeatable_and_independent_of_n_and_position(D):
    x16, c16 = _inputs(130, 75, D, 5, torch.bfloat16)
    a, b = _run(x16, c16, 0.05, 50), _run(x16, c16, 0.05, 50)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for pos in (0, 64, 129):
        one = _run(x16[pos:pos + 1], c16, 0.05, 50)
        for u, v in zip(one, a):
            assert torch.equal(u[0], v[pos]), pos
    # the fp32 w of a chunked call
    parts = [_run(x16[lo:lo + 50], c16, 0.05, 50)[0] for lo in range(0, 130, 50)]
    assert torch.equal(torch.cat(parts), a[0])


def test_nan_row_is_contained():
    x16, c16 = _inputs(70, 75, 64, 13, torch.bfloat16)
    clean = _run(x16, c16, 0.05, 20)
    bad = x16.clone()
    bad[33, 5] = float("nan")
    got = _run(bad, c16, 0.05, 20)
    keep = torch.arange(70) != 33
    for u, v in zip(got, clean):
        assert torch.equal(u.cpu()[keep], v.cpu()[keep])
    assert torch.isnan(got[0][33]).all()
    for k in (1, 2, 4, 5):
        assert torch.isnan(got[k][33]), k


def test_kkt_readout_is_small_and_bounds_the_true_violation():
    x16, c16 = _inputs(8, 75, 32, 0, torch.bfloat16)
    l1 = 0.1
    got = _run(x16, c16, l1, 1000)
    w = got[0].cpu().double().numpy()
    kkt = got[5].cpu().double().numpy()
    true = R.readouts(R.rows64(x16), R.rows64(c16), w, w, l1)["kkt"]
    off = np.abs(kkt - true)
    print(f"[concepts] kkt at 1000 iterations: kernel {kkt.max():.3e}, float64 at the returned w {true.max():.3e}, "
          f"max |kernel - float64| {off.max():.3e}")
    # small: at 1000 iterations the float64 recurrence is at the optimum (kkt < 2^-30, tests/test_concepts_cpu.py), so the
    # kernel's kkt here is its whole deviation from the reference's - bounded like every kkt read-out of this file, by 4 x
    # the 2.6e-6 measured over its cases (seen here: 1.86e-6)
    assert kkt.max() <= KKT_TOL
    # it bounds the true violation, from both sides: the kernel's g and the float64 g at the same w differ by the operand
    # split alone.  Asserted: 4 x the measured KKT_SEEN
    assert (off <= 4 * KKT_SEEN).all()


def test_error_paths_leave_the_outputs_untouched():
    import ctypes
    from cclip_hip._lib import lib
    ops = _ops()
    N, V, D = 8, 20, 64
    x16, c16 = _inputs(N, V, D, 1, torch.bfloat16)
    x, c = x16.cuda(), c16.cuda()
    w = torch.full((N, V), -3.0, device="cuda")
    outs = [torch.full((N,), -3.0, device="cuda") for _ in range(4)]
    nnz = torch.full((N,), -3, device="cuda", dtype=torch.int32)
    ws = torch.empty(ops.concept_codes_workspace(N, V, D) // 4, device="cuda")
    assert ops.concept_codes_workspace(N, V, D) == 4 * N * V and ops.concept_codes_workspace(N, V, 48) == 0
    P = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    L, I, F = ctypes.c_int64, ctypes.c_int32, ctypes.c_float

    def call(**kw):
        a = dict(x=P(x), ldx=D, N=N, c=P(c), ldc=D, V=V, D=D, l1=0.1, eta=0.5, iters=3, w=P(w), ldw=V, resid2=P(outs[0]),
                 l1norm=P(outs[1]), nnz=P(nnz), delta=P(outs[2]), kkt=P(outs[3]), ws=P(ws), wsb=ws.numel() * 4)
        a.update(kw)
        return lib.cclip_concept_codes(a["x"], L(a["ldx"]), L(a["N"]), a["c"], L(a["ldc"]), L(a["V"]), I(a["D"]), F(a["l1"]),
                                       F(a["eta"]), I(a["iters"]), a["w"], L(a["ldw"]), a["resid2"], a["l1norm"], a["nnz"],
                                       a["delta"], a["kkt"], a["ws"], L(a["wsb"]), ctypes.c_void_p(0))

    null = ctypes.c_void_p(0)
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)   # noqa: E731
    bad = [dict(x=null), dict(c=null), dict(w=null), dict(resid2=null), dict(l1norm=null), dict(nnz=null), dict(delta=null),
           dict(kkt=null), dict(ws=null), dict(N=0), dict(N=2 ** 31), dict(V=0), dict(V=2 ** 24 + 1), dict(D=16), dict(D=48),
           dict(D=1056), dict(ldx=D - 8), dict(ldx=D + 4), dict(ldc=D + 4), dict(x=off(x, 2)), dict(c=off(c, 8)), dict(ldw=V - 4),
           dict(ldw=V + 1), dict(w=off(w, 4)), dict(ws=off(ws, 4)), dict(kkt=off(outs[3], 2)), dict(l1=-0.1), dict(l1=float("nan")),
           dict(l1=float("inf")), dict(eta=-1.0), dict(eta=float("nan")), dict(iters=-1), dict(wsb=ws.numel() * 4 - 1)]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (w == -3.0).all() and (nnz == -3).all() and all((o == -3.0).all() for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert (w >= 0).all() and (nnz >= 0).all()
    for kw in (dict(l1=-1.0), dict(iters=-1)):
        with pytest.raises(ValueError):
            ops.concept_codes(x, c, kw.get("l1", 0.1), 0.5, kw.get("iters", 3))
