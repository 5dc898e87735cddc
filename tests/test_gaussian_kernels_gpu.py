"""GPU: cclip_class_moments and cclip_gauss_scores through the ops binding against the float64 reference (tests/gaussian_ref.py)
on the same 16-bit inputs, at the smallest shapes at which the kernels can go wrong: tile and block edges in N / Q, every D
rung, column blocks that are not full (D = 32, 64), two class blocks (C = 256), R around the tile of 16, a split into ragged
parts, strides with poisoned gaps, NaN rows, the bitwise properties and the error paths of the contract, in its order.

Bounds.  class_moments and z: derived, any order of fp32 additions of n exact products is within n 2^-24 sum |terms| of the
true sum (n 2^-24 << 1).  d2, lse, dmin: 4 x the worst normalised deviation measured on an MI355X over this file's cases
(the margin is for the draw-to-draw variation of the conditioning, the project's convention of 6.24).
Measured 2026-10-21 (bf16 / fp16 worst): d2 and dmin 1.90e-6 / 2.43e-6 where d2 has more than one term, 2.00e-3 / 1.48e-3 at
R = 1; lse 1.16e-6 / 1.30e-6 and 1.48e-5 / 1.55e-5 at R = 1.  See D2_SEEN / LSE_SEEN below."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussian_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BOTH = (torch.bfloat16, torch.float16)
# worst normalised deviations measured over this file's cases on an MI355X, 2026-10-21 (d2 and dmin by d2 itself, lse by
# max(1, |lse|)); asserted: 4 x
# Two regimes, each with its own measured worst: with R = 1 d2 is ONE squared difference, which z's rounding (bounded
# relative to sum |t x|, not to z - m) moves by any fraction once z - m is small; with more terms the sum is dominated by
# the terms that are not; lse inherits it.  d2: 1.998e-3 (bf16) / 1.477e-3 (fp16) at R = 1, 2.434e-6 over every other case
# (D = R = 1024, C = 256, fp16); lse: 1.551e-5 at R = 1, 1.302e-6 over every other case.
D2_SEEN = {True: 1.998e-3, False: 2.434e-6}              # keyed by R == 1
LSE_SEEN = {True: 1.551e-5, False: 1.302e-6}
D2_TOL = 4 * D2_SEEN[False]


def d2_tol(Rr):
    return 4 * D2_SEEN[Rr == 1]


def lse_tol(Rr):
    return 4 * LSE_SEEN[Rr == 1]


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"[gaussian] worst of this run: {WORST}")


def _ops():
    from cclip_hip import ops
    return ops


def _worst(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


# ---------------------------------------------------------------------------------------------------------------------------
# class_moments
# ---------------------------------------------------------------------------------------------------------------------------
def _labels(N, C, seed, outside=False):
    g = np.random.default_rng(seed)
    y = g.integers(0, C, N)
    if outside and N >= 4:
        y[::5] = -1
        y[3::7] = C
    return y


def _moments(x16, y, C, **kw):
    ops = _ops()
    xd = x16.cuda() if not x16.is_cuda else x16
    yd = None if y is None else torch.from_numpy(np.asarray(y)).to(torch.int32).cuda()
    count, s, g = ops.class_moments(xd, yd, C, **kw)
    torch.cuda.synchronize()
    return count.cpu().numpy(), s.cpu().double().numpy(), g.cpu().double().numpy()


RAGGED_N = 2 * 256 + 100         # tiles of 32 in parts of 8: 8 + 8 + 4 tiles, the last tile with 4 rows

MOMENT_CASES = [(N, 64, 9) for N in (1, 63, 64, 65, 130, RAGGED_N)] + \
               [(N, D, C) for D, C in ((32, 2), (512, 9), (1024, 2)) for N in (65, 130)] + \
               [(130, 64, 1), (130, 64, 256), (65, 512, 256), (RAGGED_N, 32, 1)]


def test_ragged_case_has_three_parts():
    assert _ops().moments_parts(RAGGED_N, 9, 64) == 3
    assert _ops().moments_parts(130, 9, 64) == 1


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N,D,C", MOMENT_CASES)
def test_moments_exact_small_integers(N, D, C, dtype):
    """entries from {-2 .. 2}: every partial sum is an integer below 2^24, so the result is the float64 reference, bitwise"""
    g = np.random.default_rng(N * 7 + D + C)
    x16 = torch.from_numpy(g.integers(-2, 3, (N, D)).astype(np.float32)).to(dtype)
    y = None if C == 1 else _labels(N, C, N + D, outside=True)
    count, s, gram = _moments(x16, y, C)
    rc, rs, rg = R.moments64(R.rows64(x16), y, C)
    assert np.array_equal(count, rc)
    assert np.array_equal(s, rs)
    assert np.array_equal(gram, rg)
    assert np.array_equal(gram, gram.T)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N,D,C", MOMENT_CASES)
def test_moments_random_unit_rows(N, D, C, dtype):
    x16 = R.rows16(N, D, N + D + C, dtype)
    y = None if C == 1 else _labels(N, C, N + D + 1, outside=True)
    count, s, gram = _moments(x16, y, C)
    X = R.rows64(x16)
    rc, rs, rg = R.moments64(X, y, C)
    yy = np.zeros(N, dtype=np.int64) if y is None else y
    live = (yy >= 0) & (yy < C)
    A = np.abs(X[live])
    n = int(live.sum()) + 16                               # the rows' additions and the merge's
    bound_g = n * 2.0 ** -24 * (A.T @ A) + 1e-38
    mag_s = np.zeros((C, D))
    np.add.at(mag_s, yy[live], A)
    bound_s = n * 2.0 ** -24 * mag_s + 1e-38
    assert np.array_equal(count, rc)
    rg_ratio = float((np.abs(gram - rg) / bound_g).max())
    rs_ratio = float((np.abs(s - rs) / bound_s).max())
    print(f"[gaussian] moments N={N} D={D} C={C} {dtype}: worst ratio to the bound gram {rg_ratio:.3e} sum {rs_ratio:.3e}")
    _worst("moments ratio gram", rg_ratio)
    _worst("moments ratio sum", rs_ratio)
    assert rg_ratio <= 1.0 and rs_ratio <= 1.0
    assert np.array_equal(gram, gram.T)


def test_moments_outside_labels_contribute_nothing():
    N, D, C = 130, 64, 9
    x16 = R.rows16(N, D, 5, torch.bfloat16)
    y = _labels(N, C, 6, outside=True)
    live = (y >= 0) & (y < C)
    a = _moments(x16, y, C)
    xz = x16.clone()
    xz[torch.from_numpy(~live)] = float("nan")               # whatever a dropped row holds
    b = _moments(xz, y, C)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert a[0].sum() == live.sum()


@pytest.mark.parametrize("dtype", BOTH)
def test_moments_strided_with_poisoned_gaps(dtype):
    N, D, C = 130, 64, 9
    x16 = R.rows16(N, D, 8, dtype)
    y = _labels(N, C, 9)
    big = torch.full((N, D + 24), float("nan"), dtype=dtype).cuda()
    big[:, :D] = x16.cuda()
    a = _moments(big[:, :D], y, C)
    b = _moments(x16, y, C)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_moments_nan_row_poisons_its_own_entries(bad):
    """a row that is zero outside 3 columns, one of them non-finite: the entries its outer product touches under IEEE
    arithmetic (NaN * 0 is NaN) and its own class's sum in that column - nothing else"""
    N, D, C = 70, 64, 9
    x16 = R.rows16(N, D, 10, torch.bfloat16)
    y = _labels(N, C, 11)
    x16[40] = 0
    x16[40, 5], x16[40, 17], x16[40, 50] = 0.5, bad, -0.25
    count, s, gram = _moments(x16, y, C)
    X = R.rows64(x16)
    with np.errstate(invalid="ignore"):
        rc, rs, rg = R.moments64(X, y, C)
    assert np.array_equal(np.isnan(gram), np.isnan(rg)) and np.array_equal(np.isinf(gram), np.isinf(rg))
    assert np.array_equal(np.isnan(s), np.isnan(rs)) and np.array_equal(np.isinf(s), np.isinf(rs))
    assert (~np.isfinite(s)).sum() == 1 and not np.isfinite(s[y[40], 17])
    clean = x16.clone()
    clean[40, 17] = 0
    _, s0, g0 = _moments(clean, y, C)
    fin = np.isfinite(rg)
    assert np.array_equal(gram[fin], g0[fin])
    fin = np.isfinite(rs)
    assert np.array_equal(s[fin], s0[fin])


def test_moments_two_calls_prefix_and_buffers():
    ops = _ops()
    N, D, C = RAGGED_N, 64, 9
    x16 = R.rows16(N + 50, D, 12, torch.bfloat16).cuda()
    y = torch.from_numpy(_labels(N + 50, C, 13)).to(torch.int32).cuda()
    a = ops.class_moments(x16[:N], y[:N], C)
    b = ops.class_moments(x16[:N].clone(), y[:N].clone(), C)
    ws = torch.empty(ops.moments_workspace(N, C, D) // 4 + 8, device="cuda", dtype=torch.float32)
    out = (torch.empty(C, device="cuda", dtype=torch.int32), torch.empty(C, D, device="cuda"), torch.empty(D, D, device="cuda"))
    c = ops.class_moments(x16[:N], y[:N], C, out=out, workspace=ws)
    assert all(u is v for u, v in zip(c, out))
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert ops.moments_workspace(N, C, D) == 65536 * 3 * 2 + 4 * C * D


def test_moments_error_paths_in_order():
    ops = _ops()
    x = R.rows16(8, 64, 1, torch.bfloat16).cuda()
    y = torch.zeros(8, dtype=torch.int32).cuda()
    with pytest.raises(TypeError, match="class_moments.*cuda"):
        ops.class_moments(x.cpu(), y, 2)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.class_moments(x.float(), y, 2)
    with pytest.raises(ValueError, match="2-D view"):
        ops.class_moments(x[0], y, 2)
    with pytest.raises(ValueError, match="labels"):
        ops.class_moments(x, y.cpu(), 2)
    with pytest.raises(ValueError, match="labels"):
        ops.class_moments(x, y.long(), 2)
    with pytest.raises(ValueError, match="labels"):
        ops.class_moments(x, y[:7], 2)
    with pytest.raises(NotImplementedError, match="D = 48"):
        ops.class_moments(R.rows16(8, 48, 1, torch.bfloat16).cuda(), y, 2)
    with pytest.raises(NotImplementedError, match="C = 257"):
        ops.class_moments(x, y, 257)
    with pytest.raises(NotImplementedError, match="C = 0"):
        ops.class_moments(x, y, 0)
    with pytest.raises(ValueError, match="C must be 1"):
        ops.class_moments(x, None, 2)
    wide = R.rows16(8, 72, 1, torch.bfloat16).cuda()
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.class_moments(wide[:, 4:68], y, 2)
    with pytest.raises(ValueError, match="workspace"):
        ops.class_moments(x, y, 2, workspace=torch.empty(16, device="cuda"))
    with pytest.raises(ValueError, match="gram"):
        ops.class_moments(x, y, 2, out=(None, None, torch.empty(64, 32, device="cuda")))


# ---------------------------------------------------------------------------------------------------------------------------
# gauss_scores
# ---------------------------------------------------------------------------------------------------------------------------
_FITS = {}


def _fit(D, C, kind, dtype):
    """the whitening of planted classes: "mid" = lam 0.5 (well conditioned), "auto" = Wang et al. fitted at N < D"""
    key = (D, C, kind, dtype)
    if key not in _FITS:
        N = 2 * C if kind == "auto" else max(4 * C, 40)
        x16, y = R.planted(N, C, D, D + C, dtype)
        _FITS[key] = R.fit64(R.rows64(x16), y, C, "auto" if kind == "auto" else 0.5)
    return _FITS[key]


def _gauss_inputs(Q, D, Rr, C, kind, dtype, seed=0):
    f = _fit(D, max(C, 1) if C else 2, kind, dtype)
    x16, _ = R.planted(Q, max(C, 2), D, 1000 + D + seed, dtype)
    T = np.ascontiguousarray(f["T32"][:Rr])
    t0 = np.ascontiguousarray(f["t032"][:Rr])
    centres = None if C == 0 else np.ascontiguousarray(f["centres32"][:, :Rr])
    offset = None if C == 0 else f["offset32"]
    return x16, T, t0, centres, offset, f["cond"]


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _run(x16, T, t0, centres, offset, **kw):
    out = _ops().gauss_scores(x16 if x16.is_cuda else x16.cuda(), _dev(T), t0=_dev(t0), centres=_dev(centres), offset=_dev(offset), **kw)
    torch.cuda.synchronize()
    return out


def _check_scores(x16, T, t0, centres, offset, got, tag):
    dtype = x16.dtype
    X = R.rows64(x16)
    D = X.shape[1]
    ref = R.scores64(X, T, dtype, t0, centres, offset)
    pred, lse, nearest, dmin, d2, z = got
    z = z.cpu().double().numpy()
    zb = (2 * D + 2) * 2.0 ** -24 * ref["zmag"] * 1.01 + 1e-37
    zr = float((np.abs(z - ref["z"]) / zb).max())
    _worst("z ratio to the bound", zr)
    msg = f"[gaussian] {tag}: z ratio {zr:.3e}"
    assert zr <= 1.0, (tag, zr)
    if centres is None:
        print(msg)
        return
    d2, lse, dmin = d2.cpu().double().numpy(), lse.cpu().double().numpy(), dmin.cpu().double().numpy()
    pred, nearest = pred.cpu().numpy(), nearest.cpu().numpy()
    e_d2 = float((np.abs(d2 - ref["d2"]) / np.maximum(ref["d2"], 1e-30)).max())
    e_dm = float((np.abs(dmin - ref["dmin"]) / np.maximum(ref["dmin"], 1e-30)).max())
    e_lse = float((np.abs(lse - ref["lse"]) / np.maximum(1.0, np.abs(ref["lse"]))).max())
    print(msg + f"; normalised deviations d2 {e_d2:.3e} dmin {e_dm:.3e} lse {e_lse:.3e}")
    _worst(f"d2 {dtype}{' R=1' if T.shape[0] == 1 else ''}", max(e_d2, e_dm))
    _worst(f"lse {dtype}{' R=1' if T.shape[0] == 1 else ''}", e_lse)
    tol = d2_tol(T.shape[0])
    assert e_d2 <= tol and e_dm <= tol, (tag, e_d2, e_dm)
    assert e_lse <= lse_tol(T.shape[0]), (tag, e_lse)
    # the kernel's own consistency, exactly: dmin is d2 at nearest, nearest and pred are argmin / argmax of its own numbers
    rows = np.arange(len(d2))
    assert np.array_equal(dmin, d2[rows, nearest]) and np.array_equal(nearest, d2.argmin(1))
    # against float64 wherever the top-two gap exceeds twice the asserted tolerance; at most 2 % of the rows may be left out
    keep_p, keep_n = R.outside_margin(ref, tol)
    assert (~keep_p).mean() <= 0.02 and (~keep_n).mean() <= 0.02, (tag, (~keep_p).mean(), (~keep_n).mean())
    assert np.array_equal(pred[keep_p], ref["pred"][keep_p]), tag
    assert np.array_equal(nearest[keep_n], ref["nearest"][keep_n]), tag


GAUSS_CASES = [(Q, 64, 64, 9, "mid") for Q in (1, 63, 64, 65, 130)] + \
              [(65, 64, 1, 2, "mid")] + [(65, 64, Rr, 9, "mid") for Rr in (31, 32, 33)] + \
              [(65, D, D, 9, kind) for D in (32, 512, 1024) for kind in ("mid", "auto")] + \
              [(130, 64, 64, 9, "auto"), (65, 64, 33, 2, "auto"), (65, 512, 33, 2, "mid"), (33, 1024, 31, 9, "auto")] + \
              [(65, 64, 64, C, "mid") for C in (1, 2, 256)] + [(33, 1024, 1024, 256, "mid"), (65, 64, 33, 0, "mid"), (17, 1024, 1024, 0, "auto")]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("Q,D,Rr,C,kind", GAUSS_CASES)
def test_gauss_scores_against_float64(Q, D, Rr, C, kind, dtype):
    x16, T, t0, centres, offset, cond = _gauss_inputs(Q, D, Rr, C, kind, dtype)
    got = _run(x16, T, t0, centres, offset, want_d2=C > 0, want_z=True)
    _check_scores(x16, T, t0, centres, offset, got, f"Q={Q} D={D} R={Rr} C={C} {kind} cond {cond:.2e} {dtype}")


def test_gauss_z_alone_writes_nothing_else():
    x16, T, t0, _, _, _ = _gauss_inputs(65, 64, 33, 0, "mid", torch.bfloat16)
    pred, lse, nearest, dmin, d2, z = _run(x16, T, t0, None, None)
    assert pred is None and lse is None and nearest is None and dmin is None and d2 is None and tuple(z.shape) == (65, 33)
    a = _run(x16, T, None, None, None)[5]
    ref = R.scores64(R.rows64(x16), T, torch.bfloat16)
    assert np.abs(a.cpu().double().numpy() - ref["z"]).max() <= (2 * 64 + 2) * 2.0 ** -24 * ref["zmag"].max()
    with pytest.raises(ValueError, match="need centres"):
        _run(x16, T, t0, None, None, want_d2=True)


def test_gauss_without_optional_outputs():
    x16, T, t0, centres, offset, _ = _gauss_inputs(65, 64, 64, 9, "mid", torch.bfloat16)
    full = _run(x16, T, t0, centres, offset, want_d2=True, want_z=True)
    lean = _run(x16, T, t0, centres, offset)
    assert lean[4] is None and lean[5] is None
    for u, v in zip(full[:4], lean[:4]):
        assert torch.equal(u, v)
    bare = _run(x16, T, None, centres, None)
    ref = R.scores64(R.rows64(x16), T, torch.bfloat16, None, centres, None)
    assert np.abs(bare[3].cpu().double().numpy() - ref["dmin"]).max() <= D2_TOL * ref["dmin"].max()


def test_gauss_exact_ties_go_to_the_lower_class():
    """exactly representable inputs: T = identity rows, centres +-e_r and duplicates - equal distances, bitwise"""
    D, Rr = 32, 4
    x = torch.zeros(3, D)
    x[1, 0] = 1.0
    x[2, 1] = -2.0
    T = np.eye(Rr, D, dtype=np.float32)
    centres = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, -1, 0, 0], [1, 0, 0, 0]], dtype=np.float32)
    pred, lse, nearest, dmin, d2, _ = _run(x.to(torch.bfloat16), T, None, centres, None, want_d2=True)
    assert pred.tolist() == [0, 0, 3] and nearest.tolist() == [0, 0, 3]
    assert dmin.tolist() == [1.0, 0.0, 1.0]
    assert d2[0].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0] and d2[2].tolist() == [5.0, 5.0, 9.0, 1.0, 5.0]
    assert abs(float(lse[0]) - (-0.5 + np.log(5.0))) < 1e-6


@pytest.mark.parametrize("dtype", BOTH)
def test_gauss_strided_nan_row_position_and_two_calls(dtype):
    Q, D, Rr, C = 130, 64, 33, 9
    x16, T, t0, centres, offset, _ = _gauss_inputs(Q, D, Rr, C, "auto", dtype)
    kw = dict(want_d2=True, want_z=True)
    a = _run(x16, T, t0, centres, offset, **kw)
    b = _run(x16.clone(), T, t0, centres, offset, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # strided rows with poisoned gaps
    big = torch.full((Q, D + 40), float("nan"), dtype=dtype).cuda()
    big[:, :D] = x16.cuda()
    for u, v in zip(a, _run(big[:, :D], T, t0, centres, offset, **kw)):
        assert torch.equal(u, v)
    # a row's outputs depend on neither Q nor its position
    perm = torch.from_numpy(np.random.default_rng(3).permutation(Q))
    c = _run(x16[perm][:77].contiguous(), T, t0, centres, offset, **kw)
    for u, v in zip(a, c):
        assert torch.equal(u[perm.cuda()][:77], v)
    one = _run(x16[64:65].contiguous(), T, t0, centres, offset, **kw)
    for u, v in zip(a, one):
        assert torch.equal(u[64:65], v)
    # a NaN row: NaN d2, lse, dmin; pred = nearest = 0 (NaN ranks lowest, ties to the lower class); no other row changes
    xn = x16.clone()
    xn[70, 9] = float("nan")
    n = _run(xn, T, t0, centres, offset, **kw)
    keep = torch.arange(Q).cuda() != 70
    for u, v in zip(a, n):
        assert torch.equal(u[keep], v[keep])
    assert torch.isnan(n[4][70]).all() and torch.isnan(n[1][70]) and torch.isnan(n[3][70]) and torch.isnan(n[5][70]).all()
    assert int(n[0][70]) == 0 and int(n[2][70]) == 0


def test_gauss_error_paths_in_order():
    ops = _ops()
    x = R.rows16(8, 64, 1, torch.bfloat16).cuda()
    T = torch.zeros(5, 64, device="cuda")
    m = torch.zeros(3, 5, device="cuda")
    with pytest.raises(TypeError, match="gauss_scores.*cuda"):
        ops.gauss_scores(x.cpu(), T)
    with pytest.raises(TypeError, match="gauss_scores.*cuda"):
        ops.gauss_scores(x, T.cpu())
    with pytest.raises(TypeError, match="gauss_scores: T.*cuda"):          # cuda over both operands comes before any dtype
        ops.gauss_scores(x.float(), T.cpu())
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        ops.gauss_scores(x.float(), T)
    with pytest.raises(TypeError, match="float32"):
        ops.gauss_scores(x, T.double())
    with pytest.raises(ValueError, match="T must be"):
        ops.gauss_scores(x, T[:, :32].contiguous())
    with pytest.raises(ValueError, match="t0"):
        ops.gauss_scores(x, T, t0=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match="centres"):
        ops.gauss_scores(x, T, centres=torch.zeros(3, 6, device="cuda"))
    with pytest.raises(ValueError, match="offset"):
        ops.gauss_scores(x, T, centres=m, offset=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match="need centres"):
        ops.gauss_scores(x, T, offset=torch.zeros(0, device="cuda"))
    with pytest.raises(NotImplementedError, match="D = 48"):
        ops.gauss_scores(R.rows16(8, 48, 1, torch.bfloat16).cuda(), torch.zeros(5, 48, device="cuda"))
    with pytest.raises(NotImplementedError, match="R = 1025"):
        ops.gauss_scores(x, torch.zeros(1025, 64, device="cuda"))
    with pytest.raises(NotImplementedError, match="C = 257"):
        ops.gauss_scores(x, T, centres=torch.zeros(257, 5, device="cuda"))
    wide = R.rows16(8, 72, 1, torch.bfloat16).cuda()
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.gauss_scores(wide[:, 4:68], T)
    with pytest.raises(ValueError, match="out must be"):
        ops.gauss_scores(x, T, out=(None,) * 5)
    with pytest.raises(ValueError, match="z"):
        ops.gauss_scores(x, T, out=(None,) * 5 + (torch.zeros(8, 4, device="cuda"),))
    assert ops.gauss_scores_workspace(33, 64) == 4 * 48 * 64 and ops.gauss_scores_workspace(0, 64) == 0
