"""The three label-spreading kernels (csrc/label_spread.hip) on the MI355X against the float64 reference of
tests/label_spread_ref.py, under its derived bounds, at the kernels' own edges: every class count at which the lane layout
(CW = 2 .. 64), the edge-group count (G = 8, 4, 2, 1), the classes per lane (1, 2, 4) or the number of passes (C > 256, 512,
768) changes; rows of 0, 1, G - 1, G, G + 1 and 600 entries and a row of zero weights; row counts below, at and above a
work-group's rows.  Every case prints its largest err / tol before it asserts."""
import ctypes
import functools

import pytest
import torch

import label_spread_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ISSUE_C = [2, 9, 16, 17, 64, 65, 257, 1024]
EDGE_C = [3, 4, 5, 8, 32, 33, 128, 129, 256, 512, 513, 768, 769]                  # CW, G, NQ and pass-count edges of spread_plan
NS = [1, 2, 63, 257, 1025]
STEP_CASES = [(NS[(i + 2) % 5], C, i % 2 == 0, i % 3 != 0) for i, C in enumerate(ISSUE_C + EDGE_C)] + \
             [(N, C, True, True) for N in NS for C in (2, 9)]


def ratio(name, got, ref, tol):
    err = (got.double().cpu() - ref.double()).abs()
    r = (err / tol.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    r = float("inf") if torch.isnan(err).any() else r
    print(f"[label spread] {name}: largest err / tol {r:.3f}")
    return r


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def csr_case(N, C):
    """Rows of 0, 1, G - 1, G, G + 1 and 600 entries, a row of 5 zero weights, then 0 .. 40 entries at random; columns at
    random (a column may repeat inside a row: the entries add up)"""
    G = R.spread_plan(C)[1]
    g = torch.Generator().manual_seed(31 * N + C)
    head = [0, 1, max(G - 1, 0), G, G + 1, 600, 5]
    if N < len(head):
        head = [600, 0][:N]                                                       # N = 1: the hub row; N = 2: it and an empty row
    n = torch.tensor(head + torch.randint(0, 41, (N - len(head),), generator=g).tolist())
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(n, 0)])
    nnz = int(offsets[-1])
    cols = torch.randint(0, N, (nnz,), generator=g).to(torch.int32)
    vals = (0.05 + torch.rand(nnz, generator=g)).float()
    if N >= 7:
        vals[offsets[6]:offsets[7]] = 0.0
    return offsets, cols, vals


@functools.lru_cache(maxsize=None)
def label_case(N, C):
    g = torch.Generator().manual_seed(7 * N + C)
    lab = torch.randint(-1, C, (N,), generator=g).to(torch.int32)
    if N > 8:
        lab[3], lab[4], lab[5] = C, C + 7, 2 ** 31 - 1                            # labels >= C: unlabelled, and they index nothing
        lab[6] = -(2 ** 31)
    cw = (0.01 + torch.rand(C, generator=g)).float()
    cw[C // 2] = 0.0                                                              # a class without a labelled row
    F = torch.rand(N, C, generator=g).float()
    return lab, cw, F


@pytest.mark.parametrize("N,C", [(NS[i % 5], C) for i, C in enumerate([2, 9, 33])] + [(N, 4) for N in NS])
def test_normalize(N, C):
    from cclip_hip import ops
    offsets, cols, vals = csr_case(N, C)
    ref = R.normalize_ref(offsets, cols, vals, N)
    od, cd, vd = offsets.to(DEV), cols.to(DEV), vals.to(DEV)
    deg, out = ops.label_graph_normalize(od, cd, vd)
    r = max(ratio(f"normalize N{N} deg", deg, ref["deg"], ref["deg_tol"]), ratio(f"normalize N{N} vals", out, ref["vals"], ref["vals_tol"]))
    assert r <= 1.0 and torch.isfinite(out).all()
    if N >= 7:
        assert deg[0].item() == 0.0 and deg[6].item() == 0.0                      # the empty row, the row of zero weights
        assert (out[offsets[6]:offsets[7]] == 0).all() and (out[cols.long().to(DEV) == 6] == 0).all()
    inplace = vd.clone()
    deg2, out2 = ops.label_graph_normalize(od, cd, inplace, out_vals=inplace)     # vals_out == vals is legal
    assert out2 is inplace and same_bits(out, out2) and same_bits(deg, deg2)


@pytest.mark.parametrize("N,C,weighted,with_delta", STEP_CASES)
def test_step(N, C, weighted, with_delta):
    from cclip_hip import ops
    offsets, cols, vals = csr_case(N, C)
    lab, cw, F = label_case(N, C)
    cw = cw if weighted else None
    ref = R.step_ref(F, lab, cw, offsets, cols, vals, 0.9)
    args = (F.to(DEV), lab.to(DEV), offsets.to(DEV), cols.to(DEV), vals.to(DEV), 0.9, None if cw is None else cw.to(DEV))
    F_in = args[0].clone()
    out, delta = ops.label_spread_step(*args, delta=with_delta)
    out2, delta2 = ops.label_spread_step(*args, delta=with_delta)
    assert out.data_ptr() != args[0].data_ptr() and same_bits(args[0], F_in)
    r = ratio(f"step N{N} C{C} out", out, ref["out"], ref["tol"])
    if with_delta:
        r = max(r, ratio(f"step N{N} C{C} delta", delta, ref["delta"], ref["delta_tol"]))
    else:
        assert delta is None
    assert r <= 1.0
    assert same_bits(out, out2) and (not with_delta or same_bits(delta, delta2))


def test_step_all_unlabelled_and_empty_graph():
    from cclip_hip import ops
    N, C = 257, 9
    offsets, cols, vals = csr_case(N, C)
    _, cw, F = label_case(N, C)
    lab = torch.full((N,), -1, dtype=torch.int32)
    ref = R.step_ref(F, lab, cw, offsets, cols, vals, 0.5)
    out, _ = ops.label_spread_step(F.to(DEV), lab.to(DEV), offsets.to(DEV), cols.to(DEV), vals.to(DEV), 0.5, cw.to(DEV))
    assert ratio("step all unlabelled", out, ref["out"], ref["tol"]) <= 1.0 and (out[0] == 0).all()
    # no edge at all: F_out is the label term alone, (1 - alpha) w rounded once
    lab2, _, _ = label_case(N, C)
    zero_off = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    none = torch.zeros(0, device=DEV)
    out, delta = ops.label_spread_step(F.to(DEV), lab2.to(DEV), zero_off, none.to(torch.int32), none, 0.9, cw.to(DEV))
    want = (1.0 - R.f32(0.9)) * R.one_hot(lab2, cw, C, torch.float64)
    assert ((out.cpu().double() - want).abs() <= R.U * want).all()


def test_clamped_offsets_and_cols():
    """offsets outside [0, nnz] and running backwards, cols outside [0, N): inputs the contract declares legal - both are
    clamped before use, and the reference restates the clamp"""
    from cclip_hip import ops
    N, C, nnz = 257, 9, 4000
    g = torch.Generator().manual_seed(99)
    offsets = torch.randint(-50, nnz + 50, (N + 1,), generator=g)
    offsets[10], offsets[11], offsets[12] = 3000, 100, -(2 ** 62)
    offsets[20] = 2 ** 62
    cols = torch.randint(-20, N + 20, (nnz,), generator=g).to(torch.int32)
    cols[0], cols[1] = 2 ** 31 - 1, -(2 ** 31)
    vals = torch.rand(nnz, generator=g).float()
    lab, cw, F = label_case(N, C)
    row, entry, col, n = R.rows_of(offsets, cols, N)
    assert int(n.max()) > 600 and int((n == 0).sum()) > 50 and int(entry.max()) < nnz and int(col.max()) == N - 1
    ref = R.step_ref(F, lab, cw, offsets, cols, vals, 0.9)
    od, cd, vd = offsets.to(DEV), cols.to(DEV), vals.to(DEV)
    out, delta = ops.label_spread_step(F.to(DEV), lab.to(DEV), od, cd, vd, 0.9, cw.to(DEV))
    r = max(ratio("clamped step out", out, ref["out"], ref["tol"]), ratio("clamped step delta", delta, ref["delta"], ref["delta_tol"]))
    nref = R.normalize_ref(offsets, cols, vals, N)
    deg, scaled = ops.label_graph_normalize(od, cd, vd)
    assert max(r, ratio("clamped normalize deg", deg, nref["deg"], nref["deg_tol"])) <= 1.0
    seen = torch.zeros(nnz, dtype=torch.bool)
    seen[entry] = True                                                            # entries of overlapping rows have no one value:
    assert torch.isfinite(scaled.cpu()[seen]).all()                               # only that they are finite


@functools.lru_cache(maxsize=None)
def finish_case(N, C):
    g = torch.Generator().manual_seed(13 * N + C)
    F = torch.rand(N, C, generator=g).float()
    F[:, 0] *= 1e-3                                                               # a wide range inside a row
    special = {}
    if N > 40:
        F[3] = 0.0                                                                # z == 0
        F[5] = 0.25                                                               # every class tied
        F[7, C - 1] = F[7, 1] = 2.0                                               # the top tied between class 1 and the last
        F[9] = 0.0
        F[9, C // 2] = 0.5                                                        # one-hot: certainty 1
        F[11, C - 1] = float("nan")
        special = dict(zero=3, flat=5, tie=7, hot=9, nan=11)
    return F, special


@pytest.mark.parametrize("N,C", [(NS[(i + 3) % 5], C) for i, C in enumerate(ISSUE_C + EDGE_C)] + [(N, 9) for N in NS])
def test_finish(N, C):
    from cclip_hip import ops
    F, sp = finish_case(N, C)
    ref = R.finish_ref(F)
    dist, pred, conf, cert = ops.label_spread_finish(F.to(DEV))
    again = ops.label_spread_finish(F.to(DEV).clone())
    ok = ~ref["nan"]
    assert 1.0 - ref["decided"][ok].double().mean().item() <= 0.01                # the reference leaves no clean row out
    r = max(ratio(f"finish N{N} C{C} dist", dist.cpu()[ok], ref["dist"][ok], ref["dist_tol"][ok]),
            ratio(f"finish N{N} C{C} conf", conf.cpu()[ok], ref["conf"][ok], ref["conf_tol"][ok]),
            ratio(f"finish N{N} C{C} cert", cert.cpu()[ok], ref["cert"][ok], ref["cert_tol"][ok]))
    assert r <= 1.0
    assert torch.equal(pred.cpu().long()[ok], ref["pred"][ok])
    if sp:
        assert pred[sp["zero"]].item() == -1 and conf[sp["zero"]].item() == 0.0 and cert[sp["zero"]].item() == 0.0
        assert (dist[sp["zero"]] == 0).all()
        assert pred[sp["flat"]].item() == 0 and abs(cert[sp["flat"]].item()) <= ref["cert_tol"][sp["flat"]].item()
        assert pred[sp["tie"]].item() == 1
        assert pred[sp["hot"]].item() == C // 2 and cert[sp["hot"]].item() == 1.0 and conf[sp["hot"]].item() == 1.0
        k = sp["nan"]
        assert pred[k].item() == -1 and torch.isnan(conf[k]) and torch.isnan(cert[k]) and torch.isnan(dist[k]).all()
        assert torch.isfinite(dist.cpu()[ok]).all() and torch.isfinite(cert.cpu()[ok]).all()     # the NaN stays in its row
    for a, b in zip((dist, conf, cert), (again[0], again[2], again[3])):
        assert same_bits(a[ok.to(DEV)], b[ok.to(DEV)])
    assert torch.equal(pred, again[1])
    none = ops.label_spread_finish(F.to(DEV), dist=False)
    assert none[0] is None and torch.equal(none[1], pred)


def test_refused_arguments_launch_nothing():
    from cclip_hip import load_library, ops
    lib = load_library()
    N, C = 63, 9
    offsets, cols, vals = (t.to(DEV) for t in csr_case(N, C))
    lab, cw, F = (t.to(DEV) for t in label_case(N, C))
    nnz = cols.numel()
    out = torch.full((N, C), -7.0, device=DEV)
    delta = torch.full((N,), -7.0, device=DEV)
    p = lambda t, shift=0: ctypes.c_void_p(0 if t is None else t.data_ptr() + shift)
    i64, i32, f = ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step(F_in=F, F_out=out, n=N, c=C, labels=lab, off=offsets, co=cols, va=vals, nz=nnz, alpha=0.9, shift=0):
        return lib.cclip_label_spread_step(p(F_in), p(F_out, shift), i64(n), i32(c), p(labels), p(cw), p(off), p(co), p(va), i64(nz),
                                           f(alpha), p(delta), stream)
    bad = [dict(F_out=F), dict(F_in=None), dict(F_out=None), dict(labels=None), dict(off=None), dict(co=None), dict(va=None),
           dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(nz=-1), dict(nz=2 ** 31), dict(c=1), dict(c=1025), dict(alpha=1.5),
           dict(alpha=-0.1), dict(alpha=float("nan")), dict(shift=2)]
    for kw in bad:
        assert step(**kw) == 1, kw                                                # CCLIP_ERR_ARG
    pred = torch.full((N,), -7, device=DEV, dtype=torch.int32)
    conf, cert = torch.full((N,), -7.0, device=DEV), torch.full((N,), -7.0, device=DEV)
    for kw in (dict(F=None), dict(n=0), dict(n=2 ** 31), dict(c=1), dict(c=1025), dict(pred=None), dict(shift=2)):
        a = dict(F=F, n=N, c=C, pred=pred, shift=0)
        a.update(kw)
        assert lib.cclip_label_spread_finish(p(a["F"]), i64(a["n"]), i32(a["c"]), p(None), p(a["pred"]), p(conf, a["shift"]), p(cert),
                                             stream) == 1, kw
    deg = torch.full((N,), -7.0, device=DEV)
    scaled = torch.full((nnz,), -7.0, device=DEV)
    for kw in (dict(off=None), dict(deg=None), dict(co=None), dict(n=0), dict(n=2 ** 31), dict(nz=-1), dict(nz=2 ** 31), dict(shift=2)):
        a = dict(off=offsets, deg=deg, co=cols, n=N, nz=nnz, shift=0)
        a.update(kw)
        assert lib.cclip_label_graph_normalize(p(a["off"]), p(a["co"]), p(vals), i64(a["n"]), i64(a["nz"]), p(a["deg"], a["shift"]),
                                               p(scaled), stream) == 1, kw
    torch.cuda.synchronize()
    for t in (out, delta, conf, cert, deg, scaled):
        assert (t == -7.0).all()                                                  # nothing was launched
    assert (pred == -7).all()
    # the binding's own checks
    ok = (F, lab, offsets, cols, vals, 0.9, cw)
    assert ops.label_spread_step(*ok)[0].shape == (N, C)
    swaps = [(0, F.cpu(), TypeError), (0, F.double(), TypeError), (0, F[:, :1], ValueError), (0, F.t(), ValueError),
             (1, lab.long(), TypeError), (1, lab[:5], ValueError), (2, offsets.int(), TypeError), (2, offsets[:N], ValueError),
             (3, cols.long(), TypeError), (4, vals[:1], ValueError), (4, vals.cpu(), TypeError), (5, 1.5, ValueError),
             (6, cw[:3], ValueError), (6, cw.double(), TypeError)]
    for pos, wrong, exc in swaps:
        args = list(ok)
        args[pos] = wrong
        with pytest.raises(exc):
            ops.label_spread_step(*args)
    with pytest.raises(ValueError, match="must not be F"):
        ops.label_spread_step(*ok, out_F=F)
    with pytest.raises(ValueError):
        ops.label_spread_step(*ok, out_delta=torch.empty(N - 1, device=DEV))
    with pytest.raises(ValueError):
        ops.label_spread_step(*ok, delta=False, out_delta=torch.empty(N, device=DEV))
    with pytest.raises(ValueError):
        ops.label_spread_finish(torch.zeros(4, 1025, device=DEV))
    with pytest.raises(ValueError):
        ops.label_spread_finish(F, out_pred=torch.empty(N, device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.label_graph_normalize(offsets, cols, vals[:-1])
    with pytest.raises(ValueError):
        ops.label_graph_normalize(offsets[:1], cols, vals)
