"""The linear-probe kernels on the MI355X (cclip_probe_forward / cclip_probe_backward, csrc/embed_probe.hip) against float64 on
the same 16-bit rows at hi + lo (tests/probe_ref.py) within the derived bounds, and at their edges: outputs pre-filled with
NaN, two launches bitwise equal, strided views, ignored NaN rows, position independence, ties, argument errors.
Every case prints its largest err / tol per quantity (`[probe] ...`) before it asserts; run with -s to collect them."""
import ctypes
import functools

import pytest
import torch

import probe_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]

# (N, C, D): every N of {1, 63, 64, 65, 257}, 256 / 257 around the first split into two row parts, 3001 rows = several parts with
# a ragged last one; every C of {2, 5, 64, 65, 130, 256}; every D of {32, 64, 512, 1024}
CASES = [(1, 2, 32), (63, 5, 64), (64, 64, 512), (65, 65, 1024), (257, 130, 64), (256, 5, 512), (257, 5, 512), (256, 256, 32),
         (3001, 16, 64), (3001, 256, 1024), (2100, 40, 512)]


@functools.lru_cache(maxsize=None)
def case(N, C, D, dtype):
    """operands of a case and their float64 reference, computed once and shared; never written to"""
    gen = torch.Generator().manual_seed(7 * N + 31 * C + D)
    x = torch.randn(N, D, generator=gen)
    x16 = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    W = torch.randn(C, D, generator=gen) * 3.0
    b = torch.randn(C, generator=gen)
    y = torch.randint(0, C, (N,), generator=gen).to(torch.int32)
    if N > 4:
        y[1], y[3] = -1, C + 2
    rw = torch.rand(N, generator=gen)
    if N > 8:
        rw[2], rw[6], rw[8] = 0.0, float("nan"), 2.5
    scale, l2 = 1.0 / N, 0.01
    return x16, W, b, y, rw, scale, l2, R.reference(x16, W, b, y, rw, scale, l2)


def bits(t):
    return t.view(torch.int32)


def nanfill(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -7, device="cuda", dtype=dtype)
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def run(x16, W, b, y, rw, scale, l2, logits=False):
    from cclip_hip import ops
    N, D = x16.shape
    C = W.shape[0]
    xd, Wd = x16.cuda() if not x16.is_cuda else x16, W.cuda()
    bd = None if b is None else b.cuda()
    yd = None if y is None else y.cuda()
    rd = None if rw is None else rw.cuda()
    outs = []
    for _ in range(2):
        o = (nanfill(N), nanfill(N), nanfill(N, dtype=torch.int32)) + ((nanfill(N, C),) if logits else ())
        lse, loss, pred, z = ops.probe_forward(xd, Wd, bd, yd, rd, logits=logits, out=o)
        dW, db, obj = ops.probe_backward(xd, Wd, bd, yd, lse, scale, l2, rd, loss=loss, out=(nanfill(C, D), nanfill(C), nanfill(1)))
        outs.append((lse, loss, pred, z, dW, db, obj))
    torch.cuda.synchronize()
    for a, c in zip(*outs):
        if a is not None:
            assert torch.equal(bits(a), bits(c)), "two launches differ"
    return outs[0]


def ratios(name, got, ref):
    lse, loss, pred, z, dW, db, obj = got
    live = ref["live"]
    fin = torch.isfinite(ref["lse"])
    r = dict(lse=((lse.cpu().double() - ref["lse"]).abs() / ref["lse_tol"])[fin].max().item() if fin.any() else 0.0,
             loss=((loss.cpu().double() - ref["loss"]).abs()[live] / ref["loss_tol"][live]).max().item() if live.any() else 0.0,
             dW=((dW.cpu().double() - ref["dW"]).abs() / ref["dW_tol"]).max().item(),
             db=((db.cpu().double() - ref["db"]).abs() / ref["db_tol"]).max().item(),
             obj=abs(obj.item() - ref["objective"].item()) / ref["obj_tol"].item())
    if z is not None:
        r["z"] = ((z.cpu().double() - ref["z"]).abs() / ref["z_tol"])[fin].max().item()
    print(f"[probe] {name}: err / tol " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,C,D", CASES)
def test_forward_backward_against_float64(N, C, D, dtype):
    from cclip_hip import ops
    x16, W, b, y, rw, scale, l2, ref = case(N, C, D, dtype)
    assert ops.probe_parts(N, C, D) == R.geometry(N, C, D)[2] and ops.probe_workspace(N, C, D) == R.workspace_bytes(N, C, D)
    got = run(x16, W, b, y, rw, scale, l2, logits=True)
    lse, loss, pred, z = got[:4]
    r = ratios(f"N {N} C {C} D {D} {dtype}", got, ref)
    assert all(v <= 1.0 for v in r.values()), r
    dead = ~ref["live"]
    assert (bits(loss.cpu())[dead] == 0).all(), "an ignored row's loss is not +0.0"
    # pred is the argmax of the logits the kernel wrote, ties to the lower class; and the reference's wherever its margin decides
    zc = z.cpu()
    assert torch.equal(pred.cpu().long(), R.argmax_ref(zc.double()))
    top2 = ref["z"].topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * ref["z_tol"].max(dim=1).values
    assert torch.equal(pred.cpu().long()[sure], ref["pred"][sure])
    no_z = run(x16, W, b, y, rw, scale, l2, logits=False)
    assert torch.equal(bits(no_z[0]), bits(lse)) and torch.equal(bits(no_z[4]), bits(got[4])), "the call without logits differs"


def test_parts_go_from_one_to_two():
    from cclip_hip import ops
    assert ops.probe_parts(256, 64, 64) == 1 and ops.probe_parts(257, 64, 64) == 2
    assert ops.probe_parts(256, 5, 512) == 4 and ops.probe_parts(257, 5, 512) == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_strided_rows_nan_gaps_and_ignored_nan_rows(dtype):
    N, C, D = 300, 5, 64
    x16, W, b, y, rw, scale, l2, ref = case(N, C, D, dtype)
    base = run(x16, W, b, y, rw, scale, l2)
    wide = torch.full((N, D + 40), float("nan"), dtype=dtype)
    wide[:, :D] = x16
    got = run(wide.cuda()[:, :D], W, b, y, rw, scale, l2)
    for a, c in zip(base, got):
        if a is not None:
            assert torch.equal(bits(a), bits(c)), "a strided view differs"
    # NaN content under label -1 (row 1), label >= C (row 3), weight 0 (row 2) and weight NaN (row 6) leaves no trace
    xn = x16.clone()
    xn[[1, 2, 3, 6]] = float("nan")
    got = run(xn, W, b, y, rw, scale, l2)
    assert (bits(got[1].cpu())[[1, 2, 3, 6]] == 0).all()
    for i in (1, 4, 5, 6):
        assert torch.equal(bits(base[i]), bits(got[i])), f"output {i} changed with the content of ignored rows"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_all_ignored_absent_class_and_no_optionals(dtype):
    N, C, D = 130, 6, 64
    x16, W, b, y, rw, scale, l2, _ = case(N, C, D, dtype)
    none = torch.full((N,), -1, dtype=torch.int32)
    got = run(x16, W, b, none, rw, 1.0, 0.25)
    assert (bits(got[1]) == 0).all() and (got[5] == 0).all()
    assert torch.equal(got[4].cpu(), 0.25 * W), "dW != l2 W exactly with every row ignored"
    ref = R.reference(x16, W, b, none, rw, 1.0, 0.25)
    assert abs(got[6].item() - ref["objective"].item()) <= ref["obj_tol"].item()
    # a class no row carries, no bias, no weights
    y2 = torch.where(y == 4, torch.zeros_like(y), y)
    ref = R.reference(x16, W, None, y2, None, scale, l2)
    r = ratios("absent class, no bias, no weights", run(x16, W, None, y2, None, scale, l2), ref)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_logit_scale_100_is_finite(dtype):
    N, C, D = 200, 9, 128
    x16, labels, dirs = R.planted_rows([25] * 8, D, 0.3, 11, dtype)
    W = torch.cat([dirs, dirs[:1]]) * 100.0
    y = labels.to(torch.int32)
    ref = R.reference(x16, W, None, y, None, 1.0 / N, 0.0)
    got = run(x16, W, None, y, None, 1.0 / N, 0.0)
    assert torch.isfinite(got[0]).all() and got[0].abs().max().item() > 50
    r = ratios("logit scale 100", got, ref)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_row_outputs_do_not_depend_on_position(dtype):
    from cclip_hip import ops
    N, C, D = 257, 130, 64
    x16, W, b, y, rw, *_ = case(N, C, D, dtype)
    xd, Wd, bd, yd, rd = x16.cuda(), W.cuda(), b.cuda(), y.cuda(), rw.cuda()
    full = ops.probe_forward(xd, Wd, bd, yd, rd, logits=True)
    for i in (0, 77, 256):
        one = ops.probe_forward(xd[i:i + 1], Wd, bd, yd[i:i + 1].contiguous(), rd[i:i + 1].contiguous(), logits=True)
        for a, c in zip(full, one):
            assert torch.equal(bits(a[i:i + 1]), bits(c)), f"row {i} differs between N = 1 and N = 257"


def test_ties_and_nan_logits_in_pred():
    from cclip_hip import ops
    D, C = 32, 20
    x = torch.zeros(2, D)
    x[0, 0], x[1, 0] = 1.0, float("nan")
    W = torch.zeros(C, D)
    W[3, 0] = W[17, 0] = W[9, 0] = 2.0                                   # row 0: classes 3, 9, 17 tie -> 3; row 1: all NaN -> 0
    xd = x.bfloat16().cuda()
    _, _, pred, z = ops.probe_forward(xd, W.cuda(), None, None, None, logits=True)
    assert pred.tolist() == [3, 0], (pred.tolist(), z.cpu())
    b = torch.full((C,), float("nan"))
    b[18] = -4.0                                                            # every logit NaN but class 18's, which is the lowest number
    _, _, pred, z = ops.probe_forward(xd, W.cuda(), b.cuda(), None, None, logits=True)
    assert pred.tolist() == [18, 0], (pred.tolist(), z.cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_loss_and_gradient_belong_together(dtype):
    """(f(W + hV) - f(W - hV)) / 2h of the float64 objective at hi + lo against <dW_kernel, V>: what the line search relies on."""
    N, C, D = 600, 5, 64
    x16, W, b, y, rw, scale, l2, ref = case(N, C, D, dtype)
    got = run(x16, W, b, y, rw, scale, l2)
    dW = got[4].cpu().double()
    hi, lo = R.split16(W, dtype)
    Weff = hi.double() + lo.double()
    V = torch.randn(C, D, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    h = 1e-5
    f = lambda d: R.objective64(x16, Weff + d, b.double(), y, rw, scale, l2, W_l2=W.double() + d).item()
    fd = (f(h * V) - f(-h * V)) / (2 * h)
    bound = (ref["dW_tol"] * V.abs()).sum().item() + 1e-8                   # + the finite difference's own O(h^2) term
    print(f"[probe] directional derivative {fd:.9f} kernel {(dW * V).sum().item():.9f} bound {bound:.3e}")
    assert abs(fd - (dW * V).sum().item()) <= bound


def test_argument_errors_leave_outputs_untouched():
    from cclip_hip import ops
    from cclip_hip._lib import lib
    N, C, D = 64, 4, 64
    x = torch.randn(N, D).bfloat16().cuda()
    W, b = torch.randn(C, D).cuda(), torch.randn(C).cuda()
    y = torch.zeros(N, dtype=torch.int32).cuda()
    lse, loss, pred = nanfill(N), nanfill(N), nanfill(N, dtype=torch.int32)
    dW, db, obj = nanfill(C, D), nanfill(C), nanfill(1)
    nbytes = ops.probe_workspace(N, C, D)
    ws = torch.empty(nbytes // 4 + 4, device="cuda")
    P, L, I, Fl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    st = P(torch.cuda.current_stream().cuda_stream)

    rw, z = torch.ones(N, device="cuda"), nanfill(N, C)
    base = dict(x=x.data_ptr(), ldx=D, N=N, D=D, W=W.data_ptr(), b=b.data_ptr(), C=C, y=y.data_ptr(), rw=0, lse=lse.data_ptr(),
                loss=loss.data_ptr(), pred=pred.data_ptr(), z=0, scale=1.0, l2=0.0, dW=dW.data_ptr(), db=db.data_ptr(),
                obj=obj.data_ptr(), ws=ws.data_ptr(), nb=nbytes)

    def fwd(**kw):
        a = dict(base, **kw)
        return lib.cclip_probe_forward(P(a["x"]), L(a["ldx"]), L(a["N"]), I(a["D"]), P(a["W"]), P(a["b"]), I(a["C"]), P(a["y"]),
                                       P(a["rw"]), P(a["lse"]), P(a["loss"]), P(a["pred"]), P(a["z"]), P(a["ws"]), L(a["nb"]), st)

    def bwd(**kw):
        a = dict(base, **kw)
        return lib.cclip_probe_backward(P(a["x"]), L(a["ldx"]), L(a["N"]), I(a["D"]), P(a["W"]), P(a["b"]), I(a["C"]), P(a["y"]),
                                        P(a["rw"]), P(a["lse"]), P(a["loss"]), Fl(a["scale"]), Fl(a["l2"]), P(a["dW"]), P(a["db"]),
                                        P(a["obj"]), P(a["ws"]), L(a["nb"]), st)

    # the cases both entries share: null, range, stride, alignment of the operands and of the optional arrays, workspace
    shared = [dict(x=0), dict(W=0), dict(ws=0), dict(lse=0), dict(N=0), dict(N=2 ** 31), dict(C=1), dict(C=257), dict(D=16), dict(D=48),
              dict(D=1056), dict(ldx=D - 8), dict(ldx=D + 4), dict(x=x.data_ptr() + 2), dict(ws=ws.data_ptr() + 4),
              dict(W=W.data_ptr() + 2), dict(b=b.data_ptr() + 2), dict(y=y.data_ptr() + 2), dict(rw=rw.data_ptr() + 2),
              dict(lse=lse.data_ptr() + 2), dict(loss=loss.data_ptr() + 2), dict(nb=nbytes - 1)]
    bad = shared + [dict(loss=0), dict(pred=0), dict(pred=pred.data_ptr() + 2), dict(z=z.data_ptr() + 2)]
    for kw in bad:
        assert fwd(**kw) == 1, kw
    bad_b = shared + [dict(dW=0), dict(db=0), dict(loss=0), dict(obj=0), dict(scale=float("nan")), dict(scale=float("inf")),
                      dict(scale=-1.0), dict(l2=float("nan")), dict(l2=float("inf")), dict(l2=-0.5), dict(dW=dW.data_ptr() + 2),
                      dict(db=db.data_ptr() + 2), dict(obj=obj.data_ptr() + 2)]
    for kw in bad_b:
        assert bwd(**kw) == 1, kw
    assert torch.isnan(z).all()
    torch.cuda.synchronize()
    for t in (lse, loss, dW, db, obj):
        assert torch.isnan(t).all(), "a refused call wrote an output"
    assert (pred == -7).all()
    assert fwd() == 0 and bwd() == 0 and fwd(rw=rw.data_ptr(), z=z.data_ptr()) == 0 and bwd(loss=0, obj=0) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(lse).all() and torch.isfinite(dW).all() and torch.isfinite(obj).all()
    with pytest.raises(TypeError):
        ops.probe_forward(x.cpu(), W, b, y)
    with pytest.raises(NotImplementedError):
        ops.probe_forward(x, W[:1].contiguous(), None, y)
    with pytest.raises(ValueError):
        ops.probe_forward(x, W, b, y.long())
