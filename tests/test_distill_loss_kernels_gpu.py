"""GPU: the distillation row kernel (ops.kl_rows, csrc/distill_loss.hip) against the float64 evaluation of its contract on the
same fp32 inputs (distill_loss_helpers.ref_rows; never the kernel itself).

Bounds: absolute, per scale of the logits (unit normal times 1, 10, 100), H.KERNEL_TOL = 4 x the largest deviation of loss_row,
dlogits (grad_scale = 1) and rowdot measured on an MI355X over the shapes of test_kernel_against_float64; the
margin covers input draws, not another arithmetic.  Integer outputs, the untouched teacher, padding columns and the repeat
launch are exact.  Every case prints its figures before it asserts."""
import itertools
import os
import sys
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import distill_loss_helpers as H  # noqa: E402

ROWS = (1, 3, 4, 5, 9)                                    # both sides of four rows per work-group
COLS = (1, 63, 64, 65, 255, 256, 257, 1000)               # both sides of the lane count and of the four-column trip
SCALES = (1, 10, 100)
PAD = -777.0


def _inputs(R, C, scale, seed):
    """student and teacher rows, drawn independently; on even rows the teacher's maximum is moved onto the student's arg-max
    column, so that `agree` takes both values; no ties (continuous draws, the moved maximum a whole scale above the rest)"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lg = torch.randn(R, C, device="cuda", generator=gen) * scale
    te = torch.randn(R, C, device="cuda", generator=gen) * scale
    even = torch.arange(0, R, 2, device="cuda")
    te[even, lg[even].argmax(1)] = te[even].max(1).values + scale
    return lg, te


def _wide(t, extra):
    """t as the [:, :C] view of a buffer with `extra` padding columns holding PAD"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), PAD, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


def _run(lg, te, gs, d):
    """every output on; d: the gradient's destination (a tensor, possibly `lg` itself) -> (loss_row, a copy of d, rowdot, pred,
    agree)"""
    from cclip_hip import ops
    R = lg.shape[0]
    loss_row, rowdot, agree = (torch.full((R,), float("nan"), device="cuda") for _ in range(3))
    pred = torch.full((R,), -7, device="cuda", dtype=torch.int32)
    ops.kl_rows(lg, te, loss_row=loss_row, pred=pred, agree=agree, dlogits=d, grad_scale=gs, rowdot=rowdot)
    torch.cuda.synchronize()
    return loss_row, d.clone(), rowdot, pred, agree


def _deviation(got, ref):
    """largest absolute deviation of (loss_row, dlogits, rowdot) from float64"""
    return tuple((g.double() - r).abs().max().item() for g, r in zip(got[:3], ref[:3]))


def _layouts(lg, te):
    """(name, logits, logits buffer, teacher, teacher buffer, dlogits, dlogits buffer): ld = C with the gradient to a buffer of its
    own (ldd = C + 5), and ld = C + 3 with the gradient over the logits; the teacher always at ldt = C + 7"""
    tbuf, tv = _wide(te, 7)
    dbuf, dv = _wide(torch.zeros_like(lg), 5)
    yield "ld=C, separate ldd=C+5", lg.clone(), None, tv, tbuf, dv, dbuf
    lbuf, lv = _wide(lg, 3)
    yield "ld=C+3, in place", lv, lbuf, tv, tbuf, lv, lbuf


@pytest.mark.parametrize("R,C", list(itertools.product(ROWS, COLS)) + [(16385, 8)])      # and a second trip of the capped grid
def test_kernel_against_float64(R, C):
    bad = []
    for scale in SCALES if R < 100 else (1,):
        lg, te = _inputs(R, C, scale, R * 10000 + C * 10 + scale)
        ref = H.ref_rows(lg, te, 1.0)
        tol = H.KERNEL_TOL[scale]
        for name, lv, lbuf, tv, tbuf, dv, dbuf in _layouts(lg, te):
            tkeep = tbuf.clone()
            got = _run(lv, tv, 1.0, dv)
            dev = _deviation(got, ref)
            print(f"kl_rows dev [{R},{C}] x{scale} {name}: loss_row {dev[0]:.3e} dlogits {dev[1]:.3e} rowdot {dev[2]:.3e}"
                  f" | agree {int(got[4].sum())} of {R}")
            tag = f"[{R},{C}] x{scale} {name}"
            if not all(bool(torch.isfinite(t.double()).all()) for t in got):
                bad.append(f"{tag}: non-finite output")
            bad += [f"{tag}: {what} off by {v:.3e} > {t:.3e}" for what, v, t in zip(("loss_row", "dlogits", "rowdot"), dev, tol) if v > t]
            if not torch.equal(got[3].long(), ref[3]) or not torch.equal(got[4], ref[4].float()):
                bad.append(f"{tag}: pred / agree differ from the float64 arg-max comparison")
            if not torch.equal(tbuf, tkeep):
                bad.append(f"{tag}: the teacher was written")
            if not torch.equal(dbuf[:, C:], torch.full_like(dbuf[:, C:], PAD)):
                bad.append(f"{tag}: padding columns of dlogits lost their sentinel")
            # the same launch again on the same inputs (in place: on the logits restored): bitwise equal
            if lbuf is not None:
                lbuf[:, :C] = lg
            again = _run(lv, tv, 1.0, dv)
            if not all(torch.equal(x, y) for x, y in zip(got, again)):
                bad.append(f"{tag}: two launches differ")
    assert not bad, "\n".join(bad)


def test_grad_scale_scales_the_gradient_alone():
    lg, te = _inputs(5, 257, 10, 21)
    one = _run(lg, te, 1.0, torch.empty_like(lg))
    quarter = _run(lg, te, 0.25, torch.empty_like(lg))
    assert torch.equal(quarter[0], one[0]) and torch.equal(quarter[3], one[3]) and torch.equal(quarter[4], one[4])
    tol = H.KERNEL_TOL[10]
    ref = H.ref_rows(lg, te, 0.25)
    dev = _deviation(quarter, ref)
    print(f"grad_scale 0.25: dlogits {dev[1]:.3e} rowdot {dev[2]:.3e}")
    assert dev[1] <= 0.25 * tol[1] and dev[2] <= 0.25 * tol[2]


def test_one_column_is_exactly_zero():
    lg, te = _inputs(5, 1, 10, 22)
    loss_row, d, rowdot, pred, agree = _run(lg, te, 1.0, torch.full_like(lg, float("nan")))
    assert not loss_row.any() and not d.any() and not rowdot.any() and not pred.any()
    assert torch.equal(agree, torch.ones_like(agree))


@pytest.mark.parametrize("scale", SCALES)
def test_teacher_equal_to_student(scale):
    lg, _ = _inputs(9, 257, scale, 23)
    loss_row, d, rowdot, pred, agree = _run(lg, lg.clone(), 1.0, torch.full_like(lg, float("nan")))
    tol = H.KERNEL_TOL[scale]
    print(f"teacher == student x{scale}: max |loss_row| {loss_row.abs().max().item():.3e} max |dlogits| {d.abs().max().item():.3e}")
    assert loss_row.abs().max().item() <= tol[0] and d.abs().max().item() <= tol[1] and rowdot.abs().max().item() <= tol[2]
    assert torch.equal(agree, torch.ones_like(agree)) and torch.equal(pred.long(), lg.argmax(1))


def test_near_one_hot_teacher_against_a_student_that_disagrees():
    lg, te = _inputs(9, 257, 100, 24)
    odd = torch.arange(1, 9, 2, device="cuda")                               # the rows whose teacher maximum was left where it fell
    got = _run(lg, te, 1.0, torch.empty_like(lg))
    ref = H.ref_rows(lg, te, 1.0)
    dev = _deviation(got, ref)
    print(f"x100: loss rows {got[0].tolist()} | dev loss_row {dev[0]:.3e} dlogits {dev[1]:.3e} rowdot {dev[2]:.3e}")
    assert all(bool(torch.isfinite(t.double()).all()) for t in got)
    assert all(v <= t for v, t in zip(dev, H.KERNEL_TOL[100]))
    assert got[0][odd].min().item() > 10.0 and not got[4][odd].any()         # they do disagree, by a lot
    assert got[1].abs().max().item() <= 1.0                                  # |p_s - p_t| <= 1


def test_teacher_cell_at_minus_infinity_adds_exactly_nothing():
    lg, te = _inputs(5, 257, 1, 25)
    inf, tiny = te.clone(), te.clone()
    for r, c in ((0, 0), (1, 70), (2, 63), (2, 64), (2, 256), (4, 255)):     # a lane's first cell, a later one, the trip's edges
        inf[r, c] = -float("inf")
        tiny[r, c] = -1e30                                                   # finite, and exp() of it is exactly 0 as well
    got = _run(lg, inf, 1.0, torch.empty_like(lg))
    same = _run(lg, tiny, 1.0, torch.empty_like(lg))
    for x, y in zip(got, same):
        assert torch.equal(x, y)                                             # bit for bit what a cell of probability 0 adds
    dev = _deviation(got, H.ref_rows(lg, inf, 1.0))
    print(f"-inf teacher cells: dev loss_row {dev[0]:.3e} dlogits {dev[1]:.3e} rowdot {dev[2]:.3e}")
    assert all(bool(torch.isfinite(t.double()).all()) for t in got)
    assert all(v <= t for v, t in zip(dev, H.KERNEL_TOL[1]))


@pytest.mark.parametrize("where", ["student", "teacher"])
def test_nan_stays_in_its_row(where):
    lg, te = _inputs(9, 257, 1, 26)
    clean = _run(lg, te, 1.0, torch.empty_like(lg))
    lg2, te2 = lg.clone(), te.clone()
    (lg2 if where == "student" else te2)[6, 100] = float("nan")
    got = _run(lg2, te2, 1.0, torch.empty_like(lg))
    others = torch.arange(9, device="cuda") != 6
    for x, y in zip(got, clean):
        assert torch.equal(x[others], y[others])
    assert bool(torch.isnan(got[0][6])) and bool(torch.isnan(got[1][6]).all())
    # a row of NaN has no maximum: pred is the siblings' out-of-range marker, and it agrees with nothing
    lg3 = lg.clone()
    lg3[6] = float("nan")
    got = _run(lg3, lg3.clone(), 1.0, torch.empty_like(lg))
    assert got[3][6].item() >= 257 and got[4][6].item() == 0.0 and bool(torch.isnan(got[0][6]))
    assert torch.equal(got[4][others], torch.ones(8, device="cuda"))


def test_outputs_are_optional():
    from cclip_hip import ops
    lg, te = _inputs(5, 257, 1, 27)
    keep, tkeep = lg.clone(), te.clone()
    names = ("loss_row", "dlogits", "rowdot", "pred", "agree")
    full = dict(zip(names, _run(lg, te, 0.5, torch.empty_like(lg))))
    # GRAD off: the other instantiation of the kernel, so its loss is held against float64, and every subset against it
    nograd = {n: torch.empty_like(full[n]) for n in ("loss_row", "pred", "agree")}
    ops.kl_rows(lg, te, **nograd)
    torch.cuda.synchronize()
    dev = (nograd["loss_row"].double() - H.ref_rows(lg, te)[0]).abs().max().item()
    print(f"GRAD off: dev loss_row {dev:.3e}")
    assert dev <= H.KERNEL_TOL[1][0]
    assert torch.equal(nograd["pred"], full["pred"]) and torch.equal(nograd["agree"], full["agree"])
    ops.kl_rows(lg, te)                                                      # nothing asked for
    for k in range(4):
        for subset in itertools.combinations(("loss_row", "pred", "agree", "dlogits"), k + 1):
            for with_rowdot in (False, True) if "dlogits" in subset else (False,):
                kw = {n: torch.full_like(full[n], -3) for n in subset + (("rowdot",) if with_rowdot else ())}
                ops.kl_rows(lg, te, grad_scale=0.5, **kw)
                torch.cuda.synchronize()
                want = full if "dlogits" in subset else nograd
                for n, out in kw.items():
                    assert torch.equal(out, want[n]), (subset, with_rowdot, n)
    assert torch.equal(lg, keep) and torch.equal(te, tkeep)


def _raw(lg, te, R, C, ld, ldt, *, loss_row=None, d=None, ldd=0):
    """the C entry point itself, past the binding's own checks"""
    from cclip_hip._lib import check, lib
    p = lambda t: c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    check(lib.cclip_kl_rows(p(lg), c_long(ld), p(te), c_long(ldt), c_int(R), c_int(C), c_float(1.0), p(loss_row), p(None), p(None),
                            p(d), c_long(ldd), p(None), c_void_p(torch.cuda.current_stream().cuda_stream)), "cclip_kl_rows")


def test_argument_errors_launch_nothing():
    from cclip_hip import ops
    from cclip_hip._lib import CclipError
    R, C = 5, 70
    lg, te = _inputs(R, C, 1, 28)
    keep, tkeep = lg.clone(), te.clone()
    loss_row = torch.full((R,), PAD, device="cuda")
    d = torch.full((R, C), PAD, device="cuda")
    bad = [dict(lg=None), dict(te=None), dict(R=0), dict(R=-3), dict(C=0), dict(C=-1), dict(ld=C - 1), dict(ldt=C - 1),
           dict(ldd=C - 1)]
    for change in bad:
        args = dict(lg=lg, te=te, R=R, C=C, ld=C, ldt=C, ldd=C)
        args.update(change)
        with pytest.raises(CclipError, match="status 1"):
            _raw(args["lg"], args["te"], args["R"], args["C"], args["ld"], args["ldt"], loss_row=loss_row, d=d, ldd=args["ldd"])
    # the binding's own checks: dtypes, devices, shapes, strides
    for wrong in (te.double(), te.half(), te.cpu()):
        with pytest.raises(TypeError, match="teacher"):
            ops.kl_rows(lg, wrong, loss_row=loss_row)
    with pytest.raises(TypeError, match="logits"):
        ops.kl_rows(lg.double(), te, loss_row=loss_row)
    for wrong in (te[:4], te[:, :69], torch.empty(C, R, device="cuda").t()):
        with pytest.raises(ValueError, match="teacher"):
            ops.kl_rows(lg, wrong, loss_row=loss_row)
    with pytest.raises(ValueError):
        ops.kl_rows(lg, te, dlogits=d[:, :69])
    with pytest.raises(TypeError):
        ops.kl_rows(lg, te, agree=torch.empty(R, device="cuda", dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.kl_rows(lg, te, rowdot=loss_row)                                 # a row sum without dlogits
    torch.cuda.synchronize()
    assert torch.equal(lg, keep) and torch.equal(te, tkeep)
    assert torch.equal(loss_row, torch.full_like(loss_row, PAD)) and torch.equal(d, torch.full_like(d, PAD))
