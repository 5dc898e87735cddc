"""cclip_cache_affinity_bwd (csrc/embed_cache_bwd.hip) on the MI355X against the float64 closed form and the derived
per-element bound of cache_affinity_bwd_ref.py, with every padding row of g NaN and dG pre-filled with NaN: partial and
several query tiles, an empty class, a one-row class, an exact segment and a segment plus one, more than one work-group's
block and a last block that is not full, the smallest D and the D at which the columns are cut over the grid, strides,
exclude, zero columns of dA, bitwise repeatability and argument errors."""
import pytest
import torch

import cache_affinity_bwd_ref as B
import cache_affinity_ref as R

pytestmark = pytest.mark.gpu

IDS = ["bf16", "fp16"]
SIZES = (0, 1, 16, 17, 3, 40)                     # 128 laid-out rows: two full blocks of 64
SIZES_TAIL = (0, 1, 16, 17, 3, 40, 5)             # 144 laid-out rows: the third block holds 16


def make_dA(seed, Q, C):
    """what a mean cross-entropy sends back: of order 1 / Q, both signs"""
    return (torch.randn(Q, C, generator=torch.Generator().manual_seed(seed)) / Q).float()


def run(q16, g16, labels, C, beta, dA, exclude=None, strided=False):
    """lay the problem out as the product does (NaN padding), launch twice into NaN-filled outputs, compare bitwise"""
    from cclip_hip import ops
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    assert torch.isnan(laid[gather < 0].float()).all()
    ex = None if exclude is None else R.to_laid(exclude, gather).cuda()
    qd, gd = q16.cuda(), laid.cuda()
    if strided:
        D = q16.shape[1]
        qw = torch.full((q16.shape[0], D + 8), float("nan"), dtype=q16.dtype); qw[:, 8:] = q16
        gw = torch.full((laid.shape[0], 2 * D + 64), float("nan"), dtype=q16.dtype); gw[:, 16:16 + D] = laid
        qd, gd = qw.cuda()[:, 8:], gw.cuda()[:, 16:16 + D]
    dAd = dA.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((laid.shape[0], q16.shape[1]), float("nan"), device="cuda")
        assert ops.cache_affinity_backward(qd, gd, off, ln, beta, dAd, exclude=ex, out=out) is out
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches differ"
    return outs[0].cpu(), gather


def against_reference(q16, g16, labels, C, beta, dA, what, exclude=None, strided=False):
    out, gather = run(q16, g16, labels, C, beta, dA, exclude, strided)
    dG, T, s = B.reference(q16, g16, labels, beta, dA, exclude)
    tol = B.tolerance(T, beta, q16, g16, s, dA, exclude)
    B.check(out, B.to_laid(dG, gather), B.to_laid(tol, gather), what)
    pad = out[gather < 0]
    assert (pad.view(torch.int32) == 0).all(), f"{what}: a padding row is not bitwise +0.0"
    return out, gather, dG, tol


# (Q, D, sizes): every Q of {1, 15, 17, 65, 130} and every D of {32, 64, 512, 1024}
CASES = [(1, 32, SIZES), (15, 64, SIZES_TAIL), (17, 512, SIZES), (65, 1024, SIZES_TAIL), (130, 512, SIZES_TAIL), (130, 1024, SIZES),
         (65, 32, SIZES), (17, 1024, SIZES)]


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,D,sizes", CASES)
def test_kernel_against_float64(Q, D, sizes, dtype):
    C = len(sizes)
    q16, g16, labels = R.make_problem(1000 * D + 10 * C + Q, Q, sizes, D, dtype)
    against_reference(q16, g16, labels, C, 5.5, make_dA(Q + D, Q, C), f"Q{Q} D{D} C{C} {dtype}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_many_blocks(dtype):
    """about 1900 stored rows (30 work-groups), classes that span several of them, Q over five tiles"""
    sizes = [700, 0, 1, 1133, 65]
    q16, g16, labels = R.make_problem(51, 130, sizes, 64, dtype)
    against_reference(q16, g16, labels, 5, 5.5, make_dA(52, 130, 5), f"1900 rows {dtype}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_small_norms_and_betas(dtype):
    C = len(SIZES)
    q16, g16, labels = R.make_problem(53, 17, SIZES, 64, dtype, normalise=False, scale=0.05)   # |row| about 0.4
    against_reference(q16, g16, labels, C, 5.5, make_dA(54, 17, C), f"small norms {dtype}")
    q16, g16, labels = R.make_problem(55, 17, SIZES, 64, dtype)
    against_reference(q16, g16, labels, C, 40.0, make_dA(56, 17, C), f"beta 40 {dtype}")
    against_reference(q16, g16, labels, C, -2.0, make_dA(57, 17, C), f"beta -2 {dtype}")      # padding stays +0.0
    against_reference(q16, g16, labels, C, 5.5, 1e-6 * make_dA(58, 17, C), f"tiny dA {dtype}")  # fp16: subnormal without the scale
    against_reference(q16, g16, labels, C, 5.5, 1e6 * make_dA(59, 17, C), f"huge dA {dtype}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_exclude_and_zero_columns(dtype):
    C, beta, Q = len(SIZES_TAIL), 5.5, 40
    q16, g16, labels = R.make_problem(60, Q, SIZES_TAIL, 512, dtype)
    dA = make_dA(61, Q, C)
    base, gather, _, _ = against_reference(q16, g16, labels, C, beta, dA, f"no exclude {dtype}")
    none, _ = run(q16, g16, labels, C, beta, dA, exclude=torch.full((Q,), -1))
    assert torch.equal(none.view(torch.int32), base.view(torch.int32)), "exclude = -1 differs from exclude = None"
    # every query excludes a row; all of them the one-row class's only row: that row's gradient is exactly 0
    single = SIZES_TAIL.index(1)
    only = int((labels == single).nonzero()[0, 0])
    out, gather, dG, tol = against_reference(q16, g16, labels, C, beta, dA, f"exclude only row {dtype}", exclude=torch.full((Q,), only))
    laid_only = int((gather == only).nonzero()[0, 0])
    assert (out[laid_only] == 0).all() and (base[laid_only] != 0).any()
    # a mixed exclude: as the leave-one-out objective gives it (query i is stored row i), and none for some
    ex = torch.arange(Q) % labels.numel()
    ex[::7] = -1
    q_self = q16.clone()
    q_self[ex >= 0] = g16[ex[ex >= 0]]                                         # s = 1 on the excluded pair: the largest term if it leaked
    against_reference(q_self, g16, labels, C, beta, dA, f"leave one out {dtype}", exclude=ex)
    # dA[:, c] = 0 for one class: its rows are exactly 0, the others unchanged
    big = SIZES_TAIL.index(40)
    dA0 = dA.clone(); dA0[:, big] = 0.0
    out0, gather, _, _ = against_reference(q16, g16, labels, C, beta, dA0, f"zero column {dtype}")
    rows = torch.tensor([int(labels[n]) == big if n >= 0 else False for n in gather.tolist()])
    assert (out0[rows] == 0).all() and rows.sum() == 40
    keep = torch.tensor([n >= 0 and int(labels[n]) != big for n in gather.tolist()])
    assert torch.equal(out0[keep].view(torch.int32), base[keep].view(torch.int32)), "a zero column moved another class"


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,D", [(15, 64), (65, 512), (17, 1024)])
def test_strided_operands(Q, D, dtype):
    """both operands as column slices of wider buffers (row strides D + 8 and 2 D + 64, 16-byte aligned offsets)"""
    C = len(SIZES_TAIL)
    q16, g16, labels = R.make_problem(62 + Q, Q, SIZES_TAIL, D, dtype)
    dA = make_dA(63, Q, C)
    ex = torch.randint(-1, labels.numel(), (Q,), generator=torch.Generator().manual_seed(3))
    a, _, _, _ = against_reference(q16, g16, labels, C, 5.5, dA, f"strided Q{Q} D{D} {dtype}", exclude=ex, strided=True)
    b, _ = run(q16, g16, labels, C, 5.5, dA, exclude=ex)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "strided and contiguous operands differ"


def test_argument_errors():
    from cclip_hip import ops
    C, D, Q = len(SIZES), 64, 4
    q16, g16, labels = R.make_problem(64, Q, SIZES, D, torch.bfloat16)
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    qd, gd, dA = q16.cuda(), laid.cuda(), make_dA(65, Q, C).cuda()
    Np = laid.shape[0]
    out = torch.full((Np, D), float("nan"), device="cuda")
    bad_off = off.clone(); bad_off[3] += 8
    calls = [
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA.cpu(), out=out)),               # a host dA
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA.double(), out=out)),
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA, out=out.cpu())),
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA, out=out.double())),
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd.half(), off, ln, 5.5, dA, out=out)),
        (TypeError, lambda: ops.cache_affinity_backward(qd.cpu(), gd, off, ln, 5.5, dA, out=out)),
        (TypeError, lambda: ops.cache_affinity_backward(qd, gd, off.cuda(), ln.cuda(), 5.5, dA, out=out)),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA, out=out[:-16])),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA, out=out[:, :32])),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA[:, :C - 1], out=out)),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA.t().contiguous().t(), out=out)),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, bad_off, ln, 5.5, dA, out=out)),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, float("inf"), dA, out=out)),
        (ValueError, lambda: ops.cache_affinity_backward(qd, gd, off, ln, 5.5, dA, exclude=torch.zeros(Q + 1, device="cuda", dtype=torch.int32), out=out)),
        (NotImplementedError, lambda: ops.cache_affinity_backward(torch.zeros(Q, 40, device="cuda", dtype=torch.bfloat16),
                                                                  torch.zeros(Np, 40, device="cuda", dtype=torch.bfloat16), off, ln, 5.5, dA)),
    ]
    for kind, call in calls:
        with pytest.raises(kind):
            call()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to out"
