"""cclip_cache_affinity (csrc/embed_cache.hip) on the MI355X against the float64 reference and the derived per-element bound of
cache_affinity_ref.py (its docstring holds the derivation and the largest err / tol measured), on rows normalised and then
rounded to 16 bits, `out` pre-filled with NaN and every padding row NaN: segment ends on, before and after sub-tile and tile
edges, empty classes, several splits, exclude, bitwise repeatability, independence of Q, strides, argument errors, no Q x N buffer."""
import ctypes

import pytest
import torch

import cache_affinity_ref as R

pytestmark = pytest.mark.gpu

MIX = [0, 1, 15, 16, 17, 63, 65]                # class sizes, cycled over the classes of a problem
IDS = ["bf16", "fp16"]


def sizes_for(C):
    return [MIX[(c + 1) % len(MIX)] if C < len(MIX) else MIX[c % len(MIX)] for c in range(C)]


def run(q16, g16, labels, C, beta, exclude=None):
    """lay the problem out as the product does (NaN padding), launch twice into NaN-filled outputs, compare bitwise"""
    from cclip_hip import ops
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    assert torch.isnan(laid[gather < 0].float()).all()
    ex = None if exclude is None else R.to_laid(exclude, gather).cuda()
    qd, gd = q16.cuda(), laid.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((q16.shape[0], C), float("nan"), device="cuda")
        assert ops.cache_affinity(qd, gd, off, ln, beta, exclude=ex, out=out) is out
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two launches differ"
    return outs[0].cpu()


def against_reference(q16, g16, labels, C, beta, what, exclude=None):
    out = run(q16, g16, labels, C, beta, exclude)
    A, s = R.reference(q16, g16, labels, C, beta, exclude)
    tol = R.tolerance(A, beta, q16, g16, labels, s)
    R.check(out, A, tol, what)
    empty = torch.bincount(labels, minlength=C) == 0
    assert (out[:, empty] == 0).all() and not torch.signbit(out[:, empty]).any(), f"{what}: an empty class is not exactly 0.0"
    return out, A, tol


# (Q, C, D): every Q of {1, 3, 64, 65, 130}, every C of {1, 2, 9, 64, 256}, every D of {32, 96, 512, 768, 1024}; the class
# sizes {0, 1, 15, 16, 17, 63, 65} mixed within each problem
CASES = [(1, 9, 512), (3, 2, 96), (64, 64, 32), (65, 9, 768), (130, 256, 1024), (130, 9, 512), (3, 64, 1024), (65, 1, 96), (1, 256, 768)]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,C,D", CASES)
def test_kernel_against_float64(Q, C, D, dtype):
    q16, g16, labels = R.make_problem(100 * D + 10 * C + Q, Q, sizes_for(C), D, dtype)
    against_reference(q16, g16, labels, C, 5.5, f"Q{Q} C{C} D{D} {dtype}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_several_splits(dtype):
    """about 4100 stored rows at Q = 3: 17 splits of 256 rows, classes that span many of them, an empty one between"""
    from cclip_hip import ops
    sizes = [1000, 0, 2037, 1063]
    q16, g16, labels = R.make_problem(41, 3, sizes, 512, dtype)
    against_reference(q16, g16, labels, 4, 5.5, f"4100 rows {dtype}")
    assert ops.cache_affinity_workspace(3, 4128, 4) == 3 * 17 * 4 * 4


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_one_class_and_small_norms(dtype):
    q16, g16, labels = R.make_problem(42, 65, [300], 512, dtype)
    against_reference(q16, g16, labels, 1, 5.5, f"one class {dtype}")
    q16, g16, labels = R.make_problem(43, 3, sizes_for(9), 64, dtype, normalise=False, scale=0.05)     # |row| about 0.4
    against_reference(q16, g16, labels, 9, 5.5, f"small norms {dtype}")
    q16, g16, labels = R.make_problem(44, 3, sizes_for(9), 64, dtype)
    against_reference(q16, g16, labels, 9, 40.0, f"beta 40 {dtype}")
    against_reference(q16, g16, labels, 9, 0.0, f"beta 0 {dtype}")                                     # A = the live counts


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_exclude(dtype):
    C, beta = 9, 5.5
    sizes = sizes_for(C)
    q16, g16, labels = R.make_problem(45, 6, sizes, 512, dtype)
    single = sizes.index(1)
    only = int((labels == single).nonzero()[0, 0])
    big = int((labels == sizes.index(65)).nonzero()[64, 0])                   # the 65th row of its class: alone in its sub-tile
    exclude = torch.tensor([only, -1, big, int((labels == sizes.index(17)).nonzero()[0, 0]), -1, only])
    base = run(q16, g16, labels, C, beta)
    out, A, tol = against_reference(q16, g16, labels, C, beta, f"exclude {dtype}", exclude=exclude)
    assert out[0, single] == 0 and out[5, single] == 0 and out[1, single] > 0, "a class whose only row is excluded must be exactly 0"
    s = q16.double() @ g16.double().t()
    for i, n in enumerate(exclude.tolist()):
        c = int(labels[n]) if n >= 0 else -1
        for cc in range(C):
            if cc != c:
                assert out[i, cc] == base[i, cc], "exclude touched another class"
        if n >= 0:                                                            # the class changes by exactly that term
            term = torch.exp(beta * (s[i, n] - 1.0)).item()
            A0, s0 = R.reference(q16[i:i + 1], g16, labels, C, beta)
            t0 = R.tolerance(A0, beta, q16[i:i + 1], g16, labels, s0)[0, c].item()
            assert abs((base[i, c].double() - out[i, c].double()).item() - term) <= t0 + tol[i, c].item()
    none = run(q16, g16, labels, C, beta, exclude=torch.full((6,), -1))
    assert torch.equal(none.view(torch.int32), base.view(torch.int32)), "exclude = -1 differs from exclude = None"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("sizes,D", [(MIX + [40, 3], 512), ([24000, 24016], 64), (MIX, 1024)])
def test_row_does_not_depend_on_Q(sizes, D, dtype):
    """rows of a Q = 130 launch against the same queries launched alone.  48016 stored rows is a size at which a split rule
    that looked at Q would cut the rows differently for 130 queries and for one."""
    from cclip_hip import ops
    C = len(sizes)
    q16, g16, labels = R.make_problem(46, 130, sizes, D, dtype)
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    exclude = torch.randint(-1, labels.numel(), (130,), generator=torch.Generator().manual_seed(1))
    ex = R.to_laid(exclude, gather).cuda()
    qd, gd = q16.cuda(), laid.cuda()
    full = ops.cache_affinity(qd, gd, off, ln, 5.5, exclude=ex)
    for i in (0, 15, 63, 64, 100, 129):
        alone = ops.cache_affinity(qd[i:i + 1], gd, off, ln, 5.5, exclude=ex[i:i + 1].contiguous())
        assert torch.equal(alone[0].view(torch.int32), full[i].view(torch.int32)), f"row {i} differs when launched alone"
    some = ops.cache_affinity(qd[60:70], gd, off, ln, 5.5, exclude=ex[60:70].contiguous())
    assert torch.equal(some.view(torch.int32), full[60:70].view(torch.int32))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,D", [(3, 96), (65, 512)])
def test_strided_operands(Q, D, dtype):
    """both operands as column slices of wider buffers (row strides D + 8 and 2 D + 64, 16-byte aligned offsets)"""
    from cclip_hip import ops
    C = 9
    q16, g16, labels = R.make_problem(47 + Q, Q, sizes_for(C), D, dtype)
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    qw = torch.full((Q, D + 8), float("nan"), dtype=dtype); qw[:, 8:] = q16
    gw = torch.full((laid.shape[0], 2 * D + 64), float("nan"), dtype=dtype); gw[:, 16:16 + D] = laid
    a = ops.cache_affinity(qw.cuda()[:, 8:], gw.cuda()[:, 16:16 + D], off, ln, 5.5)
    b = ops.cache_affinity(q16.cuda(), laid.cuda(), off, ln, 5.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "strided and contiguous operands differ"
    A, s = R.reference(q16, g16, labels, C, 5.5)
    R.check(a.cpu(), A, R.tolerance(A, 5.5, q16, g16, labels, s), f"strided Q{Q} D{D} {dtype}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_order_within_a_class(dtype):
    """shuffling the ORIGINAL row order (hence the order inside every class) moves the result only within tol"""
    C = 9
    q16, g16, labels = R.make_problem(48, 65, sizes_for(C), 512, dtype)
    out, A, tol = against_reference(q16, g16, labels, C, 5.5, f"order {dtype}")
    perm = torch.randperm(labels.numel(), generator=torch.Generator().manual_seed(2))
    shuffled = run(q16, g16[perm], labels[perm], C, 5.5)
    R.check(shuffled, A, tol, f"order, shuffled {dtype}")
    assert ((shuffled.double() - out.double()).abs() <= 2 * tol).all()


def test_argument_errors_leave_out_untouched():
    from cclip_hip import ops
    from cclip_hip._lib import lib
    C, D, Q = 9, 64, 4
    q16, g16, labels = R.make_problem(49, Q, sizes_for(C), D, torch.bfloat16)
    laid, gather, off, ln = R.lay_out(g16, labels, C)
    qd, gd = q16.cuda(), laid.cuda()
    Np = laid.shape[0]
    out = torch.full((Q, C), float("nan"), device="cuda")
    I = lambda v: torch.tensor(v, dtype=torch.int32)
    bad_off = off.clone(); bad_off[3] += 8
    swapped = off.clone(); swapped[[3, 4]] = swapped[[4, 3]]
    long_len = ln.clone(); long_len[2] = 17
    calls = [
        (TypeError, lambda: ops.cache_affinity(qd.float(), gd.float(), off, ln, 5.5, out=out)),
        (TypeError, lambda: ops.cache_affinity(qd, gd.half(), off, ln, 5.5, out=out)),
        (TypeError, lambda: ops.cache_affinity(qd.cpu(), gd, off, ln, 5.5, out=out)),
        (TypeError, lambda: ops.cache_affinity(qd, gd, off.cuda(), ln.cuda(), 5.5, out=out)),
        (TypeError, lambda: ops.cache_affinity(qd, gd, off.long(), ln, 5.5, out=out)),
        (TypeError, lambda: ops.cache_affinity(qd, gd, off, ln, 5.5, exclude=torch.zeros(Q, device="cuda", dtype=torch.int64), out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, bad_off, ln, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, swapped, ln, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, off, long_len, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd[:-16], off, ln, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, off[:-1], ln, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd[:, :32], gd, off, ln, 5.5, out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, off, ln, float("nan"), out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, off, ln, 5.5, exclude=torch.zeros(Q + 1, device="cuda", dtype=torch.int32), out=out)),
        (ValueError, lambda: ops.cache_affinity(qd, gd, off, ln, 5.5, out=out[:, :8])),
        (ValueError, lambda: ops.cache_affinity(torch.zeros(Q, 72, device="cuda", dtype=torch.bfloat16)[:, 4:68], gd, off, ln, 5.5, out=out)),
        (NotImplementedError, lambda: ops.cache_affinity(torch.zeros(Q, 40, device="cuda", dtype=torch.bfloat16),
                                                         torch.zeros(Np, 40, device="cuda", dtype=torch.bfloat16), off, ln, 5.5, out=out)),
        (NotImplementedError, lambda: ops.cache_affinity(torch.zeros(Q, 1056, device="cuda", dtype=torch.bfloat16),
                                                         torch.zeros(Np, 1056, device="cuda", dtype=torch.bfloat16), off, ln, 5.5, out=out)),
        (NotImplementedError, lambda: ops.cache_affinity(qd, torch.zeros(16 * 257, D, device="cuda", dtype=torch.bfloat16),
                                                         I([16 * c for c in range(258)]), I([1] * 257), 5.5,
                                                         out=torch.full((Q, 257), float("nan"), device="cuda"))),
    ]
    for kind, call in calls:
        with pytest.raises(kind):
            call()
    # the C entry itself: CCLIP_ERR_ARG (1) before any launch
    L, I32, F = ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    offd, lend = off.cuda(), ln.cuda()
    nbytes = ops.cache_affinity_workspace(Q, Np, C)
    assert nbytes == Q * 1 * C * 4                                            # 240 laid-out rows: one split
    ws = torch.empty(nbytes // 4, device="cuda")

    def call(q=qd, g=gd, ldq=D, ldg=D, Q_=Q, Np_=Np, D_=D, o=offd, l=lend, C_=C, out_=out, w=ws, wb=nbytes, fn=lib.cclip_cache_affinity):
        return fn(P(q), L(ldq), I32(Q_), P(g), L(ldg), L(Np_), I32(D_), P(o), P(l), I32(C_), F(5.5), P(None), P(out_), P(w), L(wb),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    for kw in (dict(q=None), dict(g=None), dict(o=None), dict(l=None), dict(out_=None), dict(w=None), dict(C_=0), dict(C_=257),
               dict(Q_=0), dict(Np_=0), dict(Np_=Np - 8), dict(Np_=2 ** 31), dict(D_=0), dict(D_=40), dict(D_=1056), dict(ldq=D - 8),
               dict(ldg=D + 4), dict(wb=nbytes - 4), dict(fn=lib.cclip_cache_affinity_f16, Np_=Np + 1)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to out"
    for args in ((0, Np, C), (Q, 0, C), (Q, Np + 1, C), (Q, Np, 0), (Q, Np, 257), (Q, 2 ** 31, C)):
        assert ops.cache_affinity_workspace(*args) == 0
    assert call() == 0 and call(fn=lib.cclip_cache_affinity_f16) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()


def test_workspace_is_the_only_scratch():
    """no Q x N buffer: the peak rises by the workspace and the output, far below the Q x Np x 4 bytes of a score matrix; the
    workspace follows Np alone (times Q, C)"""
    from cclip_hip import ops
    Q, C, D = 256, 4, 64
    sizes = [1 << 16] * C
    Np = sum(sizes)
    gen = torch.Generator(device="cuda").manual_seed(4)
    g = torch.randn(Np, D, device="cuda", generator=gen).bfloat16()
    q = torch.randn(Q, D, device="cuda", generator=gen).bfloat16()
    _, off, ln = ops.cache_layout(torch.arange(C).repeat_interleave(1 << 16), C)
    ops.cache_affinity(q[:1], g, off, ln, 0.01)                               # the layout's device copies exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    A = ops.cache_affinity(q, g, off, ln, 0.01)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    ws = ops.cache_affinity_workspace(Q, Np, C)
    print(f"[cache-mem] peak rise {rise} bytes, workspace {ws} bytes, matrix {Q * Np * 4} bytes")
    assert ws == Q * 512 * C * 4 and ws <= Q * min(512, (Np + 255) // 256) * C * 4
    assert rise <= ws + Q * C * 4 + 4096 and rise < Q * Np * 4 // 8
    assert torch.isfinite(A).all() and (A > 0).all()
    for QQ in (1, 64, 1000):
        assert ops.cache_affinity_workspace(QQ, Np, C) == QQ * 512 * C * 4
