"""The assignment step of k-means on the MI355X (cclip_kmeans_assign, csrc/embed_kmeans.hip) against float64 on the same 16-bit
operands (tests/kmeans_ref.py), against similarity_topk bit for bit, and at its edges: position independence, ties, NaN,
strided views, argument errors, the absence of an N x K buffer.

tol = D 2^-22 max|x| max|c| is the derived bound of test_retrieval_gpu.py (kmeans_ref.assign_tol), not a measured one.
Every case prints its figures (`[kmeans-assign] ...`) before it asserts; run with -s to collect them.
"""
import functools

import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]

# (N, K, D): one row, partial 16-row tiles, a row just past a block (65, 257), K just past a tile (17, 65, 257), chunk counts that
# are no power of two (96, 160, 768), the widest D, many row blocks
CASES = [(1, 1, 32), (5, 3, 128), (65, 2, 64), (100, 17, 768), (257, 65, 512), (1000, 257, 96), (4097, 1000, 160), (300, 4096, 1024),
         (100003, 16, 64)]


@functools.lru_cache(maxsize=None)
def case_inputs(N, K, D, dtype):
    """the operands of a case and their float64 scores, computed once and shared; never written to"""
    gen = torch.Generator().manual_seed(1000 * D + N + K)
    x16 = torch.randn(N, D, generator=gen).to(dtype)
    c16 = torch.randn(K, D, generator=gen).to(dtype)
    return x16, c16, R.scores64(x16, c16)


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,K,D", CASES)
def test_kernel_against_float64_and_topk(N, K, D, dtype):
    from cclip_hip import ops
    x16, c16, ref = case_inputs(N, K, D, dtype)
    tol = R.assign_tol(D, x16, c16)
    xd, cd = x16.cuda(), c16.cuda()
    a1, b1, s1 = ops.kmeans_assign(xd, cd, want_second=True)
    a2, b2, s2 = ops.kmeans_assign(xd, cd, want_second=True)
    a3, b3, none = ops.kmeans_assign(xd, cd)
    torch.cuda.synchronize()
    assert none is None and a1.dtype == torch.int32 and b1.dtype == torch.float32 and s1.dtype == torch.float32
    assert a1.shape == b1.shape == s1.shape == (N,) and a1.is_cuda
    assert torch.equal(a1, a2) and torch.equal(bits(b1), bits(b2)) and torch.equal(bits(s1), bits(s2)), "two launches differ"
    assert torch.equal(a1, a3) and torch.equal(bits(b1), bits(b3)), "the call without `second` differs"
    a, b, s = a1.cpu().long(), b1.cpu().double(), s1.cpu().double()
    assert (a >= 0).all() and (a < K).all()
    own = ref[torch.arange(N), a]
    err_best = (b - own).abs().max().item()
    short = (ref.max(dim=1).values - own).max().item()
    if K > 1:
        err_second = (s[:, None] - ref).abs().min(dim=1).values.max().item()
        assert (s1 <= b1).all(), "second above best"                                                                      # 3
    else:
        err_second = 0.0
        assert torch.isnan(s).all(), "K == 1: second must be NaN"
    print(f"[kmeans-assign] N{N} K{K} D{D} {dtype}: best err {err_best:.3e} second err {err_second:.3e} shortfall {short:.3e} tol {tol:.3e}")
    assert err_best <= tol, f"best off its own pair by {err_best:.3e} > {tol:.3e}"                                        # 1
    assert short <= 2 * tol, f"the named centroid falls {short:.3e} short of the row's maximum (2 tol = {2 * tol:.3e})"   # 2
    assert err_second <= tol, f"second is {err_second:.3e} from every float64 score of its row"                          # 3
    ts, ti = ops.similarity_topk(xd, cd, min(2, K))                                                                       # 4
    assert torch.equal(ti[:, 0], a1) and torch.equal(bits(ts[:, 0].contiguous()), bits(b1)), "differs from similarity_topk's first"
    if K > 1:
        assert torch.equal(bits(ts[:, 1].contiguous()), bits(s1)), "second differs from similarity_topk's second"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,K,D", [(257, 65, 512), (4097, 1000, 160), (300, 4096, 1024), (1000, 257, 96), (100, 17, 768)])
def test_row_outputs_do_not_depend_on_the_batch(N, K, D, dtype):
    """rule 5: alone (the one-tile variant), in a slice that starts elsewhere, and in the full batch (the two-tile variant)"""
    from cclip_hip import ops
    x16, c16, _ = case_inputs(N, K, D, dtype)
    xd, cd = x16.cuda(), c16.cuda()
    a, b, s = ops.kmeans_assign(xd, cd, want_second=True)
    for row in (0, 63, 64, N // 2, N - 1):
        a1, b1, s1 = ops.kmeans_assign(xd[row:row + 1], cd, want_second=True)
        assert a1.item() == a[row].item() and torch.equal(bits(b1), bits(b[row:row + 1])) and torch.equal(bits(s1), bits(s[row:row + 1])), \
            f"row {row} alone differs"
    for lo, hi in ((8, 72), (N // 3 // 8 * 8, N), (0, 50)):
        a2, b2, s2 = ops.kmeans_assign(xd[lo:hi], cd, want_second=True)
        assert torch.equal(a2, a[lo:hi]) and torch.equal(bits(b2), bits(b[lo:hi])) and torch.equal(bits(s2), bits(s[lo:hi])), \
            f"slice {lo}:{hi} differs"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_planted_ties_go_to_the_lower_index(dtype):
    from cclip_hip import ops
    N, K, D = 200, 150, 64
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, D, generator=gen)
    x[:, 0] = x[:, 0].abs() + 1.0
    x16 = x.to(dtype)
    c16 = (0.01 * torch.randn(K, D, generator=gen)).to(dtype)
    win = torch.zeros(D)
    win[0] = 4.0                                                               # scores >= 4 against |others| << 1
    for k in (130, 7, 66, 149):                                               # identical copies across sub-tiles, tiles and lanes
        c16[k] = win.to(dtype)
    ref = R.scores64(x16, c16)
    assert (ref.argmax(dim=1) == 7).all() and (ref[:, 7] == ref[:, 149]).all()
    a, b, s = ops.kmeans_assign(x16.cuda(), c16.cuda(), want_second=True)
    a, b, s = a.cpu(), b.cpu(), s.cpu()
    print(f"[kmeans-assign] ties {dtype}: chosen {sorted(set(a.tolist()))}")
    assert (a == 7).all(), "a tie did not go to the lowest copy"
    assert torch.equal(bits(b), bits(s)), "the runner-up of a tie carries the same score"
    same = torch.zeros(3, D).to(dtype).cuda()                                  # every score +0 / -0: centroid 0
    a0, b0, s0 = ops.kmeans_assign(x16.cuda(), same, want_second=True)
    assert (a0 == 0).all() and (b0 == 0).all() and (s0 == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_nan_centroid_is_never_chosen_while_a_number_exists(dtype):
    from cclip_hip import ops
    N, K, D = 130, 70, 64
    gen = torch.Generator().manual_seed(12)
    x16 = torch.randn(N, D, generator=gen).to(dtype)
    c16 = torch.randn(K, D, generator=gen).to(dtype)
    c16[0, 3] = float("nan")
    c16[33] = float("nan")
    c16[69, 63] = float("nan")
    clean = torch.tensor([k for k in range(K) if k not in (0, 33, 69)])
    a, b, s = ops.kmeans_assign(x16.cuda(), c16.cuda(), want_second=True)
    ra, rb, rs = R.assign_ref(x16, c16[clean])
    a, b, s = a.cpu().long(), b.cpu(), s.cpu()
    assert not torch.isnan(b).any() and not torch.isnan(s).any()
    tol = R.assign_tol(D, x16, c16[clean])
    decided = (rb - rs) > 2 * tol
    assert decided.sum() > N // 2
    assert torch.equal(a[decided], clean[ra][decided]) and (b.double() - rb)[decided].abs().max().item() <= tol
    # one finite centroid among NaN ones: chosen, and the runner-up is a NaN
    only = c16.clone()
    only[:] = float("nan")
    only[41] = c16[41]
    a, b, s = ops.kmeans_assign(x16.cuda(), only.cuda(), want_second=True)
    assert (a == 41).all() and not torch.isnan(b).any() and torch.isnan(s).all()
    only[41] = float("nan")                                                    # nothing but NaN: centroid 0, NaN scores
    a, b, s = ops.kmeans_assign(x16.cuda(), only.cuda(), want_second=True)
    assert (a == 0).all() and torch.isnan(b).all() and torch.isnan(s).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_strided_views(dtype):
    """both operands as column slices of wider buffers (row strides D + 8 and 2 D + 64, 16-byte aligned offsets)"""
    from cclip_hip import ops
    N, K, D = 300, 130, 128
    gen = torch.Generator().manual_seed(13)
    xw = torch.randn(N, D + 8, generator=gen).to(dtype).cuda()
    cw = torch.randn(K, 2 * D + 64, generator=gen).to(dtype).cuda()
    xv, cv = xw[:, 8:], cw[:, 16:16 + D]
    assert xv.stride(0) > D and cv.stride(0) > D
    a, b, s = ops.kmeans_assign(xv, cv, want_second=True)
    a2, b2, s2 = ops.kmeans_assign(xv.contiguous(), cv.contiguous(), want_second=True)
    assert torch.equal(a, a2) and torch.equal(bits(b), bits(b2)) and torch.equal(bits(s), bits(s2))
    ra, rb, _ = R.assign_ref(xv.cpu(), cv.cpu())
    assert (b.cpu().double() - rb).abs().max().item() <= R.assign_tol(D, xv.cpu(), cv.cpu())
    outs = (torch.empty(N, device="cuda", dtype=torch.int32), torch.empty(N, device="cuda"), torch.empty(N, device="cuda"))
    got = ops.kmeans_assign(xv, cv, out_assign=outs[0], out_best=outs[1], out_second=outs[2])
    assert all(g is o for g, o in zip(got, outs)) and torch.equal(outs[0], a) and torch.equal(bits(outs[2]), bits(s))


def test_argument_errors():
    from cclip_hip import ops
    x = torch.randn(100, 64, device="cuda").bfloat16()
    c = torch.randn(4, 64, device="cuda").bfloat16()
    with pytest.raises(NotImplementedError, match="D % 32 == 0"):
        ops.kmeans_assign(torch.randn(4, 40, device="cuda").bfloat16(), torch.randn(3, 40, device="cuda").bfloat16())
    with pytest.raises(NotImplementedError, match="D <= 1024"):
        ops.kmeans_assign(torch.randn(4, 1056, device="cuda").bfloat16(), torch.randn(3, 1056, device="cuda").bfloat16())
    with pytest.raises(ValueError, match="columns"):
        ops.kmeans_assign(x, torch.randn(4, 96, device="cuda").bfloat16())
    with pytest.raises(ValueError, match="empty"):
        ops.kmeans_assign(x, c[:0])
    with pytest.raises(ValueError, match="empty"):
        ops.kmeans_assign(x[:0], c)
    with pytest.raises(ValueError, match="2-D"):
        ops.kmeans_assign(x[0], c)
    wide = torch.randn(100, 72, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.kmeans_assign(wide[:, 4:68], c)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.kmeans_assign(x, torch.randn(4, 68, device="cuda").bfloat16()[:, :64])
    with pytest.raises(TypeError, match="cuda"):
        ops.kmeans_assign(x.cpu(), c)
    with pytest.raises(TypeError, match="cuda"):
        ops.kmeans_assign(x, c.cpu())
    with pytest.raises(TypeError, match="mixed"):
        ops.kmeans_assign(x, c.half())
    with pytest.raises(TypeError):
        ops.kmeans_assign(x.float(), c.float())
    with pytest.raises(ValueError, match="out_assign"):
        ops.kmeans_assign(x, c, out_assign=torch.empty(100, device="cuda", dtype=torch.int64))
    with pytest.raises(ValueError, match="out_best"):
        ops.kmeans_assign(x, c, out_best=torch.empty(99, device="cuda"))
    with pytest.raises(ValueError, match="out_second"):
        ops.kmeans_assign(x, c, out_second=torch.empty(100, dtype=torch.float32))
    torch.cuda.synchronize()


def test_c_entry_refuses_bad_arguments():
    """the same limits at the C ABI: CCLIP_ERR_ARG (1), nothing launched"""
    import ctypes
    from cclip_hip import load_library
    lib = load_library()
    P, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    N, K = 100, 4
    x = torch.randn(N, 64, device="cuda").bfloat16()
    c = torch.randn(K, 72, device="cuda").bfloat16()
    a = torch.empty(N + 1, device="cuda", dtype=torch.int32)
    b = torch.empty(N + 1, device="cuda")
    s = torch.empty(N + 1, device="cuda")

    def call(xp=x.data_ptr(), ldx=64, N_=N, cp=c.data_ptr(), ldc=72, K_=K, D=64, ap=a.data_ptr(), bp=b.data_ptr(), sp=s.data_ptr(),
             fn=lib.cclip_kmeans_assign):
        return fn(P(xp), L(ldx), L(N_), P(cp), L(ldc), L(K_), I(D), P(ap), P(bp), P(sp), P(0))

    assert call() == 0 and call(sp=0) == 0 and call(fn=lib.cclip_kmeans_assign_f16) == 0
    for bad in (dict(D=40), dict(D=1056), dict(D=0), dict(N_=0), dict(N_=2 ** 31), dict(K_=0), dict(K_=2 ** 31), dict(ldc=68), dict(ldx=60),
                dict(ldc=56), dict(cp=c.data_ptr() + 8), dict(xp=x.data_ptr() + 2), dict(xp=0), dict(cp=0), dict(ap=0), dict(bp=0),
                dict(ap=a.data_ptr() + 2), dict(bp=b.data_ptr() + 2), dict(sp=s.data_ptr() + 2)):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize()


def test_assign_allocates_no_score_matrix():
    from cclip_hip import ops
    N, K, D = 20000, 1024, 512
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(N, D, device="cuda", generator=gen).bfloat16()
    c = torch.randn(K, D, device="cuda", generator=gen).bfloat16()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    a, b, s = ops.kmeans_assign(x, c, want_second=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[kmeans-assign-mem] peak rise {rise} bytes, 16-bit matrix {N * K * 2} bytes")
    assert rise < N * K * 2 // 4, f"kmeans_assign raised the peak by {rise} bytes"                                        # 10
    assert (a >= 0).all() and (a < K).all()
