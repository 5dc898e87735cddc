"""The two kernels of the hubness correction on the MI355X, through cclip_hip.ops, against float64 on the same 16-bit operands
(tests/hubness_ref.py) and at their exact edges.

ops.bank_lse (csrc/embed_hub.hip): lse[j] = log sum_b exp(beta <bank[b], g[j]>).
  LSE_TOL is 4 x the largest deviation |lse - ref| / max(1, |ref|) measured on an MI355X over the cases of
  test_bank_lse_against_float64 (the factor 4 is the convention of 6.24: it covers other seeds, not other
  shapes).  The second bound is derived, holds the ABSOLUTE error and no constant loosens it: beta D 2^-24 sum_d |bank_d g_d|
  for the score, plus (B + 64) 2^-23 for the exponentials, their sum and the logarithm.
ops.similarity_topk_biased (csrc/embed_topk.hip): the exact top-k of fmaf(scale, s, bias[n]).
Every case prints its figures (`[hubness-kernels] ...`) before it asserts; run with -s to collect them.
"""
import math

import pytest
import torch

import hubness_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]

LSE_TWO_SPLIT_B = 257            # the smallest bank cclip_bank_lse cuts in two for these N (checked below)
# (N, B): every N of {1, 15, 17, 63, 65, 129} and every B of {1, 15, 17, 65, two splits}
LSE_PAIRS = [(1, 1), (15, 17), (17, 15), (63, 65), (65, LSE_TWO_SPLIT_B), (129, LSE_TWO_SPLIT_B), (129, 1), (1, LSE_TWO_SPLIT_B)]
LSE_DIMS = [32, 160, 512, 768, 1024]
LSE_BETA = 20.0
LSE_TOL = 4 * 4.34e-7            # 4 x the worst measured (MI355X, 2026-10-21): 4.339e-07, fp16 at D = 768; bf16 4.182e-07


def bits(t):
    return t.contiguous().view(torch.int32)


def unit16(n, D, dtype, gen):
    x = torch.randn(n, D, generator=gen, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.float32).to(dtype)


def small_ints(n, D, dtype, gen, hi=2):
    return torch.randint(-hi, hi + 1, (n, D), generator=gen).to(torch.float32).to(dtype)


def padded(x, pad):
    """the same rows as a strided view of a wider buffer"""
    buf = torch.zeros(x.shape[0], x.shape[1] + pad, dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def topk_scores_by_row(bank1, g):
    """s[j] = <bank1[0], g[j]> with the bits similarity_topk returns, matched to the gallery rows (64 rows a call: k <= 64)"""
    from cclip_hip import ops
    out = torch.empty(g.shape[0], device=g.device, dtype=torch.float32)
    for lo in range(0, g.shape[0], 64):
        part = g[lo:lo + 64]
        s, i = ops.similarity_topk(bank1, part, part.shape[0])
        out[lo + i[0].long()] = s[0]
    return out


def test_the_two_split_bank_is_the_smallest():
    from cclip_hip import ops
    for N, B in LSE_PAIRS:
        assert ops.bank_lse_splits(N, B) == (2 if B == LSE_TWO_SPLIT_B else 1), (N, B)
        assert ops.bank_lse_splits(N, LSE_TWO_SPLIT_B - 1) == 1
        assert ops.bank_lse_workspace(N, B) == 8 * N * ops.bank_lse_splits(N, B)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", LSE_DIMS)
def test_bank_lse_against_float64(D, dtype):
    from cclip_hip import ops
    worst = 0.0
    for N, B in LSE_PAIRS:
        gen = torch.Generator().manual_seed(100 * D + N + B)
        g16, b16 = unit16(N, D, dtype, gen), unit16(B, D, dtype, gen)
        ref = R.bank_lse(g16.double(), b16.double(), LSE_BETA)
        gd, bd = g16.cuda(), b16.cuda()
        lse = ops.bank_lse(gd, bd, LSE_BETA)
        again = ops.bank_lse(gd, bd, LSE_BETA, workspace=torch.empty(ops.bank_lse_workspace(N, B) // 8 + 3, device="cuda", dtype=torch.int64))
        strided = ops.bank_lse(padded(gd, 8), padded(bd, 24), LSE_BETA)
        torch.cuda.synchronize()
        assert lse.shape == (N,) and lse.dtype == torch.float32 and lse.is_cuda
        assert torch.equal(bits(lse), bits(again)), "two launches differ"
        assert torch.equal(bits(lse), bits(strided)), "strided views differ"
        err = (lse.cpu().double() - ref).abs()                                        # absolute: what the ceiling bounds
        dev = err / ref.abs().clamp_min(1.0)
        # [N]: the largest sum_d |bank_d g_d| over the bank rows - an error of every t by at most e moves the log-sum-exp by at most e
        mag = (b16.double().abs() @ g16.double().abs().T).max(dim=0).values
        ceiling = LSE_BETA * D * 2.0 ** -24 * mag + (B + 64) * 2.0 ** -23
        print(f"[hubness-kernels] bank_lse {str(dtype)[6:]} N={N} B={B} D={D}: dev {dev.max().item():.3e} (tol {LSE_TOL:.1e}), "
              f"abs err {err.max().item():.3e} (ceiling {ceiling.min().item():.3e})")
        worst = max(worst, dev.max().item())
        assert torch.isfinite(lse).all()
        assert (err <= ceiling).all(), f"N={N} B={B}: absolute error above the derived ceiling"
        assert dev.max().item() <= LSE_TOL, f"N={N} B={B}: {dev.max().item():.3e} above 4 x measured"
    print(f"[hubness-kernels] bank_lse {str(dtype)[6:]} D={D}: worst dev {worst:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,D", [(1, 32), (15, 160), (17, 512), (63, 768), (65, 1024), (129, 160)])
def test_bank_lse_of_one_bank_row_is_the_scaled_topk_score(N, D, dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(N + D)
    gd, bd = unit16(N, D, dtype, gen).cuda(), unit16(1, D, dtype, gen).cuda()
    for beta in (LSE_BETA, 0.3):
        lse = ops.bank_lse(gd, bd, beta)
        want = torch.tensor(beta, dtype=torch.float32, device="cuda") * topk_scores_by_row(bd, gd)
        assert torch.equal(bits(lse), bits(want)), f"beta={beta}: not beta * score bit for bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,B,D", [(17, 1, 32), (65, 15, 160), (15, 17, 1024), (129, 65, 512), (63, LSE_TWO_SPLIT_B, 768), (1, 1000, 32)])
def test_bank_lse_exact_edges(N, B, D, dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(3 * N + B + D)
    gd, bd = small_ints(N, D, dtype, gen).cuda(), small_ints(B, D, dtype, gen).cuda()
    # beta = 0: every term is exp(0), the sum is B exactly: log B to one ulp
    lse0 = ops.bank_lse(gd, bd, 0.0).cpu()
    want = torch.tensor(math.log(B), dtype=torch.float64).to(torch.float32)
    ulp = max(abs(float(torch.nextafter(want, torch.tensor(math.inf)) - want)), 2.0 ** -149)
    print(f"[hubness-kernels] bank_lse beta=0 B={B}: off by {(lse0.double() - float(want)).abs().max().item() / ulp:.2f} ulp")
    assert ((lse0.double() - float(want)).abs() <= ulp).all()
    # a large beta stays finite: nothing above exp(0) is formed (scores reach 4 D here)
    big = ops.bank_lse(gd, bd, 100.0)
    ref = R.bank_lse(gd.cpu().double(), bd.cpu().double(), 100.0)
    assert torch.isfinite(big).all()
    assert ((big.cpu().double() - ref).abs() <= (B + 64) * 2.0 ** -23 * ref.abs().clamp_min(1.0)).all()     # t itself is exact here
    # a NaN in one gallery row: that entry, and no other
    base = ops.bank_lse(gd, bd, 0.25)
    for row in sorted({0, N // 2, N - 1}):
        g2 = gd.clone()
        g2[row, D // 2] = float("nan")
        out = ops.bank_lse(g2, bd, 0.25)
        keep = torch.arange(N, device="cuda") != row
        assert torch.isnan(out[row]) and torch.equal(bits(out[keep]), bits(base[keep])), f"NaN in row {row}"
    # a NaN bank row reaches every entry (documented)
    b2 = bd.clone()
    b2[B - 1, 0] = float("nan")
    assert torch.isnan(ops.bank_lse(gd, b2, 0.25)).all()


def test_bank_lse_refuses():
    from cclip_hip import ops
    g = torch.zeros(4, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.bank_lse(g, g[:, :32], 1.0)
    with pytest.raises(ValueError):
        ops.bank_lse(g, g, float("nan"))
    with pytest.raises(TypeError):
        ops.bank_lse(g, g.to(torch.float16), 1.0)
    with pytest.raises(NotImplementedError):
        ops.bank_lse(torch.zeros(4, 48, device="cuda", dtype=torch.bfloat16), torch.zeros(4, 48, device="cuda", dtype=torch.bfloat16), 1.0)
    with pytest.raises(ValueError):
        ops.bank_lse(g, g, 1.0, workspace=torch.empty(1, device="cuda", dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.bank_lse(g.cpu(), g, 1.0)


# ---- similarity_topk_biased ------------------------------------------------------------------------------------------------
def test_topk_two_split_gallery():
    from cclip_hip import ops
    for Q in (1, 17, 65):
        assert ops.similarity_topk_workspace(Q, R.TOPK_TWO_SPLIT_N, 1) == 2 * Q * 8
        assert ops.similarity_topk_workspace(Q, R.TOPK_TWO_SPLIT_N - 1, 1) == Q * 8


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,N,k,D", R.TOPK_CASES)
def test_topk_biased_random_rows(Q, N, k, D, dtype):
    from cclip_hip import ops
    q16, g16, bias = R.topk_case(Q, N, k, D, dtype)
    qd, gd, bd = q16.cuda(), g16.cuda(), bias.cuda()
    # scale = 1, bias = 0: the unbiased entry, bit for bit
    s0, i0 = ops.similarity_topk(qd, gd, k)
    s1, i1 = ops.similarity_topk_biased(qd, gd, k, torch.zeros(N, device="cuda"), 1.0)
    assert torch.equal(i0, i1) and torch.equal(bits(s0), bits(s1)), "scale 1, bias 0 differs from similarity_topk"
    s, i = ops.similarity_topk_biased(qd, gd, k, bd, R.TOPK_SCALE)
    s2, i2 = ops.similarity_topk_biased(padded(qd, 8), padded(gd, 24), k, bd, R.TOPK_SCALE)
    assert torch.equal(i, i2) and torch.equal(bits(s), bits(s2)), "launches / strided views differ"
    assert s.shape == (Q, k) and s.dtype == torch.float32 and i.dtype == torch.int32
    ref_s, ref_i, t = R.topk_biased(q16.double(), g16.double(), k, bias, R.TOPK_SCALE)
    tol = R.topk_tol(q16, g16, bias, R.TOPK_SCALE)
    close = R.kth_gap(t, k) < 2 * tol
    assert int(close.sum()) == 0, "the reference alone must leave no query out on these seeds"
    assert close.double().mean().item() <= 0.01
    got_i, got_s = i.cpu().long(), s.cpu().double()
    err = (got_s - torch.gather(t, 1, got_i)).abs().max().item()
    print(f"[hubness-kernels] topk_biased {str(dtype)[6:]} Q={Q} N={N} k={k} D={D}: score err {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    assert (got_s[:, 1:] <= got_s[:, :-1]).all(), "not descending"
    keep = ~close
    assert torch.equal(got_i[keep].sort(dim=1).values, ref_i[keep].sort(dim=1).values), "index sets differ from float64"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Q,N,k,D", [(1, 7, 7, 32), (17, 63, 64, 160), (65, 65, 7, 1024), (17, R.TOPK_TWO_SPLIT_N, 64, 32), (65, 300, 1, 160)])
def test_topk_biased_exact_on_small_integers(Q, N, k, D, dtype):
    """integer rows, a dyadic bias and scale: t is exact in fp32, so scores AND indices (ties by the lower index) equal float64"""
    from cclip_hip import ops
    k = min(k, N)
    gen = torch.Generator().manual_seed(Q + N + k + D)
    q16, g16 = small_ints(Q, D, dtype, gen), small_ints(N, D, dtype, gen)
    g16[N // 2] = g16[0]                                                                   # duplicate rows ...
    bias = torch.randint(-8, 9, (N,), generator=gen).to(torch.float32) * 0.25
    bias[N // 2] = bias[0]                                                                 # ... with equal bias
    s, i = ops.similarity_topk_biased(q16.cuda(), g16.cuda(), k, bias.cuda(), 0.5)
    ref_s, ref_i, _ = R.topk_biased(q16.double(), g16.double(), k, bias, 0.5)
    assert torch.equal(i.cpu().long(), ref_i) and torch.equal(s.cpu().double(), ref_s)
    both = (i.cpu() == 0) | (i.cpu() == N // 2)
    rows = both.sum(dim=1) == 2
    if N > 1 and rows.any():
        pos0 = (i.cpu() == 0).float().argmax(dim=1)
        posd = (i.cpu() == N // 2).float().argmax(dim=1)
        assert (pos0[rows] < posd[rows]).all(), "equal t: the lower index comes first"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_topk_biased_excluded_rows_and_nan(dtype):
    from cclip_hip import ops
    inf, nan = math.inf, math.nan
    gen = torch.Generator().manual_seed(11)
    for N, D in ((10, 32), (70, 160), (R.TOPK_TWO_SPLIT_N + 41, 64)):
        q16, g16 = small_ints(5, D, dtype, gen), small_ints(N, D, dtype, gen)
        bias = torch.zeros(N)
        gone = torch.arange(N) % 3 == 1                                                    # a third of the rows excluded
        gone[N - 1] = True
        bias[gone] = -inf
        bias[N - 2] = nan
        live = int((~gone).sum()) - 1                                                      # rows with a finite t
        for k in sorted({1, min(7, live), min(live, 64), min(N, 64)}):
            s, i = ops.similarity_topk_biased(q16.cuda(), g16.cuda(), k, bias.cuda(), 1.0)
            ref_s, ref_i, _ = R.topk_biased(q16.double(), g16.double(), k, bias, 1.0)
            got_i, got_s = i.cpu().long(), s.cpu().double()
            assert torch.equal(got_i, ref_i), (N, k)
            assert torch.equal(torch.nan_to_num(got_s, nan=12345.0), torch.nan_to_num(ref_s, nan=12345.0)), (N, k)
            if k <= live:
                assert not gone[got_i].any() and not (got_i == N - 2).any(), "an excluded row before the live ones ran out"
        if N <= 64:                                                                        # all rows: live, then -inf ascending, NaN last
            tail = got_i[:, live:]
            want = torch.cat([gone.nonzero().flatten(), torch.tensor([N - 2])])
            assert torch.equal(tail, want[None, :].expand(5, -1))


def test_topk_biased_refuses():
    from cclip_hip import ops
    q = torch.zeros(2, 32, device="cuda", dtype=torch.bfloat16)
    g = torch.zeros(9, 32, device="cuda", dtype=torch.bfloat16)
    bias = torch.zeros(9, device="cuda")
    for k in (0, 65, 10):
        with pytest.raises(ValueError):
            ops.similarity_topk_biased(q, g, k, bias)
    with pytest.raises(ValueError):
        ops.similarity_topk_biased(q, g, 2, bias[:8])
    with pytest.raises(TypeError):
        ops.similarity_topk_biased(q, g, 2, bias.double())
    with pytest.raises(TypeError):
        ops.similarity_topk_biased(q, g, 2, bias.cpu())
    with pytest.raises(TypeError):
        ops.similarity_topk_biased(q, g.to(torch.float16), 2, bias)
