"""Near-duplicate detection on the MI355X: the fixed-radius kernel (csrc/embed_range.hip) against float64 on the same 16-bit
operands, its CSR order, its self-join mode, NaN / inf, argument errors; clip.EmbeddingIndex.range_search / duplicate_pairs /
duplicate_groups on planted duplicates; clip.group_split; scripts/find_duplicates.py and train_caption.py --dedup-threshold;
the absence of an N x N buffer.

Kernel tolerance: products of two 16-bit operands are exact in fp32, so only the D - 1 additions round; sequentially that is
D 2^-24 |q| |g|, and tol = D 2^-22 max|q| max|g| leaves a factor 4 for the MFMA's internal summation order (the bound
test_retrieval_gpu.py's kernel_tol uses; derived, not measured).

A hit is decided on the kernel's own fp32 score, so a pair whose float64 score lies within tol of the threshold may go either
way: every pair with ref >= thr + tol must come back, none with ref < thr - tol may.  That band is a condition on the inputs,
asserted on the reference alone before the kernel runs: it holds at most max(2, 10 %) of the decided hits.

Every kernel case prints its figures (`[range] ... hits .. band .. err .. tol ..`) before it asserts; run with -s to collect them.
Largest measured on the MI355X: err / tol = 2.5e-3 (fp16, D = 64); the band held at most 6 % of the decided hits (D = 1024).
The tolerance stands at the derived bound and has not been tightened.
"""
import functools
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = [torch.bfloat16, torch.float16]
INF = float("inf")


def kernel_tol(D, q16, g16):
    return D * 2.0 ** -22 * q16.double().norm(dim=1).max().item() * g16.double().norm(dim=1).max().item()


def f32(x):
    """the threshold as the kernel sees it"""
    return torch.tensor(x, dtype=torch.float32).item()


@functools.lru_cache(maxsize=None)
def case_inputs(Q, N, D, dtype):
    """the operands of a kernel case and their float64 product, computed once and shared; never written to"""
    gen = torch.Generator().manual_seed(1000 * D + Q + N)
    q16 = torch.randn(Q, D, generator=gen).to(dtype)
    g16 = torch.randn(N, D, generator=gen).to(dtype)
    return q16, g16, q16.double() @ g16.double().t()


def band_condition(ref, thr, tol, what, pair_ok=None):
    """rule 5, on the reference alone: (must, must_not) masks of the decided pairs"""
    ok = torch.ones_like(ref, dtype=torch.bool) if pair_ok is None else pair_ok
    must = (ref >= thr + tol) & ok
    must_not = (ref < thr - tol) | ~ok | torch.isnan(ref)
    band = int((~must & ~must_not).sum())
    decided = int(must.sum())
    print(f"[range] {what} decided hits {decided} band {band} tol {tol:.3e}")
    assert band <= max(2, 0.10 * decided), f"{what}: {band} pairs within tol of the threshold against {decided} decided hits"
    return must, must_not


def check_range(offsets, index, scores, ref, thr, tol, must, must_not, what):
    """rules 1-4 of the float64 comparison; returns (rows, index, scores) on the host"""
    offsets, index, scores = offsets.cpu(), index.cpu().long(), scores.cpu()
    Q, N = ref.shape
    H = index.numel()
    assert offsets.dtype == torch.int64 and offsets.shape == (Q + 1,) and scores.dtype == torch.float32
    assert scores.shape == (H,) and index.shape == (H,)
    assert offsets[0].item() == 0 and offsets[-1].item() == H and (offsets.diff() >= 0).all(), f"{what}: offsets"          # 3
    rows = torch.repeat_interleave(torch.arange(Q), offsets.diff())
    assert (index >= 0).all() and (index < N).all(), f"{what}: index out of range"                                         # 2
    same_row = rows[1:] == rows[:-1]
    assert (index.diff()[same_row] > 0).all(), f"{what}: indices of a row not strictly ascending"                          # 2
    assert not torch.isnan(scores).any(), f"{what}: NaN returned"
    assert (scores >= torch.tensor(thr, dtype=torch.float32)).all(), f"{what}: a returned score is below the threshold"    # 1
    own = ref[rows, index]
    finite = torch.isfinite(own)
    err = (scores.double() - own)[finite].abs().max().item() if finite.any() else 0.0
    print(f"[range] {what} hits {H} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: score off its own pair by {err:.3e} > {tol:.3e}"                                           # 1
    assert torch.equal(scores.double()[~finite], own[~finite]), f"{what}: infinite scores differ"
    got = torch.zeros(Q, N, dtype=torch.bool)
    got[rows, index] = True
    assert got[must].all(), f"{what}: {int((must & ~got).sum())} pairs above thr + tol are missing"                         # 4
    assert not got[must_not].any(), f"{what}: {int((must_not & got).sum())} pairs below thr - tol were returned"            # 4
    return rows, index, scores


def check_topk_bits(qd, gd, rows, index, scores, offsets, what):
    """rule 7: the hits of up to 16 query rows with 1 .. 64 hits carry the score bits similarity_topk returns for them"""
    from cclip_hip import ops
    hits = offsets.cpu().diff()
    cand = torch.nonzero((hits >= 1) & (hits <= 64)).flatten()
    if cand.numel() == 0:
        return 0
    pick = cand[torch.linspace(0, cand.numel() - 1, min(16, cand.numel())).long().unique()]
    k = int(hits[pick].max())
    ts, ti = ops.similarity_topk(qd, gd, k)
    ts, ti = ts.cpu(), ti.cpu().long()
    for row in pick.tolist():
        h = int(hits[row])
        lo = int(offsets[row])
        order = ti[row, :h].argsort()
        assert torch.equal(ti[row, :h][order], index[lo:lo + h]), f"{what}: row {row}: top-{h} rows differ from the range hits"
        assert torch.equal(ts[row, :h][order].view(torch.int32), scores[lo:lo + h].view(torch.int32)), \
            f"{what}: row {row}: score bits differ from similarity_topk's"
    return pick.numel()


# (Q, N, D): one row, partial 16-row tiles, Q just past one block (65), N just past a tile and a split (257, 4097),
# chunk counts that are no power of two (96, 160, 768), the widest D, many splits
CASES = [(1, 1, 32), (3, 5, 128), (16, 64, 512), (65, 257, 64), (100, 1000, 768), (1024, 1000, 96), (100, 4097, 160),
         (1024, 4097, 128), (16, 20000, 1024), (3, 100003, 64)]
THRESHOLDS = [(Q, N, D, "top") for Q, N, D in CASES] + [(1, 1, 32, "all"), (3, 5, 128, "all")]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q,N,D,which", THRESHOLDS)
def test_kernel_against_float64(Q, N, D, which, dtype):
    from cclip_hip import ops
    q16, g16, ref = case_inputs(Q, N, D, dtype)
    thr = f32(2.9 * math.sqrt(D)) if which == "top" else -INF
    tol = kernel_tol(D, q16, g16)
    what = f"Q{Q} N{N} D{D} {which} {dtype}"
    must, must_not = band_condition(ref, thr, tol, what)
    qd, gd = q16.cuda(), g16.cuda()
    o1, i1, s1 = ops.similarity_range(qd, gd, thr)
    o2, i2, s2 = ops.similarity_range(qd, gd, thr)
    torch.cuda.synchronize()
    assert i1.dtype == torch.int32 and i1.is_cuda and s1.is_cuda and o1.is_cuda
    assert torch.equal(o1, o2) and torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32)), \
        "two launches differ"                                                                                              # 6
    rows, index, scores = check_range(o1, i1, s1, ref, thr, tol, must, must_not, what)
    if which == "all":
        assert index.numel() == Q * N, "threshold -inf must return every pair"
    n = check_topk_bits(qd, gd, rows, index, scores, o1, what)
    print(f"[range] {what} top-k bit comparison on {n} rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,D", [(257, 64), (1000, 768), (4097, 128)])
def test_self_join_equals_filtered_plain_call(N, D, dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(1000 * D + 2 * N)
    x16 = torch.randn(N, D, generator=gen).to(dtype)
    ref = x16.double() @ x16.double().t()
    thr = f32(2.9 * math.sqrt(D))
    tol = kernel_tol(D, x16, x16)
    upper = torch.arange(N)[None, :] > torch.arange(N)[:, None]
    must, must_not = band_condition(ref, thr, tol, f"self-join N{N} D{D} {dtype}", pair_ok=upper)
    xd = x16.cuda()
    po, pi, ps = ops.similarity_range(xd, xd, thr)
    so, si, ss = ops.similarity_range(xd, xd, thr, self_join=True)
    so2, si2, ss2 = ops.similarity_range(xd, xd, thr, self_join=True)
    assert torch.equal(so, so2) and torch.equal(si, si2) and torch.equal(ss.view(torch.int32), ss2.view(torch.int32))
    check_range(so, si, ss, ref, thr, tol, must, must_not, f"self-join N{N} D{D} {dtype}")
    po, pi, ps = po.cpu(), pi.cpu(), ps.cpu()
    rows = torch.repeat_interleave(torch.arange(N), po.diff())
    keep = pi.long() > rows
    want_off = torch.zeros(N + 1, dtype=torch.int64)
    want_off[1:] = torch.bincount(rows[keep], minlength=N).cumsum(0)
    assert torch.equal(so.cpu(), want_off)
    assert torch.equal(si.cpu(), pi[keep]) and torch.equal(ss.cpu().view(torch.int32), ps[keep].view(torch.int32))
    assert (pi.long() == rows).sum().item() == N, "the plain call returns every row's pair with itself"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_self_join_of_identical_rows_returns_every_pair(dtype):
    from cclip_hip import ops
    N, D = 130, 64
    x16 = torch.randn(1, D, generator=torch.Generator().manual_seed(3)).to(dtype).repeat(N, 1).cuda()
    o, i, s = ops.similarity_range(x16, x16, 0.0, self_join=True)
    assert i.numel() == N * (N - 1) // 2
    assert o.cpu().diff().tolist() == [N - 1 - r for r in range(N)]
    assert i.cpu().tolist() == [n for r in range(N) for n in range(r + 1, N)]
    assert (s == s[0]).all() and s[0].item() > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_kernel_strided_rows(dtype):
    """both operands as column slices of wider buffers (row strides D + 8 and 2 D + 64, 16-byte aligned offsets)"""
    from cclip_hip import ops
    Q, N, D = 100, 4097, 128
    gen = torch.Generator().manual_seed(7 + Q)
    qw = torch.randn(Q, D + 8, generator=gen).to(dtype)
    gw = torch.randn(N, 2 * D + 64, generator=gen).to(dtype)
    q16, g16 = qw[:, 8:], gw[:, 16:16 + D]
    ref = q16.double() @ g16.double().t()
    thr, tol = f32(2.9 * math.sqrt(D)), kernel_tol(D, q16, g16)
    must, must_not = band_condition(ref, thr, tol, f"strided {dtype}")
    qd, gd = qw.cuda()[:, 8:], gw.cuda()[:, 16:16 + D]
    o, i, s = ops.similarity_range(qd, gd, thr)
    check_range(o, i, s, ref, thr, tol, must, must_not, f"strided {dtype}")
    o2, i2, s2 = ops.similarity_range(qd.contiguous(), gd.contiguous(), thr)
    assert torch.equal(o, o2) and torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32)), \
        "strided and contiguous operands differ"
    # self-join on a strided view
    o3, i3, s3 = ops.similarity_range(gd, gd, thr, self_join=True)
    gc = gd.contiguous()
    o4, i4, s4 = ops.similarity_range(gc, gc, thr, self_join=True)
    assert torch.equal(o3, o4) and torch.equal(i3, i4) and torch.equal(s3.view(torch.int32), s4.view(torch.int32))


def test_nan_and_infinite_scores():
    from cclip_hip import ops
    g16 = torch.zeros(200, 64, dtype=torch.float16)
    g16[:, 0] = torch.arange(200).half()
    g16[17, 0] = float("nan")
    g16[150, 0] = INF
    g16[151, 0] = -INF
    q16 = torch.zeros(1, 64, dtype=torch.float16)
    q16[0, 0] = 1.0
    qd, gd = q16.cuda(), g16.cuda()
    o, i, s = ops.similarity_range(qd, gd, 100.0)
    assert i.tolist() == [n for n in range(100, 200) if n != 151] and o.tolist() == [0, 99]
    assert s.tolist() == [INF if n == 150 else float(n) for n in range(100, 200) if n != 151]
    o, i, s = ops.similarity_range(qd, gd, -INF)                               # everything but the NaN row
    assert i.tolist() == [n for n in range(200) if n != 17] and not torch.isnan(s).any()
    assert s[150].item() == -INF                                               # row 151: -inf >= -inf
    o, i, s = ops.similarity_range(qd, gd, INF)                                # only +inf scores
    assert i.tolist() == [150] and s.tolist() == [INF] and o.tolist() == [0, 1]
    o, i, s = ops.similarity_range(qd, gd[:40], 0.0)
    assert i.tolist() == [n for n in range(40) if n != 17]


@pytest.mark.parametrize("self_join", [False, True])
def test_zero_hits(self_join):
    from cclip_hip import ops
    x = torch.randn(300, 64, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
    o, i, s = ops.similarity_range(x, x, 1e30, self_join=self_join)
    assert o.dtype == torch.int64 and o.shape == (301,) and not o.any()
    assert i.dtype == torch.int32 and i.shape == (0,) and s.dtype == torch.float32 and s.shape == (0,)
    assert i.is_cuda and s.is_cuda and o.is_cuda


# ------------------------------------------------------------------------------------------------------------------------
# argument errors: raised by the binding / refused by the C entries, nothing launched
# ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from cclip_hip import ops
    q = torch.randn(4, 64, device="cuda").bfloat16()
    g = torch.randn(100, 64, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="NaN"):
        ops.similarity_range(q, g, float("nan"))
    with pytest.raises(NotImplementedError, match="D % 32 == 0"):
        ops.similarity_range(torch.randn(4, 40, device="cuda").bfloat16(), torch.randn(100, 40, device="cuda").bfloat16(), 0.5)
    with pytest.raises(NotImplementedError, match="D <= 1024"):
        ops.similarity_range(torch.randn(4, 1056, device="cuda").bfloat16(), torch.randn(10, 1056, device="cuda").bfloat16(), 0.5)
    with pytest.raises(ValueError, match="columns"):
        ops.similarity_range(q, torch.randn(100, 96, device="cuda").bfloat16(), 0.5)
    with pytest.raises(ValueError, match="empty"):
        ops.similarity_range(q, g[:0], 0.5)
    wide = torch.randn(100, 72, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.similarity_range(q, wide[:, 4:68], 0.5)                               # misaligned view: offset of 8 bytes
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.similarity_range(q, torch.randn(100, 68, device="cuda").bfloat16()[:, :64], 0.5)
    with pytest.raises(TypeError, match="cuda"):
        ops.similarity_range(q.cpu(), g, 0.5)
    with pytest.raises(TypeError, match="cuda"):
        ops.similarity_range(q, g.cpu(), 0.5)
    with pytest.raises(TypeError, match="mixed"):
        ops.similarity_range(q, g.half(), 0.5)
    with pytest.raises(TypeError):
        ops.similarity_range(q.float(), g.float(), 0.5)
    with pytest.raises(ValueError, match="self_join"):
        ops.similarity_range(q, g, 0.5, self_join=True)                           # another tensor, Q != N
    with pytest.raises(ValueError, match="self_join"):
        ops.similarity_range(g, g.clone(), 0.5, self_join=True)                   # equal values, other memory
    with pytest.raises(ValueError, match="self_join"):
        ops.similarity_range(g[:50], g, 0.5, self_join=True)                      # same address, Q != N
    torch.cuda.synchronize()


def test_c_entries_refuse_bad_arguments():
    """the same limits at the C ABI: CCLIP_ERR_ARG (1), nothing launched"""
    import ctypes
    from cclip_hip import load_library
    lib = load_library()
    lib.cclip_similarity_range_workspace.restype = ctypes.c_int64
    P, L, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    Q, N = 4, 100
    q = torch.randn(Q, 64, device="cuda").bfloat16()
    g = torch.randn(N, 72, device="cuda").bfloat16()
    nbytes = lib.cclip_similarity_range_workspace(I(Q), L(N))
    assert nbytes > 0 and nbytes % (4 * Q) == 0
    assert lib.cclip_similarity_range_workspace(I(0), L(N)) == 0 and lib.cclip_similarity_range_workspace(I(Q), L(2 ** 31)) == 0
    counts = torch.zeros(nbytes // 4 + 16, device="cuda", dtype=torch.int32)
    starts = torch.zeros(nbytes // 4 + 1, device="cuda", dtype=torch.int64)
    index = torch.empty(Q * N, device="cuda", dtype=torch.int32)
    scores = torch.empty(Q * N, device="cuda")

    def head(qp, ldq, Q_, gp, ldg, N_, D, thr, sj):
        return (P(qp), L(ldq), I(Q_), P(gp), L(ldg), L(N_), I(D), F(thr), I(sj))

    def count(qp=q.data_ptr(), ldq=64, Q_=Q, gp=g.data_ptr(), ldg=72, N_=N, D=64, thr=0.5, sj=0, cp=counts.data_ptr(), wb=nbytes,
              fn=lib.cclip_similarity_range_count):
        return fn(*head(qp, ldq, Q_, gp, ldg, N_, D, thr, sj), P(cp), L(wb), P(0))

    def emit(qp=q.data_ptr(), ldq=64, Q_=Q, gp=g.data_ptr(), ldg=72, N_=N, D=64, thr=0.5, sj=0, sp=starts.data_ptr(), total=0,
             H=Q * N, ip=index.data_ptr(), op=scores.data_ptr(), fn=lib.cclip_similarity_range_emit):
        return fn(*head(qp, ldq, Q_, gp, ldg, N_, D, thr, sj), P(sp), L(total), L(H), P(ip), P(op), P(0))

    assert count() == 0
    assert count(fn=lib.cclip_similarity_range_count_f16) == 0
    assert count(qp=g.data_ptr(), ldq=72, Q_=N, sj=1, cp=torch.zeros(4 * N, device="cuda", dtype=torch.int32).data_ptr(), wb=16 * N) == 0
    shape = (dict(D=40), dict(D=1056), dict(D=0), dict(N_=2 ** 31), dict(ldg=68), dict(ldq=60), dict(ldg=56), dict(gp=g.data_ptr() + 8),
             dict(qp=q.data_ptr() + 2), dict(qp=0), dict(gp=0), dict(Q_=0), dict(N_=0), dict(sj=2), dict(sj=1),
             dict(sj=1, qp=g.data_ptr(), ldq=72), dict(sj=1, qp=g.data_ptr(), ldq=64, Q_=N))
    for bad in shape + (dict(cp=0), dict(cp=counts.data_ptr() + 2), dict(wb=nbytes - 4)):
        assert count(**bad) == 1, bad
    assert emit() == 0                                                        # total 0: accepted, nothing launched
    assert emit(fn=lib.cclip_similarity_range_emit_f16) == 0
    for bad in shape + (dict(sp=0), dict(sp=starts.data_ptr() + 4), dict(ip=0), dict(op=0), dict(ip=index.data_ptr() + 2),
                        dict(total=-1), dict(H=-1), dict(total=5, H=4)):
        assert emit(**bad) == 1, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# EmbeddingIndex: planted duplicates
# ------------------------------------------------------------------------------------------------------------------------
def planted(N, E, copies, seed):
    """N unit rows, every tenth re-emitted as `copies` noisy copies (base + 0.15 / sqrt(E) randn, re-normalised), shuffled.
    Returns (features, origin): origin[r] = the base row that row r shows."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.randn(N, E, generator=gen)
    base = base / base.norm(dim=1, keepdim=True)
    src = torch.arange(0, N, 10).repeat(copies)
    noisy = base[src] + 0.15 / math.sqrt(E) * torch.randn(src.numel(), E, generator=gen)
    feats = torch.cat([base, noisy / noisy.norm(dim=1, keepdim=True)])
    origin = torch.cat([torch.arange(N), src])
    perm = torch.randperm(feats.shape[0], generator=gen)
    return feats[perm], origin[perm]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,E,copies,P", [(300, 128, 1, 30), (2000, 512, 2, 600), (5000, 768, 1, 500)])
def test_index_finds_exactly_the_planted_duplicates(N, E, copies, P, dtype):
    import clip
    feats, origin = planted(N, E, copies, N + E)
    R = feats.shape[0]
    index = clip.EmbeddingIndex(feats, dtype=dtype)
    rows16 = index.features.cpu()
    ref = rows16.double() @ rows16.double().t()
    tol = kernel_tol(E, rows16, rows16)
    same = origin[:, None] == origin[None, :]
    upper = torch.arange(R)[None, :] > torch.arange(R)[:, None]
    assert int((same & upper).sum()) == P
    lo, hi = ref[same].min().item(), ref[~same].max().item()
    print(f"[range] planted N{N} E{E} {dtype}: planted pairs >= {lo:.4f}, every other pair <= {hi:.4f}, tol {tol:.3e}")
    assert lo >= 0.9 + tol and hi < 0.9 - tol, "the planted data leaves pairs within tol of the threshold"
    pairs, scores = index.duplicate_pairs(0.9)
    assert pairs.dtype == torch.int64 and pairs.is_cuda and scores.dtype == torch.float32 and pairs.shape == (P, 2)
    pairs, scores = pairs.cpu(), scores.cpu()
    assert torch.equal(pairs, torch.nonzero(same & upper)), "not exactly the planted pairs in (first, second) order"
    assert (scores.double() - ref[pairs[:, 0], pairs[:, 1]]).abs().max().item() <= tol
    groups = index.duplicate_groups(0.9)
    first = {}
    for r, o in enumerate(origin.tolist()):
        first.setdefault(o, r)
    assert groups.dtype == torch.int64 and groups.tolist() == [first[o] for o in origin.tolist()]
    # the same graph from the query side: range_search of the stored rows = the pairs both ways plus every row itself
    off, idx, sc = index.range_search(index.features.float(), 0.9)
    assert idx.dtype == torch.int64 and off.shape == (R + 1,)
    rows = torch.repeat_interleave(torch.arange(R), off.cpu().diff())
    got = torch.zeros(R, R, dtype=torch.bool)
    got[rows, idx.cpu()] = True
    assert rows.numel() == 2 * P + R and torch.equal(got, same)


def test_index_range_search_errors_and_single_query():
    import clip
    feats, _ = planted(300, 128, 1, 5)
    index = clip.EmbeddingIndex(feats)
    off, idx, sc = index.range_search(feats[7], 0.9)                            # one 1-D query
    assert off.tolist()[0] == 0 and 7 in idx.tolist() and off.tolist()[1] == idx.numel()
    with pytest.raises(ValueError, match="expected"):
        index.range_search(torch.randn(2, 64), 0.9)
    empty = clip.EmbeddingIndex(torch.zeros(0, 128))
    with pytest.raises(ValueError, match="empty"):
        empty.range_search(torch.randn(2, 128), 0.9)
    pairs, scores = empty.duplicate_pairs()
    assert pairs.shape == (0, 2) and scores.shape == (0,) and empty.duplicate_groups().shape == (0,)


# ------------------------------------------------------------------------------------------------------------------------
# group_split
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,frac,seed", [(330, 0.25, 567), (64, 0.25, 567), (1000, 0.1, 3), (10, 0.9, 1)])
def test_group_split_keeps_groups_whole(N, frac, seed):
    import clip
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(N))
    t = N // 10
    a, b, c = perm[:t], perm[t:2 * t], perm[2 * t:2 * t + t // 2]
    labels = torch.arange(N)
    labels[a] = b                                                               # pairs (a, b), and triples (a, b, c)
    labels[c] = a[:c.numel()]
    groups = clip.connected_components(N, torch.stack([torch.arange(N), labels], dim=1))
    assert torch.bincount(torch.bincount(groups), minlength=4).tolist()[1:4] == [N - 2 * t - c.numel(), t - c.numel(), c.numel()]
    train, val = clip.group_split(groups, frac, seed)
    assert train == sorted(train) and val == sorted(val) and sorted(train + val) == list(range(N))
    assert train and val
    assert not set(groups[train].tolist()) & set(groups[val].tolist()), "a group straddles the split"
    want = max(1, int(round(frac * N)))
    if len(val) < want:                                                         # only when all groups but one have moved
        assert len(set(groups[train].tolist())) == 1
    else:                                                                       # the last group moved was needed
        sizes = torch.bincount(groups)
        assert len(val) - int(sizes[groups[val]].max()) < want or len(val) == want
    assert clip.group_split(groups, frac, seed) == (train, val)
    if N >= 64:
        assert clip.group_split(groups, frac, seed + 1) != (train, val)


@pytest.mark.parametrize("N,frac,seed", [(64, 0.25, 567), (806, 0.1, 567), (7, 0.5, 2), (5, 0.99, 9), (3, 0.01, 4)])
def test_group_split_of_singletons_is_the_trainers_split(N, frac, seed):
    """with every group of size 1: exactly what scripts/train_caption.py --val-fraction draws"""
    import clip
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed)).tolist()
    n_val = min(N - 1, max(1, int(round(frac * N))))
    train, val = clip.group_split(torch.arange(N), frac, seed)
    assert val == sorted(perm[:n_val]) and train == sorted(perm[n_val:])


# ------------------------------------------------------------------------------------------------------------------------
# scripts, memory
# ------------------------------------------------------------------------------------------------------------------------
def _lines(capsys):
    return [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]


def test_find_duplicates_script_synthetic(tmp_path, capsys):
    import clip
    import find_duplicates
    out = str(tmp_path / "deduped.pkl")
    find_duplicates.main(["--synthetic", "--threshold", "0.9", "--write-deduped", out])
    lines = _lines(capsys)
    groups, summary = lines[:-1], lines[-1]["summary"]
    assert len(groups) == 52 and all(set(g) == {"rows", "file_names", "min_score"} for g in groups)
    for g in groups:
        assert len(g["rows"]) in (2, 3) and g["rows"] == sorted(g["rows"]) and len(g["file_names"]) == len(g["rows"])
        assert len({name.split("_")[1] for name in g["file_names"]}) == 1, "a group mixes two photos"
        assert 0.9 <= g["min_score"] <= 1.01
    assert summary["rows"] == 590 and summary["duplicate_groups"] == 52 and summary["rows_in_groups"] == 130
    assert summary["rows_kept"] == 512 and summary["pairs"] == 26 * 1 + 26 * 3
    index = clip.EmbeddingIndex.from_pickle(out)
    assert len(index) == 512 and [c["clip_embedding"] for c in index.metadata] == list(range(512))
    assert len({c["file_name"].split("_")[1] for c in index.metadata}) == 512
    assert index.duplicate_pairs(0.9)[0].shape == (0, 2)


def test_train_caption_script_splits_by_group(capsys):
    import train_caption
    n = train_caption.main(["--synthetic", "--gpt2", "test-tiny", "--epochs", "1", "--bs", "8", "--val-fraction", "0.25",
                            "--dedup-threshold", "0.95"])
    lines = _lines(capsys)
    log = [ln for ln in lines if "groups" in ln]
    assert len(log) == 1 and log[0]["groups"] == 64 and log[0]["rows_kept_together"] == 0
    assert log[0]["train_rows"] == 48 and log[0]["val_rows"] == 16 and n == 6
    val = [ln for ln in lines if "val_loss" in ln]
    assert len(val) == 1 and val[0]["val_captions"] == 16 and math.isfinite(val[0]["val_loss"])


def test_duplicate_pairs_allocates_no_score_matrix():
    import clip
    N, E = 60000, 64
    gen = torch.Generator(device="cuda").manual_seed(4)
    feats = torch.randn(N, E, device="cuda", generator=gen)
    feats[N // 2:N // 2 + 100] = feats[:100] + 0.01 * torch.randn(100, E, device="cuda", generator=gen)
    index = clip.EmbeddingIndex(feats)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pairs, scores = index.duplicate_pairs(0.95)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[range-mem] peak rise {rise} bytes, {pairs.shape[0]} pairs, matrix {N * N * 4} bytes")
    assert rise < 256 * 2 ** 20, f"duplicate_pairs raised the peak by {rise} bytes"
    assert (pairs[:, 0] < pairs[:, 1]).all()
    planted_pairs = torch.stack([torch.arange(100), torch.arange(100) + N // 2], dim=1)
    assert (pairs.cpu()[:, None, :] == planted_pairs[None]).all(dim=2).any(dim=0).all(), "a planted pair is missing"
