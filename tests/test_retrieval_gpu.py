"""Retrieval on the MI355X: the fused similarity top-k kernel (csrc/embed_topk.hip) against float64 on the same 16-bit
operands, its tie order, its argument errors; clip.EmbeddingIndex (build, add, pickle, model queries), clip.retrieval_recall
against a float64 recall on planted labels, the absence of a Q x N buffer, and scripts/search_images.py.

Kernel tolerance: products of two 16-bit operands are exact in fp32, so only the D - 1 additions round; sequentially that is
D 2^-24 |q| |g|, and tol = D 2^-22 max|q| max|g| leaves a factor 4 for the MFMA's internal summation order.

Largest measured error: NOT MEASURED - this file has not yet run on an MI355X, so tol stands at the derived bound above and
has not been tightened.  Every kernel case prints its figures (`[topk] ... honest .. rank .. tol ..` and `[topk-rel] D .. rel ..`
= error / (max|q| max|g|)) before it asserts; run with -s to collect them.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DTYPES = [torch.bfloat16, torch.float16]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def kernel_tol(D, q16, g16):
    return D * 2.0 ** -22 * q16.double().norm(dim=1).max().item() * g16.double().norm(dim=1).max().item()


def check_topk(scores, index, ref, k, tol, what=""):
    """conditions 1-4 of the float64 comparison; returns the largest error of condition 3"""
    scores, index = scores.cpu(), index.cpu().long()
    Q, N = ref.shape
    assert scores.shape == (Q, k) and index.shape == (Q, k) and scores.dtype == torch.float32
    assert not torch.isnan(scores).any(), what
    assert (scores[:, 1:] <= scores[:, :-1]).all(), f"{what}: scores not descending"                          # 1
    assert (index >= 0).all() and (index < N).all(), f"{what}: index out of range"                            # 2
    assert (index.sort(dim=1).values.diff(dim=1) > 0).all() if k > 1 else True, f"{what}: repeated index"     # 2
    honest = (scores.double() - ref.gather(1, index)).abs().max().item()                                      # 3
    ranks = (scores.double() - ref.topk(k, dim=1).values).abs().max().item()                                  # 4
    print(f"[topk] {what} honest {honest:.3e} rank {ranks:.3e} tol {tol:.3e}")
    assert honest <= tol, f"{what}: score off its own pair by {honest:.3e} > {tol:.3e}"
    assert ranks <= tol, f"{what}: rank value off by {ranks:.3e} > {tol:.3e}"
    return honest


# (Q, N, D, k): every Q, N, D and k of the list appears; Q N D of a case <= 5e9.  The last rows add widths whose rows are not a
# power-of-two number of 16-byte chunks (96, 160, 768) and the largest (1024) and smallest (32) widths.
CASES = [
    (1, 1, 64, 1), (3, 5, 128, 5), (16, 5, 64, 5), (16, 64, 512, 10), (1024, 64, 128, 64), (100, 1000, 768, 64),
    (1, 1000, 768, 10), (1024, 1000, 768, 64), (3, 4097, 64, 64), (100, 4097, 512, 1), (1024, 4097, 512, 10),
    (1, 100003, 512, 10), (3, 100003, 64, 10), (16, 100003, 768, 64), (100, 100003, 128, 5), (1, 100003, 64, 1),
    (16, 1000, 1024, 10), (3, 1000, 32, 5), (100, 1000, 96, 5), (100, 4097, 160, 10),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q,N,D,k", CASES)
def test_kernel_against_float64(Q, N, D, k, dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(1000 * D + Q + N + k)
    q16 = torch.randn(Q, D, generator=gen).to(dtype)
    g16 = torch.randn(N, D, generator=gen).to(dtype)
    ref = q16.double() @ g16.double().t()
    qd, gd = q16.cuda(), g16.cuda()
    s1, i1 = ops.similarity_topk(qd, gd, k)
    s2, i2 = ops.similarity_topk(qd, gd, k)
    torch.cuda.synchronize()
    assert s1.dtype == torch.float32 and i1.dtype == torch.int32
    assert torch.equal(s1, s2) and torch.equal(i1, i2), "two launches differ"
    tol = kernel_tol(D, q16, g16)
    err = check_topk(s1, i1, ref, k, tol, f"Q{Q} N{N} D{D} k{k} {dtype}")
    scale = tol / (D * 2.0 ** -22)
    print(f"[topk-rel] D {D} {dtype} rel {err / scale:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q,N,D,k", [(3, 1000, 64, 5), (100, 4097, 128, 10), (16, 100003, 512, 64)])
def test_kernel_strided_rows(Q, N, D, k, dtype):
    """both operands as column slices of wider buffers (row strides D + 8 and 2 D + 64, 16-byte aligned offsets), outputs given"""
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(7 + Q)
    qw = torch.randn(Q, D + 8, generator=gen).to(dtype)
    gw = torch.randn(N, 2 * D + 64, generator=gen).to(dtype)
    q16, g16 = qw[:, 8:], gw[:, 16:16 + D]
    ref = q16.double() @ g16.double().t()
    qd, gd = qw.cuda()[:, 8:], gw.cuda()[:, 16:16 + D]
    out_s = torch.full((Q, k), float("nan"), device="cuda")
    out_i = torch.full((Q, k), -1, device="cuda", dtype=torch.int32)
    s, i = ops.similarity_topk(qd, gd, k, out_scores=out_s, out_index=out_i)
    assert s is out_s and i is out_i
    check_topk(s, i, ref, k, kernel_tol(D, q16, g16), f"strided Q{Q} N{N} D{D} k{k} {dtype}")
    s2, i2 = ops.similarity_topk(qd.contiguous(), gd.contiguous(), k)
    assert torch.equal(s, s2) and torch.equal(i, i2), "strided and contiguous operands differ"


# ------------------------------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q,M,D,k", [(16, 4000, 64, 64), (100, 10000, 128, 30), (1, 40000, 512, 64)])
def test_duplicates_come_in_index_order(Q, M, D, k, dtype):
    """every distinct row three times at scattered positions, over many splits and tiles"""
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(Q + M)
    base = torch.randn(M, D, generator=gen).to(dtype)
    ident = torch.arange(M).repeat(3)[torch.randperm(3 * M, generator=gen)]      # gallery row -> distinct row
    g16 = base[ident]
    q16 = torch.randn(Q, D, generator=gen).to(dtype)
    s, i = ops.similarity_topk(q16.cuda(), g16.cuda(), k)
    s, i = s.cpu(), i.cpu().long()
    check_topk(s, i, q16.double() @ g16.double().t(), k, kernel_tol(D, q16, g16), f"dup Q{Q} M{M} D{D} {dtype}")
    ident = ident.tolist()
    copies = {}
    for n, r in enumerate(ident):
        copies.setdefault(r, []).append(n)                                          # ascending
    for q in range(Q):
        idx, sc = i[q].tolist(), s[q].tolist()
        got = set(idx)
        for j in range(1, k):
            if sc[j] == sc[j - 1]:
                assert idx[j] > idx[j - 1], f"query {q}: equal scores at ranks {j - 1}, {j} out of index order"
        for j, n in enumerate(idx):
            same = [sc[jj] for jj, nn in enumerate(idx) if ident[nn] == ident[n]]
            assert len(set(same)) == 1, f"query {q}: copies of one row scored differently"
            for lower in copies[ident[n]]:
                if lower < n:
                    assert lower in got, f"query {q}: copy {n} returned, lower copy {lower} missing"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("Q,k,D", [(1, 1, 64), (3, 10, 512), (100, 64, 128), (16, 64, 768)])
def test_identical_rows_return_arange(Q, k, D, dtype):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(3)
    g16 = torch.randn(1, D, generator=gen).to(dtype).repeat(300, 1)
    q16 = torch.randn(Q, D, generator=gen).to(dtype)
    s, i = ops.similarity_topk(q16.cuda(), g16.cuda(), k)
    assert torch.equal(i.cpu(), torch.arange(k, dtype=torch.int32).repeat(Q, 1))
    assert (s == s[:, :1]).all()


@pytest.mark.parametrize("N,D", [(1, 64), (5, 128), (64, 512), (37, 768)])
def test_k_equal_n_is_a_permutation(N, D):
    from cclip_hip import ops
    gen = torch.Generator().manual_seed(N)
    q16, g16 = torch.randn(16, D, generator=gen).bfloat16(), torch.randn(N, D, generator=gen).bfloat16()
    s, i = ops.similarity_topk(q16.cuda(), g16.cuda(), N)
    assert torch.equal(i.cpu().long().sort(dim=1).values, torch.arange(N).repeat(16, 1))
    check_topk(s, i, q16.double() @ g16.double().t(), N, kernel_tol(D, q16, g16), f"k == N == {N}")


def test_nan_and_infinite_scores_rank_last():
    from cclip_hip import ops
    g16 = torch.zeros(200, 64, dtype=torch.float16)
    g16[:, 0] = torch.arange(200).half()
    g16[17, 0] = float("nan")
    g16[150, 0] = float("-inf")
    q16 = torch.zeros(1, 64, dtype=torch.float16)
    q16[0, 0] = 1.0
    s, i = ops.similarity_topk(q16.cuda(), g16.cuda(), 64)
    assert i[0, :3].tolist() == [199, 198, 197]
    s, i = ops.similarity_topk(q16.cuda(), g16[:40].cuda(), 40)
    assert i[0, -1].item() == 17 and torch.isnan(s[0, -1]) and not torch.isnan(s[0, :-1]).any()
    assert i[0, :-1].tolist() == [n for n in range(39, -1, -1) if n != 17]
    s, i = ops.similarity_topk(q16.cuda(), g16[140:160].cuda(), 20)
    assert i[0, -1].item() == 10 and s[0, -1].item() == float("-inf")


# ------------------------------------------------------------------------------------------------------------------------
# argument errors: raised by the binding, nothing launched
# ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from cclip_hip import ops
    q = torch.randn(4, 64, device="cuda").bfloat16()
    g = torch.randn(100, 64, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="1 .. 64"):
        ops.similarity_topk(q, g, 0)
    with pytest.raises(ValueError, match="1 .. 64"):
        ops.similarity_topk(q, torch.randn(200, 64, device="cuda").bfloat16(), 65)
    with pytest.raises(ValueError, match="above the gallery's 5 rows"):
        ops.similarity_topk(q, g[:5], 6)
    with pytest.raises(NotImplementedError, match="D % 32 == 0"):
        ops.similarity_topk(torch.randn(4, 40, device="cuda").bfloat16(), torch.randn(100, 40, device="cuda").bfloat16(), 5)
    with pytest.raises(NotImplementedError, match="D <= 1024"):
        ops.similarity_topk(torch.randn(4, 1056, device="cuda").bfloat16(), torch.randn(10, 1056, device="cuda").bfloat16(), 5)
    wide = torch.randn(100, 72, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.similarity_topk(q, wide[:, 4:68], 5)                                   # misaligned view: offset of 8 bytes
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.similarity_topk(q, torch.randn(100, 68, device="cuda").bfloat16()[:, :64], 5)
    with pytest.raises(TypeError, match="cuda"):
        ops.similarity_topk(q.cpu(), g, 5)
    with pytest.raises(TypeError, match="cuda"):
        ops.similarity_topk(q, g.cpu(), 5)
    with pytest.raises(TypeError, match="mixed"):
        ops.similarity_topk(q, g.half(), 5)
    with pytest.raises(TypeError):
        ops.similarity_topk(q.float(), g.float(), 5)
    torch.cuda.synchronize()


def test_c_entry_refuses_bad_arguments():
    """the same limits at the C ABI: CCLIP_ERR_ARG (1), nothing launched"""
    import ctypes
    from cclip_hip import load_library
    lib = load_library()
    lib.cclip_similarity_topk_workspace.restype = ctypes.c_int64
    q = torch.randn(4, 64, device="cuda").bfloat16()
    g = torch.randn(100, 72, device="cuda").bfloat16()
    s = torch.empty(4, 64, device="cuda")
    i = torch.empty(4, 64, device="cuda", dtype=torch.int32)
    ws = torch.empty(1 << 16, device="cuda", dtype=torch.int64)
    P, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32

    def call(qp=q.data_ptr(), ldq=64, Q=4, gp=g.data_ptr(), ldg=72, N=100, D=64, k=5, sp=s.data_ptr(), ip=i.data_ptr(),
             wp=ws.data_ptr(), wb=ws.numel() * 8, fn=lib.cclip_similarity_topk):
        return fn(P(qp), L(ldq), I(Q), P(gp), L(ldg), L(N), I(D), I(k), P(sp), P(ip), P(wp), L(wb), P(0))

    assert call() == 0
    assert call(fn=lib.cclip_similarity_topk_f16) == 0
    for bad in (dict(k=0), dict(k=65), dict(k=6, N=5), dict(D=40), dict(D=1056), dict(N=2 ** 31), dict(ldg=68), dict(ldq=60),
                dict(ldg=56), dict(gp=g.data_ptr() + 8), dict(qp=q.data_ptr() + 2), dict(qp=0), dict(gp=0), dict(sp=0), dict(ip=0),
                dict(wp=0), dict(wb=8), dict(Q=0), dict(N=0)):
        assert call(**bad) == 1, bad
    assert lib.cclip_similarity_topk_workspace(I(4), L(100), I(5)) > 0
    assert lib.cclip_similarity_topk_workspace(I(4), L(100), I(5)) % 8 == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# EmbeddingIndex
# ------------------------------------------------------------------------------------------------------------------------
def index_tol(D, dtype):
    u = UNIT[dtype]
    return (2 * u + u * u) + D * 2.0 ** -22


def unit64(x):
    x = x.float()
    return (x / x.norm(dim=1, keepdim=True)).double()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,E,Q,k,on_device", [(5000, 512, 33, 10, False), (20000, 768, 4, 64, True), (300, 128, 100, 5, False)])
def test_index_against_float64(N, E, Q, k, on_device, dtype):
    import clip
    gen = torch.Generator().manual_seed(N + E)
    feats = torch.randn(N, E, generator=gen) * 3.0
    queries = torch.randn(Q, E, generator=gen) * 0.2
    ref = unit64(queries) @ unit64(feats).t()
    index = clip.EmbeddingIndex(feats.cuda() if on_device else feats, dtype=dtype)
    assert len(index) == N and index.features.shape == (N, E) and index.features.dtype == dtype and index.features.is_cuda
    s, i = index.search(queries.double() if on_device else queries, k)
    assert s.is_cuda and i.is_cuda and i.dtype == torch.int64
    check_topk(s, i, ref, k, index_tol(E, dtype), f"index N{N} E{E} {dtype}")
    assert (index.features.double().norm(dim=1) - 1).abs().max().item() <= 2 * UNIT[dtype]


def test_index_default_dtype_and_errors():
    import clip
    index = clip.EmbeddingIndex(torch.randn(10, 64))
    assert index.dtype == torch.bfloat16 and index.features.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="expected"):
        index.search(torch.randn(2, 32))
    with pytest.raises(ValueError, match="above the gallery"):
        index.search(torch.randn(2, 64), k=11)
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        clip.EmbeddingIndex(torch.randn(10, 40))
    with pytest.raises(ValueError, match="metadata"):
        clip.EmbeddingIndex(torch.randn(10, 64), metadata=[1, 2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_add_in_pieces_equals_bulk(dtype):
    import clip
    gen = torch.Generator().manual_seed(11)
    feats = torch.randn(3001, 512, generator=gen)
    meta = [{"file_name": f"{n}.png"} for n in range(3001)]
    queries = torch.randn(20, 512, generator=gen)
    bulk = clip.EmbeddingIndex(feats, dtype=dtype, metadata=meta)
    parts = clip.EmbeddingIndex(feats[:7], dtype=dtype, metadata=meta[:7])
    parts.add(feats[7:1200].cuda(), meta[7:1200])
    parts.add(feats[1200:], meta[1200:])
    assert len(parts) == 3001 and parts.metadata == meta
    assert torch.equal(parts.features, bulk.features)
    (sa, ia), (sb, ib) = parts.search(queries, 10), bulk.search(queries, 10)
    assert torch.equal(sa, sb) and torch.equal(ia, ib)


def test_from_pickle_metadata(tmp_path):
    import clip
    from clip_caption.data import save_embeddings
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(400, 512, generator=gen)
    captions = [{"id": 1000 + n, "file_name": f"images/site_{n:04d}.png", "clip_embedding": n, "caption": f"c{n}"} for n in range(400)]
    path = str(tmp_path / "emb.pkl")
    save_embeddings(path, feats, captions)
    index = clip.EmbeddingIndex.from_pickle(path)
    assert len(index) == 400 and index.metadata == captions
    picks = [3, 77, 399]
    s, i = index.search(feats[picks] + 0.01 * torch.randn(3, 512, generator=gen), k=3)
    for row, n in enumerate(picks):
        assert index.metadata[int(i[row, 0])]["file_name"] == f"images/site_{n:04d}.png"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_model_queries_equal_search_of_encodings(dtype):
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_images
    g = torch.load(os.path.join(GOLD, "clip_test_small.pt"), weights_only=True)
    geo = MODELS[g["model"]]
    model = clip.build_model(init_state_dict(geo, g["seed"]), dtype).cuda().eval()
    img = synthetic_images(g["n"], geo, g["seed"] + 1)
    txt = g["text"]
    with torch.no_grad():
        fi, ft = model.encode_image(img.cuda()), model.encode_text(txt.cuda())
    index = clip.EmbeddingIndex(fi, dtype=model.compute_dtype)
    k = min(5, len(index))
    (sa, ia), (sb, ib) = index.search_text(model, txt, k), index.search(ft, k)
    assert torch.equal(sa, sb) and torch.equal(ia, ib)
    (sa, ia), (sb, ib) = index.search_image(model, img, k), index.search(fi, k)
    assert torch.equal(sa, sb) and torch.equal(ia, ib)


# ------------------------------------------------------------------------------------------------------------------------
# recall
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_recall_of_a_set_against_itself_is_one(dtype):
    import clip
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(500, 512, generator=gen)
    assert clip.retrieval_recall(feats, feats, dtype=dtype) == {1: 1.0, 5: 1.0, 10: 1.0}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_recall_on_planted_labels_equals_float64(dtype):
    """Groups of 4 gallery rows = one query + noise; every third query carries a label no gallery row has.  In float64 every
    group leads every foreign row by more than 10 tol, so the 16-bit search must find exactly the float64 hits."""
    import clip
    from clip.retrieval import recall_from_indices
    E, Q = 128, 96
    gen = torch.Generator().manual_seed(9)
    queries = torch.randn(Q, E, generator=gen)
    queries = queries / queries.norm(dim=1, keepdim=True)
    noise = torch.randn(Q, 4, E, generator=gen)
    gallery = (queries[:, None, :] + 0.3 * noise / noise.norm(dim=2, keepdim=True)).reshape(4 * Q, E)
    perm = torch.randperm(4 * Q, generator=gen)
    gallery, group = gallery[perm], (torch.arange(4 * Q) // 4)[perm]
    query_labels = torch.arange(Q)
    query_labels[::3] = -1
    ref = unit64(queries) @ unit64(gallery).t()
    own = group[None, :] == torch.arange(Q)[:, None]
    margin = (ref.masked_fill(~own, 9.0).min(dim=1).values - ref.masked_fill(own, -9.0).max(dim=1).values).min().item()
    tol = index_tol(E, dtype)
    assert margin > 10 * tol, f"the planted data is not separated: margin {margin:.3e} vs 10 tol {10 * tol:.3e}"
    ks = (1, 5, 10)
    want = recall_from_indices(ref.topk(10, dim=1).indices, query_labels, group, ks).tolist()
    assert want == [2 / 3] * 3
    got = clip.retrieval_recall(queries, gallery, ks=ks, query_labels=query_labels, gallery_labels=group, dtype=dtype)
    assert got == dict(zip(ks, want))
    # a label that only a foreign group carries is met only past the own group's four rows
    shifted = (torch.arange(Q) + 1) % Q
    want = recall_from_indices(ref.topk(4, dim=1).indices, shifted, group, (1, 4)).tolist()
    got = clip.retrieval_recall(queries, gallery, ks=(1, 4), query_labels=shifted, gallery_labels=group, dtype=dtype)
    assert want == [0.0, 0.0] and got == {1: 0.0, 4: 0.0}


# ------------------------------------------------------------------------------------------------------------------------
# no Q x N buffer; the script
# ------------------------------------------------------------------------------------------------------------------------
def test_search_allocates_no_score_matrix():
    import clip
    Q, N, D = 256, 1 << 20, 64
    gen = torch.Generator(device="cuda").manual_seed(4)
    index = clip.EmbeddingIndex(torch.randn(N, D, device="cuda", generator=gen))
    queries = torch.randn(Q, D, device="cuda", generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    s, i = index.search(queries, k=10)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[topk-mem] peak rise {rise} bytes, matrix {Q * N * 4} bytes")
    assert rise < Q * N * 4 // 8, f"search raised the peak by {rise} bytes"
    assert (s[:, 1:] <= s[:, :-1]).all() and (i >= 0).all() and (i < N).all()


def test_search_script_synthetic():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "search_images.py"), "--synthetic", "--k", "5"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    hits = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(hits) == 5
    assert [h["rank"] for h in hits] == [1, 2, 3, 4, 5]
    assert all(set(h) == {"rank", "score", "index", "file_name"} for h in hits)
    assert all(hits[j]["score"] >= hits[j + 1]["score"] for j in range(4))
    assert all(h["file_name"].startswith("images/fall_") for h in hits)
