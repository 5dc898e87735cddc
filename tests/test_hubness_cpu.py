"""CPU: the float64 reference of the hubness correction against itself (tests/hubness_ref.py), the planted-hub fixture's
conditions on the reference alone, `clip.hubness` on hand-made index tables, `QueryBank` validation and the size queries of
cclip_bank_lse, and the seeds of the random biased top-k cases the GPU tests use.  No kernel runs here."""
import ctypes
import math

import pytest
import torch

import hubness_ref as R

SEEDS = (0, 1)                                    # the seeds the GPU tests use
DTYPES = (torch.bfloat16, torch.float16)
SCORE_TOL = R.score_tol(R.HUB_D)


def test_order_keys_ties_inf_and_nan():
    inf, nan = math.inf, math.nan
    t = torch.tensor([[1.0, nan, -inf, 1.0, nan, 5.0, -inf]], dtype=torch.float64)
    assert R.order_keys(t).tolist() == [[5, 0, 3, 2, 6, 1, 4]]


def test_lse_reference_against_the_definition():
    gen = torch.Generator().manual_seed(5)
    g, bank = torch.randn(7, 32, generator=gen, dtype=torch.float64), torch.randn(5, 32, generator=gen, dtype=torch.float64)
    want = torch.tensor([math.log(sum(math.exp(0.5 * float(bank[b] @ g[j])) for b in range(5))) for j in range(7)], dtype=torch.float64)
    assert torch.allclose(R.bank_lse(g, bank, 0.5), want, rtol=1e-12, atol=1e-12)
    assert torch.equal(R.bank_lse(g, bank[:1], 2.0), 2.0 * R.scores(bank[:1], g)[0])
    assert torch.allclose(R.bank_lse(g, bank, 0.0), torch.full((7,), math.log(5.0), dtype=torch.float64), rtol=0, atol=1e-15)


def test_biased_topk_reference():
    q = torch.eye(3, 32, dtype=torch.float64)
    g = torch.zeros(6, 32, dtype=torch.float64)
    g[:, 0] = torch.tensor([1.0, 2.0, 2.0, 3.0, 0.0, 2.0])
    bias = torch.tensor([0.0, 0.5, 0.5, -math.inf, math.nan, 0.25])
    s, i, t = R.topk_biased(q, g, 6, bias, 2.0)
    assert i[0].tolist() == [1, 2, 5, 0, 3, 4]                       # ties by the lower index, -inf, then NaN
    assert s[0, :4].tolist() == [4.5, 4.5, 4.25, 2.0] and s[0, 4] == -math.inf and math.isnan(s[0, 5])
    assert R.kth_gap(t, 2)[0] == 0.25 and R.kth_gap(t, 6)[0] == math.inf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", (0, 1, 2, 3))
def test_planted_hubs_conditions_on_the_reference(seed, dtype):
    q, g, bank = (R.round16(x, dtype) for x in R.planted_hubs(seed))
    assert g.shape == (R.HUB_PAIRS + R.HUB_HUBS, R.HUB_D) and q.shape == (R.HUB_PAIRS, R.HUB_D)
    raw = R.search(q, g, 2)
    raw_r1 = R.recall_at_1(raw[1])
    assert raw_r1 <= 0.7, raw_r1
    hubs = list(range(R.HUB_PAIRS, R.HUB_PAIRS + R.HUB_HUBS))
    for method in ("is", "dis", "csls"):
        qb = R.fit(g, bank, method)
        _, idx, gate, raw_t, adj_t = R.search(q, g, 2, qb)
        assert R.recall_at_1(idx) >= 0.99, (method, R.recall_at_1(idx))
        if method == "dis":
            assert 0.25 <= float(gate.double().mean()) <= 0.60
            assert qb.active.nonzero().flatten().tolist() == hubs
            assert torch.equal(gate, raw[1][:, 0] >= R.HUB_PAIRS)
        else:
            assert bool(gate.all())
        if seed in SEEDS:                                            # the GPU comparison leaves no query out on these seeds
            assert float(R.kth_gap(raw_t, 1).min()) >= 2 * SCORE_TOL
            assert float(R.kth_gap(adj_t, 1).min()) >= 2 * R.adjusted_tol(method, R.HUB_D, R.HUB_BANK)
    counts, skew, never = R.hubness_counts(raw[1][:, :1], g.shape[0])
    assert sorted(torch.argsort(counts, descending=True, stable=True)[:R.HUB_HUBS].tolist()) == hubs and skew > 5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q,N,k,D", R.TOPK_CASES)
def test_random_topk_cases_leave_no_query_out(Q, N, k, D, dtype):
    """the seeds (and the salt) of the random biased top-k cases of test_hubness_kernels_gpu.py: the reference's own gap between
    its k-th and (k+1)-th t stays above twice the kernel's tolerance on every query, so that comparison leaves none out"""
    q16, g16, bias = R.topk_case(Q, N, k, D, dtype)
    assert q16.dtype == dtype and q16.shape == (Q, D) and g16.shape == (N, D) and bias.shape == (N,) and bias.dtype == torch.float32
    _, _, t = R.topk_biased(q16.double(), g16.double(), k, bias, R.TOPK_SCALE)
    tol = R.topk_tol(q16, g16, bias, R.TOPK_SCALE)
    assert 0 < tol < 1e-4
    assert int((R.kth_gap(t, k) < 2 * tol).sum()) == 0


def test_random_topk_cases_cover_the_issue_shapes():
    for col, want in enumerate(({1, 17, 65}, None, {1, 7, 64}, {32, 160, 1024})):
        if want is not None:
            assert {c[col] for c in R.TOPK_CASES} == want
    assert {63, 65, R.TOPK_TWO_SPLIT_N} <= {c[1] for c in R.TOPK_CASES} and any(c[1] == c[2] for c in R.TOPK_CASES)
    assert set(R.TOPK_SEED_SALT) <= set(R.TOPK_CASES)


def test_mask_composes_in_the_reference():
    q, g, bank = (R.round16(x, torch.bfloat16) for x in R.planted_hubs(0))
    mask = torch.zeros(g.shape[0], dtype=torch.bool)
    mask[R.HUB_PAIRS:] = True                                        # leave the hubs out: raw search is right again
    _, idx, _, _, _ = R.search(q, g, 3, None, mask)
    assert R.recall_at_1(idx) >= 0.99 and int(idx.max()) < R.HUB_PAIRS
    _, idx, gate, _, _ = R.search(q, g, 3, R.fit(g, bank, "dis"), mask)
    assert not bool(gate.any()) and int(idx.max()) < R.HUB_PAIRS


def test_hubness_on_hand_made_tables():
    import clip
    idx = torch.tensor([[0, 3], [0, 3], [0, 1], [0, 2]])
    rep = clip.hubness(idx, 6, top=3)
    assert rep.counts.tolist() == [4, 1, 1, 2, 0, 0] and rep.counts.dtype == torch.int64
    assert rep.top == [0, 3, 1] and rep.top_counts == [4, 2, 1]     # equal counts by the lower row
    assert rep.never == pytest.approx(2 / 6)
    counts, skew, never = R.hubness_counts(idx, 6)
    assert rep.skewness == pytest.approx(skew, rel=1e-12) and skew > 0
    even = clip.hubness(torch.arange(8).reshape(4, 2).to(torch.int32), 8)
    assert even.skewness == 0.0 and even.never == 0.0 and even.top == list(range(8))
    assert clip.hubness(idx, 6, top=0).top == []
    for bad in (torch.tensor([[0, 6]]), torch.tensor([[-1, 0]])):
        with pytest.raises(ValueError, match="outside"):
            clip.hubness(bad, 6)
    with pytest.raises(ValueError):
        clip.hubness(torch.zeros(2, 2), 6)
    with pytest.raises(ValueError):
        clip.hubness(torch.zeros(4, dtype=torch.long), 6)


def test_querybank_validation():
    import clip
    ok = dict(method="dis", beta=20.0, k=10, n=4, n_bank=3, scale=20.0, bias=torch.zeros(4), active=torch.ones(4, dtype=torch.bool))
    qb = clip.QueryBank(**ok)
    assert qb.check(4) is qb
    with pytest.raises(ValueError, match="fit it again"):
        qb.check(5)
    for change in (dict(method="softmax"), dict(bias=torch.zeros(5)), dict(bias=torch.zeros(4, dtype=torch.float64)),
                   dict(active=torch.ones(4)), dict(active=torch.ones(3, dtype=torch.bool)), dict(scale=math.nan), dict(n=0, bias=torch.zeros(0),
                                                                                                               active=torch.zeros(0, dtype=torch.bool))):
        with pytest.raises(ValueError):
            clip.QueryBank(**{**ok, **change})
    with pytest.raises(ValueError, match="method"):
        clip.fit_querybank(torch.zeros(4, 32), torch.zeros(2, 32), method="softmax")


def test_bank_lse_size_queries():
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip import load_library
    lib = load_library()
    lib.cclip_bank_lse_splits.restype = ctypes.c_int32
    lib.cclip_bank_lse_workspace.restype = ctypes.c_int64
    L = ctypes.c_int64
    assert lib.cclip_bank_lse_splits(L(0), L(5)) == 0 and lib.cclip_bank_lse_splits(L(5), L(0)) == 0
    assert lib.cclip_bank_lse_splits(L(5), L(2 ** 31)) == 0 and lib.cclip_bank_lse_workspace(L(0), L(5)) == 0
    for N in (1, 65, 129, 100_000):
        assert lib.cclip_bank_lse_splits(L(N), L(256)) == 1          # a split keeps at least 256 bank rows
        for B in (1, 257, 5000):
            s = lib.cclip_bank_lse_splits(L(N), L(B))
            assert 1 <= s <= (B + 255) // 256 and lib.cclip_bank_lse_workspace(L(N), L(B)) == N * s * 8
    assert lib.cclip_bank_lse_splits(L(17), L(257)) == 2             # the smallest two-split bank the kernel tests use
