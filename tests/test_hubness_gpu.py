"""Hubness-corrected retrieval on the MI355X through the public path - clip.fit_querybank, EmbeddingIndex.search(querybank=,
mask=, return_gate=), retrieval_recall(bank_features=), clip.hubness - on the planted-hub fixture of tests/hubness_ref.py,
against the float64 composition of the same stored 16-bit rows.

A query is left out of the top-1 comparison only where the reference's own raw or adjusted top-1 / top-2 gap is below 2 x the
tolerance of that value (hubness_ref.score_tol, adjusted_tol); the seeds are chosen so that none is (test_hubness_cpu.py)."""
import functools

import pytest
import torch

import hubness_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
SEEDS = (0, 1)
METHODS = ("is", "dis", "csls")
HUBS = list(range(R.HUB_PAIRS, R.HUB_PAIRS + R.HUB_HUBS))


@functools.lru_cache(maxsize=None)
def fixture(seed, dtype):
    """(index, queries fp32 on the device, bank fp32 on the device, and the stored / normalised 16-bit rows as float64 on the
    host: q, g, bank) - built once per (seed, dtype), never written to"""
    import clip
    from clip.retrieval import normalize_rows
    q, g, bank = (x.to(torch.float32).cuda() for x in R.planted_hubs(seed))
    index = clip.EmbeddingIndex(g, dtype=dtype)
    rows = tuple(t.cpu().double() for t in (normalize_rows(q, dtype), index.features, normalize_rows(bank, dtype)))
    return index, q, bank, rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_no_keyword_is_the_plain_topk(seed, dtype):
    from cclip_hip import ops
    from clip.retrieval import normalize_rows
    index, q, _, _ = fixture(seed, dtype)
    s, i = index.search(q, 5)
    ws, wi = ops.similarity_topk(normalize_rows(q, dtype), index.features, 5)
    assert i.dtype == torch.int64 and torch.equal(i, wi.long()) and torch.equal(s.view(torch.int32), ws.view(torch.int32))
    s2, i2, gate = index.search(q, 5, return_gate=True)
    assert torch.equal(i2, i) and torch.equal(s2.view(torch.int32), s.view(torch.int32)) and gate.dtype == torch.bool and not gate.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_search_with_a_querybank_reproduces_the_reference(seed, dtype):
    import clip
    index, q, bank, (q64, g64, b64) = fixture(seed, dtype)
    raw_s, raw_i = index.search(q, 2)
    raw_r1 = R.recall_at_1(raw_i)
    assert raw_r1 <= 0.7
    rep = clip.hubness(raw_i[:, :1], len(index), top=R.HUB_HUBS)
    assert sorted(rep.top) == HUBS and rep.skewness > 5 and rep.counts.is_cuda and int(rep.counts.sum()) == R.HUB_PAIRS
    for method in METHODS:
        qb = index.querybank(bank, method=method)
        assert (qb.method, qb.n, qb.n_bank) == (method, len(index), R.HUB_BANK) and qb.bias.is_cuda and qb.active.is_cuda
        ref = R.fit(g64, b64, method)
        _, ref_i, ref_gate, raw_t, adj_t = R.search(q64, g64, 2, ref)
        s, i, gate = index.search(q, 2, querybank=qb, return_gate=True)
        bias_err = (qb.bias.cpu().double() - ref.bias).abs().max().item()
        tol_raw, tol_adj = R.score_tol(R.HUB_D), R.adjusted_tol(method, R.HUB_D, R.HUB_BANK)
        close = (R.kth_gap(raw_t, 1) < 2 * tol_raw) | (R.kth_gap(adj_t, 1) < 2 * tol_adj)
        r1 = R.recall_at_1(i)
        print(f"[hubness] seed {seed} {str(dtype)[6:]} {method}: raw R@1 {raw_r1:.3f} -> {r1:.3f}, gate {gate.float().mean().item():.3f}, "
              f"bias err {bias_err:.2e}, left out {int(close.sum())}")
        assert int(close.sum()) == 0, "the reference alone must leave no query out on these seeds"
        assert close.double().mean().item() <= 0.02
        assert qb.scale == ref.scale and bias_err <= tol_adj
        assert torch.equal(qb.active.cpu(), ref.active)
        keep = ~close
        assert torch.equal(i.cpu()[keep, 0], ref_i[keep, 0]), "top-1 differs from the float64 composition"
        assert torch.equal(gate.cpu()[keep], ref_gate[keep])
        assert r1 >= 0.99
        if method == "dis":
            assert 0.25 <= gate.float().mean().item() <= 0.60 and qb.active.nonzero().flatten().tolist() == HUBS
            off = ~gate                                              # the queries that kept their raw result: bit for bit
            assert torch.equal(i[off], raw_i[off]) and torch.equal(s[off].view(torch.int32), raw_s[off].view(torch.int32))
            assert (i[gate, 0] < R.HUB_PAIRS).all()
        else:
            assert gate.all()
        got = clip.retrieval_recall(q, R.planted_hubs(seed)[1].float(), ks=(1, 2), query_labels=torch.arange(R.HUB_PAIRS),
                                   gallery_labels=torch.arange(len(index)), dtype=dtype, bank_features=bank, method=method)
        assert got[1] == pytest.approx(r1) and got[2] >= got[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mask_and_stale_bank(dtype):
    import clip
    index, q, bank, (q64, g64, b64) = fixture(0, dtype)
    N = len(index)
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[R.HUB_PAIRS:] = True                                        # the hubs
    mask[::7] = True
    s, i = index.search(q, 10, mask=mask)
    assert not mask[i].any() and torch.isfinite(s).all()
    _, ref_i, _, raw_t, _ = R.search(q64, g64, 10, None, mask.cpu())
    ok = R.kth_gap(raw_t, 1) >= 2 * R.score_tol(R.HUB_D)            # raw_t carries the mask's -inf
    assert torch.equal(i.cpu()[ok, 0], ref_i[ok, 0]) and ok.double().mean() >= 0.98
    for method in METHODS:
        qb = index.querybank(bank, method=method)
        s, i, gate = index.search(q, 10, querybank=qb, mask=mask, return_gate=True)
        assert not mask[i].any(), method
        _, ref_i, ref_gate, _, _ = R.search(q64, g64, 10, R.fit(g64, b64, method), mask.cpu())
        assert torch.equal(gate.cpu(), ref_gate) and (i.cpu()[:, 0] == ref_i[:, 0]).double().mean() >= 0.98
    keep_few = torch.ones(N, dtype=torch.bool, device="cuda")
    keep_few[:3] = False                                             # three rows left: they lead, the masked ones trail with -inf
    s, i = index.search(q[:4], 5, mask=keep_few)
    assert (i[:, :3].sort(dim=1).values == torch.arange(3, device="cuda")).all() and torch.isinf(s[:, 3:]).all()
    assert torch.equal(i[:, 3:], torch.tensor([3, 4], device="cuda").expand(4, -1))
    with pytest.raises(ValueError):
        index.search(q, 3, mask=mask[:-1])
    with pytest.raises(ValueError):
        index.search(q, 3, mask=mask.float())
    # a bank fitted before `add` is stale
    grown = clip.EmbeddingIndex(index.features.float(), dtype=dtype)
    qb = grown.querybank(bank)
    grown.add(q[:2])
    with pytest.raises(ValueError, match="fit it again"):
        grown.search(q, 3, querybank=qb)
    assert grown.search(q, 3, querybank=grown.querybank(bank))[1].shape == (R.HUB_PAIRS, 3)
