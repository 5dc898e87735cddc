"""The float64 decode reference (tests/decode_ref.py) checked on the CPU, so that what tests/test_decode_kernels_gpu.py compares the
kernels with is itself pinned: step_ref against the oracle's full GPT-2 forward, select_ref against the host loop of
clip_caption/generate.py, and the TEETH of the kernel test's bound - for each deliberately wrong step (decode_ref.MUTATIONS) the
bound of the step-arithmetic test must reject it on the cases that reach the mutated path, computed from the reference alone."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests")]

import decode_ref as R  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_step_ref_equals_oracle_forward(dtype):
    """step_ref(rounded=False), fed one position at a time with its own (unrounded) keys / values cached, is the causal full
    forward of the oracle on the same weights: both float64, so they agree to 1e-9 relative."""
    from oracle import caption_oracle as CO
    m = R.SynthGPT2(128, 512, 2, 300, 16, dtype, 3)
    S, nb = 7, 2
    emb = torch.randn(nb, S, m.D, generator=torch.Generator().manual_seed(4), dtype=F64) * 0.3
    want = CO.gpt2_forward(m.oracle_state_dict(), emb, None, m.heads, dtype=F64)
    kc = torch.zeros(m.n_layer, nb, m.max_len, m.D, dtype=F64)
    vc = torch.zeros_like(kc)
    slot = torch.arange(8, dtype=torch.int32).repeat(m.max_len, 1)        # identity: row b reads its own slot
    for t in range(S):
        logits, _, k, v = R.step_ref(m, emb[:, t] + m.wpe[t].to(F64), kc, vc, slot, t, False)
        kc[:, :, t], vc[:, :, t] = k, v
        err = (logits - want[:, t]).abs().max().item()
        assert err <= 1e-9 * want[:, t].abs().max().item(), (t, err)


def _host_step(beams, logp, stop):
    beams.extend(logp, stop)
    return beams


@pytest.mark.parametrize("k", [1, 3, 8])
def test_select_ref_equals_host_loop(k):
    """select_ref against the literal torch loop of clip_caption/generate.py (_Beams.start / _Beams.extend, float32) on random CPU
    logits with the stop token likely at two steps, so stopped beams are present: fed the host loop's own pre-step state, tokens, sources'
    lengths and flags are identical wherever the float64 margin exceeds the float32 evaluation error, scores agree to 1e-6."""
    from clip_caption.generate import _Beams
    V, stop, T, steps = 200, 7, 0.5, 12
    g = torch.Generator().manual_seed(10 + k)
    slot = torch.zeros(32, 8, dtype=torch.int32)
    compared = stopped_seen = 0
    logits = torch.randn(1, V, generator=g) * 2
    beams = _Beams.start((logits / T).softmax(-1).log(), k, None)
    ref = R.select_ref(logits, torch.zeros(k), torch.ones(k), torch.zeros(k), torch.zeros(1, 0, dtype=torch.long), slot, 4, T, stop, True)
    assert ref.margin > 8 * ref.d32
    assert torch.equal(ref.tokens, beams.tokens) and (ref.scores - beams.total.double()).abs().max() < 1e-6
    for s in range(steps):
        # the host loop raises a beam's stop flag at the start of the NEXT step; the reference (as the kernel) right away
        pre_stopped = beams.stopped | beams.tokens[:, -1].eq(stop)
        pre = (beams.total.clone(), beams.lengths.clone(), pre_stopped.clone(), beams.tokens.clone())
        logits = torch.randn(k, V, generator=g) * 2
        if s in (2, 5):
            logits[0, stop] += 8.0                                      # beam 0 very likely takes the stop token here
        beams.extend((logits / T).softmax(-1).log(), stop)
        ref = R.select_ref(logits, pre[0], pre[1], pre[2], pre[3], slot, 5 + s, T, stop, False)
        stopped_seen += int(pre_stopped.any())
        if ref.margin <= 8 * ref.d32:
            continue
        compared += 1
        assert torch.equal(ref.tokens, beams.tokens), (s, ref.tokens, beams.tokens)
        assert torch.equal(ref.seq_len, beams.lengths.double())
        assert torch.equal(ref.stopped, beams.stopped | beams.tokens[:, -1].eq(stop))
        assert (ref.scores - beams.total.double()).abs().max() < 1e-6
    assert compared >= steps - 1 and stopped_seen > 0


def test_select_ref_ties_take_the_lower_flat_index():
    """equal logits (multiples of 0.5 at T = 0.5: exact quotients) are exact ties, ordered by the flat index, and do not count as a
    small margin; a stopped row offers column 0 only and keeps its length"""
    V = 40
    lg = torch.full((2, V), -4.0)
    lg[0, 30] = lg[0, 9] = 1.0
    slot = torch.arange(8, dtype=torch.int32).repeat(16, 1)
    r = R.select_ref(lg, torch.tensor([-1.0, -1.0]), torch.tensor([2.0, 2.0]), torch.zeros(2), torch.zeros(2, 2, dtype=torch.long), slot, 3,
                     0.5, -1, False)
    assert r.tokens[:, -1].tolist() == [9, 30] and r.src.tolist() == [0, 0] and r.margin > 0
    r = R.select_ref(lg, torch.tensor([-1.0, -0.125]), torch.tensor([2.0, 2.0]), torch.tensor([0, 1]), torch.zeros(2, 2, dtype=torch.long), slot, 3,
                     0.5, -1, False)
    assert r.src.tolist() == [1, 0] and r.tokens[:, -1].tolist() == [0, 9] and r.seq_len.tolist() == [2.0, 3.0]
    assert r.stopped.tolist() == [True, False] and r.scores[0].item() == -0.125
    assert r.slot_of[:4, 0].tolist() == [1, 1, 1, 1] and r.slot_of[4, :2].tolist() == [0, 1]


# mutation -> the cases whose path it breaks (every case that the kernel test runs at these shapes)
TEETH = [("drop_last_key", "floor"), ("drop_last_key", "chunk128"), ("slot0", "floor"), ("slot0", "chunk128"),
         ("drop_k768", "ragged-K"), ("drop_k768", "medium"), ("no_rescale", "chunk128"), ("no_rescale", "pos256"), ("ln960", "medium"),
         ("tail_identity", "pos256")]
_SIM = {}


def _exact_and_rounded(name, dtype):
    """per step of the simulated search: (state, exact outputs, rounded outputs), computed once per (case, dtype)"""
    key = (name, dtype)
    if key not in _SIM:
        m = R.case_model(name, dtype)
        _SIM[key] = (m, [(st, R.step_outputs(R.step_ref(m, st[1], st[2], st[3], st[4], st[0], False)),
                          R.step_outputs(R.step_ref(m, st[1], st[2], st[3], st[4], st[0], True))) for st in R.simulate(m, name, 0)])
    return _SIM[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mutate,name", TEETH)
def test_bound_rejects_mutation(mutate, name, dtype):
    """the bound of the kernel test, 3 x d_round + 2^-22 K_max max|exact| per compared tensor, must be broken by the mutated step
    on the very states the case goes through; the unmutated rounded step is inside it by construction"""
    m, steps = _exact_and_rounded(name, dtype)
    k_max = max(m.D, m.Hd)
    worst = 0.0
    for (pos, x, kc, vc, slot, _), exact, rnd in steps:
        mut = R.step_outputs(R.step_ref(m, x, kc, vc, slot, pos, True, mutate))
        for n in exact:
            bound, _ = R.step_bound(exact[n], rnd[n], k_max)
            worst = max(worst, (mut[n] - exact[n]).abs().max().item() / bound)
    assert worst > 1.0, f"{mutate} on {name}: the largest error is {worst:.2f} x the bound - the kernel test could not see this bug"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_reorder_the_beams(name, dtype):
    """no case may run a search whose beams never change places: at least one selection has sources other than the identity
    and is followed by a step, which then attends through the permuted slot table; in pos256 that selection is made at a position
    of 256 or more, so the permuted rows include the tail rows past 256 (the step after it is at 257 or later)"""
    m = R.case_model(name, dtype)
    steps = [(st[0], st[5]) for st in R.simulate(m, name, 0)]
    hits = [pos for pos, src in steps[1:] if R.reordered(src) and (name != "pos256" or pos > 256)]     # (steps[0]: the first selection, one row)
    assert hits, (name, [(pos, src.tolist()) for pos, src in steps])
