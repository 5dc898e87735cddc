"""GPU: the persistent beam-search kernels (csrc/decode_persist.hip, decode_persist_batch.hip, decode_persist_impl.h), the skinny
decode projections (gemm_skinny_impl.h) and the native decode driver (decode_driver.hip) at the kernel boundary, against the
float64 reference of tests/decode_ref.py (itself checked in tests/test_decode_ref_cpu.py), in bfloat16 and float16.

A search is driven ONE STEP PER LAUNCH (gpt2_beam_search(first_logits=None, n_steps=1, logits=buf)), so that every step's
logits and state can be read back and the two halves of a step are checked apart:

(a) step arithmetic: step_ref, fed the kernel's own pre-step state, against the kernel's logits, the k / v rows it appended in
    every layer and (where the selection does not overwrite it: the last position) the residual stream.  Per compared tensor
        max|kernel - exact| <= 3 * max|step_ref(rounded=True) - step_ref(rounded=False)| + 2^-22 * K_max * max|exact|
    The first term is the 16-bit rounding at the kernel's own rounding points as the reference measures it (d_round); 3, because
    the kernel's fp32 values can flip any of those roundings - its deviation is a second draw of the same size - and a maximum
    over many elements needs headroom; the second term is fp32 accumulation order over the longest contraction.  The CPU teeth
    tests show that this bound rejects a dropped key, a wrong cache slot, dropped weight rows, a missing online-softmax rescale
    and truncated LayerNorm statistics on these very cases.
(b) selection: select_ref applied to the kernel's OWN logits and pre-step state.  Tokens, lengths, flags, the whole slot table and
    the token-column count must be identical, x must be wte[tok] + wpe[pos + 1] exactly, scores within 8 * d32 (d32: float32
    torch evaluation against float64 over the step's candidates).  A step whose float64 margin is below that tolerance is
    ambiguous and skipped: at most 5 % of a case's steps, none in the crafted cases.
(c) crafted first selections (logits that are multiples of 0.5 at T = 0.5: exact quotients, bit-equal candidates; the seeds of
    their backgrounds are admitted on the reference alone, see CRAFTED), (d) stopped
    beams that win, lose and exactly tie a live candidate, (e) the batched kernel and the native driver on the same reference.
    The batched kernel has no logits output, so its scores are compared with the float64 REPLAY of its own tokens: tolerance
    8 * d32 plus 2 * d_round / T per step (d_round of the step's logits, no headroom).  Every step case must reorder its beams
    and then step through the permuted slot table (pos256: with the rows past 256 permuted); run_case asserts it.

Measured err / d_round per case and the ambiguous-step counts: not run on a GPU yet.
"""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_ref as R  # noqa: E402

DTS = [torch.bfloat16, torch.float16]
T = 0.5
SENT = -7.25                       # exact in every type: guard rows behind each cache slot
_MODELS = {}


def ops():
    from cclip_hip import ops as o
    return o


def get_model(name, dtype):
    """(reference model, its device copy, the ctypes block array) of a case, built once per (geometry, dtype)"""
    c = R.CASES[name]
    key = (c["D"], c["Hd"], c["L"], c["V"], c["max_len"], dtype)
    if key not in _MODELS:
        m = R.SynthGPT2(*key[:5], dtype, 0)
        d = m.to_device()
        _MODELS[key] = (m, d, ops().block_ptr_array(d.blocks))
    return _MODELS[key]


def guarded_cache(kc):
    """device copy of a [L, n, max_len, D] cache whose slots are each followed by two guard rows of SENT (not part of the view)"""
    L, n, ml, D = kc.shape
    buf = torch.full((L, n, ml + 2, D), SENT, device="cuda", dtype=kc.dtype)
    buf[:, :, :ml] = kc.cuda()
    return buf, buf[:, :, :ml]


class Single:
    """one search on the one-caption kernel, driven launch by launch"""

    def __init__(self, name, dtype, nb, pos0, seed, grid_cap=0, stop=-1, prompt=0, n_tokens=16, cache=None):
        self.m, self.d, self.arr = get_model(name, dtype)
        m = self.m
        self.nb, self.pos0, self.grid_cap, self.stop, self.prompt = nb, pos0, grid_cap, stop, prompt
        kc, vc = cache if cache is not None else R.fill_cache(m, nb, pos0, seed)
        self.kbuf, self.k = guarded_cache(kc)
        self.vbuf, self.v = guarded_cache(vc)
        self.st = ops().BeamState(nb, m.max_len, prompt + n_tokens, "cuda")
        if prompt:
            g = torch.Generator().manual_seed(seed + 7)
            self.st.tokens[0, :prompt] = torch.randint(0, m.V, (prompt,), generator=g).to(torch.int32).cuda()
            self.st.state[4] = prompt
        self.scratch = torch.empty(nb * (5 * m.D + m.Hd), device="cuda", dtype=dtype)
        self.logits = torch.full((nb, m.V), float("nan"), device="cuda")

    def launch(self, pos, n_steps, first_logits=None, want_logits=True):
        m, d = self.m, self.d
        fl = None if first_logits is None else first_logits.float().contiguous().cuda()
        ops().gpt2_beam_search(self.arr, m.n_layer, self.st, self.k, self.v, pos, self.scratch, n_steps, heads=m.heads, hidden=m.Hd,
                               act=ops().ACT_GELU_NEW, lnf_w=d.lnf_w, lnf_b=d.lnf_b, wte16=d.wte16, wte_f32=d.wte, wpe_f32=d.wpe,
                               temperature=T, stop_token=self.stop, first_logits=fl, logits=self.logits if want_logits else None,
                               grid_cap=self.grid_cap)
        torch.cuda.synchronize()
        state = self.st.state.tolist()
        # the barrier-timeout flag: fail at once, nothing more is launched by this test
        assert state[1] == 0, "a phase hand-over of the persistent kernel timed out"
        return state

    def read(self):
        st = self.st
        return SimpleNamespace(x=None if st.x is None else st.x.cpu(), tokens=st.tokens.cpu().long(), scores=st.scores.cpu().double(),
                               seq_len=st.seq_lengths.cpu().double(), stopped=st.is_stopped.cpu().bool(), slot=st.slot_of.cpu(),
                               state=st.state.tolist(), k=self.k.cpu(), v=self.v.cpu())

    def guards_intact(self):
        return bool((self.kbuf[:, :, self.m.max_len:] == SENT).all() and (self.vbuf[:, :, self.m.max_len:] == SENT).all())


def compare_selection(sel, post, pos, ntok, tol):
    """the kernel's post-step state against a select_ref result: everything identical, scores within tol"""
    assert torch.equal(post.tokens[:, :ntok + 1], sel.tokens), (pos, post.tokens[:, :ntok + 1], sel.tokens)
    assert torch.equal(post.seq_len, sel.seq_len) and torch.equal(post.stopped, sel.stopped), (pos, post.seq_len, sel.seq_len)
    assert torch.equal(post.slot, sel.slot_of), pos
    assert post.state[4] == ntok + 1
    err = (post.scores - sel.scores).abs().max().item()
    print(f"  select pos {pos}: score err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (pos, err, tol, post.scores, sel.scores)
    if sel.x is not None:
        assert torch.equal(post.x, sel.x), pos                          # one fp32 add
    if sel.all_stopped:
        assert post.state[2] == 1


def check_selection(m, logits, pre, post, pos, stop, first, ntok):
    """(b): select_ref on the kernel's own logits and pre-step state against the kernel's post-step state; returns the
    reference's selection, or None where the step is ambiguous"""
    nb = post.scores.shape[0]
    if first:
        sel = R.select_ref(logits, torch.zeros(nb), torch.ones(nb), torch.zeros(nb), pre.tokens[:1, :ntok], pre.slot, pos, T, stop, True, m)
    else:
        sel = R.select_ref(logits, pre.scores, pre.seq_len, pre.stopped, pre.tokens[:, :ntok], pre.slot, pos, T, stop, False, m)
    tol = 8 * sel.d32
    print(f"  select pos {pos}: margin {sel.margin:.3e} d32 {sel.d32:.3e} src {sel.src.tolist()}")
    if sel.margin < tol:
        return None
    compare_selection(sel, post, pos, ntok, tol)
    return sel


def check_step(m, got, pre, pos, ratios):
    """(a): `got` (name -> kernel tensor) against step_ref on the pre-step state; returns the logits' bound"""
    exact = R.step_outputs(R.step_ref(m, pre.x, pre.k, pre.v, pre.slot, pos, False))
    rnd = R.step_outputs(R.step_ref(m, pre.x, pre.k, pre.v, pre.slot, pos, True))
    k_max = max(m.D, m.Hd)
    bounds = {}
    for n, g in got.items():
        bound, d_round = R.step_bound(exact[n], rnd[n], k_max)
        assert torch.isfinite(g).all(), (n, pos)
        err = (g.double() - exact[n]).abs().max().item()
        key = n[0] if n[0] in "kv" else n
        if d_round > 0:
            ratios[key] = max(ratios.get(key, 0.0), err / d_round)
        print(f"  step pos {pos} {n}: err {err:.3e} d_round {d_round:.3e} bound {bound:.3e}")
        bounds[n] = bound
        assert err <= bound, f"{n} at position {pos}: err {err:.3e} > bound {bound:.3e} (d_round {d_round:.3e})"
    return bounds, exact


def run_case(name, dtype, nb=None, grid_cap=0, seed=0, tag=None):
    c = R.CASES[name]
    nb = nb or c["beams"]
    pos0, prompt = c["pos0"], c.get("prompt", 0)
    h = Single(name, dtype, nb, pos0, seed, grid_cap=grid_cap, prompt=prompt)
    m = h.m
    g = torch.Generator().manual_seed(seed + 1)
    first_logits = torch.randn(m.V, generator=g) * 2.0
    pre = h.read()
    h.launch(pos0, 0, first_logits=first_logits)
    post = h.read()
    decided = [check_selection(m, first_logits.double(), pre, post, pos0 - 1, -1, True, prompt)]
    ratios = {}
    ntok = prompt + 1
    through_permuted = []            # steps that attended through a slot table the selection before them had permuted
    for i in range(c["steps"]):
        pos = pos0 + i
        pre = post
        h.logits.fill_(float("nan"))
        h.launch(pos, 1)
        post = h.read()
        if pos >= m.max_len:                                          # past the cache: the launch must change nothing
            for f in ("tokens", "scores", "seq_len", "stopped", "slot", "k", "v", "x"):
                assert torch.equal(getattr(pre, f), getattr(post, f)), (f, pos)
            assert post.state[2:5] == pre.state[2:5] and bool(torch.isnan(h.logits).all())
            continue
        if i > 0 and decided[-1] is not None and R.reordered(decided[-1].src):
            through_permuted.append(pos)
        lg = h.logits.cpu().double()
        got = {"logits": lg}
        for l in range(m.n_layer):
            got[f"k{l}"], got[f"v{l}"] = post.k[l, :nb, pos], post.v[l, :nb, pos]
        if pos + 1 >= m.max_len:
            got["x"] = post.x                                         # no next input row is written: x is the step's residual stream
        check_step(m, got, pre, pos, ratios)
        # nothing but row `pos` of the cache may change
        keep = torch.ones(m.max_len, dtype=torch.bool)
        keep[pos] = False
        assert torch.equal(pre.k[:, :, keep], post.k[:, :, keep]) and torch.equal(pre.v[:, :, keep], post.v[:, :, keep])
        decided.append(check_selection(m, lg, pre, post, pos, -1, False, ntok))
        ntok += 1
    assert h.guards_intact()
    skipped = decided.count(None)
    # the search is not a degenerate one: the beams changed places and a step followed (pos256: with the tail rows past 256 permuted)
    if nb > 1:
        assert [p for p in through_permuted if name != "pos256" or p > 256], (name, through_permuted)
    print(f"RATIOS {tag or name} {str(dtype)[6:]} nb={nb} grid_cap={grid_cap}: " + " ".join(f"{k}={v:.2f}" for k, v in sorted(ratios.items()))
          + f" ambiguous={skipped}/{len(decided)} through_permuted={through_permuted}")
    assert skipped <= 0.05 * len(decided), f"{skipped} of {len(decided)} selections ambiguous: pick another seed"
    return h, post


STEP_CASES = [("floor", None, 0), ("chunk128", None, 0), ("pos256", None, 0), ("prompt300", None, 0), ("ragged-K", None, 0),
              ("medium", None, 0), ("vocab-max", None, 0), ("vocab-57345", None, 0),
              ("floor", 1, 0), ("floor", 4, 0), ("floor", 5, 0), ("floor", 8, 0), ("chunk128", None, 4), ("chunk128", None, 8)]


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name,nb,grid_cap", STEP_CASES)
def test_step_and_selection(name, nb, grid_cap, dtype):
    run_case(name, dtype, nb=nb, grid_cap=grid_cap)


def test_grid_cap_too_small_for_the_vocabulary_is_refused():
    """the issue's `grid_cap = 3` on the V = 1000 model needs 352 vocabulary rows per workgroup, more than the 256 a slice holds:
    the entry point refuses it (CCLIP_ERR_ARG) and touches nothing; grid_cap = 4 (256 rows: every lane value live) is the
    smallest grid this vocabulary runs on and is a case of test_step_and_selection"""
    from cclip_hip._lib import CclipError
    h = Single("chunk128", torch.bfloat16, 3, 126, 0, grid_cap=3)
    pre = h.read()
    with pytest.raises(CclipError):
        h.launch(126, 0, first_logits=torch.zeros(h.m.V))
    post = h.read()
    assert torch.equal(pre.tokens, post.tokens) and torch.equal(pre.slot, post.slot) and post.state == pre.state


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
def test_search_ends_at_max_len(dtype):
    """pos0 = 60 of 64 positions, 6 steps requested: steps at 60..63, the last without a next input row (has_next false), then two
    launches past the cache that change nothing; one launch asked for all 6 steps ends in the same state; guard rows intact"""
    h, post = run_case("end", dtype)
    assert post.state[4] == 5 and post.state[2] == 0
    c = R.CASES["end"]
    h2 = Single("end", dtype, c["beams"], c["pos0"], 0)
    fl = torch.randn(h2.m.V, generator=torch.Generator().manual_seed(1)) * 2.0
    h2.launch(c["pos0"], 0, first_logits=fl)
    h2.launch(c["pos0"], 6, want_logits=False)
    p2 = h2.read()
    for f in ("tokens", "scores", "seq_len", "stopped", "slot", "k", "v"):
        assert torch.equal(getattr(post, f), getattr(p2, f)), f
    assert h2.guards_intact() and p2.state[4] == 5


# ---- (c) crafted first selections ------------------------------------------------------------------------------------------
def slice_rows(V, grid_cap=0):
    """vocabulary rows per workgroup slice, as persist_grid chooses them"""
    G = min(max((V + 223) // 224, 96), 256, torch.cuda.get_device_properties(0).multi_processor_count)
    if grid_cap:
        G = min(G, grid_cap)
    return (-(-V // G) + 31) // 32 * 32


def crafted(kind, V, Rw, k, seed):
    """(logits [V], stop token): multiples of 0.5 (exact at T = 0.5); ties are decided by the index rule"""
    g = torch.Generator().manual_seed(seed)
    lg = 0.5 * torch.randint(-24, -12, (V,), generator=g).double()
    stop = -1
    if kind == "ties":           # across a slice boundary, inside one lane's four values (rows j, j + 64 of a slice), at the tail
        same_lane = Rw + 5 + 64 if Rw > 64 else Rw + 6
        lg[[Rw - 1, Rw, Rw + 5, same_lane, V - 2, V - 1]] = 3.0
        lg[1], lg[2] = 2.5, 2.0
    elif kind == "stop_best":
        lg[17], lg[40], lg[3] = 4.0, 3.0, 2.5
        stop = 17
    elif kind == "sparse":       # -inf on all but 8 k entries
        idx = torch.randperm(V, generator=g)[:8 * k]
        val = 0.5 * torch.randperm(8 * k, generator=g).double() - 6.0
        lg[:] = -math.inf
        lg[idx] = val
    elif kind == "one_slice":    # the top 8 inside one slice
        idx = 2 * Rw + torch.randperm(min(Rw, V - 2 * Rw), generator=g)[:8]
        lg[idx] = 0.5 * torch.randperm(8, generator=g).double() + 1.0
    elif kind == "spread":       # the top 8 over 8 slices
        idx = torch.arange(8) * Rw + torch.randint(0, min(Rw, V - 7 * Rw), (8,), generator=g)
        lg[idx] = 0.5 * torch.randperm(8, generator=g).double() + 1.0
    return lg, stop


# (kind, k, seed of the background).  Every logit / T is an integer here, so every log-probability is an integer minus ONE
# log-sum-exp and the float32-against-float64 difference d32 of a row is a sample of that single number's rounding: it can fall
# to nothing.  A float32 evaluation through exp, a division and log, each good to one ulp, can be more than one ulp of the
# score off, so a seed is admissible only if the reference's tolerance 8 d32 is at least two ulps of the row's largest winning
# score; the test asserts this on the reference before it launches.
CRAFTED = [("ties", 3, 3), ("ties", 8, 4), ("stop_best", 1, 5), ("stop_best", 3, 6), ("sparse", 3, 7), ("sparse", 8, 8), ("one_slice", 8, 9),
           ("spread", 8, 11)]


def crafted_seed_admissible(lg, stop, k):
    """the reference alone: 8 d32 of the crafted row against two float32 ulps of its largest winning score"""
    sel = R.select_ref(lg, torch.zeros(k), torch.ones(k), torch.zeros(k), torch.zeros(1, 0, dtype=torch.long),
                       torch.zeros(64, 8, dtype=torch.int32), 4, T, stop, True)
    ulp = 2.0 ** (math.floor(math.log2(sel.scores.abs().max().item())) - 23)
    return 8 * sel.d32 >= 2 * ulp


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["floor", "vocab-max", "vocab-57345"])
def test_crafted_first_selection(name, dtype):
    """n_steps = 0 on both kernels: the one-caption kernel case by case, the batched kernel on the same rows as captions of one
    launch; expected state from select_ref with no ambiguity allowed"""
    m, d, arr = get_model(name, dtype)
    Rw, pos0 = slice_rows(m.V), 5
    for k in sorted({k for _, k, _ in CRAFTED}):
        rows = [crafted(kind, m.V, Rw, k, seed) + (kind,) for kind, kk, seed in CRAFTED if kk == k]
        want = []
        for lg, stop, kind in rows:
            assert crafted_seed_admissible(lg, stop, k), f"{kind} k={k}: d32 of this seed is below the scores' float32 spacing"
            h = Single(name, dtype, k, pos0, 0, stop=stop, n_tokens=4)
            pre = h.read()
            h.launch(pos0, 0, first_logits=lg, want_logits=False)
            post = h.read()
            assert check_selection(m, lg, pre, post, pos0 - 1, stop, True, 0), f"{kind} k={k}: ambiguous"
            assert post.state[2] == int(k == 1 and stop >= 0) and h.guards_intact()
            if kind == "stop_best":
                assert post.tokens[0, 0] == stop and bool(post.stopped[0]) and post.seq_len[0] == 1 and not post.stopped[1:].any()
            if kind == "ties":
                same_lane = Rw + 5 + 64 if Rw > 64 else Rw + 6
                assert post.tokens[:, 0].tolist() == [Rw - 1, Rw, Rw + 5, same_lane, m.V - 2, m.V - 1, 1, 2][:k]
            want.append(post)
        # the batched kernel: captions with different rows (one stop token per launch: the rows that share it)
        for stop in sorted({s for _, s, _ in rows}):
            sel = [i for i, r in enumerate(rows) if r[1] == stop]
            nc = len(sel)
            bst = ops().BeamBatchState(nc, k, m.max_len, 1, "cuda")
            kc = torch.zeros(m.n_layer, nc * k, m.max_len, m.D, device="cuda", dtype=dtype)
            vc = torch.zeros_like(kc)
            scratch = torch.empty(nc * k * (5 * m.D + m.Hd), device="cuda", dtype=dtype)
            fl = torch.stack([rows[i][0] for i in sel]).float().contiguous().cuda()
            ops().gpt2_beam_search_batch(arr, m.n_layer, bst, kc, vc, pos0, scratch, 0, heads=m.heads, hidden=m.Hd, act=ops().ACT_GELU_NEW,
                                         lnf_w=d.lnf_w, lnf_b=d.lnf_b, wte16=d.wte16, wte_f32=d.wte, wpe_f32=d.wpe, temperature=T,
                                         stop_token=stop, first_logits=fl)
            torch.cuda.synchronize()
            assert bst.state.tolist()[1] == 0, "a phase hand-over of the batched kernel timed out"
            cap_state = bst.cap_state.tolist()
            for j, i in enumerate(sel):
                w = want[i]                                            # the one-caption kernel's state, already equal to select_ref's
                rs = slice(j * k, (j + 1) * k)
                assert torch.equal(bst.tokens[rs, :1].cpu().long(), w.tokens[:, :1]), (rows[i][2], k)
                assert torch.equal(bst.scores[rs].cpu().double(), w.scores) and torch.equal(bst.seq_lengths[rs].cpu().double(), w.seq_len)
                assert torch.equal(bst.is_stopped[rs].cpu().bool(), w.stopped) and torch.equal(bst.x[rs].cpu(), w.x)
                assert torch.equal(bst.slot_of[j].cpu(), w.slot) and cap_state[j][4] == 1 and cap_state[j][2] == w.state[2]
            assert not kc.any() and not vc.any()                       # no step: the cache is untouched


# ---- (d) stopped beams ------------------------------------------------------------------------------------------------------
def _poke(h, stopped, scores, lengths):
    h.st.is_stopped.copy_(torch.tensor(stopped, dtype=torch.int32))
    h.st.scores.copy_(torch.tensor(scores, dtype=torch.float32))
    h.st.seq_lengths.copy_(torch.tensor(lengths, dtype=torch.float32))


def _snapshot(h):
    st = h.st
    return [t.clone() for t in (st.x, st.tokens, st.scores, st.seq_lengths, st.is_stopped, st.slot_of, st.state)]


def _restore(h, snap):
    st = h.st
    for t, s in zip((st.x, st.tokens, st.scores, st.seq_lengths, st.is_stopped, st.slot_of, st.state), snap):
        t.copy_(s)


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("nb,stopped", [(3, [0]), (3, [2]), (3, [0, 2]), (8, [0, 1, 2, 4, 5, 6, 7])])
def test_stopped_beams(nb, stopped, dtype):
    """is_stopped / scores / seq_lengths overwritten between launches, then ONE step from the same state per variant: the stopped
    beams' one candidate (column 0 at their unchanged length) wins, loses, and exactly ties the best live candidate."""
    pos0 = 5
    h = Single("floor", dtype, nb, pos0, 0, n_tokens=8)
    m = h.m
    h.launch(pos0, 0, first_logits=torch.randn(m.V, generator=torch.Generator().manual_seed(2)) * 2.0)
    h.launch(pos0, 1)
    pos, ntok = pos0 + 1, 2
    flags = [int(b in stopped) for b in range(nb)]
    live_score = [-1.0 - 0.25 * b for b in range(nb)]
    base = _snapshot(h)

    def one_step(scores, lengths):
        _restore(h, base)
        _poke(h, flags, scores, lengths)
        pre = h.read()
        h.launch(pos, 1)
        return pre, h.read(), h.logits.cpu().double()
    # wins: an average no live candidate can reach; loses: far below every live candidate
    for variant, sc in (("wins", -0.01), ("loses", -1000.0)):
        scores = [sc - 0.001 * b if f else live_score[b] for b, f in enumerate(flags)]
        pre, post, lg = one_step(scores, [2.0] * nb)
        assert check_selection(m, lg, pre, post, pos, -1, False, ntok), variant
        if variant == "wins":
            for i, b in enumerate(stopped[:nb]):                       # best first: the stopped beams in their order, length kept
                assert post.tokens[i, ntok] == 0 and post.seq_len[i] == 2 and bool(post.stopped[i]) and post.slot[pos, i] == b
        else:
            assert not post.stopped.any() and (post.seq_len == 3).all()     # every winner extends a live beam
    # exact tie.  Live lengths 3 -> 4 after the step, so the best live candidate's score read back is 4 * its average exactly;
    # the stopped beam `tie` (length 1) gets that average as its score: the kernel, which is deterministic, then sees two
    # bit-equal candidates and must take the lower flat index first.
    lens = [1.0 if f else 3.0 for f in flags]
    scores = [-1000.0 if f else live_score[b] for b, f in enumerate(flags)]
    pre, post, lg = one_step(scores, lens)
    assert post.seq_len[0] == 4 and not post.stopped[0]
    best_avg, best_tok, best_src = post.scores[0].item() / 4.0, int(post.tokens[0, ntok]), int(post.slot[pos, 0])
    tie = stopped[0]
    scores[tie] = best_avg
    pre, post, lg2 = one_step(scores, lens)
    assert torch.equal(lg, lg2), "the step is not reproducible from the same state"
    first_two = sorted([(tie * m.V, 0, tie, 1.0), (best_src * m.V + best_tok, best_tok, best_src, 4.0)])
    for i, (_, tok, src, ln) in enumerate(first_two):
        assert post.tokens[i, ntok] == tok and post.slot[pos, i] == src and post.seq_len[i] == ln, (i, first_two, post.tokens[:, ntok])
    assert post.scores[0] / post.seq_len[0] == post.scores[1] / post.seq_len[1] == best_avg
    # the whole state against select_ref.  In float64 the two tied candidates are a float32 rounding apart, so select_ref may order
    # them either way; its first two winners are put in the order of the flat index (the tie rule), everything else is as in (b)
    sel = R.select_ref(lg, pre.scores, pre.seq_len, pre.stopped, pre.tokens[:, :ntok], pre.slot, pos, T, -1, False, m)
    assert sorted(zip(sel.src[:2].tolist(), sel.tokens[:2, ntok].tolist())) == sorted((s_, t_) for _, t_, s_, _ in first_two)
    if sel.src[0] * m.V + sel.tokens[0, ntok] > sel.src[1] * m.V + sel.tokens[1, ntok]:
        swap = torch.arange(nb)
        swap[0], swap[1] = 1, 0
        sel.tokens, sel.scores, sel.seq_len, sel.stopped, sel.x = sel.tokens[swap], sel.scores[swap], sel.seq_len[swap], sel.stopped[swap], sel.x[swap]
        sel.slot_of[:pos + 1, :nb] = sel.slot_of[:pos + 1, :nb][:, swap]
    compare_selection(sel, post, pos, ntok, 8 * sel.d32)


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
def test_all_beams_stopped(dtype):
    pos0 = 5
    h = Single("floor", dtype, 3, pos0, 0, n_tokens=8)
    h.launch(pos0, 0, first_logits=torch.randn(h.m.V, generator=torch.Generator().manual_seed(2)) * 2.0)
    _poke(h, [1, 1, 1], [-1.0, -2.0, -3.0], [1.0, 1.0, 1.0])
    pre = h.read()
    state = h.launch(pos0, 1)
    post = h.read()
    assert check_selection(h.m, h.logits.cpu().double(), pre, post, pos0, -1, False, 1)
    assert state[2] == 1 and state[3] == 1 and post.tokens[:, 1].tolist() == [0, 0, 0] and post.seq_len.tolist() == [1, 1, 1]
    state = h.launch(pos0 + 1, 1)                                      # the search is over: nothing may change
    last = h.read()
    for f in ("tokens", "scores", "seq_len", "stopped", "slot", "k", "v", "x"):
        assert torch.equal(getattr(post, f), getattr(last, f)), f
    assert state[2:5] == post.state[2:5]


# ---- (e) the batched kernel and the native driver ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("n_cap,nb", [(1, 1), (17, 1), (16, 3), (8, 8)])
@pytest.mark.parametrize("name", ["chunk128", "ragged-K"])
def test_batched_kernel(name, n_cap, nb, dtype):
    """gpt2_beam_search_batch, 3 steps in one launch, replayed in float64 with its own tokens along every final beam's ancestry (the
    slot table names the cache rows): the last layer's appended k / v rows within the bound of (a), final scores within
    8 d32 + sum of 2 d_round / T (the kernel's logits are not output; a log-probability moves by at most twice the logits'
    deviation over T, taken at the size of the 16-bit rounding the reference measures, without the headroom of (a)), and caption
    c's tokens equal to the one-caption kernel's on caption c alone, for every caption."""
    m, d, arr = get_model(name, dtype)
    c = R.CASES[name]
    pos0, steps, Rn = c["pos0"], 3, n_cap * nb
    kc0, vc0 = R.fill_cache(m, Rn, pos0, 5, filled_slots=[i * nb for i in range(n_cap)])
    first = torch.randn(n_cap, m.V, generator=torch.Generator().manual_seed(6)) * 2.0
    kc, vc = kc0.cuda(), vc0.cuda()
    bst = ops().BeamBatchState(n_cap, nb, m.max_len, steps + 1, "cuda")
    scratch = torch.empty(Rn * (5 * m.D + m.Hd), device="cuda", dtype=dtype)
    ops().gpt2_beam_search_batch(arr, m.n_layer, bst, kc, vc, pos0, scratch, steps, heads=m.heads, hidden=m.Hd, act=ops().ACT_GELU_NEW,
                                 lnf_w=d.lnf_w, lnf_b=d.lnf_b, wte16=d.wte16, wte_f32=d.wte, wpe_f32=d.wpe, temperature=T, stop_token=-1,
                                 first_logits=first.contiguous().cuda())
    torch.cuda.synchronize()
    assert bst.state.tolist()[1] == 0, "a phase hand-over of the batched kernel timed out"
    tokens, scores, slot = bst.tokens.cpu().long(), bst.scores.cpu().double(), bst.slot_of.cpu()
    K, Vc = kc.cpu(), vc.cpu()
    assert (bst.seq_lengths.cpu() == steps + 1).all() and not bst.is_stopped.any()
    l = m.n_layer - 1
    k_max = max(m.D, m.Hd)
    ratio, reordered = 0.0, 0
    for cap in range(n_cap):
        rs = slice(cap * nb, (cap + 1) * nb)
        tk, sl = tokens[rs], slot[cap]
        lp = (first[cap].double() / T).softmax(-1).log()
        ref_score, tol = lp[tk[:, 0]].clone(), 0.0
        d32 = 0.0
        for s in range(steps):
            pos = pos0 + s
            x = m.embed(tk[:, s], pos)
            exact = R.step_ref(m, x, K[:, rs], Vc[:, rs], sl, pos, False)
            rnd = R.step_ref(m, x, K[:, rs], Vc[:, rs], sl, pos, True)
            own = sl[pos, :nb].long()                                  # the slot each final beam's ancestor appended to
            for got, e, r in ((K[l, rs][own, pos], exact[2][l], rnd[2][l]), (Vc[l, rs][own, pos], exact[3][l], rnd[3][l])):
                bound, d_round = R.step_bound(e, r, k_max)
                err = (got.double() - e).abs().max().item()
                ratio = max(ratio, err / d_round)
                assert err <= bound, (cap, pos, err, bound)
            d_round = R.step_bound(exact[0], rnd[0], k_max)[1]
            lp = (exact[0] / T).softmax(-1).log()
            l32 = (exact[0].float() / T).softmax(-1).log()
            d32 = max(d32, (l32.double() - lp).abs()[torch.arange(nb), tk[:, s + 1]].max().item())
            ref_score += lp[torch.arange(nb), tk[:, s + 1]]
            tol += 2 * d_round / T
        err = (scores[rs] - ref_score).abs().max().item()
        assert err <= 8 * max(d32, 2.0 ** -24 * ref_score.abs().max().item()) + tol, (cap, err, tol)
        print(f"  caption {cap}: score err {err:.3e} tol {8 * d32 + tol:.3e}")
        # the one-caption kernel on this caption alone: the same tokens, whatever the margins (the two kernels share one core)
        cache = (kc0[:, cap * nb:(cap + 1) * nb], vc0[:, cap * nb:(cap + 1) * nb])
        h = Single(name, dtype, nb, pos0, 0, n_tokens=steps + 1, cache=cache)
        h.launch(pos0, 0, first_logits=first[cap], want_logits=False)
        h.launch(pos0, steps, want_logits=False)
        one = h.read()
        assert torch.equal(one.tokens[:, :steps + 1], tk), (cap, one.tokens, tk)
        assert torch.equal(one.seq_len, torch.full((nb,), steps + 1.0, dtype=torch.float64))
        reordered += int(any(sl[pos0 + s, :nb].tolist() != list(range(nb)) for s in range(steps)))
    assert nb == 1 or reordered > 0                                    # some caption's beams changed places
    print(f"RATIOS batch-{name} {str(dtype)[6:]} n_cap={n_cap} nb={nb}: kv={ratio:.2f} captions reordered {reordered}/{n_cap}")


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("rows", [1, 5, 8])
@pytest.mark.parametrize("name", ["floor", "ragged-K", "medium"])
def test_native_decode_step(name, rows, dtype):
    """gpt2_decode_step (the stand-alone skinny kernels, one launch each): logits, appended k / v rows and the residual stream of
    `rows` sequences, each with its own cache slot, within the bound of (a)"""
    m, d, arr = get_model(name, dtype)
    pos = R.CASES[name]["pos0"]
    kc, vc = R.fill_cache(m, rows, pos, 11, filled_slots=range(rows))
    kbuf, k = guarded_cache(kc)
    vbuf, v = guarded_cache(vc)
    x0 = torch.randn(rows, m.D, generator=torch.Generator().manual_seed(12)) * 0.3
    x = x0.cuda()
    logits = torch.full((rows, (m.V + 7) // 8 * 8), float("nan"), device="cuda")[:, :m.V]
    scratch = torch.empty(rows * (5 * m.D + m.Hd), device="cuda", dtype=dtype)
    ops().gpt2_decode_step(arr, m.n_layer, x, k, v, pos, scratch, heads=m.heads, hidden=m.Hd, act=ops().ACT_GELU_NEW, linear_layout=False,
                           lnf_w=d.lnf_w, lnf_b=d.lnf_b, wte16=d.wte16, logits=logits)
    torch.cuda.synchronize()
    slot = torch.arange(8, dtype=torch.int32).repeat(m.max_len, 1)
    pre = SimpleNamespace(x=x0, k=kc, v=vc, slot=slot)
    got = {"logits": logits.cpu().double(), "x": x.cpu()}
    for l in range(m.n_layer):
        got[f"k{l}"], got[f"v{l}"] = k[l, :, pos].cpu(), v[l, :, pos].cpu()
    ratios = {}
    check_step(m, got, pre, pos, ratios)
    assert bool((kbuf[:, :, m.max_len:] == SENT).all() and (vbuf[:, :, m.max_len:] == SENT).all())
    print(f"RATIOS driver-{name} {str(dtype)[6:]} rows={rows}: " + " ".join(f"{k_}={v_:.2f}" for k_, v_ in sorted(ratios.items())))
