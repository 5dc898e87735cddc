"""A plain float64 reference of what the decode kernels compute (csrc/decode_persist*.hip, gemm_skinny_impl.h,
decode_driver.hip): one KV-cached GPT-2 step for a few rows (`step_ref`) and the beam selection that follows it (`select_ref`,
the generate_beam loop body that select_merge cites), on synthetic Conv1D-layout weights (`SynthGPT2`).  Helper module of
tests/test_decode_ref_cpu.py (which checks this reference itself) and tests/test_decode_kernels_gpu.py; torch on the CPU only.

Rounding points of the kernels, reproduced by step_ref(rounded=True): the LayerNorm outputs (LN1, LN2, LN_f), the packed qkv row
and with it the cached k / v rows, the attention output and the MLP hidden row are rounded to the 16-bit operand type; the
residual stream x, the softmax and the logits stay fp32 in the kernels and so unrounded here.
"""
import math
from types import SimpleNamespace

import torch

F64 = torch.float64
BLOCK_FIELDS = ("ln1_w", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_w", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj")
MUTATIONS = ("drop_last_key", "slot0", "drop_k768", "no_rescale", "ln960", "tail_identity")

# name: D, Hd, layers, V, max_len, pos0, beams, steps (the issue's table; `beams` / `grid` / `vocab` variants are made by the tests)
CASES = {
    "floor": dict(D=64, Hd=32, L=1, V=300, max_len=64, pos0=5, beams=3, steps=5),
    "chunk128": dict(D=128, Hd=512, L=2, V=1000, max_len=320, pos0=126, beams=3, steps=5),
    "pos256": dict(D=128, Hd=512, L=2, V=1000, max_len=320, pos0=254, beams=3, steps=5),
    "prompt300": dict(D=128, Hd=512, L=2, V=1000, max_len=320, pos0=20, beams=3, steps=4, prompt=300),
    "ragged-K": dict(D=832, Hd=1056, L=1, V=300, max_len=64, pos0=5, beams=3, steps=4),
    "medium": dict(D=1024, Hd=4096, L=1, V=2048, max_len=64, pos0=5, beams=3, steps=4),
    "vocab-max": dict(D=64, Hd=32, L=1, V=65536, max_len=64, pos0=3, beams=3, steps=4),
    "vocab-57345": dict(D=64, Hd=32, L=1, V=57345, max_len=64, pos0=3, beams=3, steps=4),
    "end": dict(D=64, Hd=32, L=1, V=300, max_len=64, pos0=60, beams=3, steps=6),
}


def case_model(name, dtype, seed=0):
    c = CASES[name]
    return SynthGPT2(c["D"], c["Hd"], c["L"], c["V"], c["max_len"], dtype, seed)


class SynthGPT2:
    """Random GPT-2 weights in the layout the decode kernels read: Conv1D [in, out] 16-bit matrices, fp32 biases and LayerNorm
    parameters, a 16-bit lm_head (`wte16`) next to the fp32 embedding tables.  Standard deviations are those of
    clip_caption.weights.init_caption_state_dict, except the head: 2 / sqrt(D), so that the logits have a spread of about two units
    (the kernels take the head and the fp32 input table `wte` as separate arguments; here they are independent draws: with
    one table behind both, the row of a beam's last token dominates its hidden state, its own logit is about 2 sqrt(D), every
    beam repeats its token and no selection ever reorders the beams), and the query bias: 4, so that the attention is sharp (scores spread by about one unit over keys of the size of the model's
    own) - under the near-uniform softmax of 0.02-sized projections a wrong key or a wrong rescale would move the output by less
    than its 16-bit rounding."""

    def __init__(self, D, Hd, n_layer, V, max_len, dtype, seed):
        assert D % 64 == 0 and Hd % 32 == 0
        self.D, self.Hd, self.n_layer, self.V, self.max_len, self.dtype, self.heads = D, Hd, n_layer, V, max_len, dtype, D // 64
        g = torch.Generator().manual_seed(seed)

        def rn(*shape, std):
            return torch.randn(*shape, generator=g) * std
        self.blocks = []
        for _ in range(n_layer):
            self.blocks.append(SimpleNamespace(
                ln1_w=1.0 + rn(D, std=0.1), ln1_b=rn(D, std=0.1),
                w_qkv=rn(D, 3 * D, std=0.02).to(dtype), b_qkv=rn(3 * D, std=0.02) + torch.cat((rn(D, std=4.0), torch.zeros(2 * D))),
                w_o=rn(D, D, std=0.02 / math.sqrt(2 * n_layer)).to(dtype), b_o=rn(D, std=0.02),
                ln2_w=1.0 + rn(D, std=0.1), ln2_b=rn(D, std=0.1),
                w_fc=rn(D, Hd, std=0.02).to(dtype), b_fc=rn(Hd, std=0.02),
                w_proj=rn(Hd, D, std=0.02 / math.sqrt(2 * n_layer)).to(dtype), b_proj=rn(D, std=0.02)))
        self.lnf_w, self.lnf_b = 1.0 + rn(D, std=0.1), rn(D, std=0.1)
        self.wte16 = rn(V, D, std=2.0 / math.sqrt(D)).to(dtype)
        self.wpe = rn(max_len, D, std=0.02)
        self.wte = rn(V, D, std=0.02)
        self._b64 = None

    @property
    def blocks64(self):
        if self._b64 is None:
            self._b64 = [SimpleNamespace(**{n: getattr(b, n).to(F64) for n in BLOCK_FIELDS}) for b in self.blocks]
            self._head64 = (self.lnf_w.to(F64), self.lnf_b.to(F64), self.wte16.to(F64))
        return self._b64

    def to_device(self, device="cuda"):
        """the same weights on the device: .blocks carry the twelve BlockPtrs fields (for ops.block_ptr_array)"""
        d = SimpleNamespace(blocks=[SimpleNamespace(**{n: getattr(b, n).to(device).contiguous() for n in BLOCK_FIELDS}) for b in self.blocks])
        for n in ("lnf_w", "lnf_b", "wte", "wte16", "wpe"):
            setattr(d, n, getattr(self, n).to(device).contiguous())
        return d

    def oracle_state_dict(self):
        """the weights under the keys oracle.caption_oracle.gpt2_forward reads (the 16-bit matrices as they are; lm_head = wte16)"""
        p = "model.transformer."
        sd = {p + "wte.weight": self.wte16, p + "wpe.weight": self.wpe, p + "ln_f.weight": self.lnf_w, p + "ln_f.bias": self.lnf_b}
        names = dict(ln1_w="ln_1.weight", ln1_b="ln_1.bias", w_qkv="attn.c_attn.weight", b_qkv="attn.c_attn.bias", w_o="attn.c_proj.weight",
                     b_o="attn.c_proj.bias", ln2_w="ln_2.weight", ln2_b="ln_2.bias", w_fc="mlp.c_fc.weight", b_fc="mlp.c_fc.bias",
                     w_proj="mlp.c_proj.weight", b_proj="mlp.c_proj.bias")
        for i, b in enumerate(self.blocks):
            for n, key in names.items():
                sd[f"{p}h.{i}.{key}"] = getattr(b, n)
        return sd

    def embed(self, tok, pos):
        """the kernels' next input row: wte[tok] + wpe[pos], ONE fp32 add"""
        return self.wte[tok.long()] + self.wpe[pos]


def fill_cache(model, n_slots, pos0, seed, filled_slots=(0,)):
    """(kcache, vcache) [layers, n_slots, max_len, D] in the model's 16-bit type, zero except positions < pos0 of `filled_slots`:
    random keys (std 0.1: somewhat below the model's own 0.25, so that the newest keys can hold the softmax maximum) and values of std 1"""
    g = torch.Generator().manual_seed(seed)
    k = torch.zeros(model.n_layer, n_slots, model.max_len, model.D, dtype=model.dtype)
    v = torch.zeros_like(k)
    for s in filled_slots:
        k[:, s, :pos0] = (torch.randn(model.n_layer, pos0, model.D, generator=g) * 0.1).to(model.dtype)
        v[:, s, :pos0] = torch.randn(model.n_layer, pos0, model.D, generator=g).to(model.dtype)
    return k, v


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def _ln(x, w, b, mutate):
    xs = x[:, :min(x.shape[1], 960)] if mutate == "ln960" else x
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * w + b


def _mm(a, w, mutate):
    if mutate == "drop_k768" and w.shape[0] > 768:
        return a[:, :768] @ w[:768]
    return a @ w


def _attend(q, keys, vals, mutate):
    """q [H, 64], keys / vals [S, H, 64] -> [H, 64]: softmax(q . k / 8) v.  `no_rescale` walks the 128-key chunks of the kernel's
    online softmax and leaves the first chunk's accumulator unscaled when the second chunk raises the running maximum."""
    sc = torch.einsum("hd,shd->hs", q, keys) * 0.125
    if mutate != "no_rescale":
        return torch.einsum("hs,shd->hd", torch.softmax(sc, -1), vals)
    S = sc.shape[1]
    m = torch.full((sc.shape[0],), -math.inf, dtype=F64)
    l = torch.zeros_like(m)
    o = torch.zeros(sc.shape[0], 64, dtype=F64)
    for ci, c0 in enumerate(range(0, S, 128)):
        s = sc[:, c0:c0 + 128]
        mn = torch.maximum(m, s.max(-1).values)
        resc = torch.exp(m - mn)
        e = torch.exp(s - mn[:, None])
        l = l * resc + e.sum(-1)
        o = o * (1.0 if ci == 1 else resc[:, None]) + torch.einsum("hs,shd->hd", e, vals[c0:c0 + 128])
        m = mn
    return o / l[:, None]


def step_ref(model, x, kcache, vcache, slot_of, pos, rounded, mutate=None):
    """One decode step of x.shape[0] rows at position `pos` in float64.  Row b appends its key / value at `pos` and attends to
    positions 0..pos: position t < pos is read from cache slot slot_of[t][b] (kcache / vcache [layers, slots, max_len, D] hold what
    the kernel's cache holds), position pos is the row's own new key / value.  rounded: round to the model's 16-bit type where
    the kernels do (module docstring).  mutate: one of MUTATIONS, the deliberately wrong variants of the teeth tests.
    Returns (logits [nb, V], new x [nb, D], appended k rows [layers, nb, D], appended v rows [layers, nb, D]); inputs unchanged."""
    assert mutate is None or mutate in MUTATIONS
    x = x.to(F64).clone()
    nb, D = x.shape
    H = D // 64
    blocks = model.blocks64
    lnf_w, lnf_b, wte16 = model._head64
    r = (lambda t: t.float().to(model.dtype).to(F64)) if rounded else (lambda t: t)
    tpos = torch.arange(pos)
    k_rows, v_rows = [], []
    for l, w in enumerate(blocks):
        h = r(_ln(x, w.ln1_w, w.ln1_b, mutate))
        qkv = r(_mm(h, w.w_qkv, mutate) + w.b_qkv)
        q, k, v = qkv.split(D, dim=-1)
        k_rows.append(k)
        v_rows.append(v)
        att = torch.empty(nb, D, dtype=F64)
        for b in range(nb):
            slots = torch.zeros(pos, dtype=torch.long) if mutate == "slot0" else slot_of[:pos, b].long()
            if mutate == "tail_identity":                               # the table as a selection leaves it that skips its rows past 256
                slots[256:] = b
            keys = torch.cat((kcache[l][slots, tpos].to(F64), k[b:b + 1]))
            vals = torch.cat((vcache[l][slots, tpos].to(F64), v[b:b + 1]))
            if mutate == "drop_last_key" and pos > 0:
                keys, vals = keys[:-1], vals[:-1]
            att[b] = _attend(q[b].view(H, 64), keys.view(-1, H, 64), vals.view(-1, H, 64), mutate).reshape(D)
        x = x + _mm(r(att), w.w_o, mutate) + w.b_o
        h = r(_ln(x, w.ln2_w, w.ln2_b, mutate))
        g = r(gelu_new(_mm(h, w.w_fc, mutate) + w.b_fc))
        x = x + _mm(g, w.w_proj, mutate) + w.b_proj
    logits = r(_ln(x, lnf_w, lnf_b, mutate)) @ wte16.t()
    return logits, x, torch.stack(k_rows), torch.stack(v_rows)


def step_bound(exact, rnd, k_max):
    """the bound of the step arithmetic, per compared tensor: 3 x the 16-bit rounding at the kernels' own rounding points, as the
    reference measures it (rounded - exact), + fp32 accumulation order over the longest contraction; returns (bound, d_round)"""
    d_round = (rnd - exact).abs().max().item()
    return 3.0 * d_round + 2.0 ** -22 * k_max * exact.abs().max().item(), d_round


def step_outputs(res):
    """the compared tensors of a step_ref result, by name"""
    logits, x, k, v = res
    out = {"logits": logits, "x": x}
    for l in range(k.shape[0]):
        out[f"k{l}"], out[f"v{l}"] = k[l], v[l]
    return out


def _cand(logits, scores, seq_len, stopped, T, first, dt):
    """the candidate table of the generate_beam loop body in type dt: (averages [rows, V], lengths after the step [rows])"""
    lp = (logits.to(dt) / T).softmax(-1).log()
    if first:
        return lp / 1.0, torch.ones(1, dtype=dt)
    stopped = stopped.bool()
    lp[stopped] = -math.inf
    lp[stopped, 0] = 0
    new_len = seq_len.to(dt).clone()
    new_len[~stopped] += 1
    return (scores.to(dt)[:, None] + lp) / new_len[:, None], new_len


def select_ref(logits, scores, seq_len, stopped, tokens, slot_of, pos, T, stop_token, first, model=None):
    """The selection after the step at position `pos` (first: the one-row selection on the prefill's logits, pos = pos0 - 1),
    in float64: logits / T, softmax, log; stopped rows -inf with column 0 = 0; seq_len[~stopped] += 1 (not first);
    (scores + lp) / seq_len; top-k (k = beams = len(scores)) of the flattened table, equal values in the order of the flat
    index; token append; slot-table permutation and the identity row at pos + 1; stop flags; next x = wte[tok] + wpe[pos + 1].
    tokens: [beams, columns so far] (first: row 0 is the prompt).  Returns a namespace: tokens, src, scores, seq_len, stopped,
    slot_of, x (None past max_len or without a model), all_stopped, margin, d32.
    margin: the smallest gap between two consecutive values among the first k + 1 candidates; a zero gap between two candidates
    of the SAME row with bit-equal logits is an exact tie in every precision (same operations on the same inputs), decided by
    the index rule, and does not count.  d32: the largest difference between the literal float32 torch evaluation of the
    candidates' averages / scores and the float64 one."""
    k = scores.shape[0]
    logits = logits.reshape(-1, logits.shape[-1])
    V = logits.shape[1]
    avg, new_len = _cand(logits, scores, seq_len, stopped, T, first, F64)
    a32, l32 = _cand(logits, scores, seq_len, stopped, T, first, torch.float32)
    fin = torch.isfinite(avg)
    d32 = max((a32.to(F64) - avg)[fin].abs().max().item(), ((a32 * l32[:, None]).to(F64) - avg * new_len[:, None])[fin].abs().max().item())
    flat = avg.reshape(-1)
    val, idx = torch.sort(flat, descending=True, stable=True)          # stable: equal values keep the order of the flat index
    val, idx = val[:k + 1], idx[:k + 1]
    assert torch.isfinite(val[:k]).all(), "fewer than k finite candidates"
    margin = math.inf
    for i in range(min(k, val.numel() - 1)):
        gap = (val[i] - val[i + 1]).item() if torch.isfinite(val[i + 1]) else math.inf
        ri, rj = int(idx[i]) // V, int(idx[i + 1]) // V
        if gap == 0.0 and ri == rj and logits[ri, int(idx[i]) % V] == logits[rj, int(idx[i + 1]) % V]:
            continue
        margin = min(margin, gap)
    top = idx[:k]
    src, tok = top // V, top % V
    out_len = new_len[src]
    old_stop = torch.zeros(1, dtype=torch.bool) if first else stopped.bool()
    new_stop = old_stop[src] | tok.eq(stop_token)
    new_tokens = torch.cat((tokens[src].long(), tok[:, None]), dim=1)
    slot = slot_of.clone()
    if not first:
        slot[:pos + 1, :k] = slot_of[:pos + 1][:, src]
    nxt = pos + 1
    x = None
    if nxt < slot.shape[0]:
        slot[nxt, :k] = torch.arange(k, dtype=slot.dtype)
        if model is not None:
            x = model.embed(tok, nxt)
    return SimpleNamespace(tokens=new_tokens, src=src, scores=val[:k] * out_len, seq_len=out_len, stopped=new_stop, slot_of=slot, x=x,
                           all_stopped=bool(new_stop.all()), margin=margin, d32=d32)


def reordered(src):
    """a selection's sources are not the identity: the slot table was permuted"""
    return src.tolist() != list(range(src.numel()))


def simulate(model, name, seed, mutate=None):
    """The search of CASES[name] with step_ref(rounded=True) standing in for the kernel (the CPU-side stand-in of the GPU
    harness).  Yields, per step, (pos, pre-step x, kcache, vcache, slot table, the sources of the selection that made this state);
    the state advances by the UNMUTATED step."""
    c = CASES[name]
    nb, pos0 = c["beams"], c["pos0"]
    g = torch.Generator().manual_seed(seed + 1)
    kc, vc = fill_cache(model, nb, pos0, seed)
    first_logits = torch.randn(model.V, generator=g) * 2.0
    slot = torch.zeros(model.max_len, 8, dtype=torch.int32)
    tokens = torch.zeros(1, 0, dtype=torch.long)
    sel = select_ref(first_logits, torch.zeros(nb), torch.ones(nb), torch.zeros(nb), tokens, slot, pos0 - 1, 0.5, -1, True, model)
    for s in range(c["steps"]):
        pos = pos0 + s
        if pos >= model.max_len:
            break
        yield pos, sel.x, kc, vc, sel.slot_of, sel.src
        logits, _, k, v = step_ref(model, sel.x, kc, vc, sel.slot_of, pos, True)
        kc, vc = kc.clone(), vc.clone()
        kc[:, :nb, pos] = k.to(model.dtype)
        vc[:, :nb, pos] = v.to(model.dtype)
        sel = select_ref(logits, sel.scores, sel.seq_len, sel.stopped, sel.tokens, sel.slot_of, pos, 0.5, -1, False, model)
        if sel.x is None:
            break
