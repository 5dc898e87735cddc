"""KV-cached decoding of ClipCaptionModel: the cache, the cached step (`model.model(..., use_cache=True)`) and the persistent
beam-search entry points, one caption or many.  DecodeMixin is a plain mixin of ClipCaptionModel: it uses the model's runtime
(`_arena`, `_stack`) and shared inference steps (`_positioned_rows`, `_lm_rows`, `_lm_all`), and holds what only decoding needs."""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Optional

import torch

from cclip_hip import ops


class KVCache:
    """Per-layer keys / values of the positions processed so far: k, v [n_layer, n_seq, max_len, n_embd] in the
    compute dtype, `length` positions valid.  reorder(idx) is beam search's `generated = generated[next_tokens_source]`
    (test.py:416) applied to the cache."""

    def __init__(self, n_layer: int, n_seq: int, max_len: int, width: int, device, dtype):
        self.k = torch.empty(n_layer, n_seq, max_len, width, device=device, dtype=dtype)
        self.v = torch.empty_like(self.k)
        self.length = 0

    @property
    def n_seq(self) -> int:
        return self.k.shape[1]

    @property
    def max_len(self) -> int:
        return self.k.shape[2]

    def reorder(self, idx: torch.Tensor) -> "KVCache":
        idx = idx.to(self.k.device).long()
        L = self.length
        out = KVCache.__new__(KVCache)
        out.k = torch.empty(self.k.shape[0], idx.numel(), *self.k.shape[2:], device=self.k.device, dtype=self.k.dtype)
        out.v = torch.empty_like(out.k)
        out.k[:, :, :L] = self.k[:, idx, :L]
        out.v[:, :, :L] = self.v[:, idx, :L]
        out.length = L
        return out

    def expand(self, n: int) -> "KVCache":
        """one sequence -> n identical ones (`generated.expand(beam_size, ...)`, test.py:398)"""
        assert self.n_seq == 1
        return self.reorder(torch.zeros(n, dtype=torch.long))


def _raise_on_timeout(entry_point: str, state) -> None:
    if state[1]:                          # (state: the 8 bookkeeping words of a persistent launch, read back)
        raise RuntimeError(f"{entry_point}: a grid barrier timed out (workgroups not co-resident?)")


def _n_sel(words: torch.Tensor, entry_length: int) -> torch.Tensor:
    """Selections each caption made, from its bookkeeping words [n, 8] (on the host): word 3 where the caption stopped by itself
    (word 2), else the entry_length its loop ran to."""
    return torch.where(words[:, 2] != 0, words[:, 3], torch.full_like(words[:, 3], entry_length)).long()


class DecodeMixin:
    def _decode_launch(self):
        """What the three native decode launches share: the per-layer weight pointers (rebuilt when the arena is), the layer
        count, the keywords of a step (`step`) and of a search (`beam`), the scratch of `rows` sequences and the grid-cap rule."""
        st, ar, g = self._stack, self._arena, self.model.geo
        if getattr(self, "_decode_ptrs", None) is None or self._decode_ptrs[0] is not ar:
            self._decode_ptrs = (ar, ops.block_ptr_array(st.blocks))
        p, D = ar.params, g.n_embd
        hidden = st.geo.hidden or 4 * D
        dev, dtype = p["model.transformer.wte.weight"].device, self.compute_dtype
        step = dict(heads=st.geo.heads, hidden=hidden, act=st.geo.act, lnf_w=p["model.transformer.ln_f.weight"].data,
                    lnf_b=p["model.transformer.ln_f.bias"].data, wte16=ar.b["model.transformer.wte.weight"])
        return SimpleNamespace(
            blocks=self._decode_ptrs[1], n_layer=g.n_layer, linear_layout=bool(st.geo.linear_layout), step=step,
            beam=dict(step, wte_f32=p["model.transformer.wte.weight"].data, wpe_f32=p["model.transformer.wpe.weight"].data),
            scratch=lambda rows: torch.empty(rows * (5 * D + hidden), device=dev, dtype=dtype),
            grid=lambda grid_cap: grid_cap or int(os.environ.get("CCLIP_BEAM_GRID", "0")))

    def _prefill_one(self, rows_x: torch.Tensor, kv_out) -> torch.Tensor:
        """One caption's prefill: the causal forward of its positioned rows [S, D] (keys / values kept in kv_out, one cache
        slot) and the fp32 logits [V] of its last position.  Nothing is copied to the device or read back."""
        S = rows_x.shape[0]
        xo = self._stack.forward(rows_x, 1, T=S, kv_out=kv_out)
        last = torch.full((1,), S - 1, device=rows_x.device, dtype=torch.int32)     # (a fill launch: no host-to-device copy to wait for)
        return self._lm_rows(xo, last, False)[0].view(-1)

    def _cached_logits(self, inputs_embeds: torch.Tensor, cache: Optional[KVCache]):
        """(logits [B, S_new, V], cache) for the new positions `inputs_embeds` [B, S_new, D] appended after cache.length."""
        if torch.is_grad_enabled() and inputs_embeds.requires_grad:
            raise NotImplementedError("KV-cached decode is inference only")
        self._ensure_runtime()
        self._arena.refresh_shadows()
        g = self.model.geo
        B, S, D = inputs_embeds.shape
        dev = inputs_embeds.device
        if cache is None:                                     # prefill: the ordinary causal forward, keys / values kept
            cache = KVCache(g.n_layer, B, g.n_positions, D, dev, self.compute_dtype)
            xo = self._stack.forward(self._positioned_rows(inputs_embeds), B, T=S, kv_out=(cache.k, cache.v))
            cache.length = S
            return self._lm_all(xo, B, S), cache
        if S != 1 or B != cache.n_seq:
            raise NotImplementedError(f"decode step takes one new token per cached sequence, got {tuple(inputs_embeds.shape)} for {cache.n_seq} sequences")
        pos = cache.length
        if pos >= cache.max_len:
            raise RuntimeError(f"sequence longer than n_positions = {cache.max_len}")
        x = inputs_embeds.detach().float().contiguous().view(B, D) + self._arena.params["model.transformer.wpe.weight"].data[pos]
        if os.environ.get("CCLIP_DECODE_DRIVER", "native") != "native":       # launch by launch from Python (reference form)
            logits = self._lm_all(self._stack.decode_step(x, cache.k, cache.v, pos), B, 1)
        else:                                 # the whole per-token launch sequence (and ln_f + lm_head) from one native call
            L, V = self._decode_launch(), g.vocab_size
            logits = torch.empty(B, (V + 7) // 8 * 8, device=dev, dtype=torch.float32)[:, :V].unsqueeze(1)
            ops.gpt2_decode_step(L.blocks, L.n_layer, x, cache.k, cache.v, pos, L.scratch(B), linear_layout=L.linear_layout,
                                 logits=logits[:, 0], **L.step)
        cache.length = pos + 1
        return logits, cache

    def beam_native_ok(self, beam_size: int) -> bool:
        """the persistent beam-search kernel covers GPT-2 geometry (Conv1D weights, head_dim 64, <= 24 layers) and <= 8 beams"""
        if os.environ.get("CCLIP_BEAM_NATIVE", "1") == "0" or not 1 <= beam_size <= ops.BEAM_MAX_BEAMS:
            return False
        self._ensure_runtime()
        g, sg = self.model.geo, self._stack.geo
        return (not sg.linear_layout and g.n_layer <= ops.BEAM_MAX_LAYERS and sg.head_dim == 64 and sg.width % 64 == 0
                and (sg.hidden or 4 * sg.width) % 32 == 0 and sg.act in (ops.ACT_NONE, ops.ACT_GELU_NEW) and g.n_positions <= 2048
                and -(-g.vocab_size // 256) <= 256 and next(self.parameters()).is_cuda)

    @torch.no_grad()
    def beam_search_native(self, inputs_embeds: torch.Tensor, beam_size: int, entry_length: int, temperature: float,
                           stop_token: int, prompt_tokens: Optional[torch.Tensor] = None, grid_cap: int = 0):
        """The reference's generate_beam loop (test.py:380-434) after the prefix: prefill here, then every decode step and
        every selection inside ONE persistent kernel launch (ops.gpt2_beam_search).  Returns (tokens [beams, n] int64,
        seq_lengths [beams], scores [beams]) exactly where the reference's loop stops (`is_stopped.all()` or entry_length)."""
        self._ensure_runtime()
        self._arena.refresh_shadows()
        g = self.model.geo
        B, S, D = inputs_embeds.shape
        assert B == 1, "beam search starts from one sequence"
        dev = inputs_embeds.device
        max_len = g.n_positions
        if S + entry_length - 1 > max_len:
            raise RuntimeError(f"sequence longer than n_positions = {max_len}")
        cache = KVCache(g.n_layer, beam_size, max_len, D, dev, self.compute_dtype)
        first_logits = self._prefill_one(self._positioned_rows(inputs_embeds), (cache.k, cache.v))   # prefix keys / values -> slot 0
        n_prompt = 0 if prompt_tokens is None else int(prompt_tokens.numel())
        bs = ops.BeamState(beam_size, max_len, n_prompt + entry_length, dev)
        if n_prompt:
            bs.tokens[0, :n_prompt] = prompt_tokens.view(-1).to(dev, torch.int32)
            bs.state[4] = n_prompt
        L = self._decode_launch()
        ops.gpt2_beam_search(L.blocks, L.n_layer, bs, cache.k, cache.v, S, L.scratch(beam_size), entry_length - 1,
                             temperature=float(temperature), stop_token=int(stop_token), first_logits=first_logits,
                             grid_cap=L.grid(grid_cap), **L.beam)
        state = bs.state.cpu()                                          # the one host sync of the caption
        _raise_on_timeout("cclip_gpt2_beam_search", state)
        return bs.tokens[:, :n_prompt + int(_n_sel(state[None], entry_length))].long(), bs.seq_lengths, bs.scores

    def beam_batch_native_ok(self, beam_size: int, seq_len: int = 0, entry_length: int = 1) -> bool:
        """the batched persistent kernel covers what beam_native_ok covers (<= 64 rows per launch: at least one caption);
        its cache holds seq_len + entry_length positions, which must fit n_positions"""
        return (beam_size <= ops.BEAM_BATCH_MAX_ROWS and entry_length >= 1 and seq_len + entry_length <= self.model.geo.n_positions
                and self.beam_native_ok(beam_size))

    @torch.no_grad()
    def beam_search_native_batch(self, inputs_embeds: torch.Tensor, beam_size: int, entry_length: int, temperature: float,
                                 stop_token: int, grid_cap: int = 0):
        """beam_search_native for N captions [N, S, D] at once: the prefills (caption by caption), then launches of at most
        64 // beam_size captions of cclip_gpt2_beam_search_batch, one host sync each.  Returns (tokens [N, beams, n] int64,
        seq_lengths [N, beams], scores [N, beams], n_sel [N]); caption i's tokens are valid up to n_sel[i] columns (where its
        own loop stops), the columns after that are zero."""
        return self.beam_batch_collect(self.beam_batch_enqueue(inputs_embeds, beam_size, entry_length, temperature, stop_token,
                                                               grid_cap=grid_cap))

    @torch.no_grad()
    def beam_batch_enqueue(self, inputs_embeds: torch.Tensor, beam_size: int, entry_length: int, temperature: float,
                           stop_token: int, grid_cap: int = 0, positions_added: bool = False):
        """The device half of beam_search_native_batch: every prefill and every batched launch is enqueued on the current
        stream and nothing is read back, so the host does not wait for the device here.  positions_added: the rows already
        hold `+ wpe[s]` (what cclip_caption_embed writes), so the positional add is skipped.  Returns the pending launches for
        beam_batch_collect."""
        self._ensure_runtime()
        self._arena.refresh_shadows()
        g = self.model.geo
        N, S, D = inputs_embeds.shape
        if N < 1 or entry_length < 1:
            raise ValueError(f"need N >= 1 captions and entry_length >= 1, got N = {N}, entry_length = {entry_length}")
        if S + entry_length > g.n_positions:
            raise RuntimeError(f"sequence longer than n_positions = {g.n_positions}")
        dev = inputs_embeds.device
        max_len = S + entry_length                                       # the cache holds what this search can reach
        # prefill caption by caption, as beam_search_native does: the tiled GEMMs' tile / split choice depends on the row count,
        # so one prefill of all N would make a caption's first logits (and so its tokens) depend on the batch around it
        x = self._positioned_rows(inputs_embeds, positions_added).view(N, S, D)      # (elementwise: all captions at once)
        pre = KVCache(g.n_layer, N, S, D, dev, self.compute_dtype)
        first_all = torch.empty(N, g.vocab_size, device=dev, dtype=torch.float32)
        for i in range(N):
            first_all[i] = self._prefill_one(x[i], (pre.k[:, i:i + 1], pre.v[:, i:i + 1]))
        L = self._decode_launch()
        per, grid_cap = max(1, ops.BEAM_BATCH_MAX_ROWS // beam_size), L.grid(grid_cap)
        launches = []
        for c0 in range(0, N, per):
            n = min(per, N - c0)
            k = torch.zeros(g.n_layer, n * beam_size, max_len, D, device=dev, dtype=self.compute_dtype)
            v = torch.zeros_like(k)
            k.view(g.n_layer, n, beam_size, max_len, D)[:, :, 0, :S].copy_(pre.k[:, c0:c0 + n])
            v.view(g.n_layer, n, beam_size, max_len, D)[:, :, 0, :S].copy_(pre.v[:, c0:c0 + n])
            bs = ops.BeamBatchState(n, beam_size, max_len, entry_length, dev)
            scratch = L.scratch(n * beam_size)
            ops.gpt2_beam_search_batch(L.blocks, L.n_layer, bs, k, v, S, scratch, entry_length - 1, temperature=float(temperature),
                                       stop_token=int(stop_token), first_logits=first_all[c0:c0 + n].contiguous(), grid_cap=grid_cap,
                                       linear_layout=L.linear_layout, **L.beam)
            launches.append((c0, n, bs, (k, v, scratch)))                # (the buffers live until the launch has been read)
        return dict(N=N, beams=beam_size, entry_length=entry_length, device=dev, launches=launches)

    @torch.no_grad()
    def beam_batch_collect(self, pending):
        """The host half of beam_search_native_batch: reads every pending launch back (one host sync per launch) and returns
        what beam_search_native_batch returns."""
        N, beam_size, entry_length, dev = pending["N"], pending["beams"], pending["entry_length"], pending["device"]
        tokens = torch.zeros(N, beam_size, entry_length, device=dev, dtype=torch.int64)
        lengths = torch.empty(N, beam_size, device=dev, dtype=torch.float32)
        scores = torch.empty(N, beam_size, device=dev, dtype=torch.float32)
        n_sel = torch.empty(N, dtype=torch.int64)
        for c0, n, bs, _ in pending["launches"]:
            state, cap = bs.state.tolist(), bs.cap_state.cpu()          # the one host sync of the launch
            _raise_on_timeout("cclip_gpt2_beam_search_batch", state)
            ns = _n_sel(cap, entry_length)
            n_sel[c0:c0 + n] = ns
            keep = torch.arange(entry_length)[None, :] < ns[:, None]      # columns past a caption's stop are not its tokens
            tokens[c0:c0 + n] = (bs.tokens.view(n, beam_size, entry_length).long() * keep.to(dev)[:, None, :])
            lengths[c0:c0 + n] = bs.seq_lengths.view(n, beam_size)
            scores[c0:c0 + n] = bs.scores.view(n, beam_size)
        pending["launches"] = []
        return tokens[:, :, :int(n_sel.max())], lengths, scores, n_sel
