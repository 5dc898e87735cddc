"""Caption decoding with a KV cache: `generate_beam` and `generate2` with the reference's signatures and token-for-token
semantics (/root/reference/CLIP_prefix_caption/test.py:353-514, application.py:152-229, predict.py:164-300).

The reference calls `model.gpt(inputs_embeds=generated)` on the whole growing sequence at every step and keeps the last
position's logits.  Here the prefix is run once (prefill) and every later step feeds ONE token per beam through
`BlockStack.decode_step` against the cached keys / values; beam reordering gathers the cache.  The selection
rule on the [beams, V] logits (temperature, softmax-log, length-normalised top-k; a nucleus filter that cannot move the
arg-max) is the reference's.  For GPT-2 geometry `generate_beam` / `generate2` run all of it - decode steps AND selection - inside
one persistent kernel launch (ClipCaptionModel.beam_search_native); the host-side search below (class _Beams) covers what that
kernel does not.  The reference's loops themselves are restated only in oracle/caption_oracle.py, the checker.

Attention maps (`output_attentions=True` at every step of the reference's test.py copy of generate_beam, test.py:381-390, and
`attention_map(...)`, :438): `return_attention=True` on the four generate functions.  The decode kernels are not instrumented.
GPT-2 is causal, so row t of ONE forward over a finished sequence is the distribution the decode step at position t formed:
after the search, every returned beam's own sequence [prefix, wte(tokens[:n-1])] goes through one batched forward with a
probability launch on the n query rows (ClipCaptionModel.attention_probs, csrc/attention_probs.hip), whichever path - native
kernel, batched kernel, host loop - produced the tokens.  `caption_attention_map` is the reference's `attention_map`.
"""
from __future__ import annotations

from typing import List, Optional

import torch


def _replay_attention(model, prefixes, generated, layer: int) -> List[torch.Tensor]:
    """Per sequence i the rows [H, n_i, S0 + n_i - 1] of layer `layer`: row j = the attention of query position S0-1+j, the
    one whose logits produced generated[i][j].  prefixes: [S0, D] embeddings (one shared S0), generated: 1-D token tensors.
    One forward over all sequences, right-padded to the longest: no mask is needed, a row below a sequence's length only
    sees real keys, and what lies beyond is cut off here."""
    probs = getattr(model, "attention_probs", None)
    if probs is None:
        raise NotImplementedError("return_attention needs ClipCaptionModel.attention_probs")
    S0 = prefixes[0].shape[0]
    ns = [int(g.numel()) for g in generated]
    if min(ns) < 1:
        raise ValueError("return_attention: a sequence without a generated token has no attention row")
    nmax, dev = max(ns), prefixes[0].device
    x = torch.stack([p.detach().float() for p in prefixes])
    if nmax > 1:
        ids = torch.zeros(len(ns), nmax - 1, dtype=torch.long, device=dev)
        for i, g in enumerate(generated):                                 # (the last generated token is never fed)
            ids[i, :ns[i] - 1] = g[:ns[i] - 1].to(dev)
        x = torch.cat((x, model.gpt.transformer.wte(ids)), dim=1)
    att = probs(x, None, layers=[layer], q_rows=range(S0 - 1, S0 - 1 + nmax))[0]
    return [att[i, :, :n, :S0 + n - 1].clone() for i, n in enumerate(ns)]


def caption_attention_map(attention: torch.Tensor, head: Optional[int] = -1, pad_value: float = 1.0) -> torch.Tensor:
    """`attention_map` of test.py:342-349 for one sequence's rows [H, n, S0 + n - 1] (what return_attention yields): the rows
    of one head (`head=-1`: the last, the reference's `[:, -1, -1, :]`; None: the mean over heads), each cut to its causal
    length S0 + j and right-padded with pad_value (the reference pads with 1) to the last row's length -> [n, S0 + n - 1]."""
    if attention.dim() != 3:
        raise ValueError(f"attention must be [H, n, S0 + n - 1], got {tuple(attention.shape)}")
    rows = attention.mean(dim=0) if head is None else attention[head]
    n, width = rows.shape
    causal_len = torch.arange(width - n + 1, width + 1, device=rows.device)[:, None]
    return torch.where(torch.arange(width, device=rows.device)[None, :] < causal_len, rows, torch.full_like(rows, pad_value))


def _beam_rows(tokens, seq_lengths, n_prompt: int):
    """the generated part of every beam: its int(seq_length) tokens after the prompt"""
    return [tokens[b, n_prompt:n_prompt + int(n)] for b, n in enumerate(seq_lengths.tolist())]


def _step_logits(model, embeds: torch.Tensor, cache):
    out = model.gpt(inputs_embeds=embeds, past_key_values=cache, use_cache=True)
    return out.logits[:, -1, :], out.past_key_values


@torch.no_grad()
def generate_beam(model, tokenizer, beam_size: int = 3, prompt=None, embed=None, entry_length: int = 100,
                  temperature: float = 0.5, stop_token: int = 102, return_tokens: bool = False,
                  return_attention: bool = False, attention_layer: int = -1):
    """Beam search over length-normalised log-probabilities (test.py:353-441).  Returns the decoded texts best-first;
    with return_tokens also (token tensor [beams, steps], lengths, scores) in beam order.  return_attention appends one more
    element: per beam, in the row order of the token tensor, the fp32 rows [H, n, S0 + n - 1] of layer attention_layer
    (n = the beam's length, S0 = the prefix / prompt length; row j = the distribution that produced generated token j)."""
    model.eval()
    device = next(model.parameters()).device
    tokens = None

    def finish(prefix, prompt_tokens, tokens, seq_lengths, scores):
        out = _beam_outputs(tokenizer, tokens, seq_lengths, scores, return_tokens)
        if not return_attention:
            return out
        n_prompt = 0 if prompt_tokens is None else prompt_tokens.shape[1]
        gen = _beam_rows(tokens, seq_lengths, n_prompt)
        att = _replay_attention(model, [prefix[0]] * len(gen), gen, attention_layer)
        return (*out, att) if return_tokens else (out, att)
    if getattr(model, "beam_native_ok", None) is not None and model.beam_native_ok(beam_size) and entry_length >= 1:
        # prefill, then ONE persistent kernel for every decode step and every selection (csrc/decode_persist.hip); the
        # host loop below is the same arithmetic op by op and stays as its parity reference (CCLIP_BEAM_NATIVE=0)
        if embed is not None:
            generated = embed
        else:
            tokens = torch.tensor(tokenizer.encode(prompt)).unsqueeze(0).to(device)
            generated = model.gpt.transformer.wte(tokens)
        prompt_tokens = tokens
        tokens, seq_lengths, scores = model.beam_search_native(generated, beam_size, entry_length, temperature, stop_token,
                                                               prompt_tokens=prompt_tokens)
        return finish(generated, prompt_tokens, tokens, seq_lengths, scores)
    # Host-side search (nn.Linear-layout stacks, > 8 beams, CPU stubs in the tests, CCLIP_BEAM_NATIVE=0): one KV-cached decode
    # step per position, the beam bookkeeping kept in a _Beams record.  Same selection rule as the reference (a stopped beam
    # may only extend by token 0 at no cost; candidates ranked by total log-probability / length), written as one masked
    # candidate table per step instead of the reference's in-place edits.
    if embed is not None:
        prefix = embed
    else:
        tokens = torch.tensor(tokenizer.encode(prompt)).unsqueeze(0).to(device)
        prefix = model.gpt.transformer.wte(tokens)
    inv_t = 1.0 / (temperature if temperature > 0 else 1.0)
    logp, cache = _step_logits(model, prefix, None)                     # prefill: the whole prefix once
    logp = (logp * inv_t).softmax(-1).log()                             # (softmax-then-log, as the device kernels do)
    beams = _Beams.start(logp, beam_size, tokens)
    cache = cache.expand(beam_size)
    for step in range(1, entry_length):
        step_in = model.gpt.transformer.wte(beams.last_token()).view(beam_size, 1, -1)
        logp, cache = _step_logits(model, step_in, cache)
        logp = (logp * inv_t).softmax(-1).log()
        parent = beams.extend(logp, stop_token)
        cache = cache.reorder(parent)
        # `all stopped` is a device -> host sync; a stopped beam only ever appends token 0 at score 0 and keeps its length, so
        # looking every 4th step (and on the last) returns the same texts, lengths and scores while the host runs ahead
        if ((step & 3) == 3 or step == entry_length - 1) and bool((beams.stopped | beams.last_token().eq(stop_token)).all()):
            break
    return finish(prefix, tokens, beams.tokens, beams.lengths, beams.total)


class _Beams:
    """Beam bookkeeping of the host-side search: token rows, lengths (floats, as the scores divide by them), total
    log-probabilities and the stopped flags, all [beams]-shaped device tensors."""

    def __init__(self, tokens, lengths, total, stopped):
        self.tokens, self.lengths, self.total, self.stopped = tokens, lengths, total, stopped

    @classmethod
    def start(cls, logp, k: int, prompt_tokens):
        """first position: the k most probable tokens of the single prefix row open the beams"""
        total, first = logp[0].topk(k)
        col = first.unsqueeze(1)
        toks = col if prompt_tokens is None else torch.cat((prompt_tokens.expand(k, -1), col), dim=1)
        b = cls(toks, torch.ones(k, device=logp.device), total, torch.zeros(k, dtype=torch.bool, device=logp.device))
        return b

    def last_token(self):
        return self.tokens[:, -1]

    def extend(self, logp, stop_token: int):
        """one position further: returns each new beam's parent row (for the KV-cache reorder)"""
        k, V = logp.shape
        # a beam stops on the position AFTER it emitted the stop token
        self.stopped = self.stopped | self.tokens[:, -1].eq(stop_token)
        live = ~self.stopped
        # candidate table: live rows extend by any token; a stopped row offers only token 0, free of charge
        step_cost = torch.where(live[:, None], logp, torch.full_like(logp, -float("inf")))
        step_cost[self.stopped, 0] = 0.0
        new_len = self.lengths + live.to(self.lengths.dtype)
        ranked = (self.total[:, None] + step_cost) / new_len[:, None]
        best, flat = ranked.reshape(-1).topk(k)
        parent = torch.div(flat, V, rounding_mode="floor")
        token = flat - parent * V
        self.lengths = new_len[parent]
        self.total = best * self.lengths
        self.stopped = self.stopped[parent]
        self.tokens = torch.cat((self.tokens[parent], token.unsqueeze(1)), dim=1)
        return parent


def _beam_outputs(tokenizer, tokens, seq_lengths, scores, return_tokens: bool):
    """test.py:435-441: length-normalise, order best first, decode each beam up to its length"""
    scores = scores / seq_lengths
    order = scores.argsort(descending=True)
    output_list = tokens.cpu().numpy()
    texts = [tokenizer.decode(output[: int(length)]) for output, length in zip(output_list, seq_lengths)]
    texts = [texts[i] for i in order]
    if return_tokens:
        return texts, tokens, seq_lengths, scores
    return texts


@torch.no_grad()
def generate2(model, tokenizer, tokens=None, prompt=None, embed=None, entry_count: int = 1, entry_length: int = 67,
              top_p: float = 0.8, temperature: float = 1.0, stop_token: int = 102, return_tokens: bool = False,
              return_attention: bool = False, attention_layer: int = -1):
    """Nucleus-filtered greedy decoding (test.py:443-514): tokens outside the top-p mass are removed, the arg-max of the
    rest is taken.  As in the reference's live code the sequence always starts from `embed` (test.py:472).
    return_attention appends a one-element list: the rows [H, n, S0 + n - 1] of the n tokens emitted (by the last entry)."""
    model.eval()
    device = next(model.parameters()).device
    generated_list: List[str] = []
    out_tokens: Optional[torch.Tensor] = tokens
    replay = None                                                        # (start embeddings, emitted tokens) of the last entry
    for _ in range(entry_count):
        if embed is None:
            if out_tokens is None:
                out_tokens = torch.tensor(tokenizer.encode(prompt)).unsqueeze(0).to(device)
            step_in = model.gpt.transformer.wte(out_tokens)
        else:
            step_in = embed
        if getattr(model, "beam_native_ok", None) is not None and model.beam_native_ok(1) and entry_length >= 1 and top_p > 0:
            # The nucleus filter never removes the most probable token (`remove[..., 0] = 0`, test.py:499), so the arg-max of the
            # filtered logits IS the arg-max of the logits: this loop is a greedy search = the persistent beam kernel with one
            # beam, which stops on the stop token exactly as the loop's `break` does (the stop token is the last one kept).
            prev = out_tokens
            new_tokens, _, _ = model.beam_search_native(step_in, 1, entry_length, temperature, stop_token,
                                                        prompt_tokens=prev if embed is None else None)
            # (from a prompt the kernel's token row starts with the prompt; from `embed` the running token list is kept in front)
            replay = (step_in, new_tokens[0, prev.shape[1]:] if embed is None else new_tokens[0])
            out_tokens = new_tokens if embed is None or prev is None else torch.cat((prev.to(new_tokens.device), new_tokens), dim=1)
            generated_list.append(tokenizer.decode(list(out_tokens.squeeze(0).cpu().numpy())))
            continue
        # host-side loop (stacks the persistent kernel does not cover, CPU stubs): the same observation makes the sort / cumulative
        # sum of the nucleus filter unnecessary for the arg-max - one KV-cached step and one arg-max per position
        cache = None
        start, n_before = step_in, 0 if out_tokens is None else out_tokens.shape[1]
        for _ in range(entry_length):
            logits, cache = _step_logits(model, step_in, cache)
            pick = logits.argmax(dim=-1, keepdim=True)                  # [1, 1]; the temperature does not move an arg-max
            out_tokens = pick if out_tokens is None else torch.cat((out_tokens, pick), dim=1)
            if int(pick) == stop_token:
                break
            step_in = model.gpt.transformer.wte(pick)
        if out_tokens is not None:
            replay = (start, out_tokens[0, n_before:])
        generated_list.append(tokenizer.decode(list(out_tokens.squeeze(0).cpu().numpy())))
    out = (generated_list[0], out_tokens) if return_tokens else generated_list[0]
    if not return_attention:
        return out
    att = _replay_attention(model, [replay[0][0]], [replay[1]], attention_layer)
    return (*out, att) if return_tokens else (out, att)


def _check_embeds(embeds) -> None:
    if not isinstance(embeds, torch.Tensor) or embeds.dim() != 3 or embeds.shape[0] < 1:
        shape = tuple(embeds.shape) if isinstance(embeds, torch.Tensor) else type(embeds).__name__
        raise ValueError(f"embeds must be [N, S, D] with N >= 1, got {shape}")


def _batch_native(model, beam_size: int, embeds, entry_length: int) -> bool:
    ok = getattr(model, "beam_batch_native_ok", None)
    return ok is not None and ok(beam_size, embeds.shape[1], entry_length)


@torch.no_grad()
def generate_beam_batch(model, tokenizer, embeds, beam_size: int = 3, entry_length: int = 100, temperature: float = 0.5,
                        stop_token: int = 102, return_tokens: bool = False, return_attention: bool = False,
                        attention_layer: int = -1):
    """generate_beam for N prefixes at once: embeds [N, S, D] (every caption the same S).  Returns a list of N lists of
    texts, list i best-first and equal to generate_beam(model, tokenizer, embed=embeds[i:i+1], ...); with return_tokens also
    the N per-caption (tokens [beams, n], lengths, scores) that generate_beam returns.  All captions of a launch run in one
    batched persistent kernel (ClipCaptionModel.beam_search_native_batch); where that kernel does not apply, the captions
    go one by one through generate_beam.  return_attention appends, per caption, generate_beam's list of per-beam rows
    (all N x beams sequences replayed in one forward)."""
    _check_embeds(embeds)
    model.eval()
    N = embeds.shape[0]
    if not _batch_native(model, beam_size, embeds, entry_length):
        outs = [generate_beam(model, tokenizer, beam_size=beam_size, embed=embeds[i:i + 1], entry_length=entry_length,
                              temperature=temperature, stop_token=stop_token, return_tokens=True) for i in range(N)]
        texts = [o[0] for o in outs]
        per = [tuple(o[1:]) for o in outs]
    else:
        tokens, lengths, scores, n_sel = model.beam_search_native_batch(embeds, beam_size, entry_length, temperature, stop_token)
        texts, per = [], []
        for i in range(N):
            t, tk, ln, sc = _beam_outputs(tokenizer, tokens[i, :, :int(n_sel[i])], lengths[i], scores[i], True)
            texts.append(t)
            per.append((tk, ln, sc))
    out = (texts, per) if return_tokens else texts
    if not return_attention:
        return out
    gen = [_beam_rows(tk, ln, 0) for tk, ln, _ in per]
    flat = _replay_attention(model, [embeds[i] for i, g in enumerate(gen) for _ in g], [r for g in gen for r in g], attention_layer)
    att, at = [], 0
    for g in gen:
        att.append(flat[at:at + len(g)])
        at += len(g)
    return (*out, att) if return_tokens else (out, att)


@torch.no_grad()
def generate2_batch(model, tokenizer, embeds, entry_length: int = 67, top_p: float = 0.8, temperature: float = 1.0,
                    stop_token: int = 102, return_tokens: bool = False, return_attention: bool = False,
                    attention_layer: int = -1):
    """generate2 for N prefixes at once (embeds [N, S, D]): a list of N strings, string i equal to
    generate2(model, tokenizer, embed=embeds[i:i+1], ...); with return_tokens also the N token rows [1, n].  The greedy
    search is the one-beam batched kernel, for the reason given in generate2's native branch.  return_attention appends,
    per caption, generate2's one-element list of rows (all N sequences replayed in one forward)."""
    _check_embeds(embeds)
    model.eval()
    N = embeds.shape[0]
    if top_p <= 0 or not _batch_native(model, 1, embeds, entry_length):
        outs = [generate2(model, tokenizer, embed=embeds[i:i + 1], entry_length=entry_length, top_p=top_p, temperature=temperature,
                          stop_token=stop_token, return_tokens=True) for i in range(N)]
        texts = [o[0] for o in outs]
        rows = [o[1] for o in outs]
    else:
        tokens, _, _, n_sel = model.beam_search_native_batch(embeds, 1, entry_length, temperature, stop_token)
        rows = [tokens[i, :, :int(n_sel[i])] for i in range(N)]
        texts = [tokenizer.decode(list(r.squeeze(0).cpu().numpy())) for r in rows]
    out = (texts, rows) if return_tokens else texts
    if not return_attention:
        return out
    att = [[a] for a in _replay_attention(model, [embeds[i] for i in range(N)], [r[0] for r in rows], attention_layer)]
    return (*out, att) if return_tokens else (out, att)


def _sample_outputs(tokenizer, tokens, logprobs, stop_token: int, prompt_ids, return_tokens: bool, return_logprobs: bool):
    """One image's K samples: texts best first by mean token log-probability; tokens / lengths / sums stay in draw order."""
    K, steps = tokens.shape
    at = torch.arange(1, steps + 1, device=tokens.device)
    lengths = torch.where(tokens.eq(stop_token), at, at.new_tensor(steps)).amin(dim=1)     # up to and including the first stop token
    total = logprobs.sum(dim=1)                                          # (a finished row adds exact zeros)
    order = (total / lengths).argsort(descending=True, stable=True).tolist()
    rows, lens = tokens.cpu().numpy(), lengths.tolist()
    texts = [tokenizer.decode(prompt_ids + list(rows[i][:lens[i]])) for i in order]
    if not return_tokens:
        return texts
    return (texts, tokens, lengths, total, logprobs) if return_logprobs else (texts, tokens, lengths, total)


@torch.no_grad()
def generate_sample_batch(model, tokenizer, embeds, num_samples: int = 1, entry_length: int = 67, top_p: float = 0.8,
                          top_k: int = 0, temperature: float = 1.0, stop_token: int = 102, generator=None, uniforms=None,
                          return_tokens: bool = False, return_logprobs: bool = False, _prompt_ids=None):
    """num_samples captions DRAWN from the model's distribution for each of N prefixes (embeds [N, S, D]): at every position
    the next token of each sample comes from softmax(logits / temperature) cut to the top_k most probable tokens (0 = off)
    and to the nucleus top_p (the reference's filter, test.py:492-500; 1 = off) - one KV-cached decode step over all N x K
    rows, one row-sampling launch (csrc/sample_rows.hip), one wte gather.  A sample ends with its first stop_token; from then on
    it only appends token 0.  The randomness is one uniform per (position, row): torch.rand(entry_length, N * K,
    generator=generator) drawn up front, or `uniforms` of that shape (row i * K + j = sample j of image i), so one seed gives
    one set of captions.  Returns a list of N lists of K texts, each list best first by mean token log-probability; with
    return_tokens a list of N tuples (texts, tokens int32 [K, steps], lengths [K], sum_logprob [K]) in draw order, with
    return_logprobs also the per-position log-probabilities fp32 [K, steps] (log p of the full softmax; 0 past the end)."""
    from cclip_hip import ops
    _check_embeds(embeds)
    if num_samples < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if entry_length < 1:
        raise ValueError(f"entry_length must be >= 1, got {entry_length}")
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    if not embeds.is_cuda:
        raise TypeError(f"generate_sample: expected cuda embeddings, got {embeds.device} (sampling has no host path)")
    model.eval()
    dev = embeds.device
    N, K = embeds.shape[0], int(num_samples)
    n = N * K
    if uniforms is None:
        gdev = dev if generator is None else generator.device
        uniforms = torch.rand(entry_length, n, generator=generator, device=gdev).to(dev)
    else:
        if tuple(uniforms.shape) != (entry_length, n):
            raise ValueError(f"uniforms must be [{entry_length}, {n}] (entry_length, N * num_samples), got {tuple(uniforms.shape)}")
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
    logits, cache = _step_logits(model, embeds, None)                   # prefill: every prefix once
    if K > 1:                                                           # each sample its own rows of the cache
        rows = torch.arange(N, device=dev).repeat_interleave(K)
        logits, cache = logits[rows], cache.reorder(rows)
    done = torch.zeros(n, dtype=torch.int32, device=dev)
    toks, lps = [], []
    for step in range(entry_length):
        if step:
            step_in = model.gpt.transformer.wte(toks[-1].long()).view(n, 1, -1)
            logits, cache = _step_logits(model, step_in, cache)
        tok, lp, _, _ = ops.sample_rows(logits, uniforms[step], done, inv_temperature=1.0 / temperature, top_k=top_k, top_p=top_p,
                                        stop_token=stop_token)
        toks.append(tok)
        lps.append(lp)
        # `all done` is a device -> host sync: looked at every 4th step and on the last, as generate_beam's host loop does
        if ((step & 3) == 3 or step == entry_length - 1) and bool(done.all()):
            break
    tokens, logprobs = torch.stack(toks, dim=1), torch.stack(lps, dim=1)
    prompt_ids = [] if _prompt_ids is None else list(_prompt_ids)
    return [_sample_outputs(tokenizer, tokens[i * K:(i + 1) * K], logprobs[i * K:(i + 1) * K], stop_token, prompt_ids, return_tokens,
                            return_logprobs) for i in range(N)]


@torch.no_grad()
def generate_sample(model, tokenizer, embed=None, prompt=None, num_samples: int = 1, entry_length: int = 67, top_p: float = 0.8,
                    top_k: int = 0, temperature: float = 1.0, stop_token: int = 102, generator=None, uniforms=None,
                    return_tokens: bool = False, return_logprobs: bool = False):
    """generate_sample_batch for one image (embed [1, S, D]) or one text prompt: the num_samples texts best first; with
    return_tokens (texts, tokens [K, steps], lengths, sum_logprob) in draw order.  From a prompt the texts start with the
    prompt, the token rows hold the drawn tokens only."""
    prompt_ids = None
    if embed is None:
        if prompt is None:
            raise ValueError("generate_sample needs embed= or prompt=")
        prompt_ids = list(tokenizer.encode(prompt))
        device = next(model.parameters()).device
        embed = model.gpt.transformer.wte(torch.tensor(prompt_ids, device=device).unsqueeze(0))
    if isinstance(embed, torch.Tensor) and embed.dim() == 3 and embed.shape[0] != 1:
        raise ValueError(f"generate_sample takes one prefix [1, S, D], got {tuple(embed.shape)}; use generate_sample_batch")
    return generate_sample_batch(model, tokenizer, embed, num_samples=num_samples, entry_length=entry_length, top_p=top_p, top_k=top_k,
                                 temperature=temperature, stop_token=stop_token, generator=generator, uniforms=uniforms,
                                 return_tokens=return_tokens, return_logprobs=return_logprobs, _prompt_ids=prompt_ids)[0]
