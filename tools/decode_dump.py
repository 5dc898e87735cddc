"""Bit-identity check of the two persistent beam-search kernels across a change that must not alter their results (a
refactor, a compiler update): a fixed list of searches on the test-tiny GPT-2 geometry, every output tensor saved raw.

    python tools/decode_dump.py --out before.pt        # on the build to compare against
    python tools/decode_dump.py --compare before.pt    # on the new build: exit status 1 at the first tensor that differs

One-caption kernel (cclip_gpt2_beam_search): fp16 and fp32 model (fp16 / bf16 kernels) x beams 1, 3, 5, 8 x stop token 7, -1 x
grid_cap 0, 3, and one search from the prompt "5 9 11 3"; saved: tokens, raw scores, lengths, state[2..4] and the logits buffer
as the last step left it.  Batched kernel (cclip_gpt2_beam_search_batch): N = 1, 7 x beams 1, 3, 5 with a stop token at which
the captions stop at different steps, the same under grid_cap 3, and N = 23 x beam 3 (two launches); saved: tokens, scores,
lengths, n_sel.  Host paths around the kernels: _cached_logits (prefill + two steps, CCLIP_DECODE_DRIVER native and python),
_logits_from_embeds under a key-padding mask, attention_probs of layers [0, -1] at rows [-1, 0], and beam_batch_enqueue with
positions_added=True followed by beam_batch_collect."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd")]
from cclip_hip import ops  # noqa: E402
from clip_caption import ClipCaptionModel, GPT2_MODELS, init_caption_state_dict, synthetic_caption_batch  # noqa: E402

ENTRY = 14


def build_model(half):
    geo = GPT2_MODELS["test-tiny"]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval()
    return geo, model.half() if half else model


def embeds(model, geo, n, seed=32):
    _, _, prefix, attribute = synthetic_caption_batch(n, geo, 6, seed)
    with torch.no_grad():
        pre = model.clip_project(prefix.cuda()).view(n, geo.prefix_length, geo.n_embd)
        return torch.cat((pre, model.gpt.transformer.wte(attribute.cuda())), dim=1)


def one_caption(model, emb, beam, stop, grid_cap, prompt_tokens=None):
    """beam_search_native with a logits buffer handed to the kernel; returns the raw device state of the search"""
    seen = {}
    launch = ops.gpt2_beam_search

    def with_logits(blocks_arr, n_layer, st, kcache, *args, **kw):
        seen["st"] = st
        seen["logits"] = torch.zeros(st.n_beams, kw["wte16"].shape[0], device=kcache.device, dtype=torch.float32)
        return launch(blocks_arr, n_layer, st, kcache, *args, **{**kw, "logits": seen["logits"]})

    ops.gpt2_beam_search = with_logits
    try:
        model.beam_search_native(emb, beam, ENTRY, 0.5, stop, prompt_tokens=prompt_tokens, grid_cap=grid_cap)
    finally:
        ops.gpt2_beam_search = launch
    st = seen["st"]
    return {"tokens": st.tokens, "scores": st.scores, "lengths": st.seq_lengths, "state": st.state[2:5], "logits": seen["logits"]}


def splitting_stop(model, emb, steps):
    """a token of the greedy search without stop token at which, as stop token, a caption stops early and (N > 1) the captions
    stop at two or more different steps; the most frequent such token"""
    t = model.beam_search_native_batch(emb, 1, steps, 0.5, -1)[0]
    vals, counts = t[:, :, 1:].reshape(-1).unique(return_counts=True)
    for cand in vals[counts.argsort(descending=True, stable=True)].tolist():
        n_sel = model.beam_search_native_batch(emb, 1, steps, 0.5, cand)[3]
        if int(n_sel.min()) < steps and (emb.shape[0] == 1 or len(set(n_sel.tolist())) >= 2):
            return cand
    raise SystemExit("no stop token splits the batch")


def batched(model, emb, beam, steps, stop, grid_cap=0):
    t, l, s, n = model.beam_search_native_batch(emb, beam, steps, 0.5, stop, grid_cap=grid_cap)
    return {"tokens": t, "scores": s, "lengths": l, "n_sel": n, "stop": torch.tensor([stop])}


def cached_steps(model, emb, driver):
    """prefill of emb [B, S, D], then two decode steps that feed the argmax token back"""
    old = os.environ.get("CCLIP_DECODE_DRIVER")
    os.environ["CCLIP_DECODE_DRIVER"] = driver
    try:
        with torch.no_grad():
            out = {}
            logits, cache = model._cached_logits(emb, None)
            out["prefill"] = logits
            for step in (1, 2):
                logits, cache = model._cached_logits(model.gpt.transformer.wte(logits[:, -1].argmax(-1, keepdim=True)), cache)
                out[f"step{step}"] = logits
            out["k"], out["v"] = cache.k[:, :, :cache.length], cache.v[:, :, :cache.length]
            return out
    finally:
        if old is None:
            del os.environ["CCLIP_DECODE_DRIVER"]
        else:
            os.environ["CCLIP_DECODE_DRIVER"] = old


def host_paths(model, emb, tag):
    """emb [3, S, D]: the entry points around the kernels that share host steps with the searches"""
    for driver in ("native", "python"):
        yield f"cached/{tag}/{driver}", cached_steps(model, emb, driver)
    S = emb.shape[1]
    mask = torch.ones(emb.shape[0], S, device="cuda")
    mask[1, S - 3:] = 0
    mask[2, S - 1:] = 0
    with torch.no_grad():
        yield f"masked/{tag}", {"logits": model._logits_from_embeds(emb, mask)}
        yield f"probs/{tag}", {"probs": model.attention_probs(emb, mask, layers=[0, -1], q_rows=[-1, 0])}
        wpe = model.gpt.transformer.wpe.weight.data[:S].float()
        t, l, s, n = model.beam_batch_collect(model.beam_batch_enqueue(emb + wpe, 3, ENTRY, 0.5, 7, positions_added=True))
        yield f"enqueue/{tag}/positions_added", {"tokens": t, "scores": s, "lengths": l, "n_sel": n}


def cases():
    """(name, {tensor name: tensor}) of every search, in a fixed order"""
    for half in (True, False):
        geo, model = build_model(half)
        tag = "f16" if half else "bf16"
        emb = embeds(model, geo, 1)
        for beam in (1, 3, 5, 8):
            for stop in (7, -1):
                for cap in (0, 3):
                    yield f"one/{tag}/beam{beam}/stop{stop}/cap{cap}", one_caption(model, emb, beam, stop, cap)
        prompt = torch.tensor([[5, 9, 11, 3]], device="cuda")
        yield f"one/{tag}/beam3/prompt", one_caption(model, model.gpt.transformer.wte(prompt), 3, 7, 0, prompt_tokens=prompt)
        emb7 = embeds(model, geo, 7)
        for n in (1, 7):
            stop = splitting_stop(model, emb7[:n], 40)
            for beam in (1, 3, 5):
                yield f"batch/{tag}/n{n}/beam{beam}/split", batched(model, emb7[:n], beam, 40, stop)
            yield f"batch/{tag}/n{n}/beam3/split/cap3", batched(model, emb7[:n], 3, 40, stop, grid_cap=3)
        yield f"batch/{tag}/n23/beam3", batched(model, embeds(model, geo, 23, seed=44), 3, ENTRY, 7)
        yield from host_paths(model, emb7[:3], tag)


def same_bytes(a, b):
    raw = lambda t: t.reshape(-1).view(torch.uint8)                     # noqa: E731  (numpy has no bfloat16)
    return a is not None and a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--out", help="run the searches and save every output tensor here")
    g.add_argument("--compare", help="run the searches and compare with the tensors saved here, byte by byte")
    args = ap.parse_args()
    saved = torch.load(args.compare) if args.compare else {}
    n = 0
    for name, tensors in cases():
        for key, t in tensors.items():
            now = t.detach().cpu().contiguous()
            if args.compare and not same_bytes(saved.get(f"{name}:{key}"), now):
                print(f"DIFFERENT  {name}:{key}", flush=True)
                sys.exit(1)
            saved[f"{name}:{key}"] = now
            n += 1
        print(f"{'same' if args.compare else 'run '}  {name}", flush=True)
    if args.compare:
        if n != len(saved):
            print(f"DIFFERENT  {len(saved)} tensors saved, {n} produced", flush=True)
            sys.exit(1)
        print(f"{n} tensors byte-identical to {args.compare}")
    else:
        torch.save(saved, args.out)
        print(f"{n} tensors saved to {args.out}")


if __name__ == "__main__":
    main()
