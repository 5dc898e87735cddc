"""Caption attention maps on the MI355X: the probability kernel (csrc/attention_probs.hip) against float64 on the same
16-bit operands, `output_attentions=True` of the GPT-2 drop-in against the float64 restatement of GPT-2's attention
(tests/test_caption_attention_cpu.gpt2_attentions64, itself pinned against transformers), `return_attention=True` of the four
generate functions (native kernel, batched kernel and host path: the rows come from a replay, whichever produced the tokens),
`Captioner.describe(..., return_attention=True)` and `scripts/describe_images.py --attention-out`.

Model-level errors against float64 on the fp32 master weights, measured on one MI355X over both fixtures (test-tiny 2 layers
and GPT-2-small geometry 12 layers; with and without a padding mask; the largest over the layers):

    operands   max |dP|    relative L2 (per layer, whole tensor)
    fp16       2.10e-4     1.73e-4        (test-tiny: 2.2e-5 / 2.1e-5)
    bf16       2.13e-3     1.38e-3        (test-tiny: 1.4e-4 / 1.6e-4)

ATT_ABS / ATT_REL are about twice the largest (the convention of tests/test_relevance_gpu.py).  The error is the 16-bit
rounding of q and k (and of the residual stream's projections below them); the kernel's own arithmetic is fp32 on those
operands and is held to KERNEL_TOL against float64, the bound tests/test_relevance_gpu.py holds the same exp(scale Q K^T - max)
arithmetic to.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from test_caption_attention_cpu import gpt2_attentions64  # noqa: E402

KERNEL_TOL = 1e-4
ATT_ABS = {torch.float16: 4e-4, torch.bfloat16: 4e-3}
ATT_REL = {torch.float16: 3.5e-4, torch.bfloat16: 3e-3}


class _Tok:
    def encode(self, s):
        return [int(x) for x in s.split()]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _probs64(q, k, B, T, H, causal, keep, rows):
    """float64 softmax(q k^T / 8 + mask) on the given 16-bit operands: [B, H, n_q, T]"""
    qd = q.double().view(B, T, H, 64).transpose(1, 2)
    kd = k.double().view(B, T, H, 64).transpose(1, 2)
    sc = qd @ kd.transpose(-1, -2) / 8.0
    visible = torch.ones(B, 1, T, T, dtype=torch.bool, device=q.device)
    if causal:
        visible = visible & torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    if keep is not None:
        visible = visible & (keep != 0)[:, None, None, :]
    p = torch.softmax(sc.masked_fill(~visible, float("-inf")), dim=-1)
    return p[:, :, rows.long()] if rows is not None else p, visible[:, :, rows.long()] if rows is not None else visible


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("use_keep", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("T", [1, 16, 40, 77, 128, 140, 256])
def test_probs_kernel_against_float64(T, H, causal, use_keep, use_rows, dtype):
    from cclip_hip import ops
    B = 3 if H == 2 else 2
    D = H * 64
    g = torch.Generator().manual_seed(1000 * T + 10 * H + 4 * causal + 2 * use_keep + use_rows)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).to(dtype).cuda()       # packed rows: q / k are strided views
    q, k = qkv[:, 0:D], qkv[:, D:2 * D]
    keep = None
    if use_keep:
        keep = (torch.rand(B, T, generator=g) > 0.3).float()
        keep[:, 0] = 1.0                                                        # every (causal) row sees a key
        keep = keep.cuda()
    rows = None
    if use_rows:                                                                # unsorted, repeated, across a 64-row block
        rows = torch.randint(0, T, (min(T, 70) + 3,), generator=g).to(torch.int32).cuda()
    n_q = T if rows is None else rows.numel()
    ld, guard, fill = T + 3, 64, -7.0                                           # pad columns and both ends are guards
    buf = torch.full((guard + B * H * n_q * ld + guard,), fill, device="cuda")
    body = buf[guard:guard + B * H * n_q * ld].view(B, H, n_q, ld)
    P = body[..., :T]
    ops.attention_probs(q, k, P, B=B, T=T, H=H, causal=causal, key_keep=keep, q_rows=rows)
    torch.cuda.synchronize()
    got = P.clone()
    assert torch.all(buf[:guard] == fill) and torch.all(buf[-guard:] == fill) and torch.all(body[..., T:] == fill)
    ref, visible = _probs64(q, k, B, T, H, causal, keep, rows)
    assert torch.all(got[~visible.expand_as(got)] == 0)                         # exact zeros, and every element written
    assert torch.isfinite(got).all() and (got >= 0).all()
    err = ((got.double() - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    assert err < KERNEL_TOL, f"per-row relative L2 {err:.3g}"
    assert (got.sum(-1) - 1).abs().max() < 1e-5
    body.fill_(fill)
    ops.attention_probs(q, k, P, B=B, T=T, H=H, causal=causal, key_keep=keep, q_rows=rows)
    assert torch.equal(P, got)                                                  # two launches: bit-identical


def test_probs_kernel_limit_and_contract(monkeypatch):
    from cclip_hip import ops
    from cclip_hip._lib import CclipError
    T, H = 257, 2
    q = torch.zeros(T, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
    P = torch.empty(1, H, T, T, device="cuda")
    with pytest.raises(NotImplementedError, match="256"):
        ops.attention_probs(q[:, :128], q[:, 128:256], P, B=1, T=T, H=H, causal=True)
    monkeypatch.setattr(ops, "ATTENTION_PROBS_MAX_T", 1024)                     # the library refuses on its own
    with pytest.raises(CclipError, match="cclip_attention_probs.*status 1"):
        ops.attention_probs(q[:, :128], q[:, 128:256], P, B=1, T=T, H=H, causal=True)
    monkeypatch.undo()
    with pytest.raises(CclipError, match="status 1"):                           # rows not 16-byte aligned
        ops.attention_probs(q[:16, 4:132], q[:16, 128:256], P[:, :, :16, :16], B=1, T=16, H=H)
    # a row that sees no key is zeros, not NaN
    keep = torch.zeros(1, 16, device="cuda")
    Pz = torch.full((1, H, 16, 16), -7.0, device="cuda")
    ops.attention_probs(q[:16, :128], q[:16, 128:256], Pz, B=1, T=16, H=H, key_keep=keep)
    assert torch.all(Pz == 0)


# ---------------------------------------------------------------------------------------------- 2. output_attentions
_MODELS = {}


def _model(name, dtype, seed=31):
    key = (name, dtype, seed)
    if key not in _MODELS:
        from clip_caption import ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
        geo = GPT2_MODELS[name]
        sd = init_caption_state_dict(geo, seed)
        model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
        model.load_state_dict(sd)
        model = model.cuda().eval().set_compute_dtype(dtype)
        _MODELS[key] = (geo, sd, model)
    return _MODELS[key]


def _embeds(model, geo, sd, n, lc=6, seed=32):
    """(device embeddings [n, P + A + lc, D] = cat(clip_project(prefix), wte(attribute, tokens)), mask [n, P + A + lc])"""
    from clip_caption import synthetic_caption_batch
    tokens, mask, prefix, attribute = synthetic_caption_batch(n, geo, lc, seed)
    ids = torch.cat((attribute, tokens), dim=1)
    with torch.no_grad():
        pre = model.clip_project(prefix.cuda()).view(n, geo.prefix_length, geo.n_embd)
        emb = torch.cat((pre, model.gpt.transformer.wte(ids.cuda())), dim=1)
    return emb, mask


def _errors(got, ref):
    d = got.double().cpu() - ref
    return d.abs().max().item(), (d.norm() / ref.norm()).item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["test-tiny", "ckiplab/gpt2-base-chinese"])
@pytest.mark.parametrize("masked", [False, True])
def test_output_attentions_against_float64(name, dtype, masked):
    geo, sd, model = _model(name, dtype)
    emb, mask = _embeds(model, geo, sd, 3)
    B, S, _ = emb.shape
    mask = mask.clone()
    if masked:
        mask[1, -3:] = 0
    m = mask.cuda() if masked else None
    with torch.no_grad():
        plain = model.gpt(inputs_embeds=emb, attention_mask=m)
        out = model.gpt(inputs_embeds=emb, attention_mask=m, output_attentions=True)
    assert not hasattr(plain, "attentions")
    assert torch.equal(out.logits, plain.logits)
    assert isinstance(out.attentions, tuple) and len(out.attentions) == geo.n_layer
    ref = gpt2_attentions64(sd, emb.cpu(), mask if masked else None, geo.n_head)     # the same embedding rows, fp32 masters
    worst_abs = worst_rel = 0.0
    for l, a in enumerate(out.attentions):
        assert a.shape == (B, geo.n_head, S, S) and a.dtype == torch.float32 and a.is_cuda
        assert not a.triu(1).any()
        if masked:
            assert not a[1, :, :, -3:].any()
        e_abs, e_rel = _errors(a, ref[l])
        worst_abs, worst_rel = max(worst_abs, e_abs), max(worst_rel, e_rel)
    print(f"MEASURE output_attentions {name} {dtype} masked={masked}: max abs {worst_abs:.3e} rel L2 {worst_rel:.3e}")
    assert worst_abs < ATT_ABS[dtype] and worst_rel < ATT_REL[dtype], (worst_abs, worst_rel)
    row = out.attentions[-1][:, -1, -1, :]                                       # the reference's expression, test.py:383
    assert row.shape == (B, S) and (row.sum(-1) - 1).abs().max() < 1e-5
    # the model-level entry: a subset of layers and rows is the same numbers
    sub = model.attention_probs(emb, m, layers=[-1, 0], q_rows=[S - 1, 0, -2])
    assert sub.shape == (2, B, geo.n_head, 3, S) and sub.dtype == torch.float32
    assert torch.equal(sub[0, :, :, 0], out.attentions[-1][:, :, S - 1]) and torch.equal(sub[1, :, :, 2], out.attentions[0][:, :, S - 2])


def test_output_attentions_refusals():
    geo, sd, model = _model("test-tiny", torch.float16)
    emb, _ = _embeds(model, geo, sd, 1)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        model.gpt(inputs_embeds=emb, use_cache=True, output_attentions=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model.attention_probs(emb.clone().requires_grad_(True))
    long = torch.zeros(1, 257, geo.n_embd, device="cuda")
    with pytest.raises(NotImplementedError, match="256"):
        model.attention_probs(long)
    with pytest.raises(IndexError):
        model.attention_probs(emb, layers=[geo.n_layer])


# ---------------------------------------------------------------------------------------------- 3. decoding
def _check_beam_rows(att, gen, prefix_cpu, sd, geo, dtype, layer=-1):
    """att [H, n, S0 + n - 1] of one sequence against float64 on that sequence (prefix rows + wte of its tokens but the last)"""
    S0, n = prefix_cpu.shape[0], int(gen.numel())
    assert att.shape == (geo.n_head, n, S0 + n - 1) and att.dtype == torch.float32 and att.is_cuda
    frontier = torch.arange(S0 + n - 1)[None, :] < (S0 + torch.arange(n))[:, None]
    assert not att.cpu()[:, ~frontier].any()
    assert (att.sum(-1) - 1).abs().max() < ATT_ABS[dtype] + 1e-5
    seq = torch.cat((prefix_cpu, sd["model.transformer.wte.weight"][gen.cpu()[:n - 1]]), dim=0)[None]
    ref = gpt2_attentions64(sd, seq, None, geo.n_head)[layer][0, :, S0 - 1:]
    e_abs, e_rel = _errors(att, ref)
    print(f"MEASURE replay rows {dtype} n={n}: max abs {e_abs:.3e} rel L2 {e_rel:.3e}")
    assert e_abs < ATT_ABS[dtype] and e_rel < ATT_REL[dtype], (e_abs, e_rel)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert a == b


def _stop_token(model, emb, steps):
    """a token the greedy searches emit before their last step, so that the sequences stop at different lengths"""
    t = model.beam_search_native_batch(emb, 1, steps, 0.5, -1)[0]
    vals, counts = t[:, :, 1:].reshape(-1).unique(return_counts=True)
    for cand in vals[counts.argsort(descending=True, stable=True)].tolist():
        n_sel = model.beam_search_native_batch(emb, 1, steps, 0.5, cand)[3]
        if int(n_sel.min()) < steps and len(set(n_sel.tolist())) > 1:
            return cand
    raise AssertionError("no stop token splits the batch")


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_generate_return_attention(native, dtype, monkeypatch):
    from clip_caption import generate2, generate2_batch, generate_beam, generate_beam_batch
    geo, sd, model = _model("test-tiny", dtype)
    N, E = 5, 12
    emb = _embeds(model, geo, sd, N)[0][:, :geo.prefix_length + geo.attribute_length].contiguous()
    S0 = emb.shape[1]
    stop = _stop_token(model, emb, E)
    monkeypatch.setenv("CCLIP_BEAM_NATIVE", native)
    assert model.beam_native_ok(3) == (native == "1")
    tok, kw = _Tok(), dict(entry_length=E, stop_token=stop)

    # state that must survive: gradient arena, a training step's result, KV-cached decoding
    from clip_caption import synthetic_caption_batch
    tokens, mask, prefix, attribute = (t.cuda() for t in synthetic_caption_batch(4, geo, 6, 9))
    model.train()
    model.zero_grad(set_to_none=True)
    loss0 = model.caption_loss(tokens, prefix, attribute, mask)
    loss0.backward()
    model.eval()
    gflat0 = model.arena.gflat.clone()
    grads0 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    with torch.no_grad():
        c0 = model.gpt(inputs_embeds=emb[:1], use_cache=True)
        d0 = model.gpt(inputs_embeds=emb[:1, :1], past_key_values=c0.past_key_values, use_cache=True).logits.clone()

    lengths = set()
    for beams in (1, 3):
        base = generate_beam(model, tok, beam_size=beams, embed=emb[:1], return_tokens=True, **kw)
        got = generate_beam(model, tok, beam_size=beams, embed=emb[:1], return_tokens=True, return_attention=True, **kw)
        assert len(got) == 5
        _same(got[:4], base)
        texts_only = generate_beam(model, tok, beam_size=beams, embed=emb[:1], return_attention=True, **kw)
        assert texts_only[0] == base[0] and len(texts_only[1]) == beams
        _, tk, ln, _, att = got
        assert len(att) == beams
        for b in range(beams):
            n = int(ln[b])
            _check_beam_rows(att[b], tk[b, :n], emb[0].cpu(), sd, geo, dtype)
            lengths.add(n)
    first = generate_beam(model, tok, beam_size=3, embed=emb[:1], return_tokens=True, return_attention=True, attention_layer=0, **kw)
    _check_beam_rows(first[4][0], first[1][0, :int(first[2][0])], emb[0].cpu(), sd, geo, dtype, layer=0)

    # from a prompt: S0 is the prompt's length, the token rows start with the prompt
    prompt = "5 9 17 3"
    base = generate_beam(model, tok, beam_size=3, prompt=prompt, return_tokens=True, **kw)
    got = generate_beam(model, tok, beam_size=3, prompt=prompt, return_tokens=True, return_attention=True, **kw)
    _same(got[:4], base)
    pre = sd["model.transformer.wte.weight"][torch.tensor(tok.encode(prompt))]
    for b in range(3):
        _check_beam_rows(got[4][b], got[1][b, 4:4 + int(got[2][b])], pre, sd, geo, dtype)

    base = generate2(model, tok, embed=emb[1:2], return_tokens=True, **kw)
    got = generate2(model, tok, embed=emb[1:2], return_tokens=True, return_attention=True, **kw)
    assert len(got) == 3 and len(got[2]) == 1
    _same(got[:2], base)
    _check_beam_rows(got[2][0], got[1][0], emb[1].cpu(), sd, geo, dtype)
    assert generate2(model, tok, embed=emb[1:2], return_attention=True, **kw)[0] == base[0]

    base = generate_beam_batch(model, tok, emb, beam_size=3, return_tokens=True, **kw)
    got = generate_beam_batch(model, tok, emb, beam_size=3, return_tokens=True, return_attention=True, **kw)
    assert len(got) == 3 and len(got[2]) == N
    _same(got[:2], base)
    for i in range(N):
        tk, ln, _ = got[1][i]
        assert len(got[2][i]) == 3
        for b in range(3):
            _check_beam_rows(got[2][i][b], tk[b, :int(ln[b])], emb[i].cpu(), sd, geo, dtype)
            lengths.add(int(ln[b]))

    base = generate2_batch(model, tok, emb, return_tokens=True, **kw)
    got = generate2_batch(model, tok, emb, return_tokens=True, return_attention=True, **kw)
    assert len(got) == 3 and len(got[2]) == N
    _same(got[:2], base)
    for i in range(N):
        assert len(got[2][i]) == 1
        _check_beam_rows(got[2][i][0], got[1][i][0], emb[i].cpu(), sd, geo, dtype)
        lengths.add(int(got[1][i].shape[1]))
    assert len(lengths) > 1, lengths                                            # sequences of different lengths went through the padding

    # nothing else moved
    assert torch.equal(model.arena.gflat, gflat0)
    for k, p in model.named_parameters():
        assert (p.grad is None) == (k not in grads0) and (p.grad is None or torch.equal(p.grad, grads0[k])), k
    with torch.no_grad():
        c1 = model.gpt(inputs_embeds=emb[:1], use_cache=True)
        d1 = model.gpt(inputs_embeds=emb[:1, :1], past_key_values=c1.past_key_values, use_cache=True).logits
    assert torch.equal(c1.logits, c0.logits) and torch.equal(d1, d0)
    model.train()
    model.zero_grad(set_to_none=True)
    loss1 = model.caption_loss(tokens, prefix, attribute, mask)
    loss1.backward()
    model.eval()
    assert torch.equal(loss1, loss0)
    for k, p in model.named_parameters():
        if k in grads0:
            assert torch.equal(p.grad, grads0[k]), k
    model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------- 4. Captioner and the script
@pytest.mark.parametrize("greedy", [False, True])
def test_captioner_return_attention(greedy):
    import _common as C
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_images
    from clip_caption import Captioner
    geo, sd, model = _model("test-tiny", torch.float16)
    clip_model = clip.build_model(init_state_dict(MODELS["test-tiny"], 3)).cuda().eval().half()
    tok = C.ByteCaptionTokenizer(geo.vocab_size)
    cap = Captioner(clip_model, model, tok, clip_tokenize=C.get_tokenize(clip_model), caption_types={"s": "a", "v": "b"},
                    violation_types=["c", "d", "e", "f", "g", "h", "i", "j", "k"], prefix_length=geo.prefix_length,
                    attribute_length=geo.attribute_length)
    images = synthetic_images(6, clip_model.geo, 4).cuda()
    kw = dict(beam_size=3, entry_length=12, greedy=greedy)
    base, extra0 = cap.describe(images, return_tokens=True, **kw)
    got, extra = cap.describe(images, return_tokens=True, return_attention=True, **kw)
    assert all("attention" not in r for r in base)
    S0 = geo.prefix_length + geo.attribute_length
    for i, (r0, r1) in enumerate(zip(base, got)):
        assert set(r1) == set(r0) | {"attention"}
        assert {k: v for k, v in r1.items() if k != "attention"} == r0
        _same(extra["tokens"][i], extra0["tokens"][i])
        if greedy:
            n = extra["tokens"][i].shape[1]
        else:
            tk, ln, sc = extra["tokens"][i]
            n = int(ln[int(sc.argsort(descending=True)[0])])
        a = r1["attention"]
        assert a.shape == (geo.n_head, n, S0 + n - 1) and a.dtype == torch.float32 and a.is_cuda
        assert (a.sum(-1) - 1).abs().max() < 1e-5


def test_describe_images_script_attention_out(tmp_path):
    import numpy as np
    out = tmp_path / "att.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "describe_images.py"), "--synthetic", "--n_images", "5", "--bs", "4",
                        "--entry_length", "10", "--out_dir", str(tmp_path), "--attention-out", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    from clip_caption import GPT2_MODELS
    geo = GPT2_MODELS["test-tiny"]
    S0 = geo.prefix_length + geo.attribute_length
    assert sorted(z.files) == sorted([f"attention_{i}" for i in range(5)] + [f"map_{i}" for i in range(5)])
    for i in range(5):
        a, m = z[f"attention_{i}"], z[f"map_{i}"]
        n = a.shape[1]
        assert a.shape == (geo.n_head, n, S0 + n - 1) and a.dtype == np.float32 and 1 <= n <= 10
        assert m.shape == (n, S0 + n - 1)
        for j in range(n):
            assert np.array_equal(m[j, :S0 + j], a[-1, j, :S0 + j]) and np.all(m[j, S0 + j:] == 1)
