"""generate_sample / generate_sample_batch (clip_caption/generate.py) on the GPU, at the small caption geometry of
tests/test_decode_gpu.py: greedy limit against generate2's host loop, seeding, a replay of every sample through one full
forward, the stop rule, the bookkeeping of lengths / sums / ordering, the batch form and the script."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# what tests/test_decode_gpu.py::test_kv_cache_equals_full_forward holds the cached step to against the full forward (fp16)
STEP_TOL = 2e-3
E = 12


class _Tok:
    def encode(self, s):
        return [int(x) for x in s.split()]

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


@pytest.fixture(scope="module")
def setup():
    from clip_caption import ClipCaptionModel, GPT2_MODELS, init_caption_state_dict, synthetic_caption_batch
    geo = GPT2_MODELS["test-tiny"]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval().half()
    _, _, prefix, attribute = synthetic_caption_batch(3, geo, 6, 32)
    with torch.no_grad():
        pre = model.clip_project(prefix.cuda()).view(3, geo.prefix_length, geo.n_embd)
        emb = torch.cat((pre, model.gpt.transformer.wte(attribute.cuda())), dim=1)
        # a stop token some samples reach and others do not: the second most probable first token
        stop = int(model.gpt(inputs_embeds=emb[:1]).logits[0, -1].topk(2).indices[1])
    return geo, model, emb, stop


def _replay_logprobs(model, prefix, row, n):
    """log-probabilities of row[:n] from ONE full forward over [prefix, wte(row[:n-1])]"""
    x = prefix[None]
    if n > 1:
        x = torch.cat((x, model.gpt.transformer.wte(row[None, :n - 1].long())), dim=1)
    with torch.no_grad():
        logits = model.gpt(inputs_embeds=x).logits[0, prefix.shape[0] - 1:]
    return logits.double().log_softmax(-1).gather(1, row[:n, None].long())[:, 0]


def _check_sample_rows(model, prefix, tokens, lengths, total, logprobs, stop):
    K, steps = tokens.shape
    assert tokens.dtype == torch.int32 and tuple(lengths.shape) == (K,) == tuple(total.shape) and logprobs.shape == tokens.shape
    worst = 0.0
    for j in range(K):
        n, row = int(lengths[j]), tokens[j]
        hits = (row == stop).nonzero()
        assert n == (int(hits[0]) + 1 if len(hits) else steps)          # ends at its first stop token, or at the last position
        assert (row[n:] == 0).all() and (logprobs[j, n:] == 0).all()    # a finished sample only appends token 0, at no cost
        assert abs(float(total[j]) - float(logprobs[j, :n].double().sum())) < 1e-4
        d = (_replay_logprobs(model, prefix, row, n) - logprobs[j, :n].double()).abs().max().item()
        worst = max(worst, d)
        assert d < STEP_TOL, (j, d)
    return worst


def test_top_k_1_is_generate2s_host_loop(setup, monkeypatch):
    from clip_caption import generate2, generate_sample
    geo, model, emb, stop = setup
    monkeypatch.setenv("CCLIP_BEAM_NATIVE", "0")                         # generate2's host loop: the same step kernels and logits
    assert not model.beam_native_ok(1)
    for i in range(3):
        for st in (stop, 7):
            text, want = generate2(model, _Tok(), embed=emb[i:i + 1], entry_length=E, stop_token=st, return_tokens=True)
            texts, tokens, lengths, _ = generate_sample(model, _Tok(), embed=emb[i:i + 1], num_samples=2, entry_length=E, top_k=1,
                                                        top_p=1.0, stop_token=st, return_tokens=True)
            n = want.shape[1]
            assert lengths.tolist() == [n, n]
            assert torch.equal(tokens[0, :n].long(), want[0]) and torch.equal(tokens[1], tokens[0])
            assert texts == [text, text]


def test_seeds(setup):
    from clip_caption import generate_sample
    geo, model, emb, stop = setup
    kw = dict(embed=emb[:1], num_samples=8, entry_length=E, top_p=1.0, temperature=1.0, stop_token=stop, return_tokens=True)

    def run(seed):
        return generate_sample(model, _Tok(), generator=torch.Generator(device="cuda").manual_seed(seed), **kw)
    a, b, c = run(3), run(3), run(4)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert a[1].shape != c[1].shape or not torch.equal(a[1], c[1])
    assert len({tuple(r) for r in a[1].tolist()}) > 1                    # and the 8 samples of one seed are not one caption
    cpu = generate_sample(model, _Tok(), generator=torch.Generator().manual_seed(3), **kw)      # a CPU generator seeds too
    assert torch.equal(cpu[1], generate_sample(model, _Tok(), generator=torch.Generator().manual_seed(3), **kw)[1])


@pytest.mark.parametrize("kw", [dict(top_p=1.0), dict(top_p=0.8), dict(top_p=1.0, top_k=5)])
def test_replay_stop_rule_and_bookkeeping(setup, kw):
    from clip_caption import generate_sample
    geo, model, emb, stop = setup
    g = torch.Generator(device="cuda").manual_seed(11)
    texts, tokens, lengths, total, logprobs = generate_sample(model, _Tok(), embed=emb[1:2], num_samples=8, entry_length=E, temperature=1.0,
                                                              stop_token=stop, generator=g, return_tokens=True, return_logprobs=True, **kw)
    worst = _check_sample_rows(model, emb[1], tokens, lengths, total, logprobs, stop)
    print(f"{kw}: largest |replayed - returned| log-probability {worst:.2e}")
    order = (total / lengths).argsort(descending=True, stable=True).tolist()
    assert texts == [" ".join(str(t) for t in tokens[i, :int(lengths[i])].tolist()) for i in order]
    means = [float(total[i] / lengths[i]) for i in order]
    assert means == sorted(means, reverse=True)
    assert generate_sample(model, _Tok(), embed=emb[1:2], num_samples=8, entry_length=E, temperature=1.0, stop_token=stop,
                           generator=torch.Generator(device="cuda").manual_seed(11), **kw) == texts


def test_uniforms_override_and_prompt(setup):
    from clip_caption import generate_sample
    geo, model, emb, stop = setup
    u = torch.rand(E, 4, generator=torch.Generator().manual_seed(5))
    a = generate_sample(model, _Tok(), embed=emb[:1], num_samples=4, entry_length=E, stop_token=stop, uniforms=u, return_tokens=True)
    b = generate_sample(model, _Tok(), embed=emb[:1], num_samples=4, entry_length=E, stop_token=stop, uniforms=u.cuda(), return_tokens=True)
    assert torch.equal(a[1], b[1])
    # u = 0 at every position and no filter: the lowest id with any mass, every time
    z = generate_sample(model, _Tok(), embed=emb[:1], num_samples=1, entry_length=3, top_p=1.0, stop_token=-1,
                        uniforms=torch.zeros(3, 1), return_tokens=True)
    assert z[1].tolist() == [[0, 0, 0]]
    with pytest.raises(ValueError, match="uniforms"):
        generate_sample(model, _Tok(), embed=emb[:1], num_samples=4, entry_length=E, uniforms=u[:, :3])
    texts = generate_sample(model, _Tok(), prompt="5 9 11 3", num_samples=2, entry_length=4, stop_token=-1,
                            generator=torch.Generator(device="cuda").manual_seed(1))
    assert len(texts) == 2 and all(t.startswith("5 9 11 3 ") and len(t.split()) == 8 for t in texts)


def test_batch(setup):
    from clip_caption import generate_sample, generate_sample_batch
    geo, model, emb, stop = setup
    u = torch.rand(E, 6, generator=torch.Generator().manual_seed(9))
    out = generate_sample_batch(model, _Tok(), emb, num_samples=2, entry_length=E, top_p=1.0, stop_token=stop, uniforms=u,
                                return_tokens=True, return_logprobs=True)
    plain = generate_sample_batch(model, _Tok(), emb, num_samples=2, entry_length=E, top_p=1.0, stop_token=stop, uniforms=u)
    assert len(out) == 3 == len(plain)
    for i, (texts, tokens, lengths, total, logprobs) in enumerate(out):
        assert len(texts) == 2 and texts == plain[i] and tokens.shape[0] == 2
        _check_sample_rows(model, emb[i], tokens, lengths, total, logprobs, stop)


def test_errors(setup):
    from clip_caption import generate_sample, generate_sample_batch
    geo, model, emb, stop = setup
    with pytest.raises(TypeError, match="cuda"):
        generate_sample(model, _Tok(), embed=emb[:1].cpu())
    with pytest.raises(ValueError, match="num_samples"):
        generate_sample(model, _Tok(), embed=emb[:1], num_samples=0)
    with pytest.raises(ValueError, match="entry_length"):
        generate_sample_batch(model, _Tok(), emb, entry_length=0)


def test_describe_images_script_sample(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "describe_images.py"), "--synthetic", "--n_images", "3",
                        "--entry_length", "8", "--sample", "3", "--seed", "1", "--out_dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = json.loads((tmp_path / "output_ct.json").read_text())["caption"]
    assert len(recs) == 3
    for rec in recs:
        assert set(rec) == {"caption_type", "violation_type", "prediction", "caption", "file_name", "samples"}
        assert len(rec["samples"]) == 3 and all(isinstance(s, str) for s in rec["samples"])
