"""Caption evaluation: ClipCaptionModel.score / clip_caption.evaluate_captions (one fused lm_head scoring launch pair,
no logits) against the paths they replace - forward() + log_softmax + gather, caption_loss under no_grad, and the stored
oracle losses - plus their freedom from side effects and the eval / train scripts.

Tolerances: 1e-4 absolute on a token's log-probability and on the loss against the same build's own logits (KERNEL_TOL
of the fp32-arithmetic kernels); against the oracle the loss tolerances tests/test_caption_parity_gpu.py uses for caption_loss.

The tests print what they measure (the largest log-probability difference, the losses compared).  No MI355X run of this
file has been recorded yet, so no device figure is quoted here.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DTYPES = [torch.bfloat16, torch.float16]
TOL = 1e-4
GAP = 1e-4


def _model(geo, seed, dtype):
    from clip_caption import ClipCaptionModel, init_caption_state_dict
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, seed))
    model = model.cuda().eval()
    if dtype == torch.float16:
        model.half()
    return model


def _ragged_batch(geo, b=8, lc=10, seed=21):
    """captions with different numbers of trailing zeros: one of a single token, one of full length, one with a zero inside"""
    from clip_caption import synthetic_caption_batch
    tokens, mask, prefix, attribute = synthetic_caption_batch(b, geo, lc, seed)
    tokens[0, 1:] = 0
    tokens[1] = torch.randint(1, geo.vocab_size, (lc,), generator=torch.Generator().manual_seed(seed + 1))
    tokens[2, 1] = 0                                                # an ignored target inside a caption
    assert tokens[2, 2:].ne(0).any() and len({int(n) for n in tokens.ne(0).sum(1)}) >= 4
    return tokens.cuda(), mask.cuda(), prefix.cuda(), attribute.cuda()


def _from_logits(model, geo, tokens, mask, prefix, attribute):
    """what score() replaces: forward() logits -> log_softmax -> gather (float64 on the fp32 logits)"""
    P, A = geo.prefix_length, geo.attribute_length
    with torch.no_grad():
        sl = model(tokens, prefix, attribute, mask).logits[:, P + A - 1:-1].double()
    logp = torch.log_softmax(sl, -1).gather(2, tokens[:, :, None])[:, :, 0]
    top = sl.topk(2, -1).values
    return logp, sl.argmax(-1), top[..., 0] - top[..., 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_matches_forward_logits(dtype):
    from clip_caption import CaptionScores, GPT2_MODELS
    geo = GPT2_MODELS["test-tiny"]
    model = _model(geo, 5, dtype)
    tokens, mask, prefix, attribute = _ragged_batch(geo)
    sc = model.score(tokens, prefix, attribute, mask)
    assert isinstance(sc, CaptionScores)
    B, Lc = tokens.shape
    assert sc.token_logp.shape == (B, Lc) and sc.token_logp.dtype == torch.float32
    assert sc.token_pred.shape == (B, Lc) and sc.token_pred.dtype == torch.int32
    assert sc.token_correct.shape == (B, Lc) and sc.token_correct.dtype == torch.bool
    assert sc.n_tokens.dtype == torch.int32 and sc.nll.dtype == torch.float32 and sc.nll.shape == (B,)
    ref_logp, ref_pred, gap = _from_logits(model, geo, tokens, mask, prefix, attribute)
    keep = tokens != 0
    err = (sc.token_logp.double() - ref_logp)[keep].abs().max().item()
    clear = keep & (gap > GAP)
    print(f"{dtype}: max |token_logp - log_softmax(logits)| {err:.3e} over {int(keep.sum())} targets; "
          f"{int((keep & ~clear).sum())} with a top-2 gap <= {GAP}")
    assert err < TOL
    assert torch.equal(sc.token_logp[~keep], torch.zeros_like(sc.token_logp[~keep]))        # exactly 0 where ignored
    assert int((keep & ~clear).sum()) <= 0.01 * int(keep.sum())
    assert torch.equal(sc.token_pred[clear].long(), ref_pred[clear])
    assert (sc.token_pred[~keep] == -1).all()
    assert torch.equal(sc.n_tokens.long(), keep.sum(1))
    assert torch.equal(sc.nll, -sc.token_logp.sum(1))
    assert torch.equal(sc.token_correct, keep & (sc.token_pred == tokens))
    assert not sc.token_correct[~keep].any()
    # the dense pass (packing off) gives the same scores
    model.pack_rows = False
    dense = model.score(tokens, prefix, attribute, mask)
    assert (dense.token_logp - sc.token_logp).abs().max().item() < TOL and torch.equal(dense.n_tokens, sc.n_tokens)


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_loss_matches_caption_loss(dtype):
    from clip_caption import GPT2_MODELS
    geo = GPT2_MODELS["test-tiny"]
    model = _model(geo, 5, dtype)
    tokens, mask, prefix, attribute = _ragged_batch(geo)
    with torch.no_grad():
        ref = model.caption_loss(tokens, prefix, attribute, mask)
    loss = model.score(tokens, prefix, attribute, mask).loss
    print(f"{dtype}: score().loss {loss.item():.6f} caption_loss {ref.item():.6f}")
    assert loss.shape == () and abs(loss.item() - ref.item()) < TOL


@pytest.mark.parametrize("fix,dtype,tol", [("caption_test_tiny.pt", torch.bfloat16, 5e-3), ("caption_test_tiny.pt", torch.float16, 6e-4),
                                           ("caption_gpt2_base_chinese.pt", torch.bfloat16, 5e-3),
                                           ("caption_gpt2_base_chinese.pt", torch.float16, 1e-3)])
def test_score_loss_matches_oracle(fix, dtype, tol):
    from clip_caption import GPT2_MODELS, synthetic_caption_batch
    g = torch.load(os.path.join(GOLD, fix), weights_only=True)
    geo = GPT2_MODELS[g["model"]]
    model = _model(geo, g["seed"], dtype)
    tokens, mask, prefix, attribute = [t.cuda() for t in synthetic_caption_batch(g["b"], geo, g["lc"], g["seed"] + 1)]
    loss = model.score(tokens, prefix, attribute, mask).loss.item()
    print(f"{fix} {dtype}: score().loss {loss:.6f} oracle {g['loss'].item():.6f}")
    assert abs(loss - g["loss"].item()) < tol


def test_evaluate_captions_does_not_depend_on_the_batching():
    from clip_caption import GPT2_MODELS, evaluate_captions
    geo = GPT2_MODELS["test-tiny"]
    model = _model(geo, 5, torch.bfloat16)
    batch = _ragged_batch(geo)
    whole = evaluate_captions(model, [batch])
    parts = evaluate_captions(model, [tuple(t[:5] for t in batch), tuple(t[5:] for t in batch)])
    assert set(whole) == {"loss", "perplexity", "token_accuracy", "caption_exact", "n_captions", "n_tokens"}
    assert abs(parts["loss"] - whole["loss"]) <= 1e-5 * abs(whole["loss"])
    for k in ("n_captions", "n_tokens"):
        assert isinstance(whole[k], int) and parts[k] == whole[k]
    assert parts["token_accuracy"] == whole["token_accuracy"] and parts["caption_exact"] == whole["caption_exact"]
    assert whole["perplexity"] == math.exp(whole["loss"])
    sc = model.score(*[batch[i] for i in (0, 2, 3, 1)])
    assert whole["n_captions"] == 8 and whole["n_tokens"] == int(sc.n_tokens.sum())
    assert whole["token_accuracy"] == int(sc.token_correct.sum()) / whole["n_tokens"]
    assert abs(whole["loss"] - sc.loss.item()) <= 1e-5 * abs(whole["loss"])


# ---- no side effects (the pattern of tests/test_relevance_gpu.py section 4) ---------------------------------------------
def _train_step(model, tokens, mask, prefix, attribute):
    loss = model.caption_loss(tokens, prefix, attribute, mask)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach()


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_leaves_gradients_alone(dtype):
    from clip_caption import GPT2_MODELS
    geo = GPT2_MODELS["test-tiny"]
    model = _model(geo, 5, dtype).train()
    batch = _ragged_batch(geo)
    _train_step(model, *batch)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads
    slots = model.arena.gflat.clone()
    in_train = model.score(batch[0], batch[2], batch[3], batch[1])
    torch.cuda.synchronize()
    assert torch.equal(model.arena.gflat, slots)
    for n, p in model.named_parameters():
        if n in grads:
            assert torch.equal(p.grad, grads[n]), n
    assert not in_train.token_logp.requires_grad and model.training
    model.eval()
    in_eval = model.score(batch[0], batch[2], batch[3], batch[1])
    for s, t in zip(in_train, in_eval):
        assert torch.equal(s, t)                                    # train() or eval(): the same bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_step_after_score_is_unchanged(dtype):
    from clip_caption import GPT2_MODELS
    geo = GPT2_MODELS["test-tiny"]
    a, b = _model(geo, 5, dtype).train(), _model(geo, 5, dtype).train()
    batch = _ragged_batch(geo)
    a.score(batch[0], batch[2], batch[3], batch[1])
    la, lb = _train_step(a, *batch), _train_step(b, *batch)
    assert torch.equal(la, lb)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, pb[n].grad), n


# ---- scripts ------------------------------------------------------------------------------------------------------------
def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), *args], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = []
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            lines.append(json.loads(ln))
    return lines


def test_eval_script_synthetic():
    lines = _run("eval_caption.py", "--synthetic", "--bs", "24")
    assert len(lines) == 1
    res = lines[0]
    assert set(res) == {"loss", "perplexity", "token_accuracy", "caption_exact", "n_captions", "n_tokens"}
    assert all(math.isfinite(float(v)) for v in res.values())
    assert res["n_captions"] == 64 and res["n_tokens"] > 64 and res["loss"] > 0 and 0 <= res["token_accuracy"] <= 1


def test_train_script_logs_validation_only_when_asked():
    common = ("--synthetic", "--gpt2", "test-tiny", "--epochs", "2", "--bs", "8", "--max-steps", "8")
    lines = _run("train_caption.py", *common, "--val-fraction", "0.25")
    val = [ln for ln in lines if "val_loss" in ln]
    assert [ln["epoch"] for ln in val] == [0, 1]                     # once per epoch
    for ln in val:
        assert math.isfinite(ln["val_loss"]) and ln["val_captions"] == 16
        assert abs(ln["val_perplexity"] - math.exp(ln["val_loss"])) < 1e-3 * ln["val_perplexity"] and 0 <= ln["val_token_accuracy"] <= 1
    plain = _run("train_caption.py", *common)
    assert plain and not any(k.startswith("val_") for ln in plain for k in ln)
