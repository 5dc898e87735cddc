"""Relevance maps on the MI355X: the fused kernel (csrc/attention_relevance.hip) against a float64 statement of its formula,
clip.interpret against the float64 restatement of the reference's interpret() (pinned in test_relevance_cpu.py), its batch /
packing semantics, and that it leaves no trace in the model's gradients or in a later training step.

Largest relative L2 errors of clip.interpret against float64 measured on one MI355X (fixtures tiny / small / ViT-B/32, 4 pairs,
start layers -1, 0 and the middle block; ViT-B/32 alone in parentheses):
  image relevance R[:, 0, 1:]   fp16 1.7e-3 (8.2e-4)     bf16 1.4e-2 (6.3e-3)
  text rows R[eot, :eot+1]      fp16 5.3e-4 (4.7e-5)     bf16 6.5e-3 (4.8e-4)
BOUND is about twice the largest; the arg-max patch agreed everywhere.  The kernel itself is fp32 arithmetic on the 16-bit
operands (KERNEL_TOL against float64).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from test_relevance_cpu import cams, forward64, rollout

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {torch.float16: dict(img=4e-3, txt=1.2e-3), torch.bfloat16: dict(img=3e-2, txt=1.5e-2)}
KERNEL_TOL = 1e-4


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64
# ------------------------------------------------------------------------------------------------------------------------
def _kernel_case(lens, T, H, causal, dtype, grad_scale=1.0, packed=False, seed=0, zero_da=False):
    from cclip_hip import ops
    g = torch.Generator().manual_seed(seed)
    B, D = len(lens), 64 * H
    M = sum(lens) if packed else B * T
    starts = ([sum(lens[:b]) for b in range(B)] if packed else [b * T for b in range(B)])
    qkv = (torch.randn(M, 3 * D, generator=g) * 0.6).to(dtype)
    da = torch.zeros(M, D, dtype=dtype) if zero_da else (torch.randn(M, D, generator=g) * grad_scale).to(dtype)
    R0 = torch.randn(B, T, T, generator=g)
    scale = 64 ** -0.5
    lse = torch.zeros(B, H, T)
    Rref = R0.double().clone()
    for b, (s0, Tb) in enumerate(zip(starts, lens)):
        C = torch.zeros(Tb, Tb, dtype=torch.float64)
        for h in range(H):
            q, k, v = (qkv[s0:s0 + Tb, j * D + 64 * h: j * D + 64 * h + 64].double() for j in range(3))
            s = q @ k.t() * scale
            if causal:
                s = s + torch.full((Tb, Tb), float("-inf"), dtype=torch.float64).triu(1)
            l32 = torch.logsumexp(s, dim=-1).float()
            lse[b, h, :Tb] = l32
            P = torch.exp(s - l32.double()[:, None])
            dP = da[s0:s0 + Tb, 64 * h: 64 * h + 64].double() @ v.t()
            C += (P * dP).clamp(min=0)
        C /= H * grad_scale
        Rref[b, :Tb, :Tb] = Rref[b, :Tb, :Tb] + Rref[b, :Tb, :Tb] @ C
    dev = "cuda"
    qkv_d, da_d = qkv.to(dev), da.to(dev)
    R = R0.to(dev)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev) if packed else None

    def launch(Rt):
        ops.attention_relevance(qkv_d[:, 0:D], qkv_d[:, D:2 * D], qkv_d[:, 2 * D:3 * D], lse.to(dev), da_d, Rt, B=B, T=T, H=H,
                                causal=causal, cu=cu, grad_scale=grad_scale)
    launch(R)
    R2 = R0.to(dev)
    launch(R2)
    torch.cuda.synchronize()
    return R0, R.cpu(), R2.cpu(), Rref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [2, 3, 8, 12])
@pytest.mark.parametrize("T", [1, 16, 24, 50, 77, 128])
def test_kernel_matches_fp64(T, H, causal, dtype):
    R0, R, R2, Rref = _kernel_case([T] * 3, T, H, causal, dtype, seed=T * 31 + H)
    assert torch.equal(R, R2), "two launches differ"
    d = rel(R - R0, Rref - R0.double())
    assert d < KERNEL_TOL, f"rel err of the update {d:.3g}"
    assert (R.double() - Rref).abs().max().item() < 1e-4 * max(1.0, Rref.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_kernel_packed_ragged(dtype):
    lens = [5, 77, 1, 40, 16, 33]
    T = 77
    R0, R, R2, Rref = _kernel_case(lens, T, 8, True, dtype, packed=True, seed=7)
    assert torch.equal(R, R2)
    assert (R.double() - Rref).abs().max().item() < 1e-4 * Rref.abs().max().item()
    for b, Tb in enumerate(lens):
        assert torch.equal(R[b, Tb:], R0[b, Tb:]), f"rows past length {Tb} of sequence {b} changed"
        assert torch.equal(R[b, :, Tb:], R0[b, :, Tb:]), f"columns past length {Tb} of sequence {b} changed"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_kernel_grad_scale(dtype):
    R0, R, _, Rref = _kernel_case([50, 50], 50, 12, False, dtype, grad_scale=1024.0, seed=5)
    assert rel(R - R0, Rref - R0.double()) < KERNEL_TOL


def test_kernel_zero_gradient_leaves_R():
    R0, R, _, _ = _kernel_case([77, 77], 77, 8, True, torch.bfloat16, zero_da=True)
    assert torch.equal(R, R0)


# ------------------------------------------------------------------------------------------------------------------------
# 2. clip.interpret against the float64 restatement
# ------------------------------------------------------------------------------------------------------------------------
FIXTURES = ["clip_test_tiny.pt", "clip_test_small.pt", "clip_vit_b32.pt"]
NPAIR = 4


@functools.lru_cache(maxsize=None)
def _fixture(fix):
    from clip.weights import MODELS, init_state_dict, synthetic_images
    g = torch.load(os.path.join(GOLD, fix), weights_only=True)
    geo = MODELS[g["model"]]
    sd = init_state_dict(geo, g["seed"])
    img = synthetic_images(g["n"], geo, g["seed"] + 1)[:NPAIR]
    txt = g["text"][:NPAIR]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.enable_grad():
        logits, pi, pt = forward64(sd64, img, txt)
        logits.diagonal().sum().backward()
    return sd, img, txt, cams(pi), cams(pt)


def _model(sd, dtype):
    import clip
    return clip.build_model(sd, dtype).cuda()


def _errors(r_txt, r_img, txt, rt_ref, ri_ref):
    e_img = rel(r_img, ri_ref[:, 0, 1:])
    e_txt = 0.0
    for b in range(txt.shape[0]):
        e = int(txt[b].long().argmax())
        e_txt = max(e_txt, rel(r_txt[b, e, :e + 1], rt_ref[b, e, :e + 1]))
    return e_img, e_txt


def _argmax_patch_agrees(r_img, ri_ref, bound):
    ref = ri_ref[:, 0, 1:]
    top2 = ref.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * bound * ref.abs().amax(dim=1)
    same = r_img.cpu().argmax(dim=1) == ref.argmax(dim=1)
    return bool(same[decided].all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fix", FIXTURES)
def test_interpret_matches_fp64(fix, dtype):
    import clip
    sd, img, txt, ci, ct = _fixture(fix)
    model = _model(sd, dtype)
    Li, Lt = len(ci), len(ct)
    b = BOUND[dtype]
    report = []
    for s_img, s_txt in ((-1, -1), (0, 0), (Li // 2, Lt // 2)):
        r_txt, r_img = clip.interpret(img.cuda(), txt.cuda(), model, start_layer=s_img, start_layer_text=s_txt)
        torch.cuda.synchronize()
        assert r_txt.shape == (NPAIR, txt.shape[1], txt.shape[1]) and r_img.shape == (NPAIR, ci[0].shape[-1] - 1)
        assert r_txt.dtype == torch.float32 and r_img.dtype == torch.float32 and r_txt.is_cuda
        e_img, e_txt = _errors(r_txt, r_img, txt, rollout(ct, s_txt), rollout(ci, s_img))
        report.append((s_img, s_txt, round(e_img, 6), round(e_txt, 6)))
        report[-1] += (_argmax_patch_agrees(r_img, rollout(ci, s_img), b["img"]),)
    print(f"\n[relevance] {fix} {dtype}: (start_img, start_txt, rel_img, rel_txt, argmax_ok) {report}")
    for _, _, e_img, e_txt, ok in report:
        assert e_img < b["img"] and e_txt < b["txt"] and ok, f"{fix} {dtype}: {report}"


# ------------------------------------------------------------------------------------------------------------------------
# 3. semantics
# ------------------------------------------------------------------------------------------------------------------------
def test_one_image_many_texts_is_the_repeat():
    import clip
    sd, img, txt, _, _ = _fixture("clip_test_small.pt")
    model = _model(sd, torch.bfloat16)
    a = clip.interpret(img[:1].cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    b = clip.interpret(img[:1].repeat(NPAIR, 1, 1, 1).cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pairs_at_once_equal_single_calls():
    import clip
    sd, img, txt, _, _ = _fixture("clip_test_small.pt")
    model = _model(sd, torch.float16)
    r_txt, r_img = clip.interpret(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    for i in range(NPAIR):
        t1, i1 = clip.interpret(img[i:i + 1].cuda(), txt[i:i + 1].cuda(), model, start_layer=0, start_layer_text=0)
        assert rel(i1[0], r_img[i]) < BOUND[torch.float16]["img"]
        e = int(txt[i].long().argmax())
        assert rel(t1[0, :e + 1, :e + 1], r_txt[i, :e + 1, :e + 1]) < BOUND[torch.float16]["txt"]


@pytest.mark.parametrize("tail", ["0", "1"])
@pytest.mark.parametrize("pack", [False, True])
def test_packing_and_tail_rows_agree(pack, tail, monkeypatch):
    import clip
    sd, img, txt, _, _ = _fixture("clip_vit_b32.pt")
    model = _model(sd, torch.float16)
    monkeypatch.setenv("CCLIP_TAIL_ROWS", "1")
    model.pack_text_rows = True
    base = clip.interpret(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    monkeypatch.setenv("CCLIP_TAIL_ROWS", tail)
    model.pack_text_rows = pack
    got = clip.interpret(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    assert rel(got[1], base[1]) < BOUND[torch.float16]["img"]
    for b in range(NPAIR):
        e = int(txt[b].long().argmax())
        assert rel(got[0][b, :e + 1], base[0][b, :e + 1]) < BOUND[torch.float16]["txt"]


def test_vit_b32_batch_1024():
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_text
    geo = MODELS["ViT-B/32"]
    model = _model(init_state_dict(geo, 567), torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(1)
    img = torch.randn(1024, 3, 224, 224, device="cuda", generator=g)
    txt = synthetic_text(1024, geo, 3).cuda()
    r_txt, r_img = model.relevance(img, txt, start_layer=0, start_layer_text=0)
    assert torch.isfinite(r_txt).all() and torch.isfinite(r_img).all()
    assert (r_txt >= 0).all() and (r_img >= 0).all()
    assert (r_txt.diagonal(dim1=1, dim2=2) >= 1).all() and (r_img.diagonal(dim1=1, dim2=2) >= 1).all()
    t8, i8 = model.relevance(img[:8], txt[:8], start_layer=0, start_layer_text=0)
    assert rel(r_img[:8], i8) < BOUND[torch.bfloat16]["img"]
    for b in range(8):
        e = int(txt[b].long().argmax())
        assert rel(r_txt[b, :e + 1], t8[b, :e + 1]) < BOUND[torch.bfloat16]["txt"]


# ------------------------------------------------------------------------------------------------------------------------
# 4. no side effects
# ------------------------------------------------------------------------------------------------------------------------
def _train_step(model, img, txt):
    li, lt = model(img, txt)
    lab = torch.arange(img.shape[0], device="cuda")
    loss = (torch.nn.functional.cross_entropy(li, lab) + torch.nn.functional.cross_entropy(lt, lab)) / 2
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_interpret_leaves_gradients_alone(dtype):
    import clip
    sd, img, txt, _, _ = _fixture("clip_test_small.pt")
    model = _model(sd, dtype)
    model.train()
    img, txt = img.cuda(), txt.cuda()
    _train_step(model, img, txt)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads
    slots = model.arena.gflat.clone()
    clip.interpret(img, txt, model, start_layer=0, start_layer_text=0)
    torch.cuda.synchronize()
    assert torch.equal(model.arena.gflat, slots)
    for n, p in model.named_parameters():
        if n in grads:
            assert torch.equal(p.grad, grads[n]), n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_training_step_after_interpret_is_unchanged(dtype):
    import clip
    sd, img, txt, _, _ = _fixture("clip_test_small.pt")
    img, txt = img.cuda(), txt.cuda()
    a, b = _model(sd, dtype), _model(sd, dtype)
    a.train(); b.train()
    clip.interpret(img, txt, a, start_layer=0, start_layer_text=0)
    la, lb = _train_step(a, img, txt), _train_step(b, img, txt)
    assert torch.equal(la, lb)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, pb[n].grad), n


# ------------------------------------------------------------------------------------------------------------------------
# 5. / 6. limits and the script
# ------------------------------------------------------------------------------------------------------------------------
def test_long_sequences_raise():
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_images, synthetic_text
    geo = MODELS["test-long"]
    model = _model(init_state_dict(geo, 13), torch.bfloat16)
    with pytest.raises(NotImplementedError, match="128"):
        clip.interpret(synthetic_images(2, geo, 1).cuda(), synthetic_text(2, geo, 2).cuda(), model)


def test_explain_script_synthetic(tmp_path):
    import numpy as np
    out = tmp_path / "rel.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "explain_clip.py"), "--synthetic", "--model", "test-small",
                        "--out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert z["image_map"].shape == (224, 224) and 0 <= z["image_map"].min() and z["image_map"].max() <= 1
    assert z["token_scores"].ndim == 1 and abs(z["token_scores"].sum() - 1) < 1e-4
    assert (tmp_path / "rel.png").exists()
