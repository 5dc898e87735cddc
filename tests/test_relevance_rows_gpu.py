"""Relevance rows on the MI355X: the row kernel (csrc/attention_relevance_row.hip) against a float64 statement of its formula
at every tile / key-block edge and at the long towers' lengths, against the full-matrix kernel where that one exists, its
launcher's refusals; clip.interpret_rows against the float64 restatement of the reference's interpret() (pinned in
test_relevance_cpu.py / test_relevance_rows_cpu.py) and against clip.interpret on the towers of at most 128 tokens, on the long
towers (test-long: 145 image tokens; ViT-B/16: 197), its batch / packing semantics, and that it leaves no trace in the model's
gradients or in a later training step.

Largest relative L2 errors of clip.interpret_rows against float64 measured on one MI355X on the long towers (test-long: seed 13,
4 pairs, start layers -1, 0, 1; ViT-B/16: seeded init_state_dict, 2 pairs, start layers -1, 0):
  test-long  image row R[0, 1:]    fp16 1.30e-3    bf16 1.31e-2      text row R[eot, :eot+1]   fp16 5.5e-4    bf16 5.2e-3
  ViT-B/16   image row R[0, 1:]    fp16 8.0e-4     bf16 6.3e-3       text row R[eot, :eot+1]   fp16 4.3e-5    bf16 2.7e-4
LONG_BOUND is about twice these; the arg-max patch agreed everywhere.  ViT-B/16 is at the ViT-B/32 figures of
test_relevance_gpu.py's docstring (8.2e-4 / 6.3e-3 image, 4.7e-5 / 4.8e-4 text).  test-long's text rows are more than 3x the
ViT-B/32 text figures: its text tower is 2 blocks of width 128 on 16 tokens, the family of the tiny / small fixtures, whose text
figures in that docstring are the same (5.3e-4 / 6.5e-3) and which the row path reproduces on those fixtures (5.2e-4 / 6.5e-3
measured here); the row kernel itself agrees with the full-matrix kernel and with float64 to KERNEL_TOL.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from test_relevance_cpu import cams, forward64, rollout
from test_relevance_gpu import (BOUND, FIXTURES, KERNEL_TOL, NPAIR, ROOT, _argmax_patch_agrees, _fixture, _model, _train_step,
                                rel)

pytestmark = pytest.mark.gpu

# Long towers: no bound can be derived in advance - about twice the largest error measured on one MI355X (module docstring)
LONG_BOUND = {
    "test-long": {torch.float16: dict(img=2.6e-3, txt=1.1e-3), torch.bfloat16: dict(img=2.6e-2, txt=1.0e-2)},
    "ViT-B/16": {torch.float16: dict(img=1.6e-3, txt=9e-5), torch.bfloat16: dict(img=1.3e-2, txt=5.4e-4)},
}
# two runs of the same 16-bit chain (pairs at once / single calls, packed / dense text rows): the dtype's bound, the larger of
# the models' - each run is within the measured error of float64, so they are within twice that of each other
DTYPE_BOUND = {dt: {k: max(LONG_BOUND[m][dt][k] for m in LONG_BOUND) for k in ("img", "txt")} for dt in (torch.float16, torch.bfloat16)}


# ------------------------------------------------------------------------------------------------------------------------
# 1. - 5. the kernel
# ------------------------------------------------------------------------------------------------------------------------
def _inputs(lens, T, H, causal, dtype, grad_scale=1.0, packed=False, seed=0, zero_da=False):
    """Random operands of one layer and, per sequence, the float64 C = 1/(H grad_scale) sum_h max(P_h (.) dP_h, 0) with
    P_h = exp(scale Q_h K_h^T - lse_h), lse the float64 log-sum-exp rounded to fp32 (what the kernel is given), dP_h = dA_h V_h^T."""
    g = torch.Generator().manual_seed(seed)
    B, D = len(lens), 64 * H
    M = sum(lens) if packed else B * T
    starts = ([sum(lens[:b]) for b in range(B)] if packed else [b * T for b in range(B)])
    qkv = (torch.randn(M, 3 * D, generator=g) * 0.6).to(dtype)
    da = torch.zeros(M, D, dtype=dtype) if zero_da else (torch.randn(M, D, generator=g) * grad_scale).to(dtype)
    scale = 64 ** -0.5
    lse = torch.zeros(B, H, T)
    Cs = []
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
        Cs.append(C / (H * grad_scale))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda") if packed else None
    return dict(B=B, T=T, H=H, D=D, causal=causal, lens=lens, grad_scale=grad_scale, qkv=qkv.cuda(), da=da.cuda(), lse=lse.cuda(),
                C=Cs, cu=cu)


def _r_in(B, T, seed):
    """Both signs; about a quarter of the entries exactly 0, among them one whole aligned 16-row tile where T allows (the
    kernel's skip path)."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.randn(B, T, generator=g)
    if T >= 4:
        r[torch.rand(B, T, generator=g) < 0.25] = 0
    if T >= 32:
        r[:, 16:32] = 0
    return r


def _ref(inp, r0):
    ref = r0.double().clone()
    for b, Tb in enumerate(inp["lens"]):
        ref[b, :Tb] += r0[b, :Tb].double() @ inp["C"][b]
    return ref


def _launch(inp, r_in, r_out, **over):
    from cclip_hip import ops
    D, qkv = inp["D"], inp["qkv"]
    kw = dict(B=inp["B"], T=inp["T"], H=inp["H"], causal=inp["causal"], cu=inp["cu"], grad_scale=inp["grad_scale"])
    kw.update(over)
    ops.attention_relevance_row(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], inp["lse"], inp["da"], r_in, r_out, **kw)


def _run_twice(inp, r0):
    """(first result, second result, r_in after the launches), on the host"""
    r_in = r0.cuda()
    a, b = torch.full_like(r_in, float("nan")), torch.full_like(r_in, float("nan"))
    _launch(inp, r_in, a)
    _launch(inp, r_in, b)
    torch.cuda.synchronize()
    return a.cpu(), b.cpu(), r_in.cpu()


def _update_err(out, r0, ref):
    return rel(out.double() - r0.double(), ref - r0.double())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H", [1, 3, 16])
@pytest.mark.parametrize("T", [1, 15, 16, 63, 64, 65, 128, 129, 145, 197, 257, 577])
def test_kernel_matches_fp64(T, H, causal, dtype):
    inp = _inputs([T] * 3, T, H, causal, dtype, seed=T * 31 + H)
    r0 = _r_in(3, T, T + H)
    a, b, r_after = _run_twice(inp, r0)
    assert torch.equal(a, b), "two launches differ"
    assert torch.equal(r_after, r0), "r_in was modified"
    d = _update_err(a, r0, _ref(inp, r0))
    print(f"\n[relevance row] T {T} H {H} causal {causal} {dtype}: rel err of the update {d:.3g}")
    assert d < KERNEL_TOL, f"rel err of the update {d:.3g}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("lens,T,causal,H", [([5, 77, 1, 40, 16, 33], 77, True, 8), ([130, 1, 200, 64], 200, False, 3)])
def test_kernel_packed_ragged(lens, T, causal, H, dtype):
    inp = _inputs(lens, T, H, causal, dtype, packed=True, seed=7)
    r0 = _r_in(len(lens), T, 7)
    a, b, r_after = _run_twice(inp, r0)
    assert torch.equal(a, b) and torch.equal(r_after, r0)
    d = _update_err(a, r0, _ref(inp, r0))
    assert d < KERNEL_TOL, f"rel err of the update {d:.3g}"
    for i, Tb in enumerate(lens):
        assert torch.equal(a[i, Tb:], r0[i, Tb:]), f"entries past length {Tb} of sequence {i} changed"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,causal", [(50, False), (197, False), (77, True)])
def test_kernel_one_hot_gives_the_row_of_C(T, causal, dtype):
    inp = _inputs([T] * 3, T, 4, causal, dtype, seed=T)
    pos = [T - 1, T // 2, 17]
    r0 = torch.zeros(3, T)
    r0[torch.arange(3), torch.tensor(pos)] = 1
    a, _, _ = _run_twice(inp, r0)
    rows = torch.stack([inp["C"][b][pos[b]] for b in range(3)])
    assert rel(a.double() - r0.double(), rows) < KERNEL_TOL


def test_kernel_zero_gradient_leaves_r():
    inp = _inputs([197, 197], 197, 8, False, torch.bfloat16, zero_da=True)
    r0 = _r_in(2, 197, 3)
    a, _, _ = _run_twice(inp, r0)
    assert torch.equal(a, r0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_kernel_grad_scale(dtype):
    inp = _inputs([145, 145], 145, 12, False, dtype, grad_scale=1024.0, seed=5)
    r0 = _r_in(2, 145, 5)
    a, _, _ = _run_twice(inp, r0)
    assert _update_err(a, r0, _ref(inp, r0)) < KERNEL_TOL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,causal", [(50, False), (77, True), (128, False)])
def test_kernel_agrees_with_the_full_matrix_kernel(T, causal, dtype):
    from cclip_hip import ops
    inp = _inputs([T] * 3, T, 8, causal, dtype, seed=T + 1)
    D, qkv = inp["D"], inp["qkv"]
    R0 = torch.randn(3, T, T, generator=torch.Generator().manual_seed(T))
    R = R0.cuda()
    ops.attention_relevance(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], inp["lse"], inp["da"], R, B=3, T=T, H=8, causal=causal)
    R = R.cpu()
    for i in (0, T // 2, T - 1):
        r0 = R0[:, i].contiguous()
        a, _, _ = _run_twice(inp, r0)
        d = rel(a.double() - r0.double(), R[:, i].double() - r0.double())
        assert d < KERNEL_TOL, f"row {i}: {d:.3g}"


def test_launcher_refusals():
    """Argument checks that return CCLIP_ERR_ARG before any launch; the output buffer stays as it was."""
    import ctypes
    from cclip_hip import ops
    from cclip_hip._lib import CclipError, lib
    T, H = 50, 2
    inp = _inputs([T] * 2, T, H, False, torch.bfloat16)
    D, qkv = inp["D"], inp["qkv"]
    r_in = _r_in(2, T, 1).cuda()
    keep = r_in.clone()
    out = torch.full_like(r_in, 7.0)
    with pytest.raises(CclipError, match="status 1"):
        _launch(inp, r_in, r_in)
    with pytest.raises(CclipError, match="status 1"):
        _launch(inp, r_in, out, grad_scale=0.0)
    wide = torch.zeros(qkv.shape[0], 3 * D + 1, dtype=qkv.dtype, device="cuda")      # an odd leading dimension
    wide[:, :3 * D] = qkv
    with pytest.raises(CclipError, match="status 1"):
        ops.attention_relevance_row(wide[:, 0:D], wide[:, D:2 * D], wide[:, 2 * D:3 * D], inp["lse"], inp["da"], r_in, out,
                                    B=2, T=T, H=H)
    d = ops._attn_desc(qkv[:, 0:D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D], inp["da"], inp["lse"], 2, T, H, False, None, None,
                       head_dim=32)
    d.dout, d.lddo = inp["da"].data_ptr(), inp["da"].stride(-2)
    with pytest.raises(CclipError, match="status 1"):
        ops.check(lib.cclip_attention_relevance_row(ctypes.byref(d), ctypes.c_float(1.0), ops._p(r_in), ops._p(out), ops._stream()),
                  "cclip_attention_relevance_row")
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0)) and torch.equal(r_in, keep)


# ------------------------------------------------------------------------------------------------------------------------
# 6. / 7. clip.interpret_rows on the towers of at most 128 tokens: against float64, and against clip.interpret
# ------------------------------------------------------------------------------------------------------------------------
def _row_errors(r_txt, r_img, txt, rt_ref, ri_ref):
    e_img = rel(r_img, ri_ref[:, 0, 1:])
    e_txt = 0.0
    for b in range(txt.shape[0]):
        e = int(txt[b].long().argmax())
        e_txt = max(e_txt, rel(r_txt[b, :e + 1], rt_ref[b, e, :e + 1]))
    return e_img, e_txt


def _check_against_fp64(tag, model, img, txt, ci, ct, starts, bound):
    import clip
    n = txt.shape[0]
    report = []
    for s_img, s_txt in starts:
        r_txt, r_img = clip.interpret_rows(img.cuda(), txt.cuda(), model, start_layer=s_img, start_layer_text=s_txt)
        torch.cuda.synchronize()
        assert r_txt.shape == (n, txt.shape[1]) and r_img.shape == (n, ci[0].shape[-1] - 1)
        assert r_txt.dtype == torch.float32 and r_img.dtype == torch.float32 and r_txt.is_cuda and r_img.is_cuda
        e_img, e_txt = _row_errors(r_txt, r_img, txt, rollout(ct, s_txt), rollout(ci, s_img))
        report.append((s_img, s_txt, round(e_img, 6), round(e_txt, 6), _argmax_patch_agrees(r_img, rollout(ci, s_img), bound["img"])))
    print(f"\n[relevance rows] {tag}: (start_img, start_txt, rel_img, rel_txt, argmax_ok) {report}")
    for _, _, e_img, e_txt, ok in report:
        assert e_img < bound["img"] and e_txt < bound["txt"] and ok, f"{tag}: {report}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fix", FIXTURES)
def test_interpret_rows_matches_fp64(fix, dtype):
    sd, img, txt, ci, ct = _fixture(fix)
    Li, Lt = len(ci), len(ct)
    _check_against_fp64(f"{fix} {dtype}", _model(sd, dtype), img, txt, ci, ct, ((-1, -1), (0, 0), (Li // 2, Lt // 2)), BOUND[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("fix", FIXTURES)
def test_interpret_rows_matches_interpret(fix, dtype):
    """The same forward and dgrad chain: only the fp32 summation order of the relevance step differs."""
    import clip
    sd, img, txt, ci, ct = _fixture(fix)
    model = _model(sd, dtype)
    for s in (-1, 0):
        t_full, i_full = clip.interpret(img.cuda(), txt.cuda(), model, start_layer=s, start_layer_text=s)
        t_row, i_row = clip.interpret_rows(img.cuda(), txt.cuda(), model, start_layer=s, start_layer_text=s)
        assert t_row.shape == (NPAIR, txt.shape[1]) and i_row.shape == i_full.shape
        assert t_row.dtype == torch.float32 and i_row.dtype == torch.float32 and t_row.is_cuda and i_row.is_cuda
        assert rel(i_row, i_full) < KERNEL_TOL
        for b in range(NPAIR):
            e = int(txt[b].long().argmax())
            assert rel(t_row[b, :e + 1], t_full[b, e, :e + 1]) < KERNEL_TOL
            assert torch.equal(t_row[b, e + 1:], t_full[b, e, e + 1:])            # zero in both


# ------------------------------------------------------------------------------------------------------------------------
# 8. long towers against float64
# ------------------------------------------------------------------------------------------------------------------------
LONG = {"test-long": dict(seed=13, n=4, starts=((-1, -1), (0, 0), (1, 1))), "ViT-B/16": dict(seed=21, n=2, starts=((-1, -1), (0, 0)))}


@functools.lru_cache(maxsize=None)
def _long_fixture(name):
    from clip.weights import MODELS, init_state_dict, synthetic_images, synthetic_text
    geo, seed, n = MODELS[name], LONG[name]["seed"], LONG[name]["n"]
    sd = init_state_dict(geo, seed)
    img, txt = synthetic_images(n, geo, seed + 1), synthetic_text(n, geo, seed + 2)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.enable_grad():
        logits, pi, pt = forward64(sd64, img, txt)
        logits.diagonal().sum().backward()
    return sd, img, txt, cams(pi), cams(pt)


@functools.lru_cache(maxsize=None)
def _long_model(name, dtype):
    return _model(_long_fixture(name)[0], dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", list(LONG))
def test_long_towers_match_fp64(name, dtype):
    sd, img, txt, ci, ct = _long_fixture(name)
    assert ci[0].shape[-1] > 128
    _check_against_fp64(f"{name} {dtype}", _long_model(name, dtype), img, txt, ci, ct, LONG[name]["starts"], LONG_BOUND[name][dtype])


# ------------------------------------------------------------------------------------------------------------------------
# 9. semantics on the long towers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LONG))
def test_one_image_many_texts_is_the_repeat(name):
    import clip
    _, img, txt, _, _ = _long_fixture(name)
    model, n = _long_model(name, torch.bfloat16), txt.shape[0]
    a = clip.interpret_rows(img[:1].cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    b = clip.interpret_rows(img[:1].repeat(n, 1, 1, 1).cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", list(LONG))
def test_pairs_at_once_equal_single_calls(name):
    import clip
    _, img, txt, _, _ = _long_fixture(name)
    model, bound = _long_model(name, torch.float16), DTYPE_BOUND[torch.float16]
    r_txt, r_img = clip.interpret_rows(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    for i in range(txt.shape[0]):
        t1, i1 = clip.interpret_rows(img[i:i + 1].cuda(), txt[i:i + 1].cuda(), model, start_layer=0, start_layer_text=0)
        e = int(txt[i].long().argmax())
        d_img, d_txt = rel(i1[0], r_img[i]), rel(t1[0, :e + 1], r_txt[i, :e + 1])
        print(f"\n[relevance rows] {name} pair {i} alone / in the batch: rel_img {d_img:.3g} rel_txt {d_txt:.3g}")
        assert d_img < bound["img"] and d_txt < bound["txt"]


@pytest.mark.parametrize("tail", ["0", "1"])
@pytest.mark.parametrize("pack", [False, True])
@pytest.mark.parametrize("name", list(LONG))
def test_packing_and_tail_rows_agree(name, pack, tail, monkeypatch):
    import clip
    _, img, txt, _, _ = _long_fixture(name)
    model, bound = _long_model(name, torch.float16), DTYPE_BOUND[torch.float16]
    monkeypatch.setenv("CCLIP_TAIL_ROWS", "1")
    monkeypatch.setattr(model, "pack_text_rows", True, raising=False)
    base = clip.interpret_rows(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    monkeypatch.setenv("CCLIP_TAIL_ROWS", tail)
    monkeypatch.setattr(model, "pack_text_rows", pack, raising=False)
    got = clip.interpret_rows(img.cuda(), txt.cuda(), model, start_layer=0, start_layer_text=0)
    print(f"\n[relevance rows] {name} pack {pack} tail {tail}: rel_img {rel(got[1], base[1]):.3g}")
    assert rel(got[1], base[1]) < bound["img"]
    for b in range(txt.shape[0]):
        e = int(txt[b].long().argmax())
        d = rel(got[0][b, :e + 1], base[0][b, :e + 1])
        print(f"[relevance rows] {name} pack {pack} tail {tail} text {b}: rel_txt {d:.3g}")
        assert d < bound["txt"]
        assert torch.equal(got[0][b, e + 1:], torch.zeros_like(got[0][b, e + 1:]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(LONG))
def test_rows_are_finite_and_nonnegative(name, dtype):
    _, img, txt, _, _ = _long_fixture(name)
    r_img, r_txt = _long_model(name, dtype).relevance_rows(img.cuda(), txt.cuda(), start_layer=0, start_layer_text=0)
    assert r_img.shape[0] == txt.shape[0] and r_img.shape[1] > 128 and r_txt.shape == txt.shape
    assert torch.isfinite(r_img).all() and torch.isfinite(r_txt).all()
    assert (r_img >= 0).all() and (r_txt >= 0).all()
    assert (r_img[:, 0] >= 1).all()
    eot = txt.long().argmax(dim=-1).cuda()
    assert (r_txt[torch.arange(txt.shape[0], device="cuda"), eot] >= 1).all()


# ------------------------------------------------------------------------------------------------------------------------
# 10. no side effects
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_interpret_rows_leaves_gradients_alone(dtype):
    import clip
    sd, img, txt, _, _ = _long_fixture("test-long")
    model = _model(sd, dtype)
    model.train()
    img, txt = img.cuda(), txt.cuda()
    _train_step(model, img, txt)
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads
    slots = model.arena.gflat.clone()
    clip.interpret_rows(img, txt, model, start_layer=0, start_layer_text=0)
    torch.cuda.synchronize()
    assert torch.equal(model.arena.gflat, slots)
    for n, p in model.named_parameters():
        if n in grads:
            assert torch.equal(p.grad, grads[n]), n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_training_step_after_interpret_rows_is_unchanged(dtype):
    import clip
    sd, img, txt, _, _ = _long_fixture("test-long")
    img, txt = img.cuda(), txt.cuda()
    a, b = _model(sd, dtype), _model(sd, dtype)
    a.train(); b.train()
    clip.interpret_rows(img, txt, a, start_layer=0, start_layer_text=0)
    la, lb = _train_step(a, img, txt), _train_step(b, img, txt)
    assert torch.equal(la, lb)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, pb[n].grad), n


# ------------------------------------------------------------------------------------------------------------------------
# 11. the script
# ------------------------------------------------------------------------------------------------------------------------
def test_explain_script_long_tower(tmp_path):
    import numpy as np
    out = tmp_path / "rel.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "explain_clip.py"), "--synthetic", "--model", "test-long",
                        "--out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert z["image_map"].shape == (224, 224) and 0 <= z["image_map"].min() and z["image_map"].max() <= 1
    assert z["token_scores"].ndim == 1 and abs(z["token_scores"].sum() - 1) < 1e-4
    assert z["text_relevance"].ndim == 2 and z["image_relevance"].shape[1] == 144
    assert (tmp_path / "rel.png").exists()
