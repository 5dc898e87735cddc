"""No GPU: the float64 reference of the block stack (tests/stack_ref_f64.py) is right, and the tolerance the GPU comparison
(tests/test_stack_f64_gpu.py, section C) uses can see.

(a) stack_backward64(round_to=None), written out by hand, against torch.autograd through stack_forward64 in float64: every
    parameter gradient and dx_in to 1e-9 relative per tensor, on every geometry and on the cu / key_keep / tail_rows /
    b_qkv=None variants.
(b) The forward through the 16-bit mimic (float64 math rounded at the stack's storage points), then the backward replayed
    exactly and rounded: e_round(t) = |g_round - g_exact| / |g_exact| per gradient tensor and dtype.  For every planted fault
    (stack_ref_f64.FAULTS) the tensor it touches moves by more than the acceptance regions around the true and around the
    faulty reference can bridge - so ANY device result the GPU test accepts is rejected against the faulty reference, and the
    rounded replay itself (standing in for the device) is rejected by the very formula the GPU test uses."""
import pytest
import torch

import stack_ref_f64 as S

DTS = [torch.float16, torch.bfloat16]
# (geometry, compact tail?)
VARIANTS = [("vis", False), ("txt", False), ("txt", True), ("pack", False), ("pack", True), ("pack64", False), ("gpt", False),
            ("map", False), ("txt16", False)]


@pytest.mark.parametrize("tag,tail", VARIANTS)
def test_backward64_equals_autograd(tag, tail):
    c = S.make_case(tag, torch.float64)
    ws = [{n: (None if t is None else t.double().requires_grad_(True)) for n, t in w.items()} for w in c["weights"]]
    x = c["x"].double().requires_grad_(True)
    rows = c["tail_rows"] if tail else None
    out, saved = S.stack_forward64(x, ws, c["geo"], c["B"], c["T"], c["key_keep"], c["cu"], rows)
    dx = (c["dx_tail"] if tail else c["dx"]).double()
    assert out.shape == dx.shape
    out.backward(dx)
    with torch.no_grad():
        res = S.stack_backward64(saved, ws, dx, c["geo"])
    assert S.rel_l2(res["dx_in"], x.grad) <= 1e-9
    for l, w in enumerate(ws):
        for n, t in w.items():
            if t is None:
                assert n not in res["grads"][l]
                continue
            assert res["grads"][l][n].shape == t.shape, (l, n)
            assert S.rel_l2(res["grads"][l][n], t.grad) <= 1e-9, (l, n, S.rel_l2(res["grads"][l][n], t.grad))


def test_forward64_lse_and_packing():
    """the lse the reference returns is the log-sum-exp of the masked scores, and a packed batch equals its sequences run alone"""
    c = S.make_case("pack", torch.float64)
    geo = c["geo"]
    ws = [{n: (None if t is None else t.double()) for n, t in w.items()} for w in c["weights"]]
    out, saved = S.stack_forward64(c["x"].double(), ws, geo, c["B"], c["T"], None, c["cu"])
    cu = c["cu"].tolist()
    for b in range(c["B"]):
        sl = slice(cu[b], cu[b + 1])
        n = cu[b + 1] - cu[b]
        o1, s1 = S.stack_forward64(c["x"][sl].double(), ws, geo, 1, n)
        assert torch.allclose(out[sl], o1, rtol=1e-12, atol=1e-12)
        assert torch.allclose(saved["lse"][:, b, :, :n], s1["lse"][:, 0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
@pytest.mark.parametrize("tag,tail", VARIANTS)
def test_rounded_mimic_rejects_every_fault(tag, tail, dt):
    c = S.make_case(tag, dt)
    geo, M = c["geo"], c["M"]
    rows = c["tail_rows"] if tail else None
    _, saved = S.stack_forward64(c["x"].double(), c["weights"], geo, c["B"], c["T"], c["key_keep"], c["cu"], rows, round_to=dt)
    dx = (c["dx_tail"] if tail else c["dx"]).double()
    dxb = dx.to(dt)
    run = lambda **kw: S.flat(S.stack_backward64(saved, c["weights"], dx, geo, dxb=dxb, **kw))
    exact, rounded = run(), run(round_to=dt)
    for key in exact:
        ok, e, er = S.accepts(rounded[key], exact[key], rounded[key], S.contraction(key, geo, M))
        assert ok and er < 0.1, (key, er)          # (er == 0: the last block's w_proj / b_proj see handed-in operands only)
    for fault in S.faults_of(tag, tail):
        key = S.fault_target(fault)
        K = S.contraction(key, geo, M)
        f_exact, f_round = run(fault=fault)[key], run(fault=fault, round_to=dt)[key]
        r_true = 2 * S.rel_l2(rounded[key], exact[key]) + S.acc_term(K)
        r_inj = 2 * S.rel_l2(f_round, f_exact) + S.acc_term(K)
        disp = ((f_exact - exact[key]).norm() / f_exact.norm()).item()
        need = r_inj + r_true * (exact[key].norm() / f_exact.norm()).item()
        assert disp > need, f"{fault} ({S.FAULTS[fault]}) hides under rounding in {key}: moved {disp:.3g}, regions span {need:.3g}"
        ok, e, _ = S.accepts(rounded[key], f_exact, f_round, K)
        assert not ok, (fault, key, e)


@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
def test_row_chain_first_layer_bound(dt):
    """row_chain64's per-element bound on the keys / values a new token writes in block 0 (LayerNorm bound carried through |W|,
    plus the GEMM's own) holds for the 16-bit mimic of the forward, is not vacuous, and rejects ln_2's affine used for ln_1.
    Past the first attention the worst-case propagation is useless (bf16, this geometry: 0.07 on q, 4.5 on the attention output,
    inf after two blocks), which is why the decode test judges deeper tensors like section C does, against the mimic's own error."""
    c = S.make_case("gpt", dt)
    geo, B, T, D = c["geo"], c["B"], c["T"], c["geo"].D
    out, saved = S.stack_forward64(c["x"].double(), c["weights"], geo, B, T, round_to=dt)
    last = torch.arange(B) * T + T - 1
    kv = lambda l, c0: saved["bf"][l][:, c0:c0 + D].view(B, T, D)
    K, V = [kv(l, 2 * D) for l in range(2)], [kv(l, 3 * D) for l in range(2)]
    _, _, per = S.row_chain64(c["x"][last], c["weights"], geo, K, V, dt)
    k, v, dk, dv = per[0]
    assert bool(((K[0][:, T - 1] - k).abs() <= dk).all() and ((V[0][:, T - 1] - v).abs() <= dv).all())
    assert bool((dk < 0.1 * (1 + k.abs())).all() and (dv < 0.1 * (1 + v.abs())).all()), (dk.max().item(), dv.max().item())
    wrong = [dict(w) for w in c["weights"]]
    wrong[0]["ln1_w"], wrong[0]["ln1_b"] = wrong[0]["ln2_w"], wrong[0]["ln2_b"]
    kb = S.row_chain64(c["x"][last], wrong, geo, K, V, dt)[2][0][0]
    assert bool(((K[0][:, T - 1] - kb).abs() > dk).any()), "the bound cannot see ln_2's affine used for ln_1"
