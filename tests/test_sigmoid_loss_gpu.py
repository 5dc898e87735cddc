"""GPU: the sigmoid row kernel (ops.sigmoid_rows, csrc/sigmoid_loss.hip), clip.sigmoid_loss / clip.SigmoidLoss on top of it,
and scripts/train_clip.py --loss sigmoid, against float64 evaluations of the definition (sigmoid_loss_helpers: softplus of the
signed, biased logits, gradients by autograd) within the fp32 head's bounds: gradients 1e-4 relative L2; the scalar gradients
and the per-row rowdot / rowsum 1e-4 relative to the sum of their absolute terms, + 1e-7; integer outputs exact; the loss
|got - ref| <= 1e-5 * max(1, |ref|), per row and for the mean (a sum over C columns of non-negative terms, not a log-sum).
Kernel-level logits are torch.randn * 3, so arg-max has no near-ties."""
import glob
import json
import os
import sys
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sigmoid_loss_helpers as H  # noqa: E402

BIAS = -1.25       # the (non-zero) bias of the kernel-level checks


def _ref_kernel(lg, a, b, bias, gs):
    """float64: (loss_row, pred, hit, dlogits, rowdot, rowsum, sum |dlogits * logits|, sum |dlogits|) per row"""
    L = lg.detach().double().requires_grad_(True)
    loss_row, pred, hit = H.ref_rows(L, a, b, bias.double().reshape(()))
    (loss_row.sum() * gs).backward()
    terms = L.grad * L.detach()
    return loss_row.detach(), pred, hit, L.grad, terms.sum(1), L.grad.sum(1), terms.abs().sum(1), L.grad.abs().sum(1)


def _run_kernel(lg, a, b, bias, gs, *, dlogits="new"):
    from cclip_hip import ops
    R = lg.shape[0]
    loss_row, rowdot, rowsum, hit = (torch.full((R,), float("nan"), device="cuda") for _ in range(4))
    pred = torch.full((R,), -7, device="cuda", dtype=torch.int32)
    d = torch.full_like(lg, float("nan")) if dlogits == "new" else lg
    ops.sigmoid_rows(lg, a, b, bias, loss_row=loss_row, pred=pred, hit=hit, dlogits=d, grad_scale=gs, rowdot=rowdot, rowsum=rowsum)
    torch.cuda.synchronize()
    return loss_row, pred, hit, d, rowdot, rowsum


def _compare(got, ref, tag):
    (loss_row, pred, hit, d, rowdot, rowsum), (rl, rp, rh, rd, rdot, rsum, rdot_abs, rsum_abs) = got, ref
    R = loss_row.shape[0]
    row_err = ((loss_row.double() - rl).abs() / rl.abs().clamp_min(1.0)).max().item()
    mean, rmean = loss_row.double().sum().item() / R, rl.sum().item() / R
    d_err = H.rel(d, rd)
    print(f"{tag}: max row-loss err (rel. to max(1, ref)) {row_err:.2e} | mean loss {mean:.7f} ref {rmean:.7f} | rel dlogits {d_err:.2e}"
          f" | max rowdot err {(rowdot.double() - rdot).abs().max().item():.2e} (max sum|terms| {rdot_abs.max().item():.2e})"
          f" | max rowsum err {(rowsum.double() - rsum).abs().max().item():.2e} (max sum|terms| {rsum_abs.max().item():.2e})")
    for t in got:
        assert bool(torch.isfinite(t.double()).all())
    assert H.loss_close(loss_row, rl) and H.loss_close(mean, rmean)
    assert torch.equal(pred.long(), rp)
    assert torch.equal(hit, rh.float())
    assert d_err < H.GRAD_TOL or not rd.any()
    assert H.sum_close(rowdot, rdot, rdot_abs) and H.sum_close(rowsum, rsum, rsum_abs)


def _case(R, C, seed, lo=-1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lg = torch.randn(R, C, device="cuda", generator=gen) * 3
    a = torch.randint(lo, 4, (R,), device="cuda", generator=gen, dtype=torch.int32)
    b = torch.randint(lo, 4, (C,), device="cuda", generator=gen, dtype=torch.int32)
    return lg, a, b, torch.tensor([BIAS], device="cuda")


# lane tail; one cell; one past a wave; an exact wave; one past it; the four-column trip plus the remainder loop and more than one
# block; more rows than one trip of the capped grid (4096 blocks of four rows); both sides of the four-column trip of
# row_kernels.h (at C = 255 lane 63 falls to the tail while the others take a trip); several trips and a tail
@pytest.mark.parametrize("R,C", [(7, 9), (1, 1), (5, 70), (4, 64), (3, 65), (130, 257), (16385, 8), (3, 255), (5, 256), (9, 1000)])
def test_kernel_against_float64(R, C):
    lg, a, b, bias = _case(R, C, R * 1000 + C)
    gs = 1.0 / R
    got = _run_kernel(lg, a, b, bias, gs)
    _compare(got, _ref_kernel(lg, a, b, bias, gs), f"[{R},{C}]")
    unl = a < 0                                                              # unlabelled rows: exactly nothing
    assert not got[0][unl].any() and not got[3][unl].any() and not got[4][unl].any() and not got[5][unl].any()
    again = _run_kernel(lg, a, b, bias, gs)
    for x, y in zip(got, again):                                             # no atomics, fixed order: bitwise equal
        assert torch.equal(x, y)


def test_kernel_alias_and_wide_buffer():
    R, C = 6, 70
    lg, a, b, bias = _case(R, C, 11)
    a[2] = -1
    gs = 1.0 / R
    got = _run_kernel(lg, a, b, bias, gs)
    _compare(got, _ref_kernel(lg, a, b, bias, gs), "separate buffer")
    # dlogits aliasing logits: same bits as the out-of-place launch
    lg2 = lg.clone()
    alias = _run_kernel(lg2, a, b, bias, gs, dlogits="alias")
    assert alias[3] is lg2
    for x, y in zip(alias, got):
        assert torch.equal(x, y)
    # logits as a [:, :C] view of a wider buffer (ld = ldd = C + 5), in place: the padding columns keep their sentinel
    wide = torch.full((R, C + 5), -777.0, device="cuda")
    wide[:, :C] = lg
    view = _run_kernel(wide[:, :C], a, b, bias, gs, dlogits="alias")
    for x, y in zip(view, got):
        assert torch.equal(x, y)
    assert torch.equal(wide[:, C:], torch.full((R, 5), -777.0, device="cuda"))
    # out of place into a wide buffer of its own
    wide_d = torch.full((R, C + 5), -777.0, device="cuda")
    from cclip_hip import ops
    ops.sigmoid_rows(lg, a, b, bias, dlogits=wide_d[:, :C], grad_scale=gs)
    torch.cuda.synchronize()
    assert torch.equal(wide_d[:, :C], got[3]) and torch.equal(wide_d[:, C:], torch.full((R, 5), -777.0, device="cuda"))


@pytest.mark.parametrize("bias", [10.0, -10.0])
def test_kernel_saturation(bias):
    R, C = 8, 70
    gen = torch.Generator(device="cuda").manual_seed(13)
    values = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0], device="cuda")
    lg = values[torch.randint(0, 5, (R, C), device="cuda", generator=gen)]
    lg[0] = 100.0                                                            # whole rows at either end
    lg[1] = -100.0
    a = torch.randint(0, 4, (R,), device="cuda", generator=gen, dtype=torch.int32)
    b = torch.randint(-1, 4, (C,), device="cuda", generator=gen, dtype=torch.int32)
    bt = torch.tensor([bias], device="cuda")
    gs = 0.5
    got = _run_kernel(lg, a, b, bt, gs)
    ref = _ref_kernel(lg, a, b, bt, gs)
    # arg-max on tied rows is the first maximum on both sides (torch.argmax), so _compare's exact check holds here too
    _compare(got, ref, f"saturation, bias {bias}")
    assert got[3].abs().max().item() <= gs                                   # |sigmoid| <= 1
    assert got[0].max().item() > 100.0 * 10                                  # the large terms are there, and finite


def test_kernel_edge_rows():
    R, C = 6, 70
    lg, a, b, bias = _case(R, C, 14, lo=0)
    gs = 1.0 / R
    # an all-unlabelled batch: exactly nothing (arg-max is still reported, hit is 0)
    none = torch.full((R,), -1, device="cuda", dtype=torch.int32)
    loss_row, pred, hit, d, rowdot, rowsum = _run_kernel(lg, none, b, bias, gs)
    for t in (loss_row, hit, d, rowdot, rowsum):
        assert torch.equal(t, torch.zeros_like(t))
    assert torch.equal(pred.long(), lg.argmax(1))
    # a row whose class no column carries still pays for its negatives: every cell is a negative
    a[3] = 9
    got = _run_kernel(lg, a, b, bias, gs)
    ref = _ref_kernel(lg, a, b, bias, gs)
    _compare(got, ref, "row without a positive")
    neg = torch.nn.functional.softplus(lg[3].double() + BIAS).sum()
    assert H.loss_close(got[0][3], neg) and got[0][3].item() > 0 and bool((got[3][3] > 0).all()) and got[2][3].item() == 0.0
    # every column positive for the rows of class 1
    ones = torch.ones(C, device="cuda", dtype=torch.int32)
    a1 = torch.tensor([1, 1, -1, 1, 0, 1], device="cuda", dtype=torch.int32)
    got1 = _run_kernel(lg, a1, ones, bias, gs)
    _compare(got1, _ref_kernel(lg, a1, ones, bias, gs), "every column positive")
    assert torch.equal(got1[2], torch.tensor([1., 1., 0., 1., 0., 1.], device="cuda"))
    assert bool((got1[3][0] < 0).all()) and bool((got1[3][4] > 0).all())


def test_kernel_outputs_are_optional():
    from cclip_hip import ops
    lg, a, b, bias = _case(5, 70, 12)
    gs = 0.2
    keep = lg.clone()
    full = _run_kernel(lg, a, b, bias, gs)
    names = ("loss_row", "pred", "hit", "dlogits", "rowdot", "rowsum")
    ops.sigmoid_rows(lg, a, b, bias)                                         # nothing asked for
    for i, name in enumerate(names):                                         # each output alone (the row sums come with dlogits)
        out = torch.empty_like(full[i])
        kw = {name: out}
        if name in ("rowdot", "rowsum"):
            kw["dlogits"] = torch.empty_like(lg)
        ops.sigmoid_rows(lg, a, b, bias, grad_scale=gs, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, full[i]), name
    assert torch.equal(lg, keep)


def _raw(lg, a, b, bias, R, C, ld, *, loss_row=None, d=None, ldd=0):
    """the C entry point itself, past the binding's own checks"""
    from cclip_hip._lib import check, lib
    p = lambda t: c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    check(lib.cclip_sigmoid_rows(p(lg), c_long(ld), c_int(R), c_int(C), p(a), p(b), p(bias), c_float(1.0), p(loss_row), p(None),
                                 p(None), p(d), c_long(ldd), p(None), p(None), c_void_p(torch.cuda.current_stream().cuda_stream)),
          "cclip_sigmoid_rows")


def test_argument_errors_launch_nothing():
    from cclip_hip import ops
    from cclip_hip._lib import CclipError
    R, C = 5, 70
    lg, a, b, bias = _case(R, C, 15)
    keep = lg.clone()
    loss_row = torch.full((R,), -777.0, device="cuda")
    d = torch.full((R, C), -777.0, device="cuda")
    bad = [dict(lg=None), dict(a=None), dict(b=None), dict(bias=None), dict(R=0), dict(R=-3), dict(C=0), dict(C=-1),
           dict(ld=C - 1), dict(ldd=C - 1)]
    for change in bad:
        args = dict(lg=lg, a=a, b=b, bias=bias, R=R, C=C, ld=C, ldd=C)
        args.update(change)
        with pytest.raises(CclipError, match="status 1"):
            _raw(args["lg"], args["a"], args["b"], args["bias"], args["R"], args["C"], args["ld"], loss_row=loss_row, d=d,
                 ldd=args["ldd"])
    # the binding's own checks: dtypes, shapes, strides
    with pytest.raises(TypeError):
        ops.sigmoid_rows(lg, a.long(), b, bias, loss_row=loss_row)
    with pytest.raises(TypeError):
        ops.sigmoid_rows(lg.double(), a, b, bias, loss_row=loss_row)
    with pytest.raises(TypeError):
        ops.sigmoid_rows(lg, a, b, bias.double(), loss_row=loss_row)
    with pytest.raises(TypeError):
        ops.sigmoid_rows(lg, a, b, bias.cpu(), loss_row=loss_row)
    with pytest.raises(ValueError):
        ops.sigmoid_rows(lg, a, b[:69], bias, loss_row=loss_row)
    with pytest.raises(ValueError):
        ops.sigmoid_rows(lg, a, b, torch.zeros(2, device="cuda"), loss_row=loss_row)
    with pytest.raises(ValueError):
        ops.sigmoid_rows(lg, a, b, bias, dlogits=d[:, :69])
    with pytest.raises(ValueError):
        ops.sigmoid_rows(lg.t(), b, a, bias, loss_row=torch.empty(C, device="cuda"))
    with pytest.raises(ValueError):
        ops.sigmoid_rows(lg, a, b, bias, rowsum=loss_row)                    # a row sum without dlogits
    torch.cuda.synchronize()
    assert torch.equal(lg, keep)
    assert torch.equal(loss_row, torch.full_like(loss_row, -777.0)) and torch.equal(d, torch.full_like(d, -777.0))


# ---- loss level ------------------------------------------------------------------------------------------------------------
def _loss_case(N, M, a, b, call):
    import clip
    gen = torch.Generator(device="cuda").manual_seed(1)
    fi = torch.randn(N, 512, device="cuda", generator=gen, requires_grad=True)
    ft = torch.randn(M, 512, device="cuda", generator=gen, requires_grad=True)
    ls = torch.tensor(2.6593, device="cuda", requires_grad=True)
    lb = torch.tensor(-1.5, device="cuda", requires_grad=True)
    if call == "square":
        loss, stats = clip.sigmoid_loss(fi, ft, ls, lb, labels=a)
    elif call == "pairwise":
        loss, stats = clip.sigmoid_loss(fi, ft, ls, lb)
    else:
        loss, stats = clip.sigmoid_loss(fi, ft, ls, lb, labels=a, text_labels=b)
    loss.backward()
    ref, correct, dfi, dft, dls, dlb, abs_ls, abs_lb = H.ref_loss_and_grads(fi, ft, ls, lb, a, b)
    print(f"[{N},{M}] {call}: loss {loss.item():.7f} ref {ref.item():.7f} | rel dfi {H.rel(fi.grad, dfi):.2e} dft {H.rel(ft.grad, dft):.2e}"
          f" | dls {ls.grad.item():.6e} ref {dls.item():.6e} (sum|terms| {abs_ls.item():.2e})"
          f" | dlb {lb.grad.item():.6e} ref {dlb.item():.6e} (sum|terms| {abs_lb.item():.2e})"
          f" | correct {int(stats[1].item())} ref {correct}")
    assert H.loss_close(loss, ref) and H.loss_close(stats[0], ref) and stats.shape == (2,)
    assert H.rel(fi.grad, dfi) < H.GRAD_TOL and H.rel(ft.grad, dft) < H.GRAD_TOL
    assert H.sum_close(ls.grad, dls, abs_ls) and H.sum_close(lb.grad, dlb, abs_lb)
    assert int(stats[1].item()) == correct


def test_loss_square_300_nine_classes():
    gen = torch.Generator(device="cuda").manual_seed(2)
    a = torch.randint(0, 9, (300,), device="cuda", generator=gen)
    _loss_case(300, 300, a, a, "square")


def test_loss_rectangular_300_by_9():
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randint(0, 9, (300,), device="cuda", generator=gen)
    _loss_case(300, 9, a, torch.arange(9, device="cuda"), "rect")


def test_loss_pairwise_300():
    ids = torch.arange(300, device="cuda")
    _loss_case(300, 300, ids, ids, "pairwise")


def test_module_has_one_parameter_and_leaves_a_bystander_model_alone():
    import clip
    from clip.weights import MODELS, init_state_dict
    model = clip.build_model(init_state_dict(MODELS["test-small"], 3)).to("cuda:0")
    slots = model.arena.gflat
    slots.fill_(0.25)
    head = clip.SigmoidLoss().to("cuda")
    params = dict(head.named_parameters())
    assert list(params) == ["logit_bias"]
    p = params["logit_bias"]
    assert p.dtype == torch.float32 and p.shape == () and p.is_cuda and p.item() == -10.0
    gen = torch.Generator(device="cuda").manual_seed(5)
    fi = torch.randn(12, 64, device="cuda", generator=gen, requires_grad=True)
    ft = torch.randn(12, 64, device="cuda", generator=gen, requires_grad=True)
    ls = torch.tensor(2.6593, device="cuda", requires_grad=True)
    loss, _ = head(fi, ft, ls)
    loss.backward()
    torch.cuda.synchronize()
    ref, _, _, _, dls, dlb, abs_ls, abs_lb = H.ref_loss_and_grads(fi, ft, ls, p, torch.arange(12), torch.arange(12))
    assert H.loss_close(loss, ref) and H.sum_close(p.grad, dlb, abs_lb) and H.sum_close(ls.grad, dls, abs_ls)
    assert torch.equal(slots, torch.full_like(slots, 0.25))


def test_train_clip_script_sigmoid(tmp_path, capsys, monkeypatch):
    import train_clip
    monkeypatch.setenv("CCLIP_COMPUTE_DTYPE", "bf16")
    n = train_clip.main(["--synthetic", "--model", "test-small", "--loss", "sigmoid", "--class-aware", "--max-steps", "3",
                         "--batch-size", "3", "--epochs", "1", "--out-dir", str(tmp_path), "--warmup-steps", "2"])
    assert n == 3
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "loss" in l]
    assert len(steps) == 3
    for l in steps:
        assert torch.isfinite(torch.tensor(l["loss"])) and 0.0 <= l["accuracy"] <= 1.0
        assert torch.isfinite(torch.tensor(l["logit_bias"]))
    assert len({l["loss"] for l in steps}) > 1                               # the losses change
    side = glob.glob(os.path.join(str(tmp_path), "*_logit_bias.pt"))
    ckpt = [f for f in glob.glob(os.path.join(str(tmp_path), "*.pt")) if f not in side]
    assert len(side) == 1 and len(ckpt) == 1 and side[0] == ckpt[0][:-3] + "_logit_bias.pt"
    bias = torch.load(side[0], weights_only=True)
    assert bias.dtype == torch.float32 and bias.shape == () and torch.isfinite(bias) and bias.item() != -10.0
    sd = torch.load(ckpt[0], weights_only=True)
    assert "logit_bias" not in sd and "logit_scale" in sd                     # the checkpoint stays the OpenAI layout
