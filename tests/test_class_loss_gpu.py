"""GPU: the class-aware row kernel (ops.xent_rows_classes, csrc/class_loss.hip), the class-aware clip.contrastive_loss on top
of it, and scripts/train_clip.py --class-aware, against float64 evaluations of the definition (class_loss_helpers: soft-target
cross-entropy, gradients by autograd) within the fp32 head's bounds: loss 1e-5 absolute, gradients 1e-4 relative, the
logit_scale gradient 1e-4 relative + 1e-7, integer outputs exact.  Inputs are torch.randn, so arg-max has no near-ties."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import class_loss_helpers as H  # noqa: E402

GS = 0.37          # grad_scale of the kernel-level checks


def _ref_kernel(lg, a, b, gs=GS):
    """float64: (loss_row, pred, hit, dlogits, rowdot) of logits lg [R, C] with row classes a and column classes b"""
    L = lg.detach().double().requires_grad_(True)
    loss_row, pred, hit = H.ref_rows(L, a, b)
    (loss_row.sum() * gs).backward()
    terms = L.grad * L.detach()
    return loss_row.detach(), pred, hit, L.grad, terms.sum(1), terms.abs().sum(1)


def _run_kernel(lg, a, b, *, dlogits="new", gs=GS):
    from cclip_hip import ops
    R = lg.shape[0]
    loss_row = torch.empty(R, device="cuda")
    rowdot = torch.empty(R, device="cuda")
    hit = torch.empty(R, device="cuda")
    pred = torch.empty(R, device="cuda", dtype=torch.int32)
    d = torch.full_like(lg, float("nan")) if dlogits == "new" else lg
    ops.xent_rows_classes(lg, a, b, loss_row=loss_row, pred=pred, hit=hit, dlogits=d, grad_scale=gs, rowdot=rowdot)
    torch.cuda.synchronize()
    return loss_row, pred, hit, d, rowdot


def _compare(got, ref, tag):
    (loss_row, pred, hit, d, rowdot), (rl, rp, rh, rd, rdot, rabs) = got, ref
    R = loss_row.shape[0]
    # per-row losses against the loss bound; their mean is what the 1e-5 of the issue is stated for, so it is checked too
    row_err = (loss_row.double() - rl).abs().max().item()
    mean_err = abs(loss_row.double().sum().item() - rl.sum().item()) / R
    d_err, dot_err = H.rel(d, rd), (rowdot.double() - rdot).abs().max().item()
    print(f"{tag}: max row-loss err {row_err:.2e} mean-loss err {mean_err:.2e} rel dlogits {d_err:.2e} max rowdot err {dot_err:.2e}"
          f" (max |rowdot| {rdot.abs().max().item():.2e})")
    assert row_err < H.LOSS_TOL and mean_err < H.LOSS_TOL
    assert torch.equal(pred.long(), rp)
    assert torch.equal(hit, rh.float())
    assert d_err < H.GRAD_TOL
    # rowdot is a sum of C signed terms that may cancel: the gradient bound (1e-4 relative, + 1e-7 as for the logit_scale gradient
    # it feeds) is taken against the size of what is summed, sum_c |dlogits * logits|, the scale an fp32 sum's error follows
    assert torch.all((rowdot.double() - rdot).abs() < H.GRAD_TOL * rabs + 1e-7)


# (3, 255), (5, 256): both sides of the four-column trip of row_kernels.h (at C = 255 lane 63 falls to the tail while the others
# take a trip); (9, 1000): several trips and a tail
@pytest.mark.parametrize("R,C", [(7, 9), (5, 70), (4, 64), (130, 257), (16385, 8), (3, 255), (5, 256), (9, 1000)])
def test_kernel_against_float64(R, C):
    gen = torch.Generator(device="cuda").manual_seed(R * 1000 + C)
    lg = torch.randn(R, C, device="cuda", generator=gen)
    a = torch.randint(-1, 3, (R,), device="cuda", generator=gen, dtype=torch.int32)
    b = torch.randint(-1, 3, (C,), device="cuda", generator=gen, dtype=torch.int32)
    _compare(_run_kernel(lg, a, b), _ref_kernel(lg, a, b), f"[{R},{C}]")


def test_kernel_explicit_rows_alias_and_wide_buffer():
    gen = torch.Generator(device="cuda").manual_seed(11)
    R, C = 6, 70
    lg = torch.randn(R, C, device="cuda", generator=gen)
    b = torch.randint(0, 3, (C,), device="cuda", generator=gen, dtype=torch.int32)
    b[5] = -1
    a = torch.tensor([0, 7, -1, 1, 2, 5], device="cuda", dtype=torch.int32)      # rows 1 and 5: no column of that class; row 2: unlabelled
    ref = _ref_kernel(lg, a, b)
    got = _run_kernel(lg, a, b)
    _compare(got, ref, "explicit rows")
    loss_row, pred, hit, d, rowdot = got
    for r in (1, 2, 5):                                                          # no positive: zero loss, all-zero gradient row
        assert loss_row[r].item() == 0.0 and rowdot[r].item() == 0.0 and hit[r].item() == 0.0
        assert torch.equal(d[r], torch.zeros_like(d[r]))
    # every column positive: the targets are uniform over the whole row
    ones = torch.ones(C, device="cuda", dtype=torch.int32)
    a1 = torch.tensor([1, 1, -1, 1, 0, 1], device="cuda", dtype=torch.int32)
    got1 = _run_kernel(lg, a1, ones)
    _compare(got1, _ref_kernel(lg, a1, ones), "every column positive")
    assert torch.equal(got1[2], torch.tensor([1., 1., 0., 1., 0., 1.], device="cuda"))
    # dlogits aliasing logits: same bits as the out-of-place launch
    lg2 = lg.clone()
    alias = _run_kernel(lg2, a, b, dlogits="alias")
    assert alias[3] is lg2
    for x, y in zip(alias, got):
        assert torch.equal(x, y)
    # logits as a [:, :C] view of a wider buffer (ld > C), in place: the columns beyond C keep their sentinel
    wide = torch.full((R, C + 26), -777.0, device="cuda")
    wide[:, :C] = lg
    view = _run_kernel(wide[:, :C], a, b, dlogits="alias")
    for x, y in zip(view, got):
        assert torch.equal(x, y)
    assert torch.equal(wide[:, C:], torch.full((R, 26), -777.0, device="cuda"))


def test_kernel_outputs_are_optional_and_arguments_checked():
    from cclip_hip import ops
    gen = torch.Generator(device="cuda").manual_seed(12)
    lg = torch.randn(5, 70, device="cuda", generator=gen)
    a = torch.randint(-1, 3, (5,), device="cuda", generator=gen, dtype=torch.int32)
    b = torch.randint(-1, 3, (70,), device="cuda", generator=gen, dtype=torch.int32)
    keep = lg.clone()
    loss_row = torch.empty(5, device="cuda")
    ops.xent_rows_classes(lg, a, b, loss_row=loss_row)                           # loss only: the logits stay as they are
    ops.xent_rows_classes(lg, a, b)
    torch.cuda.synchronize()
    assert torch.equal(lg, keep)
    assert (loss_row.double() - _ref_kernel(lg, a, b)[0]).abs().max().item() < H.LOSS_TOL
    with pytest.raises(TypeError):
        ops.xent_rows_classes(lg, a.long(), b)
    with pytest.raises(TypeError):
        ops.xent_rows_classes(lg.double(), a, b)
    with pytest.raises(ValueError):
        ops.xent_rows_classes(lg, a, b[:69])
    with pytest.raises(ValueError):
        ops.xent_rows_classes(lg, a, b, dlogits=torch.empty(5, 69, device="cuda"))


def _loss_case(N, M, a, b, square_call):
    import clip
    gen = torch.Generator(device="cuda").manual_seed(1)
    fi = torch.randn(N, 512, device="cuda", generator=gen, requires_grad=True)
    ft = torch.randn(M, 512, device="cuda", generator=gen, requires_grad=True)
    ls = torch.tensor(2.6593, device="cuda", requires_grad=True)
    if square_call:
        loss, stats = clip.contrastive_loss(fi, ft, ls, labels=a)
    else:
        loss, stats = clip.contrastive_loss(fi, ft, ls, labels=a, text_labels=b)
    loss.backward()
    ref, correct, dfi, dft, dls = H.ref_loss_and_grads(fi, ft, ls, a, b)
    print(f"[{N},{M}]: loss {loss.item():.7f} ref {ref.item():.7f} | rel dfi {H.rel(fi.grad, dfi):.2e} dft {H.rel(ft.grad, dft):.2e}"
          f" | dls {ls.grad.item():.6e} ref {dls.item():.6e} | correct {int(stats[1].item())} ref {correct}")
    assert abs(loss.item() - ref.item()) < H.LOSS_TOL
    assert H.rel(fi.grad, dfi) < H.GRAD_TOL and H.rel(ft.grad, dft) < H.GRAD_TOL and H.scalar_close(ls.grad, dls)
    assert int(stats[1].item()) == correct


def test_loss_square_300_nine_classes():
    gen = torch.Generator(device="cuda").manual_seed(2)
    a = torch.randint(0, 9, (300,), device="cuda", generator=gen)
    _loss_case(300, 300, a, a, square_call=True)


def test_loss_rectangular_300_by_9():
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randint(0, 9, (300,), device="cuda", generator=gen)
    _loss_case(300, 9, a, torch.arange(9, device="cuda"), square_call=False)


def test_arange_labels_equal_the_pairwise_path():
    import clip
    gen = torch.Generator(device="cuda").manual_seed(4)
    N = 300
    fi0, ft0 = torch.randn(N, 512, device="cuda", generator=gen), torch.randn(N, 512, device="cuda", generator=gen)
    res = []
    for labels in (None, torch.arange(N, device="cuda")):
        fi, ft = fi0.clone().requires_grad_(True), ft0.clone().requires_grad_(True)
        ls = torch.tensor(2.6593, device="cuda", requires_grad=True)
        loss, stats = clip.contrastive_loss(fi, ft, ls, labels=labels)
        loss.backward()
        res.append((loss.detach(), stats, fi.grad, ft.grad, ls.grad))
    (l0, s0, a0, b0, c0), (l1, s1, a1, b1, c1) = res
    assert abs(l0.item() - l1.item()) < H.LOSS_TOL and s0[1].item() == s1[1].item()
    assert H.rel(a1, a0) < H.GRAD_TOL and H.rel(b1, b0) < H.GRAD_TOL and H.scalar_close(c1, c0)


def test_class_ids_and_unique_texts_on_device():
    import clip
    gen = torch.Generator().manual_seed(9)
    base = torch.randint(1, 1000, (5, 77), generator=gen, dtype=torch.int32)
    pick = torch.tensor([3, 0, 3, 4, 1, 0, 0, 2, 4, 3, 1])
    tokens = base[pick].cuda()
    ids = clip.class_ids(tokens).cpu()
    assert ids.dtype == torch.int32 and torch.equal(ids[:, None] == ids[None, :], pick[:, None] == pick[None, :])
    uniq, inverse = clip.unique_texts(tokens)
    assert uniq.is_cuda and inverse.dtype == torch.int32 and uniq.shape == (5, 77)
    assert torch.equal(uniq[inverse.long()], tokens)


def test_train_clip_script_class_aware(tmp_path, capsys, monkeypatch):
    import train_clip
    monkeypatch.setenv("CCLIP_COMPUTE_DTYPE", "bf16")
    n = train_clip.main(["--synthetic", "--class-aware", "--batch-size", "3", "--max-steps", "2", "--model", "test-small",
                         "--epochs", "1", "--out-dir", str(tmp_path), "--warmup-steps", "2"])
    assert n == 2
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "loss" in l]
    assert len(steps) == 2
    for l in steps:
        assert torch.isfinite(torch.tensor(l["loss"])) and 0.0 <= l["accuracy"] <= 1.0
