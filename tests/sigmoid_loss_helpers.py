"""TEST-ONLY helpers of the sigmoid (SigLIP) loss tests (test_sigmoid_loss_cpu.py, test_sigmoid_loss_gpu.py):

  * the float64 reference - the definition of DESIGN.md 'Sigmoid loss' in plain torch (softplus of the signed, biased logits),
    gradients by autograd.  It never touches the code under test.
  * `ops_shim`: tests/cpu_ops_shim.py itself (it restates cclip_sigmoid_rows too), so that clip/loss.py's sigmoid choreography
    runs on CPU tensors and over gloo.

Bounds: the fp32 head's own (class_loss_helpers).  The loss is a sum over C columns of non-negative terms rather than a
log-sum, so its 1e-5 is read relatively: |got - ref| <= 1e-5 * max(1, |ref|)."""
import torch

import cpu_ops_shim as ops_shim  # noqa: F401
from class_loss_helpers import GRAD_TOL, LOSS_TOL, rel  # noqa: F401


def loss_close(got, ref):
    """elementwise |got - ref| <= LOSS_TOL * max(1, |ref|)"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return bool(torch.all((got - ref).abs() <= LOSS_TOL * ref.abs().clamp_min(1.0)))


def sum_close(got, ref, ref_abs):
    """a sum of signed terms that may cancel (logit_scale / logit_bias gradients, rowdot, rowsum): 1e-4 relative to the sum of
    the terms' absolute values, plus 1e-7"""
    got, ref, ref_abs = (torch.as_tensor(x).detach().double().cpu() for x in (got, ref, ref_abs))
    return bool(torch.all((got - ref).abs() <= GRAD_TOL * ref_abs + 1e-7))


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def signs(row_class, col_class):
    """[R, C] float64 y: +1 where the column carries the row's (non-negative) class, else -1; and the [R] labelled mask"""
    a, b = row_class.long(), col_class.long()
    pos = (a[:, None] == b[None, :]) & (a[:, None] >= 0)
    return pos.double() * 2 - 1, a >= 0


def ref_rows(L, row_class, col_class, bias):
    """per-row sigmoid loss of float64 logits L [R, C]: (loss_row [R], pred [R], hit [R] bool)"""
    y, labelled = signs(row_class, col_class)
    loss_row = torch.nn.functional.softplus(-y * (L + bias)).sum(1) * labelled.double()
    pred = L.argmax(1)
    hit = labelled & (col_class.long()[pred] == row_class.long())
    return loss_row, pred, hit


def ref_loss(fi, ft, ls, lb, a, b):
    """float64 (loss, #correct, L) of features fi [N,E], ft [M,E], log-scale ls, bias lb, image classes a [N], text classes b [M]"""
    i_n, t_n = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
    L = ls.exp() * i_n @ t_n.t()
    loss_row, _, hit = ref_rows(L, a, b, lb)
    return loss_row.sum() / L.shape[0], int(hit.sum()), L


def ref_loss_and_grads(fi, ft, ls, lb, a, b, upstream=1.0):
    """(loss, #correct, dfi, dft, dls, dlb, abs_ls, abs_lb): the last two are the sums of the absolute terms of the two scalar
    gradients, sum |dL * L| and sum |dL| (times |upstream|), the scale their bound is stated against"""
    f2, t2, l2, b2 = (x.detach().double().requires_grad_(True) for x in (fi, ft, ls, lb))
    loss, correct, L = ref_loss(f2, t2, l2, b2, a.to(f2.device), b.to(f2.device))
    L.retain_grad()
    (loss * upstream).backward()
    return (loss.detach(), correct, f2.grad, t2.grad, l2.grad, b2.grad, (L.grad * L.detach()).abs().sum(), L.grad.abs().sum())
