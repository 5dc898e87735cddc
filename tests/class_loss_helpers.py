"""TEST-ONLY helpers of the class-aware contrastive loss tests (test_class_loss_cpu.py, test_class_loss_gpu.py):

  * the float64 reference - the definition of DESIGN.md 'Class-aware contrastive loss' as soft-target cross-entropy in plain
    torch, gradients by autograd.  It never touches the code under test.
  * `ops_shim`: tests/cpu_ops_shim.py itself (it restates cclip_xent_rows_classes too), so that clip/loss.py's class-aware
    choreography runs on CPU tensors and over gloo."""
import torch

import cpu_ops_shim as ops_shim  # noqa: F401

LOSS_TOL, GRAD_TOL = 1e-5, 1e-4          # the fp32 head's own bounds (tests/test_clip_parity_gpu.py, test_head_is_fp32_exact)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def scalar_close(got, ref):
    """the logit_scale gradient bound: 1e-4 relative plus 1e-7"""
    return abs(float(got) - float(ref)) < GRAD_TOL * abs(float(ref)) + 1e-7


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def soft_targets(row_class, col_class):
    """[R, C] float64: 1/|P_r| on the columns of row r's class, an all-zero row where P_r is empty (or the row class < 0)"""
    a, b = row_class.long(), col_class.long()
    match = (a[:, None] == b[None, :]) & (a[:, None] >= 0)
    return match.double() / match.sum(1).clamp(min=1)[:, None].double()


def ref_rows(L, row_class, col_class):
    """per-row soft-target cross-entropy of float64 logits L [R, C]: (loss_row [R], pred [R], hit [R] bool)"""
    loss_row = -(soft_targets(row_class, col_class) * torch.log_softmax(L, dim=1)).sum(1)
    pred = L.argmax(1)
    hit = (row_class.long() >= 0) & (col_class.long()[pred] == row_class.long())
    return loss_row, pred, hit


def ref_loss(fi, ft, ls, a, b):
    """float64 (loss, #correct) of features fi [N,E], ft [M,E], log-scale ls, image classes a [N], text classes b [M]"""
    i_n, t_n = fi / fi.norm(dim=1, keepdim=True), ft / ft.norm(dim=1, keepdim=True)
    L = ls.exp() * i_n @ t_n.t()
    li, _, hit = ref_rows(L, a, b)
    lt, _, _ = ref_rows(L.t(), b, a)
    return (li.sum() / L.shape[0] + lt.sum() / L.shape[1]) / 2, int(hit.sum())


def ref_loss_and_grads(fi, ft, ls, a, b, upstream=1.0):
    f2, t2, l2 = (x.detach().double().requires_grad_(True) for x in (fi, ft, ls))
    loss, correct = ref_loss(f2, t2, l2, a.to(f2.device), b.to(f2.device))
    (loss * upstream).backward()
    return loss.detach(), correct, f2.grad, t2.grad, l2.grad
