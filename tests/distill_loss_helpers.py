"""TEST-ONLY helpers of the distillation loss tests (test_distill_loss_cpu.py, test_distill_loss_kernels_gpu.py,
test_distill_loss_gpu.py):

  * the float64 reference - the definition of DESIGN.md 'Distillation loss' in plain torch arithmetic: `ref_rows` (the row
    kernel's contract on float64 copies of its inputs, the gradient written out, not taken by autograd) and `ref_loss` (the whole
    loss from features, for autograd).  Neither touches the code under test.
  * `ops_shim`: tests/cpu_ops_shim.py plus `kl_rows`, a torch restatement of cclip_kl_rows (include/cclip_hip.h) in the
    tensors' own precision, so that clip/loss.py's distillation choreography runs on CPU tensors.
  * the bounds.  CPU (the shim is fp32 torch): the fp32 head's own, as for the other two losses (class_loss_helpers).  Device:
    KERNEL_TOL and LOSS_TOL_GPU, 4 x the largest absolute deviations from float64 measured on an MI355X."""
import types

import torch

import cpu_ops_shim
from class_loss_helpers import GRAD_TOL, LOSS_TOL, rel  # noqa: F401
from sigmoid_loss_helpers import sum_close  # noqa: F401

# ---- device bounds: 4 x measured (MI355X, 2026-10-20) -----------------------------------------------------
# largest |kernel - float64| over R in {1,3,4,5,9} x C in {1,63,64,65,255,256,257,1000}, unit-normal logits times the scale,
# grad_scale = 1, teacher drawn independently:  scale -> (loss_row, dlogits, rowdot)
KERNEL_MEASURED = {1: (9.490e-07, 1.819e-07, 8.518e-07), 10: (6.850e-06, 2.322e-07, 7.536e-06), 100: (4.814e-05, 8.599e-08, 5.222e-05)}
KERNEL_TOL = {s: tuple(4.0 * v for v in m) for s, m in KERNEL_MEASURED.items()}
# largest |distill_loss - float64| over the three device cases of test_distill_loss_gpu.py: (loss, d image_features,
# d text_features, d logit_scale)
LOSS_MEASURED_GPU = (2.079e-07, 2.594e-08, 3.522e-08, 3.131e-07)
LOSS_TOL_GPU = tuple(4.0 * v for v in LOSS_MEASURED_GPU)


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def ref_rows(L, G, grad_scale=1.0):
    """The row arithmetic in float64: (loss_row [R], dlogits [R, C], rowdot [R], pred [R], agree [R] bool) of student rows L and
    teacher rows G.  A cell with p_t == 0 adds 0 (a teacher cell of -inf: 0 * inf is not formed)."""
    L, G = L.detach().double(), G.detach().double()
    a = G - torch.logsumexp(G, dim=1, keepdim=True)
    b = L - torch.logsumexp(L, dim=1, keepdim=True)
    pt, ps = a.exp(), b.exp()
    terms = torch.where(pt == 0, torch.zeros_like(pt), pt * (a - b))
    d = (ps - pt) * grad_scale
    pred = L.argmax(1)
    return terms.sum(1), d, (d * L).sum(1), pred, pred == G.argmax(1)


def logits(fi, ft, scale):
    """scale * cos(image i, text j), in the tensors' own precision"""
    return scale * (fi / fi.norm(dim=1, keepdim=True)) @ (ft / ft.norm(dim=1, keepdim=True)).t()


def ref_loss(fi, ft, ls, ti, tt, ts):
    """float64 (loss, #agreeing image rows, L): the definition written directly - KL by torch's kl_div over log_softmax - for
    autograd through fi, ft and ls"""
    kl = torch.nn.functional.kl_div
    L, G = logits(fi, ft, ls.exp()), logits(ti, tt, ts)
    N, M = L.shape
    loss = (kl(torch.log_softmax(L, 1), torch.softmax(G, 1), reduction="sum") / (2 * N)
            + kl(torch.log_softmax(L.t(), 1), torch.softmax(G.t(), 1), reduction="sum") / (2 * M))
    return loss, int((L.argmax(1) == G.argmax(1)).sum()), L


def ref_loss_and_grads(fi, ft, ls, ti, tt, ts, upstream=1.0):
    """(loss, #agree, dfi, dft, dls, abs_ls): abs_ls is sum |dL * L| over both directions (times |upstream|), the scale the
    logit_scale gradient's bound is stated against"""
    f2, t2, l2 = (x.detach().double().requires_grad_(True) for x in (fi, ft, ls))
    ti, tt = ti.detach().double(), tt.detach().double()
    ts = torch.as_tensor(ts).detach().double().reshape(()).to(f2.device)
    loss, agree, L = ref_loss(f2, t2, l2, ti, tt, ts)
    (loss * upstream).backward()
    # sum |dL * L| needs each direction's own dL: by the row arithmetic, not through autograd's summed L.grad
    Ld, G = L.detach(), logits(ti, tt, ts)
    N, M = Ld.shape
    abs_ls = ((ref_rows(Ld, G, 1 / (2 * N))[1] * Ld).abs().sum() + (ref_rows(Ld.t(), G.t(), 1 / (2 * M))[1] * Ld.t()).abs().sum())
    return loss.detach(), agree, f2.grad, t2.grad, l2.grad, abs_ls * abs(upstream)


# ---- the CPU shim --------------------------------------------------------------------------------------------------------
def kl_rows(logits, teacher, *, loss_row=None, pred=None, agree=None, dlogits=None, grad_scale=1.0, rowdot=None):
    assert logits.dtype == torch.float32 and teacher.dtype == torch.float32 and teacher.shape == logits.shape
    assert dlogits is not None or rowdot is None
    a = teacher - torch.logsumexp(teacher, dim=1, keepdim=True)
    b = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    pt = a.exp()
    arg = logits.argmax(1)
    if loss_row is not None:
        loss_row.copy_(torch.where(pt == 0, torch.zeros_like(pt), pt * (a - b)).sum(1))
    if pred is not None:
        pred.copy_(arg.to(torch.int32))
    if agree is not None:
        agree.copy_((arg == teacher.argmax(1)).to(torch.float32))
    if dlogits is not None:
        d = (b.exp() - pt) * grad_scale
        if rowdot is not None:
            rowdot.copy_((d * logits).sum(1))
        dlogits.copy_(d)                                                     # last: dlogits may be `logits`


ops_shim = types.SimpleNamespace(**{k: v for k, v in vars(cpu_ops_shim).items() if not k.startswith("__")}, kl_rows=kl_rows)
