"""Symmetric contrastive loss of /root/reference/CLIP/train.py:162-173 and
/root/reference/CLIP/train_caption.py:125-136,

    label = arange(N); loss = (CE(logits_per_image, label) + CE(logits_per_text, label)) / 2
    accuracy = mean(argmax(logits_per_image, 1) == label)

fused with CLIP.forward's normalise + similarity matmul, and made data-parallel: the reference is
single-GPU; here each rank holds N_loc rows, the L2-normalised image and text
features are exchanged with ONE RCCL all-gather of a packed [N_loc, 2E] fp32 buffer over xGMI,
every rank forms its row blocks  L_i = s I_loc T_all^T  and  L_t = s T_loc I_all^T  ([N_loc, N]),
and the cross-rank part of the feature gradient comes back through ONE reduce-scatter.  The
result equals the single-GPU loss at N = world * N_loc (tests/test_dp_gloo.py).

With `labels=` the loss is class-aware (the reference keeps every batch to distinct classes by construction; a large batch
of this data cannot): the positives of a row are all columns of its class, the row kernel is ops.xent_rows_classes, and the
text side may be the U distinct texts of the batch (`unique_texts`), a rectangular [N, U] problem.  `class_ids` numbers equal
token rows equally across ranks for the data-parallel (square) form.

`sigmoid_loss` / `SigmoidLoss` is the second objective: SigLIP's pairwise sigmoid loss over the same logits plus a learnable
bias, pairwise or class-aware by the same `labels=` conventions, on ops.sigmoid_rows (one logits GEMM, one row-kernel launch).

All arithmetic goes through cclip_hip.ops (HIP kernels); torch.distributed only moves bytes.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist

from cclip_hip import ops


def _world(group) -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _collectives(group) -> bool:
    from .parallel import collectives_active
    return collectives_active(group)


class _Contrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fi, ft, logit_scale, group):
        rank, world = _world(group)
        dp = _collectives(group)              # world > 1, or a forced one-rank RCCL pass (clip.parallel.collectives_active)
        dev = fi.device
        fi, ft = fi.contiguous().float(), ft.contiguous().float()
        ls = logit_scale.detach().float().reshape(1).contiguous()
        nloc, E = fi.shape
        N = nloc * world
        need_grad = any(ctx.needs_input_grad[:3])

        packed = torch.empty(nloc, 2 * E, device=dev, dtype=torch.float32)      # [ In | Tn ]
        i_n, t_n = packed[:, :E], packed[:, E:]
        inv_i = torch.empty(nloc, device=dev, dtype=torch.float32)
        inv_t = torch.empty(nloc, device=dev, dtype=torch.float32)
        ops.l2norm_fwd(fi, i_n, inv_i)
        ops.l2norm_fwd(ft, t_n, inv_t)
        if dp:
            gathered = torch.empty(N, 2 * E, device=dev, dtype=torch.float32)
            dist.all_gather_into_tensor(gathered, packed, group=group)
        else:
            gathered = packed
        i_all, t_all = gathered[:, :E], gathered[:, E:]

        L_i = torch.empty(nloc, N, device=dev, dtype=torch.float32)
        L_t = torch.empty(nloc, N, device=dev, dtype=torch.float32)
        ops.gemm_f32(i_n, t_all, L_i, alpha_log_dev=ls)
        ops.gemm_f32(t_n, i_all, L_t, alpha_log_dev=ls)
        labels = (torch.arange(nloc, device=dev) + rank * nloc).to(torch.int32)
        loss_rows = torch.empty(2, nloc, device=dev, dtype=torch.float32)
        rowdot = torch.empty(2, nloc, device=dev, dtype=torch.float32) if need_grad else None
        pred = torch.empty(nloc, device=dev, dtype=torch.int32)
        gs = 1.0 / (2.0 * N)
        # gradients of the GLOBAL mean loss overwrite the logits in place (nothing else needs them)
        ops.xent_rows(L_i, labels, loss_row=loss_rows[0], pred=pred, dlogits=L_i if need_grad else None, grad_scale=gs,
                      rowdot=rowdot[0] if need_grad else None)
        ops.xent_rows(L_t, labels, loss_row=loss_rows[1], dlogits=L_t if need_grad else None, grad_scale=gs,
                      rowdot=rowdot[1] if need_grad else None)
        out = torch.empty(2, device=dev, dtype=torch.float32)                    # [loss, #correct]
        ops.reduce_dot(loss_rows.view(-1), None, out[0:1], alpha=gs)
        hit = (pred == labels).to(torch.float32)                                 # integer compare (bookkeeping)
        ops.reduce_dot(hit, None, out[1:2])
        if dp:
            dist.all_reduce(out, group=group)
        if need_grad:
            # d/d(normalised features): local rows + the other ranks' rows that used our features
            cross = torch.empty(N, 2 * E, device=dev, dtype=torch.float32)
            ops.gemm_f32(L_t.t(), t_n.t(), cross[:, :E], alpha_log_dev=ls)       # -> d I_all = s dL_t^T T_loc
            ops.gemm_f32(L_i.t(), i_n.t(), cross[:, E:], alpha_log_dev=ls)       # -> d T_all = s dL_i^T I_loc
            if dp:
                d = torch.empty(nloc, 2 * E, device=dev, dtype=torch.float32)
                dist.reduce_scatter_tensor(d, cross, group=group)
            else:
                d = cross
            ops.gemm_f32(L_i, t_all.t(), d[:, :E], alpha_log_dev=ls, beta=1.0)   # += s dL_i T_all
            ops.gemm_f32(L_t, i_all.t(), d[:, E:], alpha_log_dev=ls, beta=1.0)   # += s dL_t I_all
            ctx.saved = (d, packed, inv_i, inv_t, rowdot)
        ctx.mark_non_differentiable(out)
        loss = out[0].clone()
        ctx.stats = out
        return loss, out

    @staticmethod
    def backward(ctx, dloss, _dout):
        d, packed, inv_i, inv_t, rowdot = ctx.saved
        E = packed.shape[1] // 2
        g = dloss.detach().float().reshape(1).contiguous()
        dfi = torch.empty(packed.shape[0], E, device=packed.device, dtype=torch.float32)
        dft = torch.empty_like(dfi)
        ops.l2norm_bwd(d[:, :E], packed[:, :E], inv_i, dfi, mul_dev=g)
        ops.l2norm_bwd(d[:, E:], packed[:, E:], inv_t, dft, mul_dev=g)
        dscale = torch.empty(1, device=packed.device, dtype=torch.float32)
        ops.reduce_dot(rowdot.view(-1), None, dscale, mul_dev=g)
        ctx.saved = None
        return dfi, dft, dscale.reshape(()), None


class _ContrastiveClasses(torch.autograd.Function):
    """The class-aware form: row i of the image side carries class a_i, row j of the text side class b_j, and the positives of
    a row are the columns of its class (uniform soft targets, both directions; DESIGN.md 'Class-aware contrastive loss').
    Single process: I [N,E] against T [M,E], M free.  Data parallel: the square form (text j carries a_j), with the choreography
    of _Contrastive plus ONE all-gather of the int32 class vector."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, group, a_loc, b_loc):
        dp = _collectives(group)
        world = _world(group)[1] if dp else 1
        dev = fi.device
        fi, ft = fi.contiguous().float(), ft.contiguous().float()
        ls = logit_scale.detach().float().reshape(1).contiguous()
        nloc, E = fi.shape
        mloc = ft.shape[0]
        N, M = nloc * world, mloc * world
        need_grad = any(ctx.needs_input_grad[:3])

        inv_i = torch.empty(nloc, device=dev, dtype=torch.float32)
        inv_t = torch.empty(mloc, device=dev, dtype=torch.float32)
        if dp:                                                                   # square: one packed buffer, as _Contrastive
            packed = torch.empty(nloc, 2 * E, device=dev, dtype=torch.float32)  # [ In | Tn ]
            i_n, t_n = packed[:, :E], packed[:, E:]
        else:
            i_n = torch.empty(nloc, E, device=dev, dtype=torch.float32)
            t_n = torch.empty(mloc, E, device=dev, dtype=torch.float32)
        ops.l2norm_fwd(fi, i_n, inv_i)
        ops.l2norm_fwd(ft, t_n, inv_t)
        if dp:
            gathered = torch.empty(N, 2 * E, device=dev, dtype=torch.float32)
            dist.all_gather_into_tensor(gathered, packed, group=group)
            i_all, t_all = gathered[:, :E], gathered[:, E:]
            a_all = torch.empty(N, device=dev, dtype=torch.int32)
            dist.all_gather_into_tensor(a_all, a_loc, group=group)
            b_all = a_all
        else:
            i_all, t_all, a_all, b_all = i_n, t_n, a_loc, b_loc

        L_i = torch.empty(nloc, M, device=dev, dtype=torch.float32)
        L_t = torch.empty(mloc, N, device=dev, dtype=torch.float32)
        ops.gemm_f32(i_n, t_all, L_i, alpha_log_dev=ls)
        ops.gemm_f32(t_n, i_all, L_t, alpha_log_dev=ls)
        loss_rows = torch.empty(nloc + mloc, device=dev, dtype=torch.float32)
        rowdot = torch.empty(nloc + mloc, device=dev, dtype=torch.float32) if need_grad else None
        hit = torch.empty(nloc, device=dev, dtype=torch.float32)
        gs_i, gs_t = 1.0 / (2.0 * N), 1.0 / (2.0 * M)                            # fixed GLOBAL denominators: host constants
        # gradients of the GLOBAL mean loss overwrite the logits in place (nothing else needs them)
        ops.xent_rows_classes(L_i, a_loc, b_all, loss_row=loss_rows[:nloc], hit=hit, dlogits=L_i if need_grad else None,
                              grad_scale=gs_i, rowdot=rowdot[:nloc] if need_grad else None)
        ops.xent_rows_classes(L_t, b_loc, a_all, loss_row=loss_rows[nloc:], dlogits=L_t if need_grad else None,
                              grad_scale=gs_t, rowdot=rowdot[nloc:] if need_grad else None)
        out = torch.empty(2, device=dev, dtype=torch.float32)                    # [loss, #correct by class]
        ops.reduce_dot(loss_rows[:nloc], None, out[0:1], alpha=gs_i)
        ops.reduce_dot(loss_rows[nloc:], None, out[0:1], alpha=gs_t, accumulate=True)
        ops.reduce_dot(hit, None, out[1:2])
        if dp:
            dist.all_reduce(out, group=group)
        if need_grad:
            # d/d(normalised features): local rows + the other ranks' rows that used our features
            if dp:
                cross = torch.empty(N, 2 * E, device=dev, dtype=torch.float32)
                cross_i, cross_t = cross[:, :E], cross[:, E:]
            else:
                cross_i = torch.empty(N, E, device=dev, dtype=torch.float32)
                cross_t = torch.empty(M, E, device=dev, dtype=torch.float32)
            ops.gemm_f32(L_t.t(), t_n.t(), cross_i, alpha_log_dev=ls)            # -> d I_all = s dL_t^T T_loc
            ops.gemm_f32(L_i.t(), i_n.t(), cross_t, alpha_log_dev=ls)            # -> d T_all = s dL_i^T I_loc
            if dp:
                d = torch.empty(nloc, 2 * E, device=dev, dtype=torch.float32)
                dist.reduce_scatter_tensor(d, cross, group=group)
                d_i, d_t = d[:, :E], d[:, E:]
            else:
                d_i, d_t = cross_i, cross_t
            ops.gemm_f32(L_i, t_all.t(), d_i, alpha_log_dev=ls, beta=1.0)        # += s dL_i T_all
            ops.gemm_f32(L_t, i_all.t(), d_t, alpha_log_dev=ls, beta=1.0)        # += s dL_t I_all
            ctx.saved = (d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot)
        ctx.mark_non_differentiable(out)
        loss = out[0].clone()
        ctx.stats = out
        return loss, out

    @staticmethod
    def backward(ctx, dloss, _dout):
        d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot = ctx.saved
        g = dloss.detach().float().reshape(1).contiguous()
        dfi = torch.empty(i_n.shape, device=i_n.device, dtype=torch.float32)
        dft = torch.empty(t_n.shape, device=i_n.device, dtype=torch.float32)
        ops.l2norm_bwd(d_i, i_n, inv_i, dfi, mul_dev=g)
        ops.l2norm_bwd(d_t, t_n, inv_t, dft, mul_dev=g)
        dscale = torch.empty(1, device=i_n.device, dtype=torch.float32)
        ops.reduce_dot(rowdot, None, dscale, mul_dev=g)
        ctx.saved = None
        return dfi, dft, dscale.reshape(()), None, None, None


def _as_classes(labels: torch.Tensor, rows: int, device, name: str) -> torch.Tensor:
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: expected int32 or int64 class ids, got {labels.dtype}")
    if labels.shape != (rows,):
        raise ValueError(f"{name}: expected shape [{rows}] (one class id per feature row), got {tuple(labels.shape)}")
    return labels.to(device=device, dtype=torch.int32).contiguous()


def contrastive_loss(image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                     group: Optional["dist.ProcessGroup"] = None, labels: Optional[torch.Tensor] = None,
                     text_labels: Optional[torch.Tensor] = None):
    """Returns (loss, stats) where stats = tensor([global mean loss, global #correct image->text]).
    `loss` is the GLOBAL mean loss; its gradient w.r.t. this rank's features is exact, so parameter
    gradients must be SUMMED over ranks (clip.parallel.allreduce_gradients does that).

    `labels` (int32/int64 [N_loc]) makes the loss class-aware: image i carries class labels[i], and every text of that class is
    a positive of image i (uniform soft targets; the same from the text side); `#correct` then counts arg-max columns of the
    row's class.  Without `text_labels` text i carries labels[i] too (square).  With `text_labels` ([M_loc], M_loc free) the
    text side has its own classes - e.g. the U distinct texts of a batch, each encoded once (`unique_texts`); single process
    only.  A negative id is 'unlabelled': such a row adds no loss and no gradient, such a column is a negative for every row.
    The means divide by the fixed global row counts N and M.  `labels=None` is the pairwise loss (positives on the diagonal)."""
    if labels is None:
        if text_labels is not None:
            raise ValueError("text_labels needs labels (the image side's class ids)")
        return _Contrastive.apply(image_features, text_features, logit_scale, group)
    if text_labels is not None and _collectives(group):
        raise NotImplementedError("class-aware contrastive loss with text_labels (rectangular) is single-process only; "
                                  "under data parallelism pass labels alone (class_ids(tokens, group) gives them)")
    a = _as_classes(labels, image_features.shape[0], image_features.device, "labels")
    if text_labels is None:
        if text_features.shape[0] != image_features.shape[0]:
            raise ValueError("labels without text_labels is the square form: image and text features need equal row counts")
        b = a
    else:
        b = _as_classes(text_labels, text_features.shape[0], image_features.device, "text_labels")
    return _ContrastiveClasses.apply(image_features, text_features, logit_scale, group, a, b)


def class_ids(tokens: torch.Tensor, group: Optional["dist.ProcessGroup"] = None) -> torch.Tensor:
    """int32 [N_loc] class ids for `labels=`: equal token rows get equal ids, different rows different ids - across ranks too
    when a group is live (the token rows are all-gathered and numbered on the global set; every rank computes the same map)."""
    tokens = tokens.contiguous()
    if _collectives(group):
        rank, world = _world(group)
        every = torch.empty((world * tokens.shape[0],) + tuple(tokens.shape[1:]), device=tokens.device, dtype=tokens.dtype)
        dist.all_gather_into_tensor(every, tokens, group=group)
    else:
        rank, every = 0, tokens
    inverse = torch.unique(every, dim=0, return_inverse=True)[1]
    n = tokens.shape[0]
    return inverse[rank * n:(rank + 1) * n].to(torch.int32)


def unique_texts(tokens: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(unique_tokens [U, L], inverse int32 [N]) with unique_tokens[inverse] == tokens: encode the U distinct texts once and
    call contrastive_loss(fi, ft_u, logit_scale, labels=inverse, text_labels=arange(U))."""
    uniq, inverse = torch.unique(tokens, dim=0, return_inverse=True)
    return uniq, inverse.to(torch.int32)


class _Sigmoid(torch.autograd.Function):
    """The pairwise sigmoid (SigLIP) loss: every cell (i, j) of L = s I T^T is a binary problem of its own, u = L + b against
    y = +1 where text j carries image i's class and -1 elsewhere, summed and divided by the GLOBAL image count N (DESIGN.md
    'Sigmoid loss').  A plain sum over cells, and every cell lies in exactly one rank's row block: ONE logits GEMM and ONE row
    kernel launch (ops.sigmoid_rows), and under data parallelism only the normalised TEXT features travel."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, logit_bias, group, a_loc, b_loc):
        dp = _collectives(group)
        rank, world = _world(group) if dp else (0, 1)
        dev = fi.device
        fi, ft = fi.contiguous().float(), ft.contiguous().float()
        ls = logit_scale.detach().float().reshape(1).contiguous()
        lb = logit_bias.detach().float().reshape(1).contiguous()
        nloc, E = fi.shape
        mloc = ft.shape[0]
        N, M = nloc * world, mloc * world
        need_grad = any(ctx.needs_input_grad[:4])

        i_n = torch.empty(nloc, E, device=dev, dtype=torch.float32)
        t_n = torch.empty(mloc, E, device=dev, dtype=torch.float32)
        inv_i = torch.empty(nloc, device=dev, dtype=torch.float32)
        inv_t = torch.empty(mloc, device=dev, dtype=torch.float32)
        ops.l2norm_fwd(fi, i_n, inv_i)
        ops.l2norm_fwd(ft, t_n, inv_t)
        if dp:                                                                   # square; nothing reads I_all
            t_all = torch.empty(M, E, device=dev, dtype=torch.float32)
            dist.all_gather_into_tensor(t_all, t_n, group=group)
        else:
            t_all = t_n
        if a_loc is None:                                                        # pairwise: the positive of global row g is column g
            a_loc = (torch.arange(nloc, device=dev) + rank * nloc).to(torch.int32)
            b_all = torch.arange(M, device=dev).to(torch.int32)
        elif dp:
            b_all = torch.empty(M, device=dev, dtype=torch.int32)
            dist.all_gather_into_tensor(b_all, a_loc, group=group)
        else:
            b_all = b_loc

        L = torch.empty(nloc, M, device=dev, dtype=torch.float32)
        ops.gemm_f32(i_n, t_all, L, alpha_log_dev=ls)
        loss_rows = torch.empty(nloc, device=dev, dtype=torch.float32)
        hit = torch.empty(nloc, device=dev, dtype=torch.float32)
        rowdot = torch.empty(nloc, device=dev, dtype=torch.float32) if need_grad else None
        rowsum = torch.empty(nloc, device=dev, dtype=torch.float32) if need_grad else None
        gs = 1.0 / N                                                             # fixed GLOBAL denominator: a host constant
        # the gradient of the GLOBAL loss overwrites the logits in place (nothing else needs them)
        ops.sigmoid_rows(L, a_loc, b_all, lb, loss_row=loss_rows, hit=hit, dlogits=L if need_grad else None, grad_scale=gs,
                         rowdot=rowdot, rowsum=rowsum)
        out = torch.zeros(3, device=dev, dtype=torch.float32)                    # [loss, #correct, sum dL = d/d bias]
        ops.reduce_dot(loss_rows, None, out[0:1], alpha=gs)
        ops.reduce_dot(hit, None, out[1:2])
        if need_grad:
            ops.reduce_dot(rowsum, None, out[2:3])
        if dp:
            dist.all_reduce(out, group=group)                                    # the bias gradient rides with the statistics
        if need_grad:
            d_i = torch.empty(nloc, E, device=dev, dtype=torch.float32)
            cross_t = torch.empty(M, E, device=dev, dtype=torch.float32)
            ops.gemm_f32(L, t_all.t(), d_i, alpha_log_dev=ls)                    # d I_loc = s dL T_all
            ops.gemm_f32(L.t(), i_n.t(), cross_t, alpha_log_dev=ls)              # d T_all = s dL^T I_loc
            if dp:
                d_t = torch.empty(mloc, E, device=dev, dtype=torch.float32)
                dist.reduce_scatter_tensor(d_t, cross_t, group=group)
            else:
                d_t = cross_t
            ctx.saved = (d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot, out)
        stats = out[:2]
        ctx.mark_non_differentiable(stats)
        return out[0].clone(), stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot, out = ctx.saved
        dev = i_n.device
        g = dloss.detach().float().reshape(1).contiguous()
        dfi = torch.empty(i_n.shape, device=dev, dtype=torch.float32)
        dft = torch.empty(t_n.shape, device=dev, dtype=torch.float32)
        ops.l2norm_bwd(d_i, i_n, inv_i, dfi, mul_dev=g)
        ops.l2norm_bwd(d_t, t_n, inv_t, dft, mul_dev=g)
        dscale = torch.empty(1, device=dev, dtype=torch.float32)
        dbias = torch.empty(1, device=dev, dtype=torch.float32)
        ops.reduce_dot(rowdot, None, dscale, mul_dev=g)                          # this rank's part
        ops.reduce_dot(out[2:3], None, dbias, mul_dev=g)                         # already GLOBAL (all-reduced in forward)
        ctx.saved = None
        return dfi, dft, dscale.reshape(()), dbias.reshape(()), None, None, None


def sigmoid_loss(image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                 logit_bias: torch.Tensor, group: Optional["dist.ProcessGroup"] = None,
                 labels: Optional[torch.Tensor] = None, text_labels: Optional[torch.Tensor] = None):
    """The pairwise sigmoid loss of SigLIP (Zhai et al. 2023): with u_ij = exp(logit_scale) cos(image i, text j) + logit_bias
    and y_ij = +1 where text j is a positive of image i, -1 elsewhere,

        loss = (1/N) sum_ij softplus(-y_ij u_ij)                N = the GLOBAL number of image rows

    Returns (loss, stats), stats = tensor([global loss, global #correct image->text]) as for contrastive_loss.

    `labels`, `text_labels`, class_ids and unique_texts mean what they mean for contrastive_loss: labels=None is the pairwise
    form (positives on the diagonal); with labels every text of image i's class is a positive of image i (no soft targets: a
    positive is just a different sign on its cell); text_labels gives the text side classes of its own ([M_loc], rectangular,
    single process only; the division stays by N).  A negative id is 'unlabelled': such a row adds no loss and no gradient,
    such a column is a negative for every labelled row.

    Gradients under data parallelism.  The gradients w.r.t. this rank's features are exact for the global loss, and the
    logit_scale gradient is this rank's part, so parameter gradients are SUMMED over ranks as for contrastive_loss
    (clip.parallel.allreduce_gradients).  logit_bias does not live in the model's arena: this rank's sum of dL rides in the one
    all-reduce that carries the statistics, backward returns the GLOBAL bias gradient on every rank, and it must NOT be summed
    again."""
    n = image_features.shape[0]
    if labels is None:
        if text_labels is not None:
            raise ValueError("text_labels needs labels (the image side's class ids)")
        if text_features.shape[0] != n:
            raise ValueError("the pairwise form needs equal image and text row counts")
        a = b = None
    else:
        if text_labels is not None and _collectives(group):
            raise NotImplementedError("sigmoid loss with text_labels (rectangular) is single-process only; under data "
                                      "parallelism pass labels alone (class_ids(tokens, group) gives them)")
        a = _as_classes(labels, n, image_features.device, "labels")
        if text_labels is None:
            if text_features.shape[0] != n:
                raise ValueError("labels without text_labels is the square form: image and text features need equal row counts")
            b = a
        else:
            b = _as_classes(text_labels, text_features.shape[0], image_features.device, "text_labels")
    return _Sigmoid.apply(image_features, text_features, logit_scale, logit_bias, group, a, b)


class SigmoidLoss(torch.nn.Module):
    """sigmoid_loss with its learnable bias: `logit_bias` is an fp32 scalar parameter of this module (SigLIP's initial -10),
    outside the model's arena - hand it to an optimiser of its own.  Its gradient is already global on every rank (see
    sigmoid_loss): do not all-reduce it."""

    def __init__(self, group=None, init_bias: float = -10.0):
        super().__init__()
        self.group = group
        self.logit_bias = torch.nn.Parameter(torch.tensor(float(init_bias), dtype=torch.float32))

    def forward(self, image_features, text_features, logit_scale, labels=None, text_labels=None):
        return sigmoid_loss(image_features, text_features, logit_scale, self.logit_bias, self.group, labels=labels,
                            text_labels=text_labels)


class ContrastiveLoss(torch.nn.Module):
    def __init__(self, group=None):
        super().__init__()
        self.group = group

    def forward(self, image_features, text_features, logit_scale, labels=None, text_labels=None):
        return contrastive_loss(image_features, text_features, logit_scale, self.group, labels=labels, text_labels=text_labels)
