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

`distill_loss` / `DistillLoss` is the third: the KL divergence from a frozen teacher's similarity rows to the student's, both
directions, on ops.kl_rows - the soft counterpart that keeps a fine-tune on few pairs near what the pretrained model knew.

Three autograd Functions, `_Contrastive` (both softmax forms), `_Sigmoid` and `_Distill`, differ in their row kernels and statistics.  The
steps around those are written once: `_normalise_gather` (two l2norm_fwd, the all-gather), `_feature_grads` (cross GEMMs,
reduce-scatter, local GEMMs), `_backward_tail` (two l2norm_bwd, the logit_scale gradient) and `_classes` (what `labels` and
`text_labels` mean, with the refusals).  tools/loss_dump.py records the launch sequence and the results of every form.

All arithmetic goes through cclip_hip.ops (HIP kernels); torch.distributed only moves bytes.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
import torch.distributed as dist

from cclip_hip import ops

from .parallel import collectives_active as _collectives


def _world(group) -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


class _Ranks(NamedTuple):
    group: object
    dp: bool                # the collectives run: world > 1, or a forced one-rank RCCL pass (clip.parallel.collectives_active)
    rank: int
    world: int


def _ranks(group) -> _Ranks:
    dp = _collectives(group)
    return _Ranks(group, dp, *(_world(group) if dp else (0, 1)))


class _Features(NamedTuple):
    i_n: torch.Tensor       # this rank's normalised rows [N_loc, E], [M_loc, E]
    t_n: torch.Tensor
    inv_i: torch.Tensor     # their 1 / norm
    inv_t: torch.Tensor
    i_all: Optional[torch.Tensor]   # every rank's rows [N, E] (None: the one-sided form never reads them), [M, E]
    t_all: torch.Tensor
    packed: bool            # i_n | t_n are the column halves of one buffer; the gradient buffers then follow suit


def _scalar(x: torch.Tensor) -> torch.Tensor:
    """a scalar as a one-element fp32 device tensor: the launchers read it on the device, never on the host"""
    return x.detach().float().reshape(1).contiguous()


def _pair(rows_i: int, rows_t: int, E: int, dev, packed: bool):
    """fp32 buffers for an image side [rows_i, E] and a text side [rows_t, E] -> (whole, image, text).  Packed (square forms)
    they are the column halves of ONE [rows_i, 2E] buffer [ I | T ], which one collective moves whole; else whole is None."""
    if packed:
        whole = torch.empty(rows_i, 2 * E, device=dev, dtype=torch.float32)
        return whole, whole[:, :E], whole[:, E:]
    return None, torch.empty(rows_i, E, device=dev, dtype=torch.float32), torch.empty(rows_t, E, device=dev, dtype=torch.float32)


def _normalise_gather(fi, ft, mloc: int, r: _Ranks, packed: bool, one_sided: bool) -> _Features:
    """L2-normalise both sides and, under data parallelism, exchange them with ONE all-gather: of the packed [N_loc, 2E]
    buffer, or one-sided (only L = s I_loc T_all^T is formed, nothing reads I_all) of the text rows alone."""
    dev = fi.device
    nloc, E = fi.shape
    whole, i_n, t_n = _pair(nloc, mloc, E, dev, packed)
    inv_i = torch.empty(nloc, device=dev, dtype=torch.float32)
    inv_t = torch.empty(mloc, device=dev, dtype=torch.float32)
    ops.l2norm_fwd(fi, i_n, inv_i)
    ops.l2norm_fwd(ft, t_n, inv_t)
    if not r.dp:
        return _Features(i_n, t_n, inv_i, inv_t, i_n, t_n, packed)
    if one_sided:
        t_all = torch.empty(mloc * r.world, E, device=dev, dtype=torch.float32)
        dist.all_gather_into_tensor(t_all, t_n, group=r.group)
        return _Features(i_n, t_n, inv_i, inv_t, None, t_all, packed)
    gathered = torch.empty(nloc * r.world, 2 * E, device=dev, dtype=torch.float32)
    dist.all_gather_into_tensor(gathered, whole, group=r.group)
    return _Features(i_n, t_n, inv_i, inv_t, gathered[:, :E], gathered[:, E:], packed)


def _feature_grads(L_i, L_t, f: _Features, ls, r: _Ranks):
    """d/d(normalised features) -> (d_i [N_loc, E], d_t [M_loc, E]) from the logits gradients L_i [N_loc, M] and L_t [M_loc, N]:
    the other ranks' rows that used our features (cross GEMMs over all N | M rows, brought home by ONE reduce-scatter) plus our
    own rows (local GEMMs, beta = 1).  L_t None is the one-sided form: no row block has image columns, so d_i is the local
    product alone and only the text half crosses."""
    dev, E = L_i.device, f.i_n.shape[1]
    nloc, M = L_i.shape
    if L_t is None:
        d_i = torch.empty(nloc, E, device=dev, dtype=torch.float32)
        ops.gemm_f32(L_i, f.t_all.t(), d_i, alpha_log_dev=ls)                    # d I_loc = s dL_i T_all
        cross = cross_t = torch.empty(M, E, device=dev, dtype=torch.float32)
    else:
        cross, cross_i, cross_t = _pair(L_t.shape[1], M, E, dev, f.packed)
        ops.gemm_f32(L_t.t(), f.t_n.t(), cross_i, alpha_log_dev=ls)              # -> d I_all = s dL_t^T T_loc
    ops.gemm_f32(L_i.t(), f.i_n.t(), cross_t, alpha_log_dev=ls)                  # -> d T_all = s dL_i^T I_loc
    if r.dp:
        d = torch.empty(cross.shape[0] // r.world, cross.shape[1], device=dev, dtype=torch.float32)
        dist.reduce_scatter_tensor(d, cross, group=r.group)
    else:
        d = cross
    if L_t is None:
        return d_i, d
    d_i, d_t = (d[:, :E], d[:, E:]) if f.packed else (cross_i, cross_t)
    ops.gemm_f32(L_i, f.t_all.t(), d_i, alpha_log_dev=ls, beta=1.0)              # += s dL_i T_all
    ops.gemm_f32(L_t, f.i_all.t(), d_t, alpha_log_dev=ls, beta=1.0)              # += s dL_t I_all
    return d_i, d_t


def _backward_tail(saved, dloss):
    """The backward of both Functions from saved = (d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot): through the two normalisations,
    and this rank's logit_scale gradient, all times the upstream gradient g -> (g, (dfi, dft, dscale))."""
    d_i, d_t, i_n, t_n, inv_i, inv_t, rowdot = saved
    dev = i_n.device
    g = _scalar(dloss)
    dfi = torch.empty(i_n.shape, device=dev, dtype=torch.float32)
    dft = torch.empty(t_n.shape, device=dev, dtype=torch.float32)
    ops.l2norm_bwd(d_i, i_n, inv_i, dfi, mul_dev=g)
    ops.l2norm_bwd(d_t, t_n, inv_t, dft, mul_dev=g)
    dscale = torch.empty(1, device=dev, dtype=torch.float32)
    ops.reduce_dot(rowdot, None, dscale, mul_dev=g)
    return g, (dfi, dft, dscale.reshape(()))


class _Contrastive(torch.autograd.Function):
    """The softmax loss in both forms.  Class-aware (a_loc, b_loc given): row i of the image side carries class a_i, row j of
    the text side class b_j, and the positives of a row are the columns of its class (uniform soft targets, both directions;
    DESIGN.md 'Class-aware contrastive loss').  Single process: I [N,E] against T [M,E], M free.  Data parallel: the square
    form (text j carries a_j), with ONE more all-gather, of the int32 class vector.  Pairwise (no class vectors): the positive
    of global row g is column g, on ops.xent_rows, always square and always packed."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, group, a_loc, b_loc):
        r = _ranks(group)
        dev = fi.device
        fi, ft = fi.contiguous().float(), ft.contiguous().float()
        ls = _scalar(logit_scale)
        pairwise = a_loc is None
        nloc, E = fi.shape
        mloc = nloc if pairwise else ft.shape[0]
        N, M = nloc * r.world, mloc * r.world
        need_grad = any(ctx.needs_input_grad[:3])

        f = _normalise_gather(fi, ft, mloc, r, packed=pairwise or r.dp, one_sided=False)
        if pairwise:
            labels = (torch.arange(nloc, device=dev) + r.rank * nloc).to(torch.int32)
        elif r.dp:
            a_all = torch.empty(N, device=dev, dtype=torch.int32)
            dist.all_gather_into_tensor(a_all, a_loc, group=group)
            b_all = a_all
        else:
            a_all, b_all = a_loc, b_loc

        L_i = torch.empty(nloc, M, device=dev, dtype=torch.float32)
        L_t = torch.empty(mloc, N, device=dev, dtype=torch.float32)
        ops.gemm_f32(f.i_n, f.t_all, L_i, alpha_log_dev=ls)
        ops.gemm_f32(f.t_n, f.i_all, L_t, alpha_log_dev=ls)
        loss_rows = torch.empty(nloc + mloc, device=dev, dtype=torch.float32)
        rowdot = torch.empty(nloc + mloc, device=dev, dtype=torch.float32) if need_grad else None
        gs_i, gs_t = 1.0 / (2.0 * N), 1.0 / (2.0 * M)                            # fixed GLOBAL denominators: host constants
        out = torch.empty(2, device=dev, dtype=torch.float32)                    # [loss, #correct (by class)]

        def side(L, rows, gs):
            # gradients of the GLOBAL mean loss overwrite the logits in place (nothing else needs them)
            return dict(loss_row=loss_rows[rows], dlogits=L if need_grad else None, grad_scale=gs,
                        rowdot=rowdot[rows] if need_grad else None)

        image_rows, text_rows = slice(0, nloc), slice(nloc, None)
        if pairwise:
            pred = torch.empty(nloc, device=dev, dtype=torch.int32)
            ops.xent_rows(L_i, labels, pred=pred, **side(L_i, image_rows, gs_i))
            ops.xent_rows(L_t, labels, **side(L_t, text_rows, gs_t))
            ops.reduce_dot(loss_rows, None, out[0:1], alpha=gs_i)                # N == M: both halves in one launch
            hit = (pred == labels).to(torch.float32)                             # integer compare (bookkeeping)
        else:
            hit = torch.empty(nloc, device=dev, dtype=torch.float32)
            ops.xent_rows_classes(L_i, a_loc, b_all, hit=hit, **side(L_i, image_rows, gs_i))
            ops.xent_rows_classes(L_t, b_loc, a_all, **side(L_t, text_rows, gs_t))
            ops.reduce_dot(loss_rows[image_rows], None, out[0:1], alpha=gs_i)
            ops.reduce_dot(loss_rows[text_rows], None, out[0:1], alpha=gs_t, accumulate=True)
        ops.reduce_dot(hit, None, out[1:2])
        if r.dp:
            dist.all_reduce(out, group=group)
        if need_grad:
            ctx.saved = (*_feature_grads(L_i, L_t, f, ls, r), f.i_n, f.t_n, f.inv_i, f.inv_t, rowdot)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, dloss, _dout):
        _, grads = _backward_tail(ctx.saved, dloss)
        ctx.saved = None
        return (*grads, None, None, None)


def _as_classes(labels: torch.Tensor, rows: int, device, name: str) -> torch.Tensor:
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: expected int32 or int64 class ids, got {labels.dtype}")
    if labels.shape != (rows,):
        raise ValueError(f"{name}: expected shape [{rows}] (one class id per feature row), got {tuple(labels.shape)}")
    return labels.to(device=device, dtype=torch.int32).contiguous()


def _classes(what: str, image_features, text_features, group, labels, text_labels):
    """What `labels` / `text_labels` mean to both entry points -> the int32 class vectors (image side [N_loc], text side
    [M_loc]) on the features' device, or (None, None) for the pairwise form."""
    if labels is None:
        if text_labels is not None:
            raise ValueError("text_labels needs labels (the image side's class ids)")
        return None, None
    if text_labels is not None and _collectives(group):
        raise NotImplementedError(f"{what} with text_labels (rectangular) is single-process only; "
                                  "under data parallelism pass labels alone (class_ids(tokens, group) gives them)")
    a = _as_classes(labels, image_features.shape[0], image_features.device, "labels")
    if text_labels is not None:
        return a, _as_classes(text_labels, text_features.shape[0], image_features.device, "text_labels")
    if text_features.shape[0] != image_features.shape[0]:
        raise ValueError("labels without text_labels is the square form: image and text features need equal row counts")
    return a, a


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
    a, b = _classes("class-aware contrastive loss", image_features, text_features, group, labels, text_labels)
    return _Contrastive.apply(image_features, text_features, logit_scale, group, a, b)


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
    'Sigmoid loss').  A plain sum over cells, and every cell lies in exactly one rank's row block: the one-sided half of
    _Contrastive's scheme - ONE logits GEMM and ONE row kernel launch (ops.sigmoid_rows), and under data parallelism only the
    normalised TEXT features travel."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, logit_bias, group, a_loc, b_loc):
        r = _ranks(group)
        dev = fi.device
        fi, ft = fi.contiguous().float(), ft.contiguous().float()
        ls, lb = _scalar(logit_scale), _scalar(logit_bias)
        nloc, mloc = fi.shape[0], ft.shape[0]
        N, M = nloc * r.world, mloc * r.world
        need_grad = any(ctx.needs_input_grad[:4])

        f = _normalise_gather(fi, ft, mloc, r, packed=False, one_sided=True)     # square under data parallelism
        if a_loc is None:                                                        # pairwise: the positive of global row g is column g
            a_loc = (torch.arange(nloc, device=dev) + r.rank * nloc).to(torch.int32)
            b_all = torch.arange(M, device=dev).to(torch.int32)
        elif r.dp:
            b_all = torch.empty(M, device=dev, dtype=torch.int32)
            dist.all_gather_into_tensor(b_all, a_loc, group=group)
        else:
            b_all = b_loc

        L = torch.empty(nloc, M, device=dev, dtype=torch.float32)
        ops.gemm_f32(f.i_n, f.t_all, L, alpha_log_dev=ls)
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
        if r.dp:
            dist.all_reduce(out, group=group)                                    # the bias gradient rides with the statistics
        if need_grad:
            ctx.saved = (*_feature_grads(L, None, f, ls, r), f.i_n, f.t_n, f.inv_i, f.inv_t, rowdot, out)
        stats = out[:2]
        ctx.mark_non_differentiable(stats)
        return out[0].clone(), stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        g, grads = _backward_tail(ctx.saved[:7], dloss)                          # dscale: this rank's part
        dbias = torch.empty(1, device=g.device, dtype=torch.float32)
        ops.reduce_dot(ctx.saved[7][2:3], None, dbias, mul_dev=g)                # already GLOBAL (all-reduced in forward)
        ctx.saved = None
        return (*grads, dbias.reshape(()), None, None, None)


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
    a, b = _classes("sigmoid loss", image_features, text_features, group, labels, text_labels)
    if a is None and text_features.shape[0] != image_features.shape[0]:
        raise ValueError("the pairwise form needs equal image and text row counts")
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


class _Distill(torch.autograd.Function):
    """The distillation loss: each row of the student's L = s I T^T and of its transpose is pulled towards the same row of a
    frozen teacher's G = s_t I_t T_t^T by KL(softmax G_row || softmax L_row) (DESIGN.md 'Distillation loss').  Both directions
    normalise over their own rows, so this is _Contrastive's two-sided scheme with ops.kl_rows as the row kernel and the
    teacher's two row blocks, formed by the same launches, in place of the class vectors.  Single process, M free, never
    packed.  The teacher tensors arrive detached and get no gradient."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, ti, tt, teacher_scale):
        r = _Ranks(None, False, 0, 1)
        dev = fi.device
        fi, ft, ti, tt = (x.contiguous().float() for x in (fi, ft, ti, tt))
        ls = _scalar(logit_scale)
        N, M = fi.shape[0], ft.shape[0]
        need_grad = any(ctx.needs_input_grad[:3])
        # the teacher's scale arrives as exp(logit_scale): a float is a host constant of its GEMMs, a tensor goes back to the
        # log form their device-scalar argument takes (one element, on the device; nothing is read on the host)
        if isinstance(teacher_scale, torch.Tensor):
            t_scale = dict(alpha_log_dev=_scalar(teacher_scale).to(dev).log())
        else:
            t_scale = dict(alpha=float(teacher_scale))

        f = _normalise_gather(fi, ft, M, r, packed=False, one_sided=False)
        g = _normalise_gather(ti, tt, M, r, packed=False, one_sided=False)
        L_i = torch.empty(N, M, device=dev, dtype=torch.float32)
        L_t = torch.empty(M, N, device=dev, dtype=torch.float32)
        G_i, G_t = torch.empty_like(L_i), torch.empty_like(L_t)
        ops.gemm_f32(f.i_n, f.t_all, L_i, alpha_log_dev=ls)
        ops.gemm_f32(f.t_n, f.i_all, L_t, alpha_log_dev=ls)
        ops.gemm_f32(g.i_n, g.t_all, G_i, **t_scale)
        ops.gemm_f32(g.t_n, g.i_all, G_t, **t_scale)
        loss_rows = torch.empty(N + M, device=dev, dtype=torch.float32)
        rowdot = torch.empty(N + M, device=dev, dtype=torch.float32) if need_grad else None
        agree = torch.empty(N, device=dev, dtype=torch.float32)
        gs_i, gs_t = 1.0 / (2.0 * N), 1.0 / (2.0 * M)                            # fixed denominators: host constants
        out = torch.empty(2, device=dev, dtype=torch.float32)                    # [loss, #image rows agreeing with the teacher]

        def side(L, rows, gs):
            # the gradient of the mean loss overwrites the student's logits in place (nothing else needs them)
            return dict(loss_row=loss_rows[rows], dlogits=L if need_grad else None, grad_scale=gs,
                        rowdot=rowdot[rows] if need_grad else None)

        image_rows, text_rows = slice(0, N), slice(N, None)
        ops.kl_rows(L_i, G_i, agree=agree, **side(L_i, image_rows, gs_i))
        ops.kl_rows(L_t, G_t, **side(L_t, text_rows, gs_t))
        ops.reduce_dot(loss_rows[image_rows], None, out[0:1], alpha=gs_i)
        ops.reduce_dot(loss_rows[text_rows], None, out[0:1], alpha=gs_t, accumulate=True)
        ops.reduce_dot(agree, None, out[1:2])
        if need_grad:
            ctx.saved = (*_feature_grads(L_i, L_t, f, ls, r), f.i_n, f.t_n, f.inv_i, f.inv_t, rowdot)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, dloss, _dout):
        _, grads = _backward_tail(ctx.saved, dloss)
        ctx.saved = None
        return (*grads, None, None, None)


def distill_loss(image_features: torch.Tensor, text_features: torch.Tensor, logit_scale: torch.Tensor,
                 teacher_image_features: torch.Tensor, teacher_text_features: torch.Tensor, teacher_scale,
                 group: Optional["dist.ProcessGroup"] = None):
    """Contrastive relational distillation (CLIP-KD, Yang et al. 2024; the LwF regulariser when the teacher is the checkpoint
    the run started from): with the student's L = exp(logit_scale) cos(image i, text j) [N, M] and a frozen teacher's
    G = teacher_scale cos(teacher image i, teacher text j) over the same N images and M texts,

        loss = (1/2N) sum_i KL(softmax G_i || softmax L_i) + (1/2M) sum_j KL(softmax G^T_j || softmax L^T_j)

    Returns (loss, stats), stats = tensor([loss, number of image rows whose arg-max text is the teacher's]), non-differentiable.

    Only logits are compared, so the teacher's embedding width is its own.  M is free: the U distinct texts of a batch
    (unique_texts), encoded once by both models, are as good as N.  `teacher_scale` is the teacher's own exp(logit_scale), a
    float or a one-element tensor (used on the device, never read on the host; it passes through a log and an exp, one fp32
    rounding of log(teacher_scale)).  Gradients flow to the student's features and to logit_scale; the teacher's tensors are
    detached on entry.  Add it to a hard loss as `hard + weight * distill`.  Single process only."""
    if _collectives(group):
        raise NotImplementedError("distillation loss is single-process only; under data parallelism train with the hard loss "
                                  "alone (contrastive_loss or sigmoid_loss take the group)")
    for name, s, t in (("image", image_features, teacher_image_features), ("text", text_features, teacher_text_features)):
        if s.dim() != 2 or t.dim() != 2 or s.shape[0] != t.shape[0]:
            raise ValueError(f"teacher_{name}_features: expected [{s.shape[0]}, E_teacher] (one row per student {name} row), "
                             f"got {tuple(t.shape)}")
    if teacher_image_features.shape[1] != teacher_text_features.shape[1] or image_features.shape[1] != text_features.shape[1]:
        raise ValueError("image and text features of one model need equal embedding widths")
    if isinstance(teacher_scale, torch.Tensor):
        if teacher_scale.numel() != 1:
            raise ValueError(f"teacher_scale: expected a float or one element, got {tuple(teacher_scale.shape)}")
        teacher_scale = teacher_scale.detach()
    return _Distill.apply(image_features, text_features, logit_scale, teacher_image_features.detach(),
                          teacher_text_features.detach(), teacher_scale)


class DistillLoss(torch.nn.Module):
    """distill_loss with the teacher's scale (its exp(logit_scale)) held as a buffer: nothing here is learnable."""

    def __init__(self, teacher_scale, group=None):
        super().__init__()
        self.group = group
        self.register_buffer("teacher_scale", torch.as_tensor(teacher_scale, dtype=torch.float32).detach().reshape(()).clone())

    def forward(self, image_features, text_features, logit_scale, teacher_image_features, teacher_text_features):
        return distill_loss(image_features, text_features, logit_scale, teacher_image_features, teacher_text_features,
                            self.teacher_scale, self.group)


class ContrastiveLoss(torch.nn.Module):
    def __init__(self, group=None):
        super().__init__()
        self.group = group

    def forward(self, image_features, text_features, logit_scale, labels=None, text_labels=None):
        return contrastive_loss(image_features, text_features, logit_scale, self.group, labels=labels, text_labels=text_labels)
