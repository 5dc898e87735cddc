"""Label spreading over the stored embeddings: "a few photos carry a label - which label would the others take?"

The collections are mostly unlabelled (image.py writes `violation_type: ''` for every photo of the monthly folders).  k-means
hands a whole cluster its majority label; `spread_labels` is the graph-based semi-supervised step instead (Zhou et al. 2004,
"Learning with local and global consistency"; the transductive step of Iscen et al. 2019, "Label propagation for deep
semi-supervised learning"), with a confidence and a certainty per photo:

    W = A + A^T,  A_ij = exp(-beta (1 - s_ij)) on the directed kNN edges      (CacheClassifier's affinity)
    S = D^-1/2 W D^-1/2
    F <- alpha S F + (1 - alpha) Y,  from F = (1 - alpha) Y,  n_iter times    (the fixed point is (1 - alpha) (I - alpha S)^-1 Y)

The kNN graph is the exact one of the top-k kernel (`EmbeddingIndex.knn_graph`).  The normalisation, the iteration - a CSR x
dense product with the label term fused, one launch per step between two buffers - and the read-out are HIP kernels
(csrc/label_spread.hip); none uses a float atomic and every sum has one fixed order, so a result is a pure function of its
inputs.  torch is plumbing: the affinities, the sort that symmetrises them into CSR (one host read: the number of non-zeros),
the class counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex
from .tsne import _unit_rows, knn_graph, symmetric_csr


def affinity_csr(scores: torch.Tensor, index: torch.Tensor, beta: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """W = A + A^T as CSR with ascending columns, (offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz]), for
    A_ij = exp(-beta (1 - s_ij)) on the directed kNN edges: scores fp32 [N, k], index [N, k] (distinct inside a row, never
    the row itself).  An edge found from both ends holds the sum of its two affinities - a key occurs at most twice, so the
    sum has one order.  Pure torch on the operands' device; ONE host read, of nnz."""
    beta = float(beta)
    if not 0.0 <= beta < float("inf"):
        raise ValueError(f"affinity_csr: beta = {beta} must be finite and >= 0")
    A = torch.exp(-beta * (1.0 - scores.float()))
    return symmetric_csr(A.reshape(-1), index)


@dataclass
class LabelSpreadResult:
    """distributions fp32 [N, C]: the rows of F, each divided by its sum (a zero row where no label reaches); pred int64 [N]:
    the propagated label, -1 for an unreachable row; labels int64 [N]: the given label where there is one, else pred;
    confidence fp32 [N]: the largest entry of the distribution; certainty fp32 [N]: 1 - H(distribution) / log C (Iscen et
    al.'s weight); n_iter: steps run; delta: the last measured max |F_t+1 - F_t|, None if none was measured; suspects int64:
    the labelled rows whose pred differs from their label, by confidence descending (candidates for label noise); unreachable
    int64: the rows whose graph component holds no labelled row.  Tensors live on the device."""
    distributions: torch.Tensor
    pred: torch.Tensor
    labels: torch.Tensor
    confidence: torch.Tensor
    certainty: torch.Tensor
    n_iter: int
    delta: Optional[float]
    suspects: torch.Tensor
    unreachable: torch.Tensor


def _check_arguments(N: int, labels, n_classes, k, beta, alpha, n_iter, check_every, tol):
    """The argument errors of `spread_labels`, before anything touches a device: returns (labels int64 [N] on the host or
    where they were, n_classes)."""
    alpha, beta, tol = float(alpha), float(beta), float(tol)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"spread_labels: alpha = {alpha} must lie inside (0, 1)")
    if not 0.0 <= beta < float("inf"):
        raise ValueError(f"spread_labels: beta = {beta} must be finite and >= 0")
    k = int(k)
    if not 1 <= k <= ops.TSNE_MAX_K:
        raise ValueError(f"spread_labels: k = {k} outside knn_graph's range 1 .. {ops.TSNE_MAX_K}")
    if k > N - 1:
        raise ValueError(f"spread_labels: k = {k} above the {N - 1} other rows")
    if int(n_iter) < 0 or int(check_every) < 0 or not tol >= 0.0:
        raise ValueError(f"spread_labels: n_iter = {n_iter}, check_every = {check_every}, tol = {tol}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.numel() != N or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"spread_labels: labels must be {N} integers (below 0: unlabelled), got {tuple(labels.shape)} {labels.dtype}")
    labels = labels.to(torch.int64)
    top, n_labelled = torch.stack([labels.max(), (labels >= 0).sum()]).tolist()          # the documented host read
    if n_labelled == 0:
        raise ValueError("spread_labels: no labelled row (every label is below 0)")
    if n_classes is None:
        n_classes = max(2, top + 1)
    n_classes = int(n_classes)
    if not 2 <= n_classes <= ops.LABEL_SPREAD_MAX_C:
        raise ValueError(f"spread_labels: n_classes = {n_classes} outside 2 .. {ops.LABEL_SPREAD_MAX_C}")
    if top >= n_classes:
        raise ValueError(f"spread_labels: label {top} with n_classes = {n_classes}")
    return labels, n_classes


def class_weights(labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """fp32 [C]: 1 / (the number of rows labelled c), 0 for a class with no labelled row - every class then puts the same
    mass into the graph.  labels int64 [N], below 0 = unlabelled.  One bincount; no host read."""
    counts = torch.bincount(labels.clamp(min=-1) + 1, minlength=n_classes + 1)[1:n_classes + 1]
    return torch.where(counts > 0, 1.0 / counts.clamp(min=1).float(), torch.zeros(n_classes, device=labels.device))


@torch.no_grad()
def spread_labels(features: Union[torch.Tensor, EmbeddingIndex], labels, n_classes: Optional[int] = None, k: int = 15,
                  beta: float = 5.5, alpha: float = 0.9, n_iter: int = 50, class_balance: bool = True, check_every: int = 0,
                  tol: float = 1e-6, dtype: Optional[torch.dtype] = None) -> LabelSpreadResult:
    """Spread the labels of a few rows over the kNN graph of [N, E] features (any float dtype, anywhere: normalised and
    rounded to `dtype`, default bfloat16; 16-bit device rows are taken as unit rows as they are) or of an `EmbeddingIndex`.

    labels: N integers, below 0 = unlabelled (the convention of `cluster_purity`); n_classes defaults to the largest label +
    1 (at least 2).  The k exact nearest neighbours of every row (k <= 63), affinities exp(-beta (1 - s)), W = A + A^T,
    S = D^-1/2 W D^-1/2, then n_iter steps F <- alpha S F + (1 - alpha) Y from F = (1 - alpha) Y.  class_balance weighs
    class c's rows by 1 / count_c.  The loop reads nothing back; check_every > 0 reads the largest change of F every that
    many steps and stops once it is below `tol`.  Host reads besides: the largest label and the number of labelled rows (the
    argument check), the number of non-zeros of W, and the sizes of `suspects` and `unreachable` at the end.  Two calls with
    the same arguments return bitwise equal results."""
    N = len(features) if isinstance(features, EmbeddingIndex) else features.shape[0]
    labels, C = _check_arguments(N, labels, n_classes, k, beta, alpha, n_iter, check_every, tol)
    k, n_iter, check_every, alpha, tol = int(k), int(n_iter), int(check_every), float(alpha), float(tol)
    x = _unit_rows(features, dtype)
    dev = x.device
    labels = labels.to(dev)
    lab32 = labels.clamp(min=-1).to(torch.int32)

    scores, index = knn_graph(x, k)
    offsets, cols, vals = affinity_csr(scores, index, beta)
    del scores, index
    ops.label_graph_normalize(offsets, cols, vals, out_vals=vals)
    cw = class_weights(labels, C) if class_balance else None

    F = torch.zeros(N, C, device=dev, dtype=torch.float32)
    F2 = torch.empty_like(F)
    delta_row = torch.empty(N, device=dev, dtype=torch.float32) if check_every else None
    ops.label_spread_step(F, lab32, offsets, cols, vals, alpha, cw, out_F=F2, delta=False)      # S 0 = 0: F2 = (1 - alpha) Y
    F, F2 = F2, F
    steps, delta = 0, None
    for it in range(n_iter):
        measure = bool(check_every) and (it + 1) % check_every == 0
        ops.label_spread_step(F, lab32, offsets, cols, vals, alpha, cw, out_F=F2, out_delta=delta_row if measure else None,
                              delta=measure)
        F, F2 = F2, F
        steps = it + 1
        if measure:
            delta = delta_row.max().item()
            if delta < tol:
                break
    del F2
    dist, pred32, conf, cert = ops.label_spread_finish(F)
    pred = pred32.to(torch.int64)
    given = labels >= 0
    wrong = torch.nonzero(given & (pred != labels)).flatten()
    suspects = wrong[torch.sort(conf[wrong], descending=True, stable=True).indices]
    return LabelSpreadResult(distributions=dist, pred=pred, labels=torch.where(given, labels, pred), confidence=conf,
                             certainty=cert, n_iter=steps, delta=delta, suspects=suspects,
                             unreachable=torch.nonzero(pred < 0).flatten())
