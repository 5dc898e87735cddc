"""t-SNE of stored embeddings: "what does this collection look like?" - a 2-D map of the photos.

search, range_search, kmeans and the linear probe each answer a question about an embedding pickle; `tsne` lays its rows out
in a plane, so that the classes, the clusters k-means found and the odd photos can be seen (van der Maaten & Hinton 2008).
The reference's nearest piece is the PCA export of CLIP_prefix_caption/export_prediction.py:500-530.

The input is the exact kNN graph the top-k kernel returns (`EmbeddingIndex.knn_graph`).  The three device steps are HIP
kernels (csrc/tsne.hip): the neighbour probabilities by a fixed-count bisection, the O(N^2) repulsion as an N-body sum
streamed through LDS - no N x N matrix is ever formed - and the update with gains and momentum.  None uses a float atomic and
every sum runs in one fixed order, so a map is a pure function of its inputs and seed.  torch is plumbing: dropping the self
entry of the graph, the sort that symmetrises P into CSR (one host read: the number of non-zeros), the seeded initial map.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple, Union

import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex

MIN_GAIN = 0.01
MOMENTUM_EARLY, MOMENTUM_LATE = 0.5, 0.8


def drop_self(scores: torch.Tensor, index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The top k + 1 of every stored row against the store itself -> the k most similar OTHER rows: scores, index [N, k + 1]
    (best first) lose the entry whose index equals the row.  That entry is not always rank 0 - an exact duplicate with a lower
    index wins the tie - and where it is missing (more than k exact duplicates ahead of the row) the last entry goes.  Pure
    torch on the operands' device; no host read."""
    N, k1 = index.shape
    dev = index.device
    is_self = index == torch.arange(N, device=dev, dtype=index.dtype)[:, None]
    pos = torch.where(is_self.any(dim=1), is_self.to(torch.int64).argmax(dim=1), torch.full((N,), k1 - 1, device=dev, dtype=torch.int64))
    ar = torch.arange(k1 - 1, device=dev)[None, :]
    take = ar + (ar >= pos[:, None]).to(torch.int64)
    return torch.gather(scores, 1, take), torch.gather(index, 1, take)


def knn_graph(rows16: torch.Tensor, k: int, topk=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores fp32 [N, k], index int32 [N, k]): the k most similar other rows of every unit 16-bit row, by
    similarity_topk(x, x, k + 1) and `drop_self`.  `topk` replaces the kernel call (tests without a device)."""
    k = int(k)
    N = rows16.shape[0]
    if not 1 <= k <= ops.TSNE_MAX_K:
        raise ValueError(f"knn_graph: k = {k} outside 1 .. {ops.TSNE_MAX_K}: the top-k kernel returns at most "
                         f"{ops.SIMILARITY_TOPK_MAX_K} entries and one of them is the row itself")
    if k > N - 1:
        raise ValueError(f"knn_graph: k = {k} above the {N - 1} other rows")
    scores, index = (topk or ops.similarity_topk)(rows16, rows16, k + 1)
    return drop_self(scores, index)


def neighbour_count(N: int, perplexity: float) -> int:
    """k = min(N - 1, ceil(3 perplexity)), with the argument errors of `tsne`"""
    perplexity = float(perplexity)
    if N < 2:
        raise ValueError(f"tsne: {N} rows; a map needs at least 2")
    if not perplexity > 1.0:
        raise ValueError(f"tsne: perplexity = {perplexity} must be above 1")
    k = min(N - 1, math.ceil(3.0 * perplexity))
    if k > ops.TSNE_MAX_K:
        raise ValueError(f"tsne: perplexity = {perplexity} needs k = {k} neighbours, above the {ops.TSNE_MAX_K} the top-k kernel's "
                         f"limit of {ops.SIMILARITY_TOPK_MAX_K} leaves (perplexity <= {ops.TSNE_MAX_K // 3})")
    if perplexity >= k:
        raise ValueError(f"tsne: perplexity = {perplexity} must be below k = {k} (N = {N})")
    return k


def auto_learning_rate(N: int, exaggeration: float) -> float:
    """max(N / exaggeration / 4, 50) (Belkina et al. 2019, as scikit-learn's "auto")"""
    return max(N / float(exaggeration) / 4.0, 50.0)


def joint_csr(P: torch.Tensor, index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The symmetric joint probabilities (P_cond + P_cond^T) / (2 N) of conditional rows P [N, k] over the neighbours index
    [N, k] (distinct inside a row, never the row itself), as CSR with ascending columns: (offsets int64 [N + 1], cols int32
    [nnz], vals fp32 [nnz]).  Both directions of every edge are keyed row * N + col and sorted; a key occurs at most twice, so
    its sum has one order.  Pure torch on the operands' device; ONE host read, of nnz."""
    return symmetric_csr(P.reshape(-1) / (2.0 * P.shape[0]), index)


def symmetric_csr(val: torch.Tensor, index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A + A^T as CSR with ascending columns, for the directed edges row -> index [N, k] with the weights val [N * k] (row
    major): the sort `joint_csr` describes, shared with clip/propagate.py.  ONE host read, of nnz."""
    N, k = index.shape
    dev = index.device
    row = torch.arange(N, device=dev, dtype=torch.int64)[:, None].expand(N, k).reshape(-1)
    col = index.reshape(-1).to(torch.int64)
    key = torch.cat([row * N + col, col * N + row])
    val = val.repeat(2)
    key, order = torch.sort(key, stable=True)
    val = val[order]
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    twin = torch.zeros_like(val)
    twin[:-1] = torch.where(first[1:], torch.zeros_like(val[1:]), val[1:])
    where = torch.nonzero(first).flatten()                                       # the one host read (sizes the outputs)
    key, val = key[where], (val + twin)[where]
    r = torch.div(key, N, rounding_mode="floor")
    offsets = torch.searchsorted(r, torch.arange(N + 1, device=dev, dtype=torch.int64))
    return offsets, (key - r * N).to(torch.int32), val


@dataclass
class TSNEResult:
    """embedding fp32 [N, 2], centred; kl_divergence: KL(P || Q) of the returned map; n_iter; beta fp32 [N], the neighbour
    kernel's precision per row; knn_index int32 [N, k]; kl_history: [(iteration, KL of the map entering it)] when log_every >
    0.  Tensors live on the device."""
    embedding: torch.Tensor
    kl_divergence: float
    n_iter: int
    beta: torch.Tensor
    knn_index: torch.Tensor
    kl_history: List[Tuple[int, float]] = field(default_factory=list)


def _unit_rows(features_or_index, dtype) -> torch.Tensor:
    from .cluster import _rows16
    if isinstance(features_or_index, EmbeddingIndex):
        if dtype not in (None, features_or_index.dtype):
            raise ValueError(f"tsne: the index stores {features_or_index.dtype} rows, dtype = {dtype}")
        return features_or_index.features
    return _rows16(features_or_index, dtype)


@torch.no_grad()
def tsne(features: Union[torch.Tensor, EmbeddingIndex], perplexity: float = 20.0, n_iter: int = 1000, exaggeration: float = 12.0,
         exaggeration_iters: int = 250, learning_rate: Union[str, float] = "auto", seed: int = 0,
         init: Optional[torch.Tensor] = None, log_every: int = 0, dtype: Optional[torch.dtype] = None) -> TSNEResult:
    """A 2-D t-SNE map of [N, E] features (any float dtype, anywhere: normalised by normalize_rows and rounded to `dtype`,
    default bfloat16; 16-bit device rows are taken as unit rows as they are) or of an `EmbeddingIndex` (its stored rows).

    k = min(N - 1, ceil(3 perplexity)) exact nearest neighbours (k <= 63: the top-k kernel returns 64 entries, so perplexity
    <= 21 at full width), conditional probabilities at `perplexity`, the joint P as CSR, then n_iter steps of gradient descent
    with gains: P times `exaggeration` and momentum 0.5 for the first exaggeration_iters steps, momentum 0.8 after.
    learning_rate "auto" is max(N / exaggeration / 4, 50).  The initial map is 1e-4 torch.randn from a CPU generator seeded
    with `seed`, or `init` [N, 2].  The loop reads nothing back; log_every > 0 reads the KL sum every that many steps.  The map
    is centred once at the end.  Two calls with the same arguments return bitwise equal maps."""
    x = _unit_rows(features, dtype)
    N = x.shape[0]
    k = neighbour_count(N, perplexity)
    n_iter, exaggeration_iters, log_every = int(n_iter), int(exaggeration_iters), int(log_every)
    exaggeration = float(exaggeration)
    if n_iter < 0 or exaggeration_iters < 0 or log_every < 0:
        raise ValueError(f"tsne: n_iter = {n_iter}, exaggeration_iters = {exaggeration_iters}, log_every = {log_every}")
    if not exaggeration >= 1.0 or exaggeration == float("inf"):
        raise ValueError(f"tsne: exaggeration = {exaggeration} must be a finite number >= 1")
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"tsne: learning_rate = {learning_rate!r}; expected 'auto' or a positive number")
        lr = auto_learning_rate(N, exaggeration)
    else:
        lr = float(learning_rate)
        if not 0.0 < lr < float("inf"):
            raise ValueError(f"tsne: learning_rate = {learning_rate} must be positive and finite")
    if init is not None and (not isinstance(init, torch.Tensor) or tuple(init.shape) != (N, 2) or not init.is_floating_point()):
        raise ValueError(f"tsne: init must be a float [{N}, 2] tensor, got {tuple(getattr(init, 'shape', ()))}")
    dev = x.device

    scores, index = knn_graph(x, k)
    P, beta = ops.tsne_affinities(scores, perplexity)
    offsets, cols, vals = joint_csr(P, index)
    del P, scores

    if init is None:
        y = (1e-4 * torch.randn(N, 2, generator=torch.Generator().manual_seed(int(seed)))).to(dev)
    else:
        y = init.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
    y2 = torch.empty_like(y)
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    zrow = torch.empty(N, device=dev, dtype=torch.float32)
    rep, z, kl_row = torch.empty_like(y), torch.empty(1, device=dev, dtype=torch.float32), torch.empty(N, device=dev, dtype=torch.float32)
    ws = torch.empty(ops.tsne_repulsion_workspace(N) // 4, device=dev, dtype=torch.float32)
    history = []
    for it in range(n_iter):
        early = it < exaggeration_iters
        ops.tsne_repulsion(y, out_zrow=zrow, out_rep=rep, out_z=z, workspace=ws)
        ops.tsne_step(y, vel, gains, offsets, cols, vals, rep, z, exaggeration=exaggeration if early else 1.0,
                      momentum=MOMENTUM_EARLY if early else MOMENTUM_LATE, learning_rate=lr, min_gain=MIN_GAIN, out_y=y2,
                      out_kl=kl_row)
        y, y2 = y2, y
        if log_every and (it + 1) % log_every == 0:
            history.append((it, kl_row.sum().item()))
    ops.tsne_repulsion(y, out_zrow=zrow, out_rep=rep, out_z=z, workspace=ws)
    ops.tsne_step(y, None, None, offsets, cols, vals, None, z, out_kl=kl_row, update=False)
    kl = kl_row.sum().item()                                                     # the read at the end
    return TSNEResult(embedding=y - y.mean(dim=0, keepdim=True), kl_divergence=kl, n_iter=n_iter, beta=beta, knn_index=index,
                      kl_history=history)
