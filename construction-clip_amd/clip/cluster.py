"""Spherical k-means over stored embeddings: "which kinds of photo are in this set?".

Most of the reference's data is unlabelled (image.py writes `violation_type: ''` for every photo of the monthly folders); only
the `reju` folders carry a type.  `kmeans` organises such a set: it clusters the L2-normalised 16-bit rows by cosine
similarity, returns a representative of every cluster and lets a whole cluster be labelled at once.

Both steps of a Lloyd iteration are HIP kernels (csrc/embed_kmeans.hip): the assignment never forms the N x K score matrix,
the centroid sums use no float atomics, and every sum runs in one fixed order - two runs give the same bits, centroids and
clusters alike.  torch is plumbing: the sort that groups rows by cluster, the seeding draws, one small host read per iteration.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex, HALF_TYPES, normalize_rows


def _rows16(features, dtype: Optional[torch.dtype], device=None) -> torch.Tensor:
    """Unit 16-bit rows on the device.  Float rows are normalised by normalize_rows.  Device rows that already are of the working
    16-bit type are taken as they are, not copied: they are what `EmbeddingIndex.features` and normalize_rows return, and
    normalising rounded unit rows a second time would move their bits."""
    if features.dim() != 2 or not features.is_floating_point():
        raise ValueError(f"expected a 2-D float tensor of features, got {tuple(features.shape)} {features.dtype}")
    if features.is_cuda and features.dtype in HALF_TYPES and dtype in (None, features.dtype) and \
            (device is None or features.device == device):
        return features
    return normalize_rows(features, torch.bfloat16 if dtype is None else dtype, device)


@dataclass
class KMeansResult:
    """centroids: 16-bit [k, E] unit rows; labels int64 [N]; scores fp32 [N], the cosine to the own centroid; margin fp32 [N],
    best minus second-best score (NaN for k == 1); counts int64 [k]; concentration fp32 [k] = |sum of the members| / count,
    the mean resultant length (0 for an empty cluster); objective: the mean score; n_iter: assignment steps run; converged:
    the share of rows that changed cluster in the last step was <= tol.  Tensors live on the device."""
    centroids: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    margin: torch.Tensor
    counts: torch.Tensor
    concentration: torch.Tensor
    objective: float
    n_iter: int
    converged: bool

    def representatives(self, r: int = 1) -> torch.Tensor:
        """int64 [k, r]: the members of every cluster with the highest score, best first (equal scores: the lower row), -1
        where a cluster has fewer than r members.  No host read."""
        return representatives(self.labels, self.scores, self.centroids.shape[0], r)


def representatives(labels: torch.Tensor, scores: torch.Tensor, k: int, r: int = 1) -> torch.Tensor:
    r = int(r)
    if r < 1:
        raise ValueError(f"representatives: r = {r}")
    N = labels.numel()
    dev = labels.device
    by_score = torch.sort(scores, descending=True, stable=True).indices          # best first, equal scores by the lower row
    by_cluster = torch.sort(labels[by_score], stable=True)
    rows = by_score[by_cluster.indices]
    first = torch.searchsorted(by_cluster.values, torch.arange(k, device=dev, dtype=labels.dtype))
    rank = torch.arange(N, device=dev) - first[by_cluster.values]
    out = torch.full((k, r + 1), -1, device=dev, dtype=torch.int64)               # column r takes what does not fit
    out[by_cluster.values, rank.clamp(max=r)] = rows
    return out[:, :r].contiguous()


def _seed_random(N: int, k: int, seed: int) -> torch.Tensor:
    return torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:k]


def _seed_plusplus(x: torch.Tensor, k: int, seed: int) -> torch.Tensor:
    """k-means++ on the device (Arthur & Vassilvitskii 2007) with the cosine distance 1 - s: row indices int64 [k].  The weight
    of a row is clamp(1 - its best similarity to the rows chosen so far, min=0), exactly 0 for a chosen row; where every
    other row repeats a chosen one (all weights 0) the draw is uniform over the rows not chosen.  k steps of mv + multinomial."""
    N = x.shape[0]
    if N > 2 ** 24:
        raise NotImplementedError(f"kmeans: init='kmeans++' draws with torch.multinomial, which takes at most 2^24 rows (N = {N}); "
                                  f"use init='random'")
    gen = torch.Generator(device=x.device).manual_seed(int(seed))
    free = torch.ones(N, device=x.device, dtype=torch.float32)
    chosen = torch.multinomial(free, 1, generator=gen)
    picks = [chosen]
    best = torch.full((N,), -float("inf"), device=x.device, dtype=torch.float32)
    for _ in range(1, k):
        free[chosen] = 0.0
        best = torch.maximum(best, torch.mv(x, x.index_select(0, chosen)[0]).float())
        w = (1.0 - best).clamp_(min=0.0).nan_to_num_(nan=0.0) * free
        w = torch.where(w.sum() > 0, w, free)
        chosen = torch.multinomial(w, 1, generator=gen)
        picks.append(chosen)
    return torch.cat(picks)


def _lloyd(x: torch.Tensor, c: torch.Tensor, max_iter: int, tol: float, reseed_empty: bool):
    """assign -> update -> assign .. from the centroids c (not written to).  Returns the fields of a KMeansResult but the
    objective.  One host read per iteration: the rows that changed cluster and the empty clusters, together."""
    N, k = x.shape[0], c.shape[0]
    prev = None
    n_iter, converged = 0, False
    while True:
        assign, best, second = ops.kmeans_assign(x, c, want_second=True)
        n_iter += 1
        c_new, norm, counts = ops.kmeans_update(x, assign, k, c, check_range=False)   # ids straight from the kernel: in range
        changed = (assign != prev).sum() if prev is not None else torch.full((), N, device=x.device)
        n_changed, n_empty = torch.stack([changed, (counts == 0).sum()]).tolist()     # the one host read
        if prev is not None and n_changed <= tol * N:
            converged = True
            break
        if n_iter >= max_iter:
            break
        if n_empty and reseed_empty:
            # every empty cluster, in ascending order, takes the not-yet-taken row that fits its centroid worst (ties: lower row)
            empty = torch.sort((counts != 0).to(torch.uint8), stable=True).indices[:n_empty]
            worst = torch.sort(best, stable=True).indices[:n_empty]
            c_new[empty] = x[worst]
        c, prev = c_new, assign
    concentration = torch.where(counts > 0, norm / counts.clamp(min=1).float(), torch.zeros_like(norm))
    return dict(centroids=c, labels=assign.long(), scores=best, margin=best - second, counts=counts, concentration=concentration,
                n_iter=n_iter, converged=converged)


def pick_best_run(objectives: Sequence[float]) -> int:
    """The n_init rule: the run with the highest objective; equal objectives go to the earlier run (the lower seed)."""
    best = 0
    for i, v in enumerate(objectives):
        if v > objectives[best]:
            best = i
    return best


@torch.no_grad()
def kmeans(features_or_index: Union[torch.Tensor, EmbeddingIndex], k: int, *, max_iter: int = 50, tol: float = 0.0,
           init: Union[str, torch.Tensor] = "kmeans++", n_init: int = 1, seed: int = 0, reseed_empty: bool = True,
           dtype: Optional[torch.dtype] = None) -> KMeansResult:
    """Spherical k-means of [N, E] features (any float dtype, anywhere: normalised by normalize_rows and rounded to `dtype`,
    default bfloat16; 16-bit device rows of that type are taken as unit rows as they are) or of an `EmbeddingIndex` (its
    stored rows, not copied).

    Lloyd's loop, assign -> update -> assign ..: it stops when the share of rows that changed cluster is <= tol (tol = 0: an
    exact fixpoint, after which centroids and labels are consistent) or after max_iter assignment steps.  The returned
    centroids are the ones the returned labels were assigned against.
    init: "kmeans++" (D^2 sampling on the device, seeded device generator), "random" (the first k of torch.randperm(N) from a
    seeded CPU generator) or a [k, E] tensor (those rows, normalised).  n_init > 1 runs the seeds seed .. seed + n_init - 1
    and keeps the highest objective (ties: the lower seed).  reseed_empty: every empty cluster, in ascending order, restarts
    before the next assignment from the not-yet-taken row with the lowest score (ties: the lower row); False leaves the
    kernel's behaviour, an empty cluster keeps its centroid."""
    if isinstance(features_or_index, EmbeddingIndex):
        if dtype not in (None, features_or_index.dtype):
            raise ValueError(f"kmeans: the index stores {features_or_index.dtype} rows, dtype = {dtype}")
        if len(features_or_index) == 0:
            raise ValueError("kmeans: the index is empty")
        x = features_or_index.features
    else:
        x = _rows16(features_or_index, dtype)
    N, E = x.shape
    k, max_iter, n_init = int(k), int(max_iter), int(n_init)
    if N == 0:
        raise ValueError("kmeans: the index is empty")
    if E % 32 or not 32 <= E <= ops.KMEANS_MAX_D:
        raise NotImplementedError(f"kmeans: embedding width {E}; the kernels need a multiple of 32 from 32 up to {ops.KMEANS_MAX_D}")
    if k < 1:
        raise ValueError(f"kmeans: k = {k} must be at least 1")
    if k > N:
        raise ValueError(f"kmeans: k = {k} above the {N} rows")
    if max_iter < 1 or n_init < 1 or not 0.0 <= float(tol) <= 1.0:
        raise ValueError(f"kmeans: max_iter = {max_iter}, n_init = {n_init}, tol = {tol}")
    explicit = isinstance(init, torch.Tensor)
    if explicit:
        if init.dim() != 2 or tuple(init.shape) != (k, E):
            raise ValueError(f"kmeans: init must be [{k}, {E}], got {tuple(init.shape)}")
        n_init = 1
    elif init not in ("kmeans++", "random"):
        raise ValueError(f"kmeans: init = {init!r}; expected 'kmeans++', 'random' or a [k, E] tensor")
    runs, objectives = [], []
    for run in range(n_init):
        if explicit:
            c0 = _rows16(init, x.dtype, x.device)
        else:
            pick = _seed_plusplus(x, k, seed + run) if init == "kmeans++" else _seed_random(N, k, seed + run).to(x.device)
            c0 = x[pick]
        fields = _lloyd(x, c0, max_iter, float(tol), bool(reseed_empty))
        runs.append(fields)
        objectives.append(fields["scores"].mean().item())
    best = pick_best_run(objectives)
    return KMeansResult(objective=objectives[best], **runs[best])


def cluster_purity(labels, classes) -> Tuple[float, torch.Tensor]:
    """Purity of a clustering against known classes, on the host: labels [N] cluster ids, classes [N] class ids; a negative
    class id marks an unlabelled row, which is left out.  Returns (purity, majority int64 [number of clusters]): the share of
    the labelled rows that carry their cluster's majority class, and that class per cluster (equal counts: the lower class;
    -1 for a cluster without a labelled row)."""
    labels = torch.as_tensor(labels).detach().cpu().long()
    classes = torch.as_tensor(classes).detach().cpu().long()
    if labels.dim() != 1 or labels.shape != classes.shape:
        raise ValueError(f"cluster_purity: expected two [N] vectors, got {tuple(labels.shape)} and {tuple(classes.shape)}")
    if labels.numel() and int(labels.min()) < 0:
        raise ValueError("cluster_purity: negative cluster id")
    k = int(labels.max()) + 1 if labels.numel() else 0
    known = classes >= 0
    n_cls = int(classes[known].max()) + 1 if bool(known.any()) else 0
    majority = torch.full((k,), -1, dtype=torch.int64)
    if n_cls == 0:
        return 0.0, majority
    table = torch.bincount(labels[known] * n_cls + classes[known], minlength=k * n_cls).view(k, n_cls)
    top, arg = table.max(dim=1)                                                  # the first maximum: the lower class
    majority[top > 0] = arg[top > 0]
    return top.sum().item() / int(known.sum()), majority


@torch.no_grad()
def name_clusters(result: KMeansResult, text_features: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The prompt nearest to every centroid: text_features [P, E] (normalised like the rows) -> (index int64 [k], score fp32
    [k]) through the top-k kernel."""
    c = result.centroids
    t = _rows16(text_features, c.dtype, c.device)
    if t.shape[0] < 1 or t.shape[1] != c.shape[1]:
        raise ValueError(f"name_clusters: expected [P >= 1, {c.shape[1]}] text features, got {tuple(t.shape)}")
    score, index = ops.similarity_topk(c, t, 1)
    return index[:, 0].long(), score[:, 0]
