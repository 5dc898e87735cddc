"""Coreset selection over the stored embeddings: "which photos should be labelled next?"

The collections are mostly unlabelled, and every analysis here takes the labelled rows as given.  `select_coreset` is the
k-centre greedy answer (farthest-point sampling; the coreset of Sener & Savarese 2018, "Active learning for convolutional neural
networks: a core-set approach"): start from the labelled rows, pick the row farthest from everything chosen so far, repeat m
times.  The radius the picks leave uncovered is at most twice the smallest any m centres could reach.  Without seeds the same
call gives a diverse subset of a collection: a small captioning set, a contact sheet, a validation split that covers the set.

    distance[i] = min over the centres c of 1 - <x_i, x_c>            (cosine distance of the stored unit 16-bit rows)
    pick        = argmax over the rows that are no centre of weights[i] * distance[i],  equal values to the lower row

Each pick is one launch of csrc/coreset.hip that updates every row's distance to the new centre and finds the next arg-max in
the same pass; the m launches are enqueued by one native call and the pick never visits the host - pick t + 1 depends on pick
t.  Seeding reuses the assignment kernel of k-means against the seed rows.  No kernel uses a float atomic and every sum has
one fixed order, so a result is a pure function of its inputs.  torch is plumbing: the gather of the seed rows, the mean
direction, the counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex, normalize_rows
from .tsne import _unit_rows


@dataclass
class CoresetResult:
    """picks int64 [m]: the chosen rows in pick order (-1 once no eligible row was left); radius fp32 [m]: the distance of pick
    t to the centres before it, i.e. the covering radius those left (+inf for a first pick without seeds; non-increasing
    without weights); owner int64 [N]: the nearest centre of every row (the row itself for a centre, -1 if there is no centre
    at all); distance fp32 [N]: the cosine distance to it (0 for a centre); seeds int64 [S]: the rows that were centres from
    the start, ascending.  Tensors live on the device; nothing is read until the caller reads it."""
    picks: torch.Tensor
    radius: torch.Tensor
    owner: torch.Tensor
    distance: torch.Tensor
    seeds: torch.Tensor

    @property
    def centres(self) -> torch.Tensor:
        """int64 [S + m]: the seeds, then the picks"""
        return torch.cat([self.seeds, self.picks])

    @property
    def cover_radius(self) -> torch.Tensor:
        """the largest `distance`: a 0-dim fp32 device tensor, one device reduction"""
        return self.distance.max()

    def cover_counts(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(centres int64 [S + m], counts int64 [S + m]): the rows every centre is the nearest centre of, itself included; the
        counts sum to N.  A sort of `owner` and two binary searches per centre - the exact bincount without bincount's hidden
        host read (the construction of ops.kmeans_update)."""
        centres = self.centres
        owners = torch.sort(self.owner).values
        counts = torch.searchsorted(owners, centres, right=True) - torch.searchsorted(owners, centres, right=False)
        return centres, torch.where(centres >= 0, counts, torch.zeros_like(counts))

    def covered(self, threshold: float) -> torch.Tensor:
        """the share of rows within `threshold` of a centre: a 0-dim fp32 device tensor"""
        return (self.distance <= float(threshold)).float().mean()


def _seed_rows(N: int, labelled) -> torch.Tensor:
    """`labelled` in any of its three forms -> the seed rows, int64 [S] ascending, where `labelled` lives: a bool mask [N]; N
    integer labels, below 0 = unlabelled (the convention of `cluster_purity` and `spread_labels`); or row indices (any other
    length; distinct, inside [0, N))."""
    if labelled is None:
        return torch.empty(0, dtype=torch.int64)
    lab = torch.as_tensor(labelled)
    if lab.dim() != 1 or lab.is_floating_point() or lab.is_complex():
        raise ValueError(f"select_coreset: labelled must be a bool mask, {N} integer labels or a vector of row indices, got "
                         f"{tuple(lab.shape)} {lab.dtype}")
    if lab.dtype == torch.bool:
        if lab.numel() != N:
            raise ValueError(f"select_coreset: the labelled mask has {lab.numel()} entries for {N} rows")
        return torch.nonzero(lab).flatten()
    lab = lab.to(torch.int64)
    if lab.numel() == N:                                   # labels; N distinct row indices name every row, as N labels >= 0 do
        return torch.nonzero(lab >= 0).flatten()
    if lab.numel() == 0:
        return lab
    rows = torch.sort(lab).values
    lo, hi, repeats = torch.stack([rows[0], rows[-1], (rows[1:] == rows[:-1]).sum()]).tolist()     # one host read
    if lo < 0 or hi >= N or repeats:
        raise ValueError(f"select_coreset: labelled row indices must be distinct and inside [0, {N}): min {lo}, max {hi}, "
                         f"{repeats} repeated")
    return rows


def _check_arguments(N: int, m, labelled, weights, first):
    """The argument errors of `select_coreset`, before anything touches a device: returns (m, seeds int64 [S] ascending,
    weights fp32 [N] or None, first: "mean" or an int)."""
    if N < 1:
        raise ValueError("select_coreset: no rows")
    if isinstance(m, bool) or int(m) != m:
        raise ValueError(f"select_coreset: m = {m!r} must be an integer")
    m = int(m)
    seeds = _seed_rows(N, labelled)
    S = int(seeds.numel())                                 # (a shape: the one host read was nonzero's)
    if not 0 <= m <= N - S:
        raise ValueError(f"select_coreset: m = {m} outside [0, {N - S}] ({N} rows, {S} of them labelled)")
    if weights is not None:
        weights = torch.as_tensor(weights)
        if weights.dim() != 1 or weights.numel() != N or not weights.is_floating_point():
            raise ValueError(f"select_coreset: weights must be {N} floats, got {tuple(weights.shape)} {weights.dtype}")
        weights = weights.detach().to(torch.float32).contiguous()
    if isinstance(first, str):
        if first != "mean":
            raise ValueError(f"select_coreset: first = {first!r}; expected 'mean' or a row index")
    elif isinstance(first, bool) or not isinstance(first, int):
        raise ValueError(f"select_coreset: first = {first!r}; expected 'mean' or a row index")
    elif not 0 <= first < N:
        raise ValueError(f"select_coreset: first = {first} outside [0, {N})")
    return m, seeds, weights, first


def _mean_row_key(x: torch.Tensor, weights: Optional[torch.Tensor]) -> torch.Tensor:
    """The partial key (int64 [1], on the device) that makes the first pick the row most similar to the mean direction:
    similarity_topk of the normalised, rounded mean against the rows.  With weights, the most similar of the 64 nearest whose
    weight is > 0 (the nearest itself if none is).  The row never visits the host."""
    N = x.shape[0]
    mean16 = normalize_rows(x.sum(dim=0, dtype=torch.float32)[None], x.dtype, x.device)
    k = 1 if weights is None else min(N, ops.SIMILARITY_TOPK_MAX_K)
    _, index = ops.similarity_topk(mean16, x, k)
    cand = index[0].long()
    if weights is None:
        row = cand[:1]
    else:
        rank = torch.where(weights[cand] > 0, torch.arange(k, device=x.device), torch.full((k,), k, device=x.device))
        row = cand[rank.min().remainder(k)][None]                  # k (none eligible) wraps to 0: the nearest row
    return (1 << 32) | ((~row) & 0xFFFFFFFF)                       # any non-zero high word above ~row: the only non-zero key


@torch.no_grad()
def select_coreset(features: Union[torch.Tensor, EmbeddingIndex], m: int, *, labelled=None, weights=None,
                   first: Union[str, int] = "mean", dtype: Optional[torch.dtype] = None) -> CoresetResult:
    """k-centre greedy selection of m rows of [N, E] features (any float dtype, anywhere: normalised and rounded to `dtype`,
    default bfloat16; 16-bit device rows are taken as unit rows as they are) or of an `EmbeddingIndex` (its stored rows, not
    copied).

    labelled: the rows that already carry a label - row indices, a bool mask [N], or N integer labels with a value below 0
    for an unlabelled row.  They are centres from the start and are never picked.  weights: N floats; a pick maximises
    weights[i] * distance[i], and a row whose weight is not > 0 (NaN included) is never picked - e.g. 1 -
    LabelSpreadResult.certainty combines "far from what is labelled" with "the propagation is unsure here".  first (used only
    without seeds): "mean", the row most similar to the mean direction, or a row index.  m <= N - the number of seeds; m == 0
    only places the rows under the seeds.  Should the eligible rows run out, the remaining picks are -1.

    Host reads: the number of labelled rows (the argument check).  The m launches read nothing back.  Two calls with the same
    arguments return bitwise equal results."""
    N = len(features) if isinstance(features, EmbeddingIndex) else features.shape[0]
    m, seeds, weights, first = _check_arguments(N, m, labelled, weights, first)
    x = _unit_rows(features, dtype)
    dev = x.device
    seeds = seeds.to(dev)
    w = None if weights is None else weights.to(dev)
    ws = torch.zeros(2, ops.coreset_blocks(N), device=dev, dtype=torch.int64)
    start = None
    if seeds.numel():
        assign, best, _ = ops.kmeans_assign(x, x[seeds])           # every row against all seed rows at once: no per-seed loop
        mind = (1.0 - best).clamp_(min=0.0)
        owner = seeds[assign.long()].to(torch.int32)
        mind[seeds] = 0.0
        owner[seeds] = seeds.to(torch.int32)
        ops.coreset_step(x, mind, owner, ws[0], scan_only=True, weight=w)
    else:
        mind = torch.full((N,), float("inf"), device=dev, dtype=torch.float32)
        owner = torch.full((N,), -1, device=dev, dtype=torch.int32)
        if first == "mean":
            if m:
                ws[0, :1] = _mean_row_key(x, w)
        else:
            start = first
    picks, radius, _ = ops.coreset_greedy(x, mind, owner, m, first=start, workspace=ws, weight=w)
    return CoresetResult(picks=picks.long(), radius=radius, owner=owner.long(), distance=mind, seeds=seeds)
