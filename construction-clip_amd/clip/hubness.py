"""Hubness-corrected retrieval: querybank normalisation of the similarity ranking, training-free.

In a CLIP embedding cone a few stored rows - hubs: generic photos, the repeated `violation_list` strings - lie near the cone's
axis and come out first for many unrelated queries.  The three standard corrections discount every stored row by how strongly a
bank of typical queries already points at it:

  "is"    the inverted softmax (Smith et al. 2017): t[q, n] = beta s[q, n] - log sum_b exp(beta s[b, n]), the log of the
          softmax over the bank of column n.
  "dis"   QB-Norm's dynamic inverted softmax (Bogolin et al., CVPR 2022): the same, but only for the queries whose raw best
          row lies in the activation set - the rows that are among the top `activation_k` of some bank row.  Every other
          query keeps its raw result, bitwise what `EmbeddingIndex.search` returns without a querybank.
  "csls"  CSLS (Conneau et al. 2018): t[q, n] = 2 s[q, n] - r[n], r[n] the mean of the min(k, B) largest s[b, n].  Its
          query-side term (the mean similarity of the query to its own neighbours) is constant per query, cannot change a
          query's ranking and is left out, so the returned values are CSLS plus a per-query constant.

All three are one per-row bias and one scale: t = fmaf(scale, s, bias[n]).  `fit_querybank` computes the bias on the device
(csrc/embed_hub.hip for the log-sum-exp, the top-k kernel for the rest) and `EmbeddingIndex.search(querybank=)` ranks by t with
the biased form of the exact top-k kernel (csrc/embed_topk.hip); neither the Q x N nor the B x N matrix is ever formed and
nothing is read on the host.  The same biased kernel gives filtered search: `search(mask=)` puts -inf on the rows to leave out.

`hubness` measures the defect itself: the k-occurrence counts of a search result, their skewness, the share of rows never
retrieved and the worst hubs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Union

import torch

from cclip_hip import ops
from .retrieval import EmbeddingIndex, normalize_rows

METHODS = ("is", "dis", "csls")


@dataclass
class QueryBank:
    """A fitted correction for an index of `n` rows: method, beta (of "is" / "dis"), k (of "csls"), n_bank rows of the bank,
    and what the search uses - scale, bias fp32 [n], active bool [n] (all True except for "dis").  Tensors live on the device."""
    method: str
    beta: float
    k: int
    n: int
    n_bank: int
    scale: float
    bias: torch.Tensor
    active: torch.Tensor

    def __post_init__(self):
        if self.method not in METHODS:
            raise ValueError(f"QueryBank: method must be one of {METHODS}, got {self.method!r}")
        if self.n < 1 or self.n_bank < 1:
            raise ValueError(f"QueryBank: n = {self.n} and n_bank = {self.n_bank} must be positive")
        for t, name, dtype in ((self.bias, "bias", torch.float32), (self.active, "active", torch.bool)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (self.n,):
                raise ValueError(f"QueryBank: {name} must be a {str(dtype)[6:]} [{self.n}] tensor, got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if self.bias.device != self.active.device:
            raise ValueError(f"QueryBank: bias on {self.bias.device}, active on {self.active.device}")
        self.scale = float(self.scale)
        if self.scale != self.scale or self.scale in (float("inf"), float("-inf")):
            raise ValueError(f"QueryBank: scale must be finite, got {self.scale}")

    def check(self, n: int, device=None) -> "QueryBank":
        """Raises ValueError unless this bank was fitted for an index of n rows (on `device`): an index that has grown since
        (`EmbeddingIndex.add`) needs a new fit."""
        if n != self.n:
            raise ValueError(f"QueryBank: fitted for {self.n} stored rows, the index holds {n}; fit it again")
        if device is not None and self.bias.device != device:
            raise ValueError(f"QueryBank: fitted on {self.bias.device}, the index lives on {device}")
        return self


def _rows(who: str, rows, dtype: Optional[torch.dtype], device=None) -> torch.Tensor:
    from .cluster import _rows16
    if not isinstance(rows, torch.Tensor):
        raise TypeError(f"{who}: expected a tensor or an EmbeddingIndex, got {type(rows)}")
    if rows.dim() == 1:
        rows = rows[None]
    return _rows16(rows, dtype, device)


@torch.no_grad()
def fit_querybank(index_or_rows: Union[EmbeddingIndex, torch.Tensor], bank: torch.Tensor, *, method: str = "dis", beta: float = 20.0,
                  k: int = 10, activation_k: int = 1) -> QueryBank:
    """Fit the correction of `method` for the stored rows of an `EmbeddingIndex` (or [N, E] rows: 16-bit device rows are taken as
    unit rows as they are, anything else is normalised and rounded to bfloat16) from `bank` [B, E], a sample of typical queries
    (any float dtype, anywhere; always normalised and rounded exactly as `search` normalises queries, a 16-bit bank included).
    beta: the inverse temperature of "is" / "dis" (not read by "csls"); k: the neighbourhood of "csls" (min(k, B) <= 64 bank rows); activation_k: how many best rows of every bank row enter the
    activation set of "dis".  Two or three launches, no host read."""
    who = "fit_querybank"
    if method not in METHODS:
        raise ValueError(f"{who}: method must be one of {METHODS}, got {method!r}")
    if isinstance(index_or_rows, EmbeddingIndex):
        if len(index_or_rows) == 0:
            raise ValueError(f"{who}: the index is empty")
        g = index_or_rows.features
    else:
        g = _rows(who, index_or_rows, None)
    if not isinstance(bank, torch.Tensor) or bank.dim() not in (1, 2) or bank.shape[-1] != g.shape[1] or bank.numel() == 0:
        raise ValueError(f"{who}: expected a [B >= 1, {g.shape[1]}] bank, got {tuple(getattr(bank, 'shape', ()))}")
    if not bank.is_floating_point():
        raise ValueError(f"{who}: expected a float bank, got {bank.dtype}")
    b = normalize_rows(bank if bank.dim() == 2 else bank[None], g.dtype, g.device)
    N, B = g.shape[0], b.shape[0]
    k, activation_k = int(k), int(activation_k)
    active = torch.ones(N, device=g.device, dtype=torch.bool)
    if method == "csls":
        if k < 1 or min(k, B) > ops.SIMILARITY_TOPK_MAX_K:
            raise ValueError(f"{who}: k = {k} must lie in 1 .. {ops.SIMILARITY_TOPK_MAX_K} (or reach the whole bank of {B})")
        near, _ = ops.similarity_topk(g, b, min(k, B))              # [N, min(k, B)]: every stored row's nearest bank rows
        bias = near.mean(dim=1).neg_()
        scale, beta = 2.0, 0.0                                      # beta is not part of CSLS
    else:
        beta = float(beta)
        if not beta > 0 or beta == float("inf"):
            raise ValueError(f"{who}: beta = {beta} must be positive and finite")
        bias = ops.bank_lse(g, b, beta).neg_()
        scale = float(torch.tensor(beta, dtype=torch.float32))      # what the kernels multiply by
        if method == "dis":
            if activation_k < 1 or min(activation_k, N) > ops.SIMILARITY_TOPK_MAX_K:
                raise ValueError(f"{who}: activation_k = {activation_k} must lie in 1 .. {ops.SIMILARITY_TOPK_MAX_K}")
            _, hit = ops.similarity_topk(b, g, min(activation_k, N))
            active = torch.zeros(N, device=g.device, dtype=torch.bool)
            active[hit.reshape(-1).long()] = True
    return QueryBank(method=method, beta=float(beta), k=k, n=N, n_bank=B, scale=scale, bias=bias, active=active)


def mask_bias(who: str, mask: torch.Tensor, n: int, device, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n]: `bias` (zero when None) with -inf on the rows where mask is True"""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (n,):
        raise ValueError(f"{who}: mask must be a bool [{n}] tensor (True: leave the row out), got "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    base = torch.zeros(n, device=device, dtype=torch.float32) if bias is None else bias
    return base.masked_fill(mask.to(device), float("-inf"))


@torch.no_grad()
def corrected_topk(q: torch.Tensor, g: torch.Tensor, k: int, querybank: Optional[QueryBank], mask: Optional[torch.Tensor]):
    """(scores fp32 [Q, k], index int32 [Q, k], gate bool [Q]) for unit 16-bit rows q, g: what `EmbeddingIndex.search` returns
    for a querybank and / or a mask.  gate: the queries that took the normalised path."""
    who = "search"
    N, dev = g.shape[0], g.device
    if querybank is not None:
        querybank.check(N, dev)
    dynamic = querybank is not None and querybank.method == "dis"
    raw = None
    if querybank is None or dynamic:                                 # the raw ranking, over the rows the mask leaves
        raw = ops.similarity_topk(q, g, k) if mask is None else ops.similarity_topk_biased(q, g, k, mask_bias(who, mask, N, dev), 1.0)
    if querybank is None:
        return raw[0], raw[1], torch.zeros(q.shape[0], device=dev, dtype=torch.bool)
    bias = querybank.bias if mask is None else mask_bias(who, mask, N, dev, querybank.bias)
    scores, index = ops.similarity_topk_biased(q, g, k, bias, querybank.scale)
    if not dynamic:
        return scores, index, torch.ones(q.shape[0], device=dev, dtype=torch.bool)
    gate = querybank.active[raw[1][:, 0].long()]
    return torch.where(gate[:, None], scores, raw[0]), torch.where(gate[:, None], index, raw[1]), gate


@dataclass
class HubnessReport:
    """counts int64 [n] (on the device of the indices): how often every stored row occurs in the result (its k-occurrence);
    skewness of the counts (0 for a result that spreads evenly, large when a few rows take most places); never: the share of
    rows that no query retrieved; top: the rows with the largest counts, worst first (equal counts by the lower row), and
    top_counts alongside."""
    counts: torch.Tensor
    skewness: float
    never: float
    top: List[int]
    top_counts: List[int]


@torch.no_grad()
def hubness(indices: torch.Tensor, n: int, top: int = 10) -> HubnessReport:
    """The hubness of a search result: indices [Q, k] (any integer dtype, entries in [0, n)) over a gallery of n rows.  Torch
    on the indices' device; one host read brings the scalars and the `top` rows."""
    n, top = int(n), int(top)
    if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.is_floating_point() or indices.dtype == torch.bool:
        raise ValueError(f"hubness: expected an integer [Q, k] tensor of row indices, got {getattr(indices, 'dtype', type(indices))} "
                         f"{tuple(getattr(indices, 'shape', ()))}")
    if n < 1 or indices.numel() == 0:
        raise ValueError(f"hubness: n = {n} and the result {tuple(indices.shape)} must not be empty")
    flat = indices.reshape(-1).long()
    bad = (flat < 0) | (flat >= n)                                   # checked with the one read below
    counts = torch.bincount(flat.clamp(0, n - 1), minlength=n)
    c = counts.to(torch.float64)
    dev = c - c.mean()
    var = (dev * dev).mean()
    skew = torch.where(var > 0, (dev ** 3).mean() / var.clamp_min(1e-300) ** 1.5, torch.zeros_like(var))
    top = max(0, min(top, n))
    order = torch.argsort(counts, descending=True, stable=True)[:top]
    packed = torch.cat([torch.stack([skew, (counts == 0).to(torch.float64).mean(), bad.any().to(torch.float64)]),
                        order.to(torch.float64), counts[order].to(torch.float64)]).tolist()     # the one host read
    if packed[2]:
        raise ValueError(f"hubness: an index lies outside 0 .. {n - 1}")
    return HubnessReport(counts=counts, skewness=packed[0], never=packed[1], top=[int(v) for v in packed[3:3 + top]],
                         top_counts=[int(v) for v in packed[3 + top:]])
