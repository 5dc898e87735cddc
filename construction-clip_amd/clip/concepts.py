"""Concept decomposition of the stored embeddings: "what is in this photo's embedding?", in words.

SpLiCE (Bhalla et al. 2024, "Interpreting CLIP with sparse linear concept embeddings"): write every image embedding as a
SPARSE, NON-NEGATIVE combination of the text embeddings of a concept vocabulary - a few thousand words and phrases.  Per row x,

    minimise over w >= 0:   1/2 |x - sum_v w_v c_v|^2  +  l1 sum_v w_v

solved by a fixed number of FISTA iterations inside one launch of csrc/concept_codes.hip (include/cclip_hip.h states the
arithmetic).  The result reads "0.41 scaffold + 0.22 missing guard rail + 0.09 worker"; it can be averaged per cluster, class or
site (`concept_profile`, `distinctive`), and `kkt` says per row how far from the optimum the fixed iteration count stopped.
No tower is needed at decomposition time: the dictionary's text is encoded once (`ConceptDictionary.from_texts`).

Image and text embeddings of CLIP lie in two separate cones (the modality gap), so SpLiCE centres each modality: pass
`center=` to the dictionary and to `decompose` (a mean vector, or "mean" for the set's own mean).

torch is plumbing: the normalisation, the D x D Gram matrix whose largest eigenvalue is the step's 1 / L (float64, once per
dictionary), the top-k of a chunk's weights and the gather behind `cosine` / `recompose`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from cclip_hip import ops
from .cluster import _rows16
from .retrieval import EmbeddingIndex, normalize_rows

_GATHER_BYTES = 1 << 28                                    # bound of the [rows, terms, D] fp32 gather behind cosine / recompose


def _unit_rows(features_or_index, dtype: torch.dtype) -> torch.Tensor:
    """Unit 16-bit rows of `dtype` on the device: the stored rows of an index, or `_rows16` of a tensor."""
    if isinstance(features_or_index, EmbeddingIndex):
        if features_or_index.dtype != dtype:
            raise ValueError(f"decompose: the index stores {features_or_index.dtype} rows, the dictionary {dtype}")
        return features_or_index.features
    return _rows16(features_or_index, dtype)


def _unit32(features: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.normalize(features.detach().to(torch.float32), dim=1)


def _center_arg(center, D: int, who: str):
    if center is None or (isinstance(center, str) and center == "mean"):
        return center
    if isinstance(center, torch.Tensor) and center.dim() == 1 and center.numel() == D and center.is_floating_point():
        return center.detach().to(torch.float32)
    raise ValueError(f"{who}: center must be None, 'mean' or a float vector of {D} entries, got {center!r}")


class ConceptDictionary:
    """The concept vocabulary: features [V, D] (any float dtype, anywhere; text embeddings of the words) -> unit 16-bit rows on
    the device.  center: None, "mean" (the mean of the normalised rows) or a [D] vector: it is subtracted from the normalised
    rows, which are then normalised again.  Keeps `rows`, `names` (V strings or None), `mean` (fp32 [D] or None) and `L`, the
    largest eigenvalue of rows^T rows in float64 (one host read): the step of `decompose` is 1 / L."""

    def __init__(self, features: torch.Tensor, names: Optional[Sequence[str]] = None, dtype: Optional[torch.dtype] = None,
                 center=None):
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_floating_point() or features.shape[0] < 1:
            raise ValueError(f"ConceptDictionary: expected [V >= 1, D] float features, got {getattr(features, 'shape', type(features))}")
        V, D = features.shape
        if names is not None and len(names) != V:
            raise ValueError(f"ConceptDictionary: {len(names)} names for {V} concepts")
        center = _center_arg(center, D, "ConceptDictionary")
        self.dtype = torch.bfloat16 if dtype is None else dtype
        self.names = None if names is None else [str(n) for n in names]
        if center is None:
            self.mean = None
            self.rows = _unit_rows(features, self.dtype)
        else:
            unit = _unit32(features)
            self.mean = unit.mean(dim=0) if isinstance(center, str) else center.to(unit.device)
            self.rows = normalize_rows(unit - self.mean, self.dtype)
            self.mean = self.mean.to(self.rows.device)
        if self.rows.dtype != self.dtype:
            raise ValueError(f"ConceptDictionary: the rows are {self.rows.dtype}, dtype = {self.dtype}")
        c = self.rows.double()
        self.L = float(torch.linalg.eigvalsh((c.t() @ c).cpu())[-1])
        if not self.L > 0.0:
            raise ValueError("ConceptDictionary: the dictionary has no non-zero row")

    def __len__(self) -> int:
        return self.rows.shape[0]

    @property
    def dim(self) -> int:
        return self.rows.shape[1]

    def name(self, v: int) -> str:
        return str(v) if self.names is None else self.names[v]

    @classmethod
    @torch.no_grad()
    def from_texts(cls, model, tokens: torch.Tensor, names: Optional[Sequence[str]] = None, batch: int = 1024, **kw):
        """Encode the vocabulary once: tokens [V, context] (clip.tokenize of the words or of a prompt around them)."""
        dev = next(model.parameters()).device
        feats = torch.cat([model.encode_text(tokens[i:i + batch].to(dev)).float() for i in range(0, tokens.shape[0], batch)])
        return cls(feats, names=names, **kw)


@dataclass
class ConceptDecomposition:
    """indices int64 [N, K] and weights fp32 [N, K]: the K = min(max_terms, V) largest weights of every row, descending; an
    entry whose weight is not > 0 has index -1 and weight 0.  nnz int64 [N]: the positive weights of the full solution;
    truncated bool [N]: nnz > K, i.e. terms were dropped.  cosine fp32 [N]: of the row with its reconstruction from the kept
    terms (0 where nothing is kept).  kkt, delta, l1norm, resid2 fp32 [N]: the kernel's read-outs at the full solution (kkt: the
    distance from optimality; delta: the last iteration's largest change).  scale fp32 [N] and mean fp32 [D]: |x - mean| and
    the mean when centred, else None.  Tensors live where the rows do; nothing is read until the caller reads it."""
    indices: torch.Tensor
    weights: torch.Tensor
    nnz: torch.Tensor
    cosine: torch.Tensor
    kkt: torch.Tensor
    delta: torch.Tensor
    l1norm: torch.Tensor
    resid2: torch.Tensor
    truncated: torch.Tensor
    dictionary: ConceptDictionary
    scale: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self.indices.shape[0]

    def terms(self, i: int) -> List[Tuple[str, float]]:
        """[(name, weight)] of row i, largest first (one host read)"""
        idx, w = self.indices[i].tolist(), self.weights[i].tolist()
        return [(self.dictionary.name(v), float(x)) for v, x in zip(idx, w) if v >= 0]

    def to_csr(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(crow int64 [N + 1], col int64 [nnz kept], val fp32): the kept positive weights of every row, largest first"""
        keep = self.indices >= 0
        crow = torch.zeros(len(self) + 1, dtype=torch.int64, device=keep.device)
        crow[1:] = keep.sum(dim=1).cumsum(0)
        return crow, self.indices[keep], self.weights[keep]

    def _combine(self, lo: int, hi: int) -> torch.Tensor:
        c = self.dictionary.rows
        picked = c[self.indices[lo:hi].clamp(min=0)].float()                           # [rows, K, D]; index -1 has weight 0
        return (self.weights[lo:hi, :, None] * picked).sum(dim=1)

    def _rows_per_gather(self) -> int:
        return max(1, _GATHER_BYTES // (4 * max(1, self.indices.shape[1]) * self.dictionary.dim))

    def recompose(self) -> torch.Tensor:
        """fp32 unit rows [N, D] rebuilt from the kept terms: normalise(sum w c), or normalise(scale * sum w c + mean) when the
        rows were centred (a row without a kept term comes back as the normalised mean, or as zeros)."""
        step, out = self._rows_per_gather(), []
        for lo in range(0, len(self), step):
            s = self._combine(lo, lo + step)
            if self.mean is not None:
                s = self.scale[lo:lo + step, None] * s + self.mean
            out.append(torch.nn.functional.normalize(s, dim=1))
        return torch.cat(out) if out else torch.empty(0, self.dictionary.dim)


def _rows_and_center(features, dictionary: ConceptDictionary, center):
    """The 16-bit unit rows the kernel sees, and (scale, mean) when centred."""
    D = dictionary.dim
    center = _center_arg(center, D, "decompose")
    if center is None:
        return _unit_rows(features, dictionary.dtype), None, None
    if isinstance(features, EmbeddingIndex):
        if features.dtype != dictionary.dtype:
            raise ValueError(f"decompose: the index stores {features.dtype} rows, the dictionary {dictionary.dtype}")
        unit = features.features.float()
    else:
        unit = _unit32(features).to(dictionary.rows.device)
    mean = unit.mean(dim=0) if isinstance(center, str) else center.to(unit.device)
    diff = unit - mean
    return normalize_rows(diff, dictionary.dtype), diff.norm(dim=1), mean


@torch.no_grad()
def decompose(features: Union[torch.Tensor, EmbeddingIndex], dictionary: ConceptDictionary, *, l1: float = 0.1, iters: int = 200,
              max_terms: int = 32, center=None, chunk_bytes: int = 1 << 30) -> ConceptDecomposition:
    """Sparse non-negative concept codes of [N, D] features (any float dtype, anywhere; 16-bit device rows are taken as unit
    rows as they are) or of an `EmbeddingIndex` over `dictionary`.

    l1: the sparsity weight (larger: fewer concepts; at l1 >= max_v <c_v, x> a row's code is empty).  iters: FISTA iterations,
    fixed - read `kkt` to see whether they were enough.  center: None, a [D] mean to subtract from the normalised rows, or
    "mean" for the set's own; use it together with a centred dictionary.  The rows are worked through in chunks whose fp32
    state (w and w_{k-1}, [rows, V] each) stays under chunk_bytes; per chunk the max_terms largest weights of every row are
    kept (torch.topk on the device) with the read-outs, and the dense state is reused by the next chunk.  No host read."""
    if not isinstance(dictionary, ConceptDictionary):
        raise TypeError(f"decompose: dictionary must be a ConceptDictionary, got {type(dictionary)}")
    for n, v, lo in (("iters", iters, 0), ("max_terms", max_terms, 1), ("chunk_bytes", chunk_bytes, 1)):
        if isinstance(v, bool) or int(v) != v or v < lo:
            raise ValueError(f"decompose: {n} = {v!r} must be an integer >= {lo}")
    l1 = float(l1)
    if not 0.0 <= l1 < float("inf"):
        raise ValueError(f"decompose: l1 = {l1} must be finite and >= 0")
    x, scale, mean = _rows_and_center(features, dictionary, center)
    c = dictionary.rows
    N, D = x.shape
    V = len(dictionary)
    if N < 1:
        raise ValueError("decompose: no rows")
    if D != dictionary.dim:
        raise ValueError(f"decompose: rows of width {D}, dictionary of width {dictionary.dim}")
    if x.dtype != c.dtype or x.device != c.device:
        raise ValueError(f"decompose: rows are {x.dtype} on {x.device}, the dictionary {c.dtype} on {c.device}")
    dev = x.device
    Vp = (V + 3) // 4 * 4
    rows = int(min(N, max(1, int(chunk_bytes) // (8 * Vp))))
    K = int(min(max_terms, V))
    wbuf = torch.empty(rows, Vp, device=dev, dtype=torch.float32)
    ws = torch.empty(rows * Vp, device=dev, dtype=torch.float32)
    eta = 1.0 / dictionary.L
    idx = torch.empty(N, K, device=dev, dtype=torch.int64)
    wts = torch.empty(N, K, device=dev, dtype=torch.float32)
    outs = {k: [] for k in ("resid2", "l1norm", "nnz", "delta", "kkt")}
    for lo in range(0, N, rows):
        hi = min(N, lo + rows)
        w, resid2, l1norm, nnz, delta, kkt = ops.concept_codes(x[lo:hi], c, l1, eta, int(iters), out_w=wbuf[:hi - lo, :V],
                                                                workspace=ws)
        top, at = torch.topk(w, K, dim=1)
        keep = top > 0
        wts[lo:hi] = torch.where(keep, top, torch.zeros_like(top))
        idx[lo:hi] = torch.where(keep, at, torch.full_like(at, -1))
        for k, v in zip(outs, (resid2, l1norm, nnz, delta, kkt)):
            outs[k].append(v)
    o = {k: torch.cat(v) for k, v in outs.items()}
    nnz = o["nnz"].long()
    dec = ConceptDecomposition(indices=idx, weights=wts, nnz=nnz, cosine=None, kkt=o["kkt"], delta=o["delta"], l1norm=o["l1norm"],
                               resid2=o["resid2"], truncated=nnz > K, dictionary=dictionary, scale=scale, mean=mean)
    cos, step = [], dec._rows_per_gather()
    for lo in range(0, N, step):
        s = dec._combine(lo, lo + step)
        cos.append((torch.nn.functional.normalize(s, dim=1) * torch.nn.functional.normalize(x[lo:lo + step].float(), dim=1)).sum(dim=1))
    dec.cosine = torch.cat(cos)
    return dec


@dataclass
class ConceptProfile:
    """groups int64 [G] ascending: the group ids; counts int64 [G]; mean fp32 [G, V]: the mean kept weight of every concept over
    the rows of a group; overall fp32 [V]: the same over all grouped rows."""
    groups: torch.Tensor
    counts: torch.Tensor
    mean: torch.Tensor
    overall: torch.Tensor
    dictionary: ConceptDictionary


def concept_profile(decomposition: ConceptDecomposition, groups) -> ConceptProfile:
    """Mean weight per concept per group: groups, N integers (cluster, class or site ids; a value below 0 leaves the row out)."""
    g = torch.as_tensor(groups)
    N = len(decomposition)
    if g.dim() != 1 or g.numel() != N or g.is_floating_point() or g.dtype == torch.bool:
        raise ValueError(f"concept_profile: groups must be {N} integers, got {tuple(g.shape)} {g.dtype}")
    dev = decomposition.indices.device
    g = g.to(device=dev, dtype=torch.int64)
    ids = torch.unique(g[g >= 0])
    G, V, K = int(ids.numel()), len(decomposition.dictionary), decomposition.indices.shape[1]
    slot = torch.searchsorted(ids, g.clamp(min=0))
    live = ((g >= 0)[:, None] & (decomposition.indices >= 0))
    flat = (slot[:, None] * V + decomposition.indices.clamp(min=0))[live]
    total = torch.zeros(G * V, device=dev, dtype=torch.float32).index_add_(0, flat, decomposition.weights[live]).view(G, V)
    counts = torch.zeros(G, device=dev, dtype=torch.int64).index_add_(0, slot[g >= 0], torch.ones_like(slot[g >= 0]))
    n = counts.sum().clamp(min=1)
    return ConceptProfile(groups=ids, counts=counts, mean=total / counts.clamp(min=1)[:, None].float(),
                          overall=total.sum(dim=0) / n.float(), dictionary=decomposition.dictionary)


def distinctive(profile: ConceptProfile, k: int = 10) -> dict:
    """{group id: [(name, mean weight in the group - overall mean weight)]}: the k concepts whose group mean most exceeds the
    overall mean, largest first (one host read)"""
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"distinctive: k = {k!r} must be an integer >= 1")
    excess = profile.mean - profile.overall
    top, at = torch.topk(excess, min(int(k), excess.shape[1]), dim=1)
    return {int(gid): [(profile.dictionary.name(v), float(e)) for v, e in zip(row_at, row_top)]
            for gid, row_at, row_top in zip(profile.groups.tolist(), at.tolist(), top.tolist())}
