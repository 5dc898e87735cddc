"""Gaussian class models on stored embeddings: everything here rests on SECOND moments of the rows, which one kernel collects
(csrc/embed_moments.hip: count, class sums and X^T X from the 16-bit rows as stored) and one kernel applies
(csrc/gauss_scores.hip: a fp32 transform of every query, squared distances to the class centres, scores).

* `GaussianClassifier`: Gaussian discriminant analysis with ONE shared covariance - the training-free few-shot baseline of Wang
  et al. (ICLR 2024), between `CacheClassifier` (no training) and `LinearProbe` (L-BFGS).  With the whitening T of the shrunk
  covariance, z = T (x - mean) and m_c = T (mean_c - mean):
      score[q, c] = -1/2 |z_q - m_c|^2 + log prior_c
  which differs from the paper's linear form W x + b by the class-independent -1/2 x^T P x.  The distance is taken as written,
  never expanded: the covariance is ill-conditioned whenever N < D, and the embedding cone adds a dominant mean direction.
  The fit is additive: `add` adds three sums and re-solves nothing but a D x D eigenproblem.
* `mahalanobis`: the distance to the nearest class Gaussian (Lee et al. 2018) scores a NEW row against the labelled set;
  the distance to a row's own class ranks likely label errors (`suspects`).
* `pca`: the same Gram matrix without labels.

The D x D algebra (scatter, eigh) runs in float64 torch on the device: that is where the cone's cancellation lives, and D x D is
small.  T, the centres and the offsets are cast to fp32 once and kept.  There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import torch

from cclip_hip import ops
from .retrieval import HALF_TYPES, _device, normalize_rows


def _rows16(who: str, features, dim: Optional[int], dtype: torch.dtype) -> torch.Tensor:
    """LinearProbe._rows: an EmbeddingIndex -> its rows; 16-bit device rows as they are; anything else normalised and rounded."""
    if hasattr(features, "features") and hasattr(features, "metadata"):
        features = features.features
    if not isinstance(features, torch.Tensor):
        raise TypeError(f"{who}: expected a tensor or an EmbeddingIndex, got {type(features)}")
    if features.dim() == 1:
        features = features[None]
    if features.dim() != 2 or (dim is not None and features.shape[1] != dim):
        raise ValueError(f"{who}: expected [*, {dim if dim is not None else 'D'}] features, got {tuple(features.shape)}")
    if not features.is_cuda:
        raise TypeError(f"{who}: expected cuda features, got {features.device} (no CPU path)")
    if features.dtype in HALF_TYPES:
        return features.detach()
    return normalize_rows(features, dtype, features.device)


def _labels32(labels, N: int, dev) -> torch.Tensor:
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.numel() != N or labels.is_floating_point():
        raise ValueError(f"labels: expected {N} integers, got {tuple(labels.shape)} {labels.dtype}")
    return labels.to(dev).to(torch.int32).contiguous()


@dataclass
class ClassMoments:
    """The three sums of a labelled set, float64 on the device: count [C], sum [C, D], gram [D, D].  Adding two of them is the
    moments of the union of the two sets."""
    count: torch.Tensor
    sum: torch.Tensor
    gram: torch.Tensor

    @property
    def n(self) -> torch.Tensor:
        return self.count.sum()

    @property
    def mean(self) -> torch.Tensor:
        """[C, D]; a class without rows has mean 0"""
        return self.sum / self.count.clamp(min=1.0)[:, None]

    @property
    def total_mean(self) -> torch.Tensor:
        return self.sum.sum(0) / self.n.clamp(min=1.0)

    @property
    def scatter(self) -> torch.Tensor:
        """The pooled within-class scatter gram - sum_c count_c mean_c mean_c^T; the subtraction is in float64."""
        mean = self.mean
        s = self.gram - (mean * self.count[:, None]).T @ mean
        return (s + s.T) * 0.5

    def __add__(self, other: "ClassMoments") -> "ClassMoments":
        if not isinstance(other, ClassMoments):
            return NotImplemented
        if self.sum.shape != other.sum.shape:
            raise ValueError(f"ClassMoments: {tuple(self.sum.shape)} + {tuple(other.sum.shape)}")
        dev = self.gram.device
        return ClassMoments(self.count + other.count.to(dev), self.sum + other.sum.to(dev), self.gram + other.gram.to(dev))


@torch.no_grad()
def class_moments(features, labels=None, num_classes: Optional[int] = None, *, dtype: torch.dtype = torch.bfloat16) -> ClassMoments:
    """Count, class sums and Gram matrix of the rows (an EmbeddingIndex, 16-bit device rows as stored, or float rows, which are
    normalised and rounded to `dtype`) by integer labels [N]; a label outside [0, num_classes) drops the row.  Without labels
    every row is class 0.  The sums are the kernel's fp32 (exact products, fixed-order sums), returned as float64."""
    x = _rows16("class_moments", features, None, dtype)
    if labels is None:
        y, C = None, 1 if num_classes is None else int(num_classes)
        if C != 1:
            raise ValueError("class_moments: without labels there is one class")
    else:
        y = _labels32(labels, x.shape[0], x.device)
        C = int(num_classes) if num_classes is not None else int(y.max()) + 1          # (one host read without num_classes)
    count, csum, gram = ops.class_moments(x, y, C)
    return ClassMoments(count.double(), csum.double(), gram.double())


@dataclass
class MahalanobisScores:
    dmin: torch.Tensor            # fp32 [Q]: squared Mahalanobis distance to the nearest class mean
    nearest: torch.Tensor         # int64 [Q]: that class
    pred: torch.Tensor            # int64 [Q]: the classifier's class (differs from nearest only through the priors)
    log_density: torch.Tensor     # fp32 [Q]: log of the fitted mixture density at the row


class GaussianClassifier:
    """`GaussianClassifier(features, labels, *, num_classes=None, class_names=None, shrinkage="auto", priors="empirical",
    text_features=None, logit_scale=100.0, alpha=1.0)`.

    Sigma_hat = scatter / (N - C): the pooled within-class covariance (divided by N instead when N <= C, where N - C is no
    degree of freedom at all).  shrinkage="auto" is the estimator of Wang et al.: precision = D ((N - 1) Sigma_hat +
    trace(Sigma_hat) I)^-1; a float lam in [0, 1] gives Sigma = (1 - lam) Sigma_hat + lam trace(Sigma_hat) / D I, and lam = 0
    with a singular Sigma_hat is a ValueError.  priors: "empirical" (count_c / N) or "uniform".  With text_features [C, D] the
    logits are logit_scale <f, t_c> + alpha * score, as CacheClassifier adds its term."""

    def __init__(self, features, labels, *, num_classes: Optional[int] = None, class_names: Optional[Sequence[str]] = None,
                 shrinkage: Union[str, float] = "auto", priors: str = "empirical", text_features: Optional[torch.Tensor] = None,
                 logit_scale: float = 100.0, alpha: float = 1.0, dtype: Optional[torch.dtype] = None):
        self.dtype = torch.bfloat16 if dtype is None else dtype
        if self.dtype not in HALF_TYPES:
            raise ValueError(f"dtype must be torch.bfloat16 or torch.float16, got {self.dtype}")
        x = _rows16("GaussianClassifier", features, None, self.dtype)
        self.dtype = x.dtype                          # 16-bit rows are taken as stored: queries are rounded to the same type
        y = _labels32(labels, x.shape[0], x.device)
        self.class_names = None if class_names is None else list(class_names)
        if num_classes is None:
            num_classes = len(self.class_names) if self.class_names is not None else \
                (text_features.shape[0] if text_features is not None else int(y.max()) + 1)
        moments = class_moments(x, y, int(num_classes))
        self._setup(moments, self.class_names, shrinkage, priors, text_features, logit_scale, alpha)

    def _setup(self, moments: ClassMoments, class_names, shrinkage, priors, text_features, logit_scale, alpha):
        self.moments = moments
        self.num_classes, self.dim = int(moments.sum.shape[0]), int(moments.sum.shape[1])
        self.class_names = None if class_names is None else list(class_names)
        if self.class_names is not None and len(self.class_names) != self.num_classes:
            raise ValueError(f"{len(self.class_names)} class_names for {self.num_classes} classes")
        if not 1 <= self.num_classes <= ops.GAUSS_MAX_C:
            raise NotImplementedError(f"GaussianClassifier: {self.num_classes} classes; the kernels take 1 .. {ops.GAUSS_MAX_C}")
        if isinstance(shrinkage, str):
            if shrinkage != "auto":
                raise ValueError(f"shrinkage must be 'auto' or a float in [0, 1], got {shrinkage!r}")
        else:
            shrinkage = float(shrinkage)
            if not 0.0 <= shrinkage <= 1.0:
                raise ValueError(f"shrinkage must be 'auto' or a float in [0, 1], got {shrinkage}")
        if priors not in ("empirical", "uniform"):
            raise ValueError(f"priors must be 'empirical' or 'uniform', got {priors!r}")
        self.shrinkage, self.priors = shrinkage, priors
        dev = moments.gram.device
        self.text_features = None
        if text_features is not None:
            if tuple(text_features.shape) != (self.num_classes, self.dim):
                raise ValueError(f"text_features: expected [{self.num_classes}, {self.dim}], got {tuple(text_features.shape)}")
            self.text_features = text_features.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.logit_scale, self.alpha = float(logit_scale), float(alpha)
        self._log_scale = torch.full((1,), math.log(self.logit_scale), device=dev, dtype=torch.float32)
        self._rebuild()

    # ---- the D x D algebra, float64 ------------------------------------------------------------------------------------
    def covariance(self) -> torch.Tensor:
        """The shrunk covariance the scores use, float64 [D, D]."""
        m = self.moments
        N, C, D = float(m.n), self.num_classes, self.dim
        sigma_hat = m.scatter / (N - C if N > C else max(N, 1.0))
        tr = torch.trace(sigma_hat)
        eye = torch.eye(D, device=sigma_hat.device, dtype=torch.float64)
        if self.shrinkage == "auto":
            return ((N - 1.0) * sigma_hat + tr * eye) / D
        lam = float(self.shrinkage)
        return (1.0 - lam) * sigma_hat + lam * tr / D * eye

    def _rebuild(self) -> None:
        m = self.moments
        N, C, D = float(m.n), self.num_classes, self.dim                                # (host read: the fit is not a hot path)
        if N < 1:
            raise ValueError("GaussianClassifier: no live rows (every label is outside [0, num_classes))")
        sigma = self.covariance()
        evals, evecs = torch.linalg.eigh(sigma)
        top = float(evals[-1])
        if not top > 0.0 or float(evals[0]) <= top * D * 2.3e-16:
            raise ValueError(f"GaussianClassifier: the covariance is singular at N = {int(N)}, C = {C}, D = {D}"
                             f" with shrinkage = {self.shrinkage!r}; use 'auto' or a shrinkage > 0")
        T = evecs.T / evals.sqrt()[:, None]                                              # Lambda^(-1/2) U^T
        mean = m.total_mean
        self.log_det = float(evals.log().sum())
        self.T = T.float().contiguous()
        self.t0 = (T @ mean).float().contiguous()
        self.centres = ((m.mean - mean) @ T.T).float().contiguous()                      # T (mean_c - mean)
        prior = m.count / m.n if self.priors == "empirical" else torch.full_like(m.count, 1.0 / C)
        self.offset = prior.log().float().contiguous()                                   # a class without rows: -inf, never chosen

    # ---- inference -------------------------------------------------------------------------------------------------------
    def _rows(self, features) -> torch.Tensor:
        return _rows16("GaussianClassifier", features, self.dim, self.dtype)

    def _scores(self, queries, want_d2: bool = False):
        x = self._rows(queries)
        return x, ops.gauss_scores(x, self.T, t0=self.t0, centres=self.centres, offset=self.offset, want_d2=want_d2)

    @torch.no_grad()
    def logits(self, queries) -> torch.Tensor:
        """score[q, c] fp32 [Q, C]; with text_features, logit_scale <f, t_c> + alpha * score."""
        x, (_, _, _, _, d2, _) = self._scores(queries, True)
        score = -0.5 * d2 + self.offset
        if self.text_features is None:
            return score
        from .model import normalized_logits
        return normalized_logits(x.float().contiguous(), self.text_features, self._log_scale)[0] + self.alpha * score

    @torch.no_grad()
    def predict(self, queries) -> torch.Tensor:
        """int64 [Q]: the argmax class (ties to the lower class); without text_features no [Q, C] matrix is written."""
        if self.text_features is None:
            return self._scores(queries)[1][0].long()
        return self.logits(queries).argmax(1)

    @torch.no_grad()
    def predict_proba(self, queries) -> torch.Tensor:
        z = self.logits(queries)
        return torch.softmax(z, dim=1)

    @torch.no_grad()
    def score(self, queries, labels) -> float:
        """Top-1 accuracy over the rows whose label lies in [0, C); one host read."""
        pred = self.predict(queries)
        y = torch.as_tensor(labels).to(pred.device).long()
        if tuple(y.shape) != tuple(pred.shape):
            raise ValueError(f"score: expected {pred.numel()} labels, got {tuple(y.shape)}")
        live = (y >= 0) & (y < self.num_classes)
        hit, n = torch.stack([((pred == y) & live).sum(), live.sum()]).tolist()
        return hit / n if n else float("nan")

    @torch.no_grad()
    def __call__(self, images: torch.Tensor = None, image_features: torch.Tensor = None, model=None):
        """Returns (probabilities [Q, C], indices [Q], labels list) - CacheClassifier.__call__'s conventions."""
        if image_features is None:
            if model is None or images is None:
                raise ValueError("GaussianClassifier: pass image_features, or images together with the model that encodes them")
            image_features = model.encode_image(images.to(_device()))
        probs = self.predict_proba(image_features)
        idx = probs.argmax(1)
        picked = idx.tolist()
        return probs, idx, [self.class_names[i] for i in picked] if self.class_names is not None else picked

    @torch.no_grad()
    def mahalanobis(self, queries) -> MahalanobisScores:
        """Squared Mahalanobis distance of every query to the nearest class mean under the shared covariance, that class, the
        classifier's class, and the log density of the fitted mixture: lse - (log det Sigma / 2 + D / 2 log 2 pi)."""
        _, (pred, lse, nearest, dmin, _, _) = self._scores(queries)
        const = 0.5 * self.log_det + 0.5 * self.dim * math.log(2.0 * math.pi)
        return MahalanobisScores(dmin, nearest.long(), pred.long(), lse - const)

    @torch.no_grad()
    def calibrate(self, features, quantile: float = 0.95) -> float:
        """The empirical `quantile` of dmin over rows that were NOT used to fit: the threshold of `outliers`.  Rows of the fit
        bias it low: each pulled its own class mean and the covariance towards itself, so its distance is smaller than a fresh
        row's from the same distribution - by a factor near (N - C - D) / N for N > D, and without bound for N < D, where the
        fitted rows lie inside the span the covariance was estimated on.  One host read."""
        if not 0.0 < float(quantile) <= 1.0:
            raise ValueError(f"calibrate: quantile = {quantile} outside (0, 1]")
        d = self.mahalanobis(features).dmin
        return float(torch.quantile(d.double(), float(quantile)))

    @torch.no_grad()
    def outliers(self, queries, threshold: float) -> torch.Tensor:
        """bool [Q]: dmin above the threshold (a NaN row is an outlier)."""
        d = self.mahalanobis(queries).dmin
        return ~(d <= float(threshold))

    @torch.no_grad()
    def suspects(self, features, labels, top: Optional[int] = None):
        """Likely label errors: (rows int64 [k], margin fp32 [k]) ranked by d2 to the row's OWN class minus dmin, largest first;
        0 for a row whose own class is its nearest.  Rows with a label outside [0, C) are left out."""
        x, (_, _, _, dmin, d2, _) = self._scores(features, True)
        y = _labels32(labels, x.shape[0], x.device).long()
        live = (y >= 0) & (y < self.num_classes)
        own = d2.gather(1, y.clamp(0, self.num_classes - 1)[:, None])[:, 0]
        margin = torch.where(live, own - dmin, torch.full_like(own, -1.0))
        order = torch.argsort(margin, descending=True, stable=True)
        order = order[: int(live.sum())]
        if top is not None:
            order = order[: int(top)]
        return order, margin[order]

    @torch.no_grad()
    def add(self, features, labels) -> "GaussianClassifier":
        """Adds labelled rows: three sums are added and T rebuilt.  Equal to a fresh fit on the union to float64 rounding, NOT
        bitwise: the kernel's fp32 sums of the two sets are added in float64, a fresh fit sums all rows in fp32 in one order."""
        x = self._rows(features)
        self.moments = self.moments + class_moments(x, _labels32(labels, x.shape[0], x.device), self.num_classes)
        self._rebuild()
        return self

    # ---- construction and persistence ----------------------------------------------------------------------------------
    @classmethod
    def from_index(cls, index, key: str, class_names: Optional[Sequence[str]] = None, **kw) -> "GaussianClassifier":
        """Fit on an EmbeddingIndex whose metadata dicts carry the label under `key`; the index's rows are taken as they are."""
        from .fewshot import _labels_from_metadata
        labels, names = _labels_from_metadata(index.metadata, key, class_names)
        return cls(index, labels, class_names=names, dtype=index.dtype, **kw)

    @classmethod
    def from_pickle(cls, path: str, key: str, class_names: Optional[Sequence[str]] = None, dtype: Optional[torch.dtype] = None,
                    **kw) -> "GaussianClassifier":
        from .retrieval import EmbeddingIndex
        return cls.from_index(EmbeddingIndex.from_pickle(path, dtype=dtype), key, class_names, **kw)

    _STATE_KEYS = ("count", "sum", "gram", "class_names", "shrinkage", "priors", "text_features", "logit_scale", "alpha", "dtype")

    def state_dict(self) -> dict:
        """The three float64 sums on the host and the settings; T, the centres and the offsets are rebuilt from them (the same
        float64 algebra on the same numbers: the same fp32 bits on the same device and library)."""
        m = self.moments
        return dict(count=m.count.cpu().clone(), sum=m.sum.cpu().clone(), gram=m.gram.cpu().clone(),
                    class_names=None if self.class_names is None else list(self.class_names), shrinkage=self.shrinkage,
                    priors=self.priors, text_features=None if self.text_features is None else self.text_features.cpu().clone(),
                    logit_scale=self.logit_scale, alpha=self.alpha, dtype=str(self.dtype).replace("torch.", ""))

    def load_state_dict(self, state: dict, device=None) -> "GaussianClassifier":
        missing = [k for k in self._STATE_KEYS if k not in state]
        extra = sorted(k for k in state if k not in self._STATE_KEYS)
        if missing or extra:
            raise KeyError(f"load_state_dict: missing {missing}, unexpected {extra}")
        dev = torch.device(device) if device is not None else _device()
        cnt, s, g = (state[k].to(device=dev, dtype=torch.float64) for k in ("count", "sum", "gram"))
        if s.dim() != 2 or tuple(cnt.shape) != (s.shape[0],) or tuple(g.shape) != (s.shape[1], s.shape[1]):
            raise ValueError("load_state_dict: count [C], sum [C, D] and gram [D, D] do not fit each other")
        self.dtype = getattr(torch, state["dtype"])
        text = state["text_features"]
        self._setup(ClassMoments(cnt, s, g), state["class_names"], state["shrinkage"], state["priors"],
                    None if text is None else text.to(dev), state["logit_scale"], state["alpha"])
        return self

    @classmethod
    def from_state_dict(cls, state: dict, device=None) -> "GaussianClassifier":
        return cls.__new__(cls).load_state_dict(state, device)


@dataclass
class PCAResult:
    mean: torch.Tensor                        # float64 [D] (zeros without centring)
    components: torch.Tensor                  # float64 [k, D], rows of unit length, descending variance
    explained_variance: torch.Tensor          # float64 [k]
    explained_variance_ratio: torch.Tensor    # float64 [k]
    whiten: bool
    dtype: torch.dtype
    T: torch.Tensor                           # fp32 [k, D]: the kernel's transform (components, scaled when whitening)
    t0: torch.Tensor                          # fp32 [k]: T mean

    @torch.no_grad()
    def transform(self, rows) -> torch.Tensor:
        """fp32 [n, k]: the rows' coordinates (ops.gauss_scores without centres)."""
        x = _rows16("PCAResult.transform", rows, self.components.shape[1], self.dtype)
        return ops.gauss_scores(x, self.T, t0=self.t0)[5]


@torch.no_grad()
def pca(features, k: int, *, center: bool = True, whiten: bool = False, dtype: torch.dtype = torch.bfloat16) -> PCAResult:
    """Principal components of the rows from their Gram matrix: covariance (gram - N mean mean^T) / (N - 1) in float64 (the mean
    term dropped with center=False), a float64 eigh, the k leading components in descending order, each with the sign that
    makes its largest-magnitude entry positive.  whiten=True scales the coordinates to unit variance."""
    x = _rows16("pca", features, None, dtype)
    N, D = x.shape
    k = int(k)
    if not 1 <= k <= D:
        raise ValueError(f"pca: k = {k} outside 1 .. {D}")
    if N < 2:
        raise ValueError("pca: needs at least two rows")
    m = class_moments(x)
    mean = m.total_mean if center else torch.zeros_like(m.total_mean)
    cov = (m.gram - N * torch.outer(mean, mean)) / (N - 1)
    cov = (cov + cov.T) * 0.5
    evals, evecs = torch.linalg.eigh(cov)
    var = evals.flip(0)[:k].clamp(min=0.0)
    comp = evecs.flip(1).T[:k].contiguous()
    big = comp.abs().argmax(1)
    sign = torch.sign(comp.gather(1, big[:, None]))
    comp = comp * torch.where(sign == 0, torch.ones_like(sign), sign)
    T = comp / var.sqrt().clamp(min=1e-150)[:, None] if whiten else comp
    return PCAResult(mean, comp, var, var / torch.trace(cov), bool(whiten), x.dtype, T.float().contiguous(),
                     (T @ mean).float().contiguous())
