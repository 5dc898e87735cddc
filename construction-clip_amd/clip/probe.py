"""Linear probe: multinomial logistic regression on frozen, stored embeddings - the classifier CLIP itself is evaluated with
(Radford et al. 2021, section 3.2 and appendix A.3: L-BFGS, an L2 penalty swept on a validation split).

`CacheClassifier` is the tool at 1-16 shots; its model is the stored rows.  A probe is C * D parameters however many photos are
labelled.  One evaluation of the objective and its gradient is the kernel pair of csrc/embed_probe.hip: the rows stay in the
16-bit type they are stored in, the N x C logits never reach memory, there are no atomics, and two evaluations agree in every
bit - so two fresh `fit` calls return the same bits.  With x the rows, y the labels, r the per-row weights:
    objective(W, b) = scale * sum_n rw[n] * (logsumexp(z[n]) - z[n, y_n]) + l2 / 2 * |W|^2,   z = x (hi + lo)^T + b
where hi + lo is the kernel's 16-bit pair image of W (include/cclip_hip.h), rw = r / max r and scale = 1 / sum rw: the weighted
mean of the per-row cross-entropy, F.cross_entropy(weight=...)'s normalisation.  The bias is not regularised.  Rows with a
label outside [0, C) are ignored.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import List, Optional, Sequence, Tuple

import torch

from cclip_hip import ops
from .retrieval import HALF_TYPES, _device, normalize_rows


def probe_weights(labels: torch.Tensor, num_classes: int, class_weight=None) -> Tuple[Optional[torch.Tensor], float]:
    """Per-row weights in [0, 1] and the scale that go to the kernel, from integer labels [N] (any device; outside
    [0, num_classes): ignored) - (row_weight fp32 [N] on labels' device or None, scale).  With r[n] the raw weight of row n
    and L the number of live rows, the objective is sum r[n] loss[n] / sum r[n] (the weighted mean, as F.cross_entropy with
    `weight`); the kernel takes rw = r / max r and scale = max r / sum r = 1 / sum rw.
        None        r = 1: row_weight None, scale = 1 / L
        "balanced"  r[n] = L / (C * count[y_n])
        tensor [C]  r[n] = class_weight[y_n] (>= 0, finite)
    One host read (the scale is a host float argument of the kernel)."""
    C = int(num_classes)
    labels = labels.long()
    live = (labels >= 0) & (labels < C)
    y = labels.clamp(0, C - 1)
    counts = torch.bincount(y[live], minlength=C).double()
    L = live.sum().double()
    if class_weight is None:
        n_live = float(L)
        return None, (1.0 / n_live if n_live > 0 else 0.0)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"class_weight must be None, 'balanced' or a [C] tensor, got {class_weight!r}")
        cw = torch.where(counts > 0, L / (C * counts.clamp(min=1.0)), torch.zeros_like(counts))
    else:
        cw = torch.as_tensor(class_weight).detach().to(device=labels.device, dtype=torch.float64)
        if tuple(cw.shape) != (C,):
            raise ValueError(f"class_weight: expected [{C}] weights, got {tuple(cw.shape)}")
        if not bool(torch.isfinite(cw).all()) or bool((cw < 0).any()):
            raise ValueError("class_weight: weights must be finite and >= 0")
    r = torch.where(live, cw[y], torch.zeros_like(cw[y]))
    both = torch.stack([r.max() if r.numel() else L * 0, r.sum()]).tolist()           # the one host read
    rmax, rsum = both
    if rsum <= 0 or rmax <= 0:
        return torch.zeros(labels.shape, device=labels.device, dtype=torch.float32), 0.0
    return (r / rmax).float(), rmax / rsum


def best_row(table: Sequence[dict]) -> int:
    """The row of a sweep table with the best validation accuracy; equal accuracies go to the first (the smaller index)."""
    if not table:
        raise ValueError("sweep_l2: empty table")
    best = 0
    for i, row in enumerate(table):
        if row["val_accuracy"] > table[best]["val_accuracy"]:
            best = i
    return best


class ProbeLossFunction(torch.autograd.Function):
    """(W fp32 [C, D], bias fp32 [C]) -> the scalar objective, evaluated by ops.probe_forward + ops.probe_backward; its backward
    is the kernel's (dW, db), computed in the same call (an L-BFGS closure needs both every time).  The rows get no gradient:
    the towers are frozen."""

    @staticmethod
    def forward(ctx, W, bias, x16, labels_i32, row_weight, scale, l2):
        if ctx.needs_input_grad[2]:
            raise NotImplementedError("linear probe: no gradient for the rows - the towers are frozen, that path is not built")
        Wd, bd = W.detach().contiguous(), bias.detach().contiguous()
        lse, loss, _, _ = ops.probe_forward(x16.detach(), Wd, bd, labels_i32, row_weight)
        dW, db, obj = ops.probe_backward(x16.detach(), Wd, bd, labels_i32, lse, float(scale), float(l2), row_weight, loss=loss)
        ctx.save_for_backward(dW, db)
        return obj.reshape(())

    @staticmethod
    def backward(ctx, gout):
        dW, db = ctx.saved_tensors
        return gout * dW, gout * db, None, None, None, None, None


@dataclass
class ProbeFitResult:
    n_iter: int
    n_eval: int
    objective: float
    grad_norm: float            # max |d objective| over W and bias at the returned parameters: the quantity `tol` bounds
    converged: bool
    l2: float
    scale: float

    def as_dict(self) -> dict:
        return asdict(self)


class LinearProbe:
    """`LinearProbe(dim, num_classes=None, class_names=None)`: fp32 W [C, dim] and bias [C], zero until `fit`.  `dtype`: the
    16-bit type rows that are not already 16-bit device rows are normalised and rounded to (default bfloat16)."""

    def __init__(self, dim: int, num_classes: Optional[int] = None, class_names: Optional[Sequence[str]] = None,
                 dtype: Optional[torch.dtype] = None, device=None):
        self.class_names = None if class_names is None else list(class_names)
        if num_classes is None:
            if self.class_names is None:
                raise ValueError("LinearProbe: give num_classes or class_names")
            num_classes = len(self.class_names)
        self.dim, self.num_classes = int(dim), int(num_classes)
        if self.class_names is not None and len(self.class_names) != self.num_classes:
            raise ValueError(f"{len(self.class_names)} class_names for {self.num_classes} classes")
        if not 2 <= self.num_classes <= ops.PROBE_MAX_C:
            raise NotImplementedError(f"LinearProbe: {self.num_classes} classes; the kernel takes 2 .. {ops.PROBE_MAX_C}")
        if self.dim % 32 or not 32 <= self.dim <= ops.PROBE_MAX_D:
            raise NotImplementedError(f"LinearProbe: embedding width {self.dim}; the kernel needs a multiple of 32 in 32 .. {ops.PROBE_MAX_D}")
        self.dtype = torch.bfloat16 if dtype is None else dtype
        if self.dtype not in HALF_TYPES:
            raise ValueError(f"dtype must be torch.bfloat16 or torch.float16, got {self.dtype}")
        dev = torch.device(device) if device is not None else torch.device("cpu")
        self.W = torch.zeros(self.num_classes, self.dim, dtype=torch.float32, device=dev)
        self.bias = torch.zeros(self.num_classes, dtype=torch.float32, device=dev)
        self.l2 = 0.0
        self.result: Optional[ProbeFitResult] = None

    # ---- rows and labels ---------------------------------------------------------------------------------------------
    def _rows(self, features) -> torch.Tensor:
        """EmbeddingIndex -> its rows; 16-bit device rows are taken as they are; anything else is normalised and rounded."""
        if hasattr(features, "features") and hasattr(features, "metadata"):
            features = features.features
        if not isinstance(features, torch.Tensor):
            raise TypeError(f"LinearProbe: expected a tensor or an EmbeddingIndex, got {type(features)}")
        if features.dim() == 1:
            features = features[None]
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"expected [*, {self.dim}] features, got {tuple(features.shape)}")
        if not features.is_cuda:
            raise TypeError(f"LinearProbe: expected cuda features, got {features.device} (no CPU path)")
        if features.dtype in HALF_TYPES:
            return features.detach()
        return normalize_rows(features, self.dtype, features.device)

    @staticmethod
    def _labels(labels, N: int, dev) -> torch.Tensor:
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.numel() != N or labels.is_floating_point():
            raise ValueError(f"labels: expected {N} integers, got {tuple(labels.shape)} {labels.dtype}")
        return labels.to(dev).to(torch.int32).contiguous()

    def _to(self, dev):
        if self.W.device != dev:
            self.W, self.bias = self.W.to(dev), self.bias.to(dev)

    # ---- training ------------------------------------------------------------------------------------------------------
    def fit(self, features, labels, *, l2: float = 1e-3, max_iter: int = 100, tol: float = 1e-5, class_weight=None,
            init: str = "zeros", text_features: Optional[torch.Tensor] = None, logit_scale: Optional[float] = None,
            history_size: int = 10) -> ProbeFitResult:
        """Full-batch L-BFGS (torch.optim.LBFGS, strong-Wolfe line search, lr 1) on the device with the kernel as the closure.
        Stops when max |gradient| <= tol (torch's tolerance_grad), after max_iter iterations or when the line search no longer
        moves.  init: "zeros"; "zero_shot": W = logit_scale * text_features [C, dim] (CLIP's own classifier, default scale 100),
        bias 0; "warm": the current parameters.  One host read of the loss per evaluation on our side; torch's L-BFGS adds its
        own reads of the gradient's maximum and of the line search's products.  Returns and keeps a ProbeFitResult."""
        x16 = self._rows(features)
        dev = x16.device
        y = self._labels(labels, x16.shape[0], dev)
        l2, tol, max_iter = float(l2), float(tol), int(max_iter)
        if l2 < 0 or l2 != l2 or max_iter < 1:
            raise ValueError(f"fit: l2 = {l2}, max_iter = {max_iter}")
        rw, scale = probe_weights(y, self.num_classes, class_weight)
        if scale <= 0:
            raise ValueError("fit: no live rows (every label is outside [0, num_classes) or has weight 0)")
        self._to(dev)
        if init == "zeros":
            W0, b0 = torch.zeros_like(self.W), torch.zeros_like(self.bias)
        elif init == "zero_shot":
            if text_features is None or tuple(text_features.shape) != (self.num_classes, self.dim):
                raise ValueError(f"fit: init='zero_shot' needs text_features [{self.num_classes}, {self.dim}]")
            W0 = (text_features.detach().to(device=dev, dtype=torch.float32) * float(100.0 if logit_scale is None else logit_scale)).contiguous()
            b0 = torch.zeros_like(self.bias)
        elif init == "warm":
            W0, b0 = self.W.clone(), self.bias.clone()
        else:
            raise ValueError(f"fit: init must be 'zeros', 'zero_shot' or 'warm', got {init!r}")
        W, b = torch.nn.Parameter(W0), torch.nn.Parameter(b0)
        opt = torch.optim.LBFGS([W, b], lr=1.0, max_iter=max_iter, tolerance_grad=tol, tolerance_change=1e-9,
                                history_size=int(history_size), line_search_fn="strong_wolfe")
        n_eval = 0
        self.initial_objective: Optional[float] = None

        def closure():
            nonlocal n_eval
            opt.zero_grad(set_to_none=True)
            with torch.enable_grad():
                obj = ProbeLossFunction.apply(W, b, x16, y, rw, scale, l2)
                obj.backward()
            n_eval += 1
            if self.initial_objective is None:
                self.initial_objective = float(obj.detach())
            return obj

        opt.step(closure)
        n_iter = int(opt.state[opt._params[0]].get("n_iter", 0))
        with torch.no_grad():                                          # the objective and gradient AT the returned parameters
            Wd, bd = W.detach().contiguous(), b.detach().contiguous()
            lse, loss, _, _ = ops.probe_forward(x16, Wd, bd, y, rw)
            dW, db, obj = ops.probe_backward(x16, Wd, bd, y, lse, scale, l2, rw, loss=loss)
            back = torch.stack([obj[0], torch.maximum(dW.abs().max(), db.abs().max())]).tolist()
        n_eval += 1
        self.W, self.bias, self.l2 = Wd, bd, l2
        self.result = ProbeFitResult(n_iter=n_iter, n_eval=n_eval, objective=back[0], grad_norm=back[1],
                                     converged=bool(back[1] <= tol), l2=l2, scale=scale)
        self._last_weights = (rw, scale)
        return self.result

    def sweep_l2(self, train, train_labels, val, val_labels, l2s: Sequence[float], **fit_kw) -> List[dict]:
        """CLIP's protocol: one fit per l2 in the order given, each warm-started from the previous solution, scored on the
        validation rows; the probe keeps the parameters of the best validation accuracy (the first of equals).  Returns the
        table: one dict per l2 with l2, val_accuracy, objective, n_iter, n_eval, grad_norm and `best`."""
        l2s = [float(v) for v in l2s]
        if not l2s:
            raise ValueError("sweep_l2: no l2 values")
        x16, v16 = self._rows(train), self._rows(val)
        table, states = [], []
        for i, lam in enumerate(l2s):
            kw = dict(fit_kw)
            if i > 0:
                kw["init"] = "warm"
            res = self.fit(x16, train_labels, l2=lam, **kw)
            acc = self.score(v16, val_labels)
            table.append(dict(l2=lam, val_accuracy=acc, objective=res.objective, n_iter=res.n_iter, n_eval=res.n_eval,
                              grad_norm=res.grad_norm, best=False))
            states.append((self.W.clone(), self.bias.clone(), res))
        k = best_row(table)
        table[k]["best"] = True
        self.W, self.bias, self.result = states[k]
        self.l2 = l2s[k]
        return table

    # ---- inference -----------------------------------------------------------------------------------------------------
    def _forward(self, queries, logits: bool):
        x16 = self._rows(queries)
        self._to(x16.device)
        return ops.probe_forward(x16, self.W, self.bias, None, None, logits=logits)

    @torch.no_grad()
    def predict(self, queries) -> torch.Tensor:
        """int64 [Q] on the device: the argmax class of every query (ties to the lower class); no [Q, C] matrix."""
        return self._forward(queries, False)[2].long()

    @torch.no_grad()
    def predict_proba(self, queries) -> torch.Tensor:
        """fp32 [Q, C] probabilities: the one place the [Q, C] matrix is written, because it is the answer."""
        lse, _, _, z = self._forward(queries, True)
        return torch.exp(z - lse[:, None])

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
                raise ValueError("LinearProbe: pass image_features, or images together with the model that encodes them")
            image_features = model.encode_image(images.to(_device()))
        lse, _, pred, z = self._forward(image_features, True)
        probs, idx = torch.exp(z - lse[:, None]), pred.long()
        picked = idx.tolist()
        return probs, idx, [self.class_names[i] for i in picked] if self.class_names is not None else picked

    # ---- construction and persistence ----------------------------------------------------------------------------------
    @classmethod
    def from_index(cls, index, key: str, class_names: Optional[Sequence[str]] = None, **fit_kw) -> "LinearProbe":
        """Fit on an EmbeddingIndex whose metadata dicts carry the label under `key`; the index's rows are taken as they are."""
        from .fewshot import _labels_from_metadata
        labels, names = _labels_from_metadata(index.metadata, key, class_names)
        self = cls(index.dim, class_names=names, dtype=index.dtype)
        self.fit(index, labels, **fit_kw)
        return self

    @classmethod
    def from_pickle(cls, path: str, key: str, class_names: Optional[Sequence[str]] = None, dtype: Optional[torch.dtype] = None,
                    **fit_kw) -> "LinearProbe":
        from .retrieval import EmbeddingIndex
        return cls.from_index(EmbeddingIndex.from_pickle(path, dtype=dtype), key, class_names, **fit_kw)

    _STATE_KEYS = ("W", "bias", "class_names", "l2", "dtype")

    def state_dict(self) -> dict:
        """Plain tensors and lists (torch.save takes it): fp32 W and bias on the host, class names, l2, the 16-bit row type."""
        return dict(W=self.W.detach().cpu().clone(), bias=self.bias.detach().cpu().clone(),
                    class_names=None if self.class_names is None else list(self.class_names), l2=float(self.l2),
                    dtype=str(self.dtype).replace("torch.", ""))

    def load_state_dict(self, state: dict, device=None) -> "LinearProbe":
        missing = [k for k in self._STATE_KEYS if k not in state]
        extra = sorted(k for k in state if k not in self._STATE_KEYS)
        if missing or extra:
            raise KeyError(f"load_state_dict: missing {missing}, unexpected {extra}")
        W, b = state["W"], state["bias"]
        if not isinstance(W, torch.Tensor) or W.dim() != 2 or W.dtype != torch.float32 or tuple(b.shape) != (W.shape[0],) \
                or b.dtype != torch.float32:
            raise ValueError("load_state_dict: W must be fp32 [C, D] and bias fp32 [C]")
        dev = torch.device(device) if device is not None else (self.W.device if hasattr(self, "W") else torch.device("cpu"))
        self.__init__(W.shape[1], W.shape[0], state["class_names"], dtype=getattr(torch, state["dtype"]), device=dev)
        self.W, self.bias, self.l2 = W.detach().to(dev).contiguous().clone(), b.detach().to(dev).contiguous().clone(), float(state["l2"])
        return self

    @classmethod
    def from_state_dict(cls, state: dict, device=None) -> "LinearProbe":
        return cls.__new__(cls).load_state_dict(state, device)
