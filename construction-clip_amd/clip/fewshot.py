"""Few-shot classification from stored, labelled embeddings with no training: the cache model of Tip-Adapter
(Zhang et al., ECCV 2022).

The reference turns CLIP into a classifier for its 306 labelled photos by fine-tuning every parameter (CLIP/train.py:150-207).
`CacheClassifier` is the step before that: with F the stored L2-normalised image features, f a query's and t_c the class
prompts',
    A[q, c]      = sum over the stored rows n of class c of exp(beta * (<f_q, F_n> - 1))
    logits[q, c] = logit_scale * <f_q, t_c> + alpha * A[q, c]
The stored rows live on the device in the 16-bit type the towers compute in, grouped by class (ops.cache_layout), and A comes
from the fused kernel pair of csrc/embed_cache.hip: the Q x N similarity matrix is never formed, and a query's row does not
depend on the batch it is scored in.  `alpha` and `beta` are tuned without training, on validation data or - the case that
matters with a few hundred photos - on the leave-one-out logits of the stored set itself.

`fit()` is the method's second half, Tip-Adapter-F: the stored keys become an fp32 parameter and are trained on the cross-entropy
of those logits with the towers frozen (CacheAffinityFunction: the gradient of A with respect to the keys comes from
csrc/embed_cache_bwd.hip, again without the Q x N matrix and with the leave-one-out mask).  `state_dict()` /
`load_state_dict()` keep a trained cache.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from cclip_hip import ops
from .model import normalized_logits
from .retrieval import HALF_TYPES, _device, normalize_rows


def confusion_matrix(pred: torch.Tensor, labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    """int64 [C, C] on pred's device, rows = true class, columns = predicted class; no host read."""
    C = int(num_classes)
    flat = labels.to(pred.device).long() * C + pred.long()
    return torch.bincount(flat, minlength=C * C).reshape(C, C)


def _labels_from_metadata(metadata: Sequence, key: str, class_names: Optional[Sequence[str]]) -> Tuple[torch.Tensor, List[str]]:
    """Integer labels from the metadata dicts' `key` entries.  Class order: `class_names` if given (every value must be in it),
    else order of first appearance."""
    if metadata is None:
        raise ValueError(f"the index carries no metadata to read {key!r} from")
    values = []
    for i, m in enumerate(metadata):
        if not isinstance(m, dict) or key not in m:
            raise ValueError(f"metadata entry {i} has no {key!r}")
        values.append(m[key])
    names = list(class_names) if class_names is not None else list(dict.fromkeys(values))
    if len(set(names)) != len(names):
        raise ValueError(f"class_names repeats a name: {names}")
    where = {n: i for i, n in enumerate(names)}
    unknown = [v for v in dict.fromkeys(values) if v not in where]
    if unknown:
        raise ValueError(f"{key!r} values {unknown} are not among class_names {names}")
    return torch.tensor([where[v] for v in values], dtype=torch.long), names


class CacheAffinityFunction(torch.autograd.Function):
    """A = ops.cache_affinity(q16, round16(laid32), ..) with the gradient of the laid-out keys from ops.cache_affinity_backward
    (csrc/embed_cache_bwd.hip).  `laid32` is the fp32 [Np, E] laid-out key matrix (padding rows NaN); its rounding to the
    16-bit type of `q16` is passed straight through.  The queries get no gradient: the towers are frozen."""

    @staticmethod
    def forward(ctx, laid32, q16, class_off, class_len, beta, exclude):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("cache affinity: no gradient for the queries - the towers are frozen, that path is not built")
        laid16 = laid32.detach().to(q16.dtype)
        ctx.save_for_backward(laid16, q16.detach(), exclude)
        ctx.segments = (class_off, class_len, float(beta))
        return ops.cache_affinity(q16.detach(), laid16, class_off, class_len, float(beta), exclude=exclude)

    @staticmethod
    def backward(ctx, dA):
        laid16, q16, exclude = ctx.saved_tensors
        class_off, class_len, beta = ctx.segments
        dG = ops.cache_affinity_backward(q16, laid16, class_off, class_len, beta, dA.float().contiguous(), exclude=exclude)
        return dG, None, None, None, None, None


def fit_batches(M: int, batch_size: Optional[int], epochs: int, seed: int):
    """The batches of CacheClassifier.fit: per epoch a seeded permutation of the M training rows cut into batches of
    `batch_size` (the last may be shorter); one batch of all rows in their own order when batch_size is None.  Yields
    (epoch, host int64 index vector)."""
    gen = torch.Generator().manual_seed(int(seed))
    for ep in range(epochs):
        if batch_size is None or batch_size >= M:
            yield ep, torch.arange(M)
        else:
            perm = torch.randperm(M, generator=gen)
            for s in range(0, M, batch_size):
                yield ep, perm[s:s + batch_size]


class CacheClassifier:
    """Stored features [N, E] (any float dtype, anywhere) with integer labels [N] -> a classifier of new features.
    `text_features [C, E]` adds the zero-shot term logit_scale * <f, t_c>; without it the logits are the cache term alone.
    `per_class="mean"` divides A[:, c] by the class's count (empty classes stay 0).  `dtype`: the 16-bit type of the stored
    rows and of the queries (default bfloat16)."""

    def __init__(self, features: torch.Tensor, labels, *, num_classes: Optional[int] = None,
                 class_names: Optional[Sequence[str]] = None, text_features: Optional[torch.Tensor] = None,
                 logit_scale: float = 100.0, alpha: float = 1.0, beta: float = 5.5, per_class: str = "sum",
                 dtype: Optional[torch.dtype] = None):
        self.dtype = torch.bfloat16 if dtype is None else dtype
        self._init(normalize_rows(features, self.dtype), labels, num_classes, class_names, text_features, logit_scale, alpha,
                   beta, per_class)

    def _init(self, rows, labels, num_classes, class_names, text_features, logit_scale, alpha, beta, per_class):
        if self.dtype not in HALF_TYPES or rows.dtype != self.dtype:
            raise ValueError(f"CacheClassifier: stored rows must be {self.dtype}, got {rows.dtype}")
        if per_class not in ("sum", "mean"):
            raise ValueError(f"per_class must be 'sum' or 'mean', got {per_class!r}")
        E = rows.shape[1]
        if E % 32 or not 32 <= E <= ops.CACHE_AFFINITY_MAX_D:
            raise NotImplementedError(f"CacheClassifier: embedding width {E}; the affinity kernel needs a multiple of 32 in "
                                      f"32 .. {ops.CACHE_AFFINITY_MAX_D}")
        labels = torch.as_tensor(labels).detach().cpu()
        if labels.dim() != 1 or labels.numel() != rows.shape[0] or labels.is_floating_point():
            raise ValueError(f"labels: expected {rows.shape[0]} integers, got {tuple(labels.shape)} {labels.dtype}")
        self.class_names = None if class_names is None else list(class_names)
        if num_classes is None:
            num_classes = len(self.class_names) if self.class_names is not None else \
                (text_features.shape[0] if text_features is not None else int(labels.max()) + 1 if labels.numel() else 0)
        self.num_classes = int(num_classes)
        if self.class_names is not None and len(self.class_names) != self.num_classes:
            raise ValueError(f"{len(self.class_names)} class_names for {self.num_classes} classes")
        if not 1 <= self.num_classes <= ops.CACHE_AFFINITY_MAX_C:
            raise NotImplementedError(f"CacheClassifier: {self.num_classes} classes; the affinity kernel takes 1 .. "
                                      f"{ops.CACHE_AFFINITY_MAX_C}")
        self.text_features = None
        if text_features is not None:
            if tuple(text_features.shape) != (self.num_classes, E):
                raise ValueError(f"text_features: expected [{self.num_classes}, {E}], got {tuple(text_features.shape)}")
            self.text_features = text_features.detach().to(device=rows.device, dtype=torch.float32).contiguous()
        self.logit_scale, self.alpha, self.beta, self.per_class = float(logit_scale), float(alpha), float(beta), per_class
        self._log_scale = torch.full((1,), math.log(self.logit_scale), device=rows.device, dtype=torch.float32)
        self._set_rows(rows, labels.long())

    def _set_rows(self, rows: torch.Tensor, labels: torch.Tensor):
        """Lay the normalised rows (original order) out by class.  Padding rows are NaN on purpose: a masking bug shows."""
        gather, self.class_off, self.class_len = ops.cache_layout(labels, self.num_classes)
        dev = rows.device
        self.features, self.labels = rows, labels                       # original order; labels on the host
        g = gather.to(dev)
        laid = torch.full((gather.numel(), rows.shape[1]), float("nan"), device=dev, dtype=self.dtype)
        live = g >= 0
        laid[live] = rows[g[live]]
        self._laid = laid
        pos = torch.empty(rows.shape[0], dtype=torch.long)
        keep = gather >= 0
        pos[gather[keep]] = torch.arange(gather.numel())[keep]
        self._pos = pos.to(dev)                                         # original row -> laid-out row
        self._labels_dev = labels.to(dev)
        self._count = self.class_len.to(dev).float().clamp(min=1.0)

    def __len__(self) -> int:
        return self.features.shape[0]

    @property
    def dim(self) -> int:
        return self.features.shape[1]

    @classmethod
    def from_index(cls, index, key: str, class_names: Optional[Sequence[str]] = None, **kw) -> "CacheClassifier":
        """From an EmbeddingIndex whose metadata dicts carry the label under `key` (for example "violation_type").  The
        index's normalised rows are taken as they are."""
        labels, names = _labels_from_metadata(index.metadata, key, class_names)
        self = cls.__new__(cls)
        self.dtype = index.dtype
        self._init(index.features.clone(), labels, len(names), names, kw.pop("text_features", None), kw.pop("logit_scale", 100.0),
                   kw.pop("alpha", 1.0), kw.pop("beta", 5.5), kw.pop("per_class", "sum"))
        if kw:
            raise TypeError(f"from_index: unexpected arguments {sorted(kw)}")
        return self

    @classmethod
    def from_pickle(cls, path: str, key: str, class_names: Optional[Sequence[str]] = None, dtype: Optional[torch.dtype] = None,
                    **kw) -> "CacheClassifier":
        """From the embedding file of clip_caption.data.save_embeddings / scripts/extract_embeddings.py."""
        from .retrieval import EmbeddingIndex
        return cls.from_index(EmbeddingIndex.from_pickle(path, dtype=dtype), key, class_names, **kw)

    def add(self, features: torch.Tensor, labels) -> "CacheClassifier":
        """Append labelled rows and rebuild the layout.  Rows are normalised one by one, so the result equals a bulk build's."""
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError(f"add: expected [*, {self.dim}] features, got {tuple(features.shape)}")
        labels = torch.as_tensor(labels).detach().cpu()
        if labels.dim() != 1 or labels.numel() != features.shape[0] or labels.is_floating_point():
            raise ValueError(f"add: expected {features.shape[0]} integer labels, got {tuple(labels.shape)} {labels.dtype}")
        rows = normalize_rows(features, self.dtype, self.features.device)
        self._set_rows(torch.cat([self.features, rows]), torch.cat([self.labels, labels.long()]))
        return self

    # ---- the 16-bit query rows and the mapping of `exclude` -------------------------------------------------------
    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        if queries.dim() == 1:
            queries = queries[None]
        if queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"expected [*, {self.dim}] queries, got {tuple(queries.shape)}")
        return normalize_rows(queries, self.dtype, self.features.device)

    def _exclude(self, exclude, Q: int) -> Optional[torch.Tensor]:
        """ORIGINAL row numbers (or -1) -> int32 laid-out rows on the device; a host-side range check only for host input"""
        if exclude is None:
            return None
        ex = torch.as_tensor(exclude)
        if tuple(ex.shape) != (Q,) or ex.is_floating_point():
            raise ValueError(f"exclude: expected {Q} integers, got {tuple(ex.shape)} {ex.dtype}")
        if not ex.is_cuda and ex.numel() and (int(ex.min()) < -1 or int(ex.max()) >= len(self)):
            raise ValueError(f"exclude: rows must lie in -1 .. {len(self) - 1}")
        ex = ex.to(self._pos.device).long()
        return torch.where(ex >= 0, self._pos[ex.clamp(0, len(self) - 1)], ex.new_full((), -1)).to(torch.int32)

    def _affinity16(self, q16: torch.Tensor, beta: Optional[float], exclude_laid: Optional[torch.Tensor]) -> torch.Tensor:
        if len(self) == 0:
            raise ValueError("CacheClassifier: no stored rows")
        A = ops.cache_affinity(q16, self._laid, self.class_off, self.class_len, self.beta if beta is None else float(beta),
                               exclude=exclude_laid)
        return A / self._count if self.per_class == "mean" else A

    def _zero_shot16(self, q16: torch.Tensor) -> Optional[torch.Tensor]:
        if self.text_features is None:
            return None
        return normalized_logits(q16.float().contiguous(), self.text_features, self._log_scale)[0]

    def _logits16(self, q16, alpha, beta, exclude_laid) -> torch.Tensor:
        out = self._affinity16(q16, beta, exclude_laid) * (self.alpha if alpha is None else float(alpha))
        zs = self._zero_shot16(q16)
        return out if zs is None else zs + out

    # ---- public ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def affinity(self, queries: torch.Tensor, beta: Optional[float] = None, exclude=None) -> torch.Tensor:
        """queries [Q, E] (any float dtype, anywhere) -> A fp32 [Q, C] on the device.  `exclude`: per query an ORIGINAL stored
        row to leave out, or -1."""
        q16 = self._queries(queries)
        return self._affinity16(q16, beta, self._exclude(exclude, q16.shape[0]))

    @torch.no_grad()
    def logits(self, queries: torch.Tensor, alpha: Optional[float] = None, beta: Optional[float] = None, exclude=None) -> torch.Tensor:
        """logit_scale * <f, t_c> + alpha * A[q, c], fp32 [Q, C]; the zero-shot term is taken on the 16-bit query rows."""
        q16 = self._queries(queries)
        return self._logits16(q16, alpha, beta, self._exclude(exclude, q16.shape[0]))

    @torch.no_grad()
    def __call__(self, images: torch.Tensor = None, image_features: torch.Tensor = None, model=None):
        """Returns (probabilities [Q, C] softmax, indices [Q], labels list), the shape of ZeroShotClassifier.__call__; labels are
        class names, or the indices when the classifier has no names.  Pass image_features to reuse an encode."""
        if image_features is None:
            if model is None or images is None:
                raise ValueError("CacheClassifier: pass image_features, or images together with the model that encodes them")
            image_features = model.encode_image(images.to(self.features.device))
        probs = self.logits(image_features).softmax(dim=-1)
        idx = probs.argmax(dim=1)
        picked = idx.tolist()
        return probs, idx, [self.class_names[i] for i in picked] if self.class_names is not None else picked

    @torch.no_grad()
    def leave_one_out(self, alpha: Optional[float] = None, beta: Optional[float] = None) -> torch.Tensor:
        """Logits [N, C] of every stored row as a query with itself excluded."""
        return self._logits16(self.features, alpha, beta, self._pos.to(torch.int32))

    @torch.no_grad()
    def tune(self, alphas: Sequence[float], betas: Sequence[float], val_features: Optional[torch.Tensor] = None,
             val_labels=None):
        """Grid search of (alpha, beta) for top-1 accuracy on validation data, or without it on the leave-one-out logits of the
        stored rows.  One affinity launch pair per beta; the alpha sweep and the accuracies run on the device; one read-back.
        Returns (alpha, beta, accuracy, grid) with grid a host float64 [len(alphas), len(betas)] of accuracies; equal
        accuracies go to the first grid point (alphas outer, betas inner)."""
        alphas, betas = [float(a) for a in alphas], [float(b) for b in betas]
        if not alphas or not betas:
            raise ValueError("tune: empty grid")
        if (val_features is None) != (val_labels is None):
            raise ValueError("tune: give both val_features and val_labels, or neither")
        if val_features is None:
            q16, excl, target = self.features, self._pos.to(torch.int32), self._labels_dev
        else:
            q16, excl = self._queries(val_features), None
            target = torch.as_tensor(val_labels).to(q16.device).long()
            if tuple(target.shape) != (q16.shape[0],):
                raise ValueError(f"tune: expected {q16.shape[0]} val_labels, got {tuple(target.shape)}")
        if q16.shape[0] == 0:
            raise ValueError("tune: nothing to tune on")
        zs = self._zero_shot16(q16)
        A = torch.stack([self._affinity16(q16, b, excl) for b in betas])                        # [B, Q, C]
        al = torch.tensor(alphas, device=A.device, dtype=torch.float32)
        logits = al[:, None, None, None] * A[None]                                              # [A, B, Q, C]
        if zs is not None:
            logits = logits + zs
        correct = (logits.argmax(dim=-1) == target).sum(dim=-1)                                 # [A, B] int64
        back = torch.cat([correct.reshape(-1).argmax()[None], correct.reshape(-1)]).cpu()       # the one read-back
        best, counts = int(back[0]), back[1:].reshape(len(alphas), len(betas))
        grid = counts.double() / q16.shape[0]
        ia, ib = divmod(best, len(betas))
        return alphas[ia], betas[ib], float(grid[ia, ib]), grid

    # ---- training the keys (Tip-Adapter-F) and persistence --------------------------------------------------------------
    def fit(self, train_features: Optional[torch.Tensor] = None, train_labels=None, *, epochs: int = 20, lr: float = 1e-3,
            weight_decay: float = 0.0, batch_size: Optional[int] = None, seed: int = 0) -> List[float]:
        """Train the stored keys with the towers frozen (Tip-Adapter-F): the keys become an fp32 [N, E] parameter that starts
        from the normalised rows; each step rebuilds the 16-bit laid-out shadow from it, takes the cross-entropy of
        zero-shot + alpha * A and sends dA through the fused backward kernel (CacheAffinityFunction); torch.optim.AdamW with a
        cosine schedule to 0 updates the parameter.  alpha and beta stay fixed (call tune() afterwards) and the keys are not
        renormalised, as in the paper.  Without train_features the stored rows (as they are now) are the queries, each with
        its own row excluded - the leave-one-out objective; with train_features [M, E] and train_labels [M] (augmented views,
        for example) nothing is excluded.  Returns the per-epoch mean loss as a host list, read back once at the end."""
        if (train_features is None) != (train_labels is None):
            raise ValueError("fit: give both train_features and train_labels, or neither")
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError(f"fit: epochs = {epochs}")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError(f"fit: batch_size = {batch_size}")
        if len(self) == 0:
            raise ValueError("CacheClassifier: no stored rows")
        dev = self.features.device
        if train_features is None:
            q16, excl, target = self.features.clone(), self._pos.to(torch.int32), self._labels_dev
        else:
            q16, excl = self._queries(train_features), None
            target = torch.as_tensor(train_labels).to(dev).long()
            if tuple(target.shape) != (q16.shape[0],):
                raise ValueError(f"fit: expected {q16.shape[0]} train_labels, got {tuple(target.shape)}")
        M = q16.shape[0]
        if M == 0:
            raise ValueError("fit: nothing to train on")
        with torch.no_grad():
            zs = self._zero_shot16(q16)
        batches = list(fit_batches(M, None if batch_size is None else int(batch_size), epochs, seed))
        keys = torch.nn.Parameter(self.features.float())
        opt = torch.optim.AdamW([keys], lr=float(lr), weight_decay=float(weight_decay))
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=len(batches))
        Np = self._laid.shape[0]
        sums = torch.zeros(epochs, device=dev, dtype=torch.float32)
        with torch.enable_grad():
            for ep, idx in batches:
                idx = idx.to(dev)
                laid32 = torch.full((Np, self.dim), float("nan"), device=dev, dtype=torch.float32).index_put((self._pos,), keys)
                A = CacheAffinityFunction.apply(laid32, q16[idx], self.class_off, self.class_len, self.beta,
                                                None if excl is None else excl[idx].contiguous())
                if self.per_class == "mean":
                    A = A / self._count
                logits = A * self.alpha if zs is None else zs[idx] + A * self.alpha
                loss = torch.nn.functional.cross_entropy(logits, target[idx])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                sched.step()
                sums[ep] += loss.detach() * (idx.numel() / M)
        self._set_rows(keys.detach().to(self.dtype), self.labels)
        return sums.cpu().tolist()

    def state_dict(self) -> dict:
        """Plain tensors and lists (torch.save takes it): the keys as they are stored (16-bit, original order, trained or not),
        labels, class names, alpha, beta, per_class, text features and logit_scale."""
        return dict(keys=self.features.detach().cpu(), labels=self.labels.clone(), num_classes=self.num_classes,
                    class_names=None if self.class_names is None else list(self.class_names), alpha=self.alpha, beta=self.beta,
                    per_class=self.per_class, logit_scale=self.logit_scale,
                    text_features=None if self.text_features is None else self.text_features.detach().cpu())

    _STATE_KEYS = ("keys", "labels", "num_classes", "class_names", "alpha", "beta", "per_class", "logit_scale", "text_features")

    def load_state_dict(self, state: dict, device: Optional[torch.device] = None) -> "CacheClassifier":
        """Replace this classifier's content by a state_dict()'s; the keys are taken as they are (not renormalised), so the
        logits are those of the classifier that was saved, bit for bit."""
        missing = [k for k in self._STATE_KEYS if k not in state]
        extra = sorted(k for k in state if k not in self._STATE_KEYS)
        if missing or extra:
            raise KeyError(f"load_state_dict: missing {missing}, unexpected {extra}")
        keys = state["keys"]
        if not isinstance(keys, torch.Tensor) or keys.dim() != 2 or keys.dtype not in HALF_TYPES:
            raise ValueError("load_state_dict: keys must be a 2-D bfloat16 / float16 tensor")
        dev = torch.device(device) if device is not None else (self.features.device if hasattr(self, "features") else _device())
        self.dtype = keys.dtype
        text = state["text_features"]
        self._init(keys.detach().to(dev).contiguous(), state["labels"], state["num_classes"], state["class_names"],
                   None if text is None else text.to(dev), state["logit_scale"], state["alpha"], state["beta"], state["per_class"])
        return self

    @classmethod
    def from_state_dict(cls, state: dict, device: Optional[torch.device] = None) -> "CacheClassifier":
        return cls.__new__(cls).load_state_dict(state, device)
