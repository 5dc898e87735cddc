"""Few-shot dense maps: class prototypes from annotated masks, for the classes that are hard to say in words.

`segment` and `segment_photo` take their classes as a [C, E] feature tensor.  A text prompt is one way to make such a row; a
handful of annotated photos is another: pool the per-patch features of `encode_image_dense` under each class's mask into one
prototype per class - masked average pooling, the prototype form of few-shot segmentation (Shaban et al., "One-Shot Learning for
Semantic Segmentation", BMVC 2017; Wang et al., "PANet", ICCV 2019).  Training-free, like everything in clip/dense.py, and the
dense counterpart of CacheClassifier / GaussianClassifier on the embedding side.

    protos = clip.DensePrototypes(n_classes, model.geo.embed_dim, class_names)
    protos.add_photo(model, photo, mask)              # any number of photos; the sums add up on the device
    result = clip.segment_photo(model, new_photo, protos.features(text=prompts, text_weight=0.3, model=model))

The pooling is ops.dense_prototypes (csrc/dense_prototypes.hip): a patch cell contributes to class c when at least `min_share` of
its pixels carry c, with that share as its weight; the features are unit vectors; the sums are bitwise repeatable and no
C x H x W plane is ever made.  HIP only: the accumulators may live on the CPU (a loaded state, the host arithmetic of
`features`), but adding needs the device.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from cclip_hip import ops
from .dense import class_features, dense_features, plan_windows

_KEYS = ("sums", "weight", "patches", "pixels", "bad")


def _unit_rows(x: torch.Tensor) -> torch.Tensor:
    """rows divided by their norm; a zero row stays zero (no epsilon)"""
    n = x.norm(dim=1, keepdim=True)
    return torch.where(n > 0, x / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(x))


class DensePrototypes:
    """Five additive accumulators on `device`: sums fp32 [C, E] (weighted unit patch features), weight fp32 [C], patches int64
    [C], pixels int64 [C], bad int64 [1] (include/cclip_hip.h, cclip_dense_prototypes).  min_share is converted ONCE to the
    kernel's integer threshold min_share8 = round(256 * min_share): a cell contributes to class c when
    256 * count_c >= min_share8 * area, so 0.5 means "at least half the cell", 1.0 "cells wholly of one class", 0 "any overlap"."""

    def __init__(self, n_classes: int, embed_dim: int, class_names: Optional[Sequence[str]] = None, min_share: float = 0.5,
                 device: Union[str, torch.device] = "cuda"):
        if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= ops.DENSE_MAX_CLASSES:
            raise ValueError(f"DensePrototypes: n_classes must be an integer in [1, {ops.DENSE_MAX_CLASSES}], got {n_classes!r}")
        if int(embed_dim) != embed_dim or embed_dim < 4 or embed_dim % 4 or embed_dim > ops.DENSE_MAX_EMBED:
            raise ValueError(f"DensePrototypes: embed_dim must be a multiple of 4 in [4, {ops.DENSE_MAX_EMBED}], got {embed_dim!r}")
        if not 0.0 <= float(min_share) <= 1.0:
            raise ValueError(f"DensePrototypes: min_share must lie in [0, 1], got {min_share!r}")
        self.n_classes, self.embed_dim = int(n_classes), int(embed_dim)
        self.class_names = None if class_names is None else [str(c) for c in class_names]
        if self.class_names is not None and len(self.class_names) != self.n_classes:
            raise ValueError(f"DensePrototypes: {len(self.class_names)} class names for {self.n_classes} classes")
        self.min_share8 = int(round(256 * float(min_share)))
        dev = torch.device(device)
        C, E = self.n_classes, self.embed_dim
        self.sums = torch.zeros(C, E, device=dev, dtype=torch.float32)
        self.weight = torch.zeros(C, device=dev, dtype=torch.float32)
        self.patches = torch.zeros(C, device=dev, dtype=torch.int64)
        self.pixels = torch.zeros(C, device=dev, dtype=torch.int64)
        self.bad = torch.zeros(1, device=dev, dtype=torch.int64)

    @property
    def device(self) -> torch.device:
        return self.sums.device

    @property
    def min_share(self) -> float:
        return self.min_share8 / 256.0

    def _name(self, c: int) -> str:
        return f"{c}" if self.class_names is None else f"{c} ({self.class_names[c]})"

    # ---- adding support ------------------------------------------------------------------------
    def add_features(self, feat: torch.Tensor, masks: torch.Tensor, boxes, grid: int, image=None) -> "DensePrototypes":
        """The model-free entry: feat fp32 [K * grid * grid, E] (or [K, grid, grid, E]), masks uint8 [B, H, W], boxes [K, 4] =
        (x0, y0, x1, y1) of window k in picture image[k] (None: picture 0); boxes and image may be tensors, arrays or lists.
        One ops.dense_prototypes launch, added to what the accumulators hold."""
        dev = self.device
        if isinstance(feat, torch.Tensor) and feat.dim() == 4:
            feat = feat.reshape(-1, feat.shape[-1])
        boxes = torch.as_tensor(np.asarray(boxes) if isinstance(boxes, (list, tuple)) else boxes).to(device=dev, dtype=torch.int32).contiguous()
        if image is not None:
            image = torch.as_tensor(image).to(device=dev, dtype=torch.int32).contiguous()
        if isinstance(feat, torch.Tensor) and feat.dim() == 2 and feat.shape[1] != self.embed_dim:
            raise ValueError(f"DensePrototypes: features of width {feat.shape[1]} for prototypes of width {self.embed_dim}")
        ops.dense_prototypes(feat, masks, boxes, grid, self.n_classes, self.min_share8, self.sums, self.weight, self.patches,
                             self.pixels, self.bad, image=image, accumulate=True)      # the scratch comes from torch's caching allocator
        return self

    def add(self, model, image: torch.Tensor, masks: torch.Tensor, *, mode: str = "value") -> "DensePrototypes":
        """image [B, 3, R, R] (preprocessed) with masks uint8 [B, H, W] of any H, W, aligned with the crop the tower saw: one
        window per image covers its whole mask.  One encode_image_dense call and one kernel launch."""
        if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != image.shape[0]:
            raise ValueError(f"DensePrototypes.add: masks must be uint8 [{image.shape[0]}, H, W], got "
                             f"{getattr(masks, 'dtype', type(masks))} {tuple(getattr(masks, 'shape', ()))}")
        with torch.no_grad():
            feats = dense_features(model, image, mode)
        B, g, _, E = feats.shape
        H, W = int(masks.shape[1]), int(masks.shape[2])
        boxes = np.tile(np.array([[0, 0, W, H]], dtype=np.int32), (B, 1))
        return self.add_features(feats.view(B * g * g, E), masks.to(self.device).contiguous(), boxes, g, image=np.arange(B, dtype=np.int32))

    def add_photo(self, model, photo, mask, *, window=None, stride=None, mode: str = "value", batch: int = 64,
                  preprocess=None) -> "DensePrototypes":
        """One photo of ANY size with its uint8 [H, W] mask, on segment_photo's path: plan_windows, DevicePreprocess.regions,
        encode_image_dense in chunks of `batch` windows and one kernel launch per chunk."""
        from .preprocess_device import DevicePreprocess, check_downscale
        dev = self.device
        R = model.geo.image_resolution
        pre = DevicePreprocess(R, model.logit_scale.device) if preprocess is None else preprocess
        if not isinstance(pre, DevicePreprocess) or pre.n_px != R:
            raise ValueError(f"DensePrototypes.add_photo: preprocess must be a DevicePreprocess of the model's resolution {R}")
        if int(batch) != batch or batch < 1:
            raise ValueError(f"DensePrototypes.add_photo: batch must be an integer >= 1, got {batch}")
        arr = DevicePreprocess._pixels(photo)
        if arr is None:
            raise ValueError(f"DensePrototypes.add_photo: a PIL image must have mode RGB, got {photo.mode} (convert it first)")
        H, W = int(arr.shape[0]), int(arr.shape[1])
        if isinstance(mask, np.ndarray):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (H, W):
            raise ValueError(f"DensePrototypes.add_photo: mask must be uint8 [{H}, {W}] like the photo, got "
                             f"{getattr(mask, 'dtype', type(mask))} {list(getattr(mask, 'shape', ()))}")
        boxes = plan_windows(W, H, R if window is None else window, stride)
        check_downscale(boxes, R)
        crops = pre.regions(arr, boxes)
        masks = mask.to(dev).contiguous().view(1, H, W)
        for i in range(0, boxes.shape[0], int(batch)):
            with torch.no_grad():
                feats = dense_features(model, crops[i:i + batch], mode)
            b, g, _, E = feats.shape
            self.add_features(feats.view(b * g * g, E), masks, boxes[i:i + b], g)
        return self

    # ---- reading the prototypes ----------------------------------------------------------------
    def unsupported(self) -> List[int]:
        """the classes no cell has contributed to"""
        return [c for c, n in enumerate(self.patches.tolist()) if n == 0]

    def features(self, text=None, text_weight: float = 0.0, *, model=None, tokenize: Optional[Callable] = None) -> torch.Tensor:
        """fp32 [C, E] for segment / segment_photo: each class's sums row, L2-normalised.  With `text` ([C, E] features, or C
        prompt strings encoded with `model` through class_features) row c is normalise((1 - text_weight) * proto_c +
        text_weight * t^_c), and a class without support (patches == 0) takes its text row t^_c.  Without text such a class is a
        ValueError that names it."""
        if not 0.0 <= float(text_weight) <= 1.0:
            raise ValueError(f"DensePrototypes.features: text_weight must lie in [0, 1], got {text_weight!r}")
        proto = _unit_rows(self.sums)
        missing = self.unsupported()
        if text is None:
            if missing:
                raise ValueError("DensePrototypes.features: no support for class " + ", ".join(self._name(c) for c in missing) +
                                 "; add masks that show it, or give text= for a fall-back")
            return proto
        if isinstance(text, torch.Tensor):
            if tuple(text.shape) != (self.n_classes, self.embed_dim):
                raise ValueError(f"DensePrototypes.features: text must be [{self.n_classes}, {self.embed_dim}], got {tuple(text.shape)}")
            t = text.detach().to(self.device).float()
        else:
            if model is None:
                raise ValueError("DensePrototypes.features: prompt strings need model= to encode them")
            t, _ = class_features(model, text, tokenize)
            if tuple(t.shape) != (self.n_classes, self.embed_dim):
                raise ValueError(f"DensePrototypes.features: {t.shape[0]} prompts of width {t.shape[1]} for [{self.n_classes}, {self.embed_dim}]")
            t = t.to(self.device)
        t = _unit_rows(t)
        tw = float(text_weight)
        out = _unit_rows((1.0 - tw) * proto + tw * t)
        if missing:
            out[missing] = t[missing]
        return out.contiguous()

    def support(self) -> dict:
        """per class: patches, pixels, weight; the bad-pixel count; the classes without support"""
        missing = self.unsupported()
        return {"n_classes": self.n_classes, "class_names": self.class_names, "min_share8": self.min_share8,
                "patches": self.patches.tolist(), "pixels": self.pixels.tolist(), "weight": self.weight.tolist(),
                "bad": int(self.bad.item()), "unsupported": missing,
                "unsupported_names": None if self.class_names is None else [self.class_names[c] for c in missing]}

    # ---- state ---------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        sd = {k: getattr(self, k).detach().cpu().clone() for k in _KEYS}
        sd.update(n_classes=self.n_classes, embed_dim=self.embed_dim, min_share8=self.min_share8, class_names=self.class_names)
        return sd

    def load_state_dict(self, sd: dict) -> "DensePrototypes":
        if (sd["n_classes"], sd["embed_dim"], sd["min_share8"]) != (self.n_classes, self.embed_dim, self.min_share8):
            raise ValueError(f"DensePrototypes: the state is for n_classes {sd['n_classes']}, embed_dim {sd['embed_dim']}, min_share8 "
                             f"{sd['min_share8']}; this instance has {self.n_classes}, {self.embed_dim}, {self.min_share8}")
        for k in _KEYS:
            cur = getattr(self, k)
            if tuple(sd[k].shape) != tuple(cur.shape) or sd[k].dtype != cur.dtype:
                raise ValueError(f"DensePrototypes: state entry {k} must be {cur.dtype} {list(cur.shape)}, got {sd[k].dtype} {list(sd[k].shape)}")
            cur.copy_(sd[k])
        if sd.get("class_names") is not None:
            self.class_names = [str(c) for c in sd["class_names"]]
        return self

    @classmethod
    def from_state_dict(cls, sd: dict, device: Union[str, torch.device] = "cuda") -> "DensePrototypes":
        p = cls(sd["n_classes"], sd["embed_dim"], sd.get("class_names"), sd["min_share8"] / 256.0, device=device)
        return p.load_state_dict(sd)

    def __iadd__(self, other: "DensePrototypes") -> "DensePrototypes":
        if not isinstance(other, DensePrototypes):
            return NotImplemented
        if (other.n_classes, other.embed_dim, other.min_share8) != (self.n_classes, self.embed_dim, self.min_share8):
            raise ValueError(f"DensePrototypes: cannot add n_classes {other.n_classes}, embed_dim {other.embed_dim}, min_share8 "
                             f"{other.min_share8} to {self.n_classes}, {self.embed_dim}, {self.min_share8}")
        for k in _KEYS:
            getattr(self, k).add_(getattr(other, k).to(self.device))
        return self
