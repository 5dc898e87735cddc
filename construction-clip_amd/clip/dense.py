"""Dense zero-shot maps: WHERE in the photo each class is, from one forward pass, with no training, no detector and no gradients.

Training-free dense CLIP.  MaskCLIP (Zhou et al., "Extract Free Dense Labels from CLIP", ECCV 2022) observed that the last
block's value path already carries a local, text-aligned feature for every patch: drop its query / key path, residual and MLP,
push each patch's value vector through out_proj, ln_post and visual.proj, and classify the patches against the text embeddings
as the pooled feature would be.  SCLIP (Wang et al. 2023) and ClearCLIP (Lan et al. 2024) keep an attention in that block but
score it q.q^T or k.k^T, so that a patch attends to patches like itself.  `CLIP.encode_image_dense(mode=)` is the tower side
("value", "qq", "kk"); this module is the head:

    probs  [B, C, g, g]   softmax over the classes of logit_scale * cosine(patch feature, class embedding)   ops.dense_class_probs
    labels [B, S, S]      arg-max class of the bilinearly upsampled maps (255: below min_conf), conf = that probability,
    overlay [B, S, S, 3]  a palette colour per label, blended over the photo in integer arithmetic           ops.dense_label_map

both in csrc/dense_classes.hip.  The classes are a short fixed list here (the reference's caption_type / violation_type), which
is exactly the setting the method is for.  HIP only: there is no CPU path.
"""
from __future__ import annotations

import colorsys
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import torch

from cclip_hip import ops

NONE_LABEL = 255


def default_palette(n_classes: int = NONE_LABEL) -> torch.Tensor:
    """uint8 [256, 3] (CPU): class k < n_classes takes hue k * golden ratio (neighbouring indices far apart on the wheel) at one
    of three brightness steps; the rows from n_classes on, the "none" label 255 among them, are mid grey.  Deterministic; needs
    neither cv2 nor matplotlib."""
    if not 0 <= n_classes <= NONE_LABEL:
        raise ValueError(f"default_palette: n_classes must lie in [0, {NONE_LABEL}], got {n_classes}")
    pal = torch.full((256, 3), 96, dtype=torch.uint8)
    for k in range(n_classes):
        h = (k * 0.6180339887498949) % 1.0
        r, g, b = colorsys.hsv_to_rgb(h, 0.85, (1.0, 0.8, 0.6)[(k // 8) % 3])
        pal[k] = torch.tensor([int(r * 255 + 0.5), int(g * 255 + 0.5), int(b * 255 + 0.5)], dtype=torch.uint8)
    return pal


def dense_features(model, image: torch.Tensor, mode: str = "value") -> torch.Tensor:
    """fp32 [B, g, g, embed_dim]: one feature per patch, not normalised (`CLIP.encode_image_dense`)."""
    return model.encode_image_dense(image, mode=mode)


@dataclass
class DenseResult:
    probs: torch.Tensor                  # fp32 [B, C, g, g]
    labels: torch.Tensor                 # uint8 [B, S, S]; 255 = none (conf < min_conf)
    conf: torch.Tensor                   # fp32 [B, S, S]
    class_names: Optional[List[str]]     # None when the classes came as features
    min_conf: float = 0.0

    @property
    def n_classes(self) -> int:
        return self.probs.shape[1]

    def overlay(self, photo: Optional[torch.Tensor] = None, alpha: float = 0.5, palette: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [B, S, S, 3]: the palette colour of every pixel's label - over `photo` (uint8 [B, S, S, 3] or [S, S, 3], already
        at the map's size) with weight a8 / 256, a8 = round(256 alpha), as (photo (256 - a8) + colour a8 + 128) >> 8.  The labels
        and conf are recomputed by the same launch and come out as they are."""
        B, S = self.labels.shape[0], self.labels.shape[1]
        dev = self.probs.device
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"overlay: alpha must lie in [0, 1], got {alpha}")
        pal = default_palette(self.n_classes) if palette is None else palette
        if not isinstance(pal, torch.Tensor) or pal.dtype != torch.uint8 or tuple(pal.shape) != (256, 3):
            raise ValueError("overlay: palette must be a uint8 [256, 3] tensor")
        if photo is not None:
            if not isinstance(photo, torch.Tensor) or photo.dtype != torch.uint8:
                raise ValueError("overlay: photo must be a uint8 tensor [B, S, S, 3] or [S, S, 3]")
            if photo.dim() == 3:
                photo = photo.unsqueeze(0).expand(B, -1, -1, -1)
            if tuple(photo.shape) != (B, S, S, 3):
                raise ValueError(f"overlay: photo must be [{B}, {S}, {S}, 3] (resize it to the map first), got {tuple(photo.shape)}")
            photo = photo.to(dev).contiguous()
        out = torch.empty(B, S, S, 3, device=dev, dtype=torch.uint8)
        ops.dense_label_map(self.probs, S, torch.empty_like(self.labels), torch.empty_like(self.conf), min_conf=self.min_conf,
                            overlay=out, palette=pal.to(dev).contiguous(), photo=photo, alpha8=int(round(256 * alpha)))
        return out

    def area_fractions(self) -> torch.Tensor:
        """fp64 [B, C + 1]: the share of pixels per class, "none" last.  Pixel COUNTS are integers (bincount), each divided once
        by S * S: a row sums to 1."""
        B = self.labels.shape[0]
        C = self.n_classes
        lab = self.labels.reshape(B, -1).long()
        lab = torch.where(lab == NONE_LABEL, torch.full_like(lab, C), lab)
        counts = torch.zeros(B, C + 1, device=lab.device, dtype=torch.long)
        counts.scatter_add_(1, lab, torch.ones_like(lab))
        return counts.double() / lab.shape[1]

    def top_class(self) -> List[Optional[int]]:
        """per image the class with the largest area, None when no pixel has a class"""
        fr = self.area_fractions()[:, :-1].cpu()
        return [int(r.argmax()) if float(r.max()) > 0 else None for r in fr]


def class_features(model, classes: Union[torch.Tensor, Sequence[str]], tokenize: Optional[Callable] = None):
    """(fp32 [C, E] class embeddings on the model's device, class names or None): a feature tensor passes through; a list of
    prompt strings is tokenized (`tokenize`, default clip.tokenize) and encoded with model.encode_text."""
    dev = model.logit_scale.device
    if isinstance(classes, torch.Tensor):
        if classes.dim() != 2 or classes.shape[1] != model.geo.embed_dim:
            raise ValueError(f"segment: class features must be [C, {model.geo.embed_dim}], got {tuple(classes.shape)}")
        return classes.detach().to(dev).float().contiguous(), None
    names = [str(c) for c in classes]
    if not names:
        raise ValueError("segment: no classes given")
    if tokenize is None:
        from .clip import tokenize
    with torch.no_grad():
        feats = model.encode_text(tokenize(names).to(dev))
    return feats.float().contiguous(), names


def segment(model, image: torch.Tensor, classes: Union[torch.Tensor, Sequence[str]], *, mode: str = "value",
            size: Optional[int] = None, min_conf: float = 0.0, temperature: Optional[float] = None,
            tokenize: Optional[Callable] = None) -> DenseResult:
    """Label every pixel of `image` ([B, 3, R, R], preprocessed) with one of `classes` ([C, E] features or C prompt strings,
    1 <= C <= 255).  size: side of the label map (default: the model's input resolution).  temperature: the factor on the
    cosines before the softmax (default exp(model.logit_scale)).  Pixels whose best probability is below min_conf get 255."""
    text, names = class_features(model, classes, tokenize)
    feats = dense_features(model, image, mode)
    B, g, _, E = feats.shape
    C = text.shape[0]
    dev = feats.device
    S = model.geo.image_resolution if size is None else int(size)
    scale = float(model.logit_scale.detach().exp()) if temperature is None else float(temperature)
    probs = torch.empty(B, C, g, g, device=dev, dtype=torch.float32)
    labels = torch.empty(B, S, S, device=dev, dtype=torch.uint8)
    conf = torch.empty(B, S, S, device=dev, dtype=torch.float32)
    if B > 0:
        ops.dense_class_probs(feats.view(B * g * g, E), text, scale, g * g, probs.view(B, C, g * g))
        ops.dense_label_map(probs, S, labels, conf, min_conf=min_conf)
    return DenseResult(probs=probs, labels=labels, conf=conf, class_names=names, min_conf=float(min_conf))
