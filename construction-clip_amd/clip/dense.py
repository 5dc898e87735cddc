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

Whole photos.  The tower sees a square at its own resolution; a multi-megapixel, non-square site photo goes through
sliding-window inference, as MaskCLIP, SCLIP and ClearCLIP are evaluated: `plan_windows` lays overlapping squares over the
photo (several sizes for a multi-scale ensemble), `segment_photo` runs the tower on all of them and ops.dense_stitch
(csrc/dense_stitch.hip) averages the class probabilities where windows overlap, straight into the photo-sized label map,
confidence map and picture.  `segment(size=(height, width))` is the one-window case: a non-square label map.

Boundaries.  The class maps are a few patches wide and bilinearly stretched: their label boundaries are smooth blobs that ignore
the photo's edges.  `refine_maps` / `.refine(photo)` run pixel-adaptive mask refinement (PAMR; Araslanov & Roth, CVPR 2020, the
usual post-processing of training-free dense CLIP) on the maps at the output size: a few iterations of a local propagation
whose weights come from the photo's own colours (csrc/dense_refine.hip).  No training, no extra model.
"""
from __future__ import annotations

import colorsys
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
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


def _area_fractions(labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """fp64 [..., C + 1] of uint8 labels [..., H, W]: per map the share of pixels of every class, "none" (255) last.  The counts
    are integers (scatter_add_ of ones), each divided once by H * W: a map's shares sum to 1."""
    n = labels.shape[-2] * labels.shape[-1]
    lab = labels.reshape(-1, n).long()
    lab = torch.where(lab == NONE_LABEL, torch.full_like(lab, n_classes), lab)
    counts = torch.zeros(lab.shape[0], n_classes + 1, device=lab.device, dtype=torch.long)
    counts.scatter_add_(1, lab, torch.ones_like(lab))
    return (counts.double() / n).reshape(*labels.shape[:-2], n_classes + 1)


def _top_classes(fractions: torch.Tensor) -> List[Optional[int]]:
    """per row of area fractions [..., C + 1] the class with the largest area, None when no pixel has a class"""
    fr = fractions.reshape(-1, fractions.shape[-1])[:, :-1].cpu()
    return [int(r.argmax()) if float(r.max()) > 0 else None for r in fr]


class _LabelledResult:
    """What DenseResult, PhotoDenseResult and RefinedDenseResult do with their labels ([B, H, W], or [H, W] for a single photo),
    conf, class_names and n_classes.  No fields of its own."""

    def area_fractions(self) -> torch.Tensor:
        """fp64 [B, C + 1] ([C + 1] for a single photo): the share of pixels per class, "none" last.  Pixel COUNTS are integers,
        each divided once by H * W: a row sums to 1."""
        return _area_fractions(self.labels, self.n_classes)

    def top_class(self):
        """the class with the largest area (None when no pixel has a class): a list per image, one value for a single photo"""
        top = _top_classes(self.area_fractions())
        return top if self.labels.dim() == 3 else top[0]

    def components(self, connectivity: int = 4) -> "ComponentsResult":
        """the connected components of the label maps with their mean confidences, on the device (`label_components`), image by
        image"""
        return label_components(self.labels, self.conf, connectivity=connectivity)

    def instances(self, min_area: int = 1, min_score: float = 0.0, classes: Optional[Sequence[int]] = None,
                  connectivity: int = 4) -> List[dict]:
        """one record per connected component: components(connectivity).instances(...) with this result's class names"""
        return self.components(connectivity).instances(min_area=min_area, min_score=min_score, classes=classes,
                                                       class_names=self.class_names)

    def evaluate(self, gt: torch.Tensor, *, band: Optional[int] = None, per_image: bool = False) -> "SegmentationScores":
        """mean IoU and boundary IoU of these labels against a ground-truth mask of the same [H, W] (uint8, class indices, 255 =
        ignore): `evaluate_labels` with this result's n_classes and class names"""
        want = tuple(self.labels.shape)
        got = tuple(getattr(gt, "shape", ()))
        if got != want and not (len(want) == 3 and want[0] == 1 and got == want[1:]):
            raise ValueError(f"evaluate: gt must have the labels' shape {list(want)}, got {list(got)}")
        return evaluate_labels(self.labels, gt.reshape(want), self.n_classes, band=band, per_image=per_image,
                               class_names=self.class_names)


@dataclass
class DenseResult(_LabelledResult):
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
        and conf are recomputed by the same launch and come out as they are.  A result of segment(size=(height, width)) works the
        same way, S, S read as height, width: one dense_stitch launch per image."""
        B, H, W = self.labels.shape
        dev = self.probs.device
        pal, photo, a8 = _overlay_inputs(alpha, palette, self.n_classes, photo, (B, H, W, 3), dev)
        out = torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8)
        lab, conf = torch.empty_like(self.labels), torch.empty_like(self.conf)
        if H != W:
            _stretch_maps(self.probs, lab, conf, self.min_conf, overlay=out, palette=pal, photo=photo, alpha8=a8)
        else:
            ops.dense_label_map(self.probs, H, lab, conf, min_conf=self.min_conf, overlay=out, palette=pal, photo=photo, alpha8=a8)
        return out

    def refine(self, photo, *, dilations: Sequence[int] = ops.REFINE_DEFAULT_DILATIONS, iterations: int = 10,
               min_conf: Optional[float] = None) -> "RefinedDenseResult":
        """Snap the class maps to the photo's edges: the maps stretched to the labels' size (ops.dense_stitch_maps, one window
        over the picture per image), `refine_maps` under `photo` (uint8 [B, S, S, 3] or [S, S, 3], already at the map's size, as
        overlay(photo=) takes it), ops.dense_maps_label.  min_conf: default this result's.  Memory: two C x H x W fp32 buffers
        plus 16 bytes per pixel and image - about 0.9 GB for 12 megapixels and nine classes; label a smaller picture
        (segment_images.py --max-side) when that is too much."""
        B, H, W = self.labels.shape
        dev = self.probs.device
        guide = _refine_guide(photo, (B, H, W, 3), dev)
        maps = torch.empty(B, self.n_classes, H, W, device=dev, dtype=torch.float32)
        box = _device_boxes(np.array([[0, 0, W, H]]), dev)
        for b in range(B):
            ops.dense_stitch_maps(self.probs[b:b + 1], box, H, W, maps[b])
        return _refined(maps, guide, None, self.class_names, self.min_conf if min_conf is None else min_conf, dilations, iterations)


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
            size: Union[None, int, Tuple[int, int]] = None, min_conf: float = 0.0, temperature: Optional[float] = None,
            tokenize: Optional[Callable] = None) -> DenseResult:
    """Label every pixel of `image` ([B, 3, R, R], preprocessed) with one of `classes` ([C, E] features or C prompt strings,
    1 <= C <= 255).  size: side of the label map (default: the model's input resolution), or (height, width) for a map that
    is not square - the class maps are then stretched over it, each axis with its own scale (one ops.dense_stitch launch per
    image, one window covering the map).  temperature: the factor on the cosines before the softmax (default
    exp(model.logit_scale)).  Pixels whose best probability is below min_conf get 255."""
    text, names = class_features(model, classes, tokenize)
    feats = dense_features(model, image, mode)
    B, g, _, E = feats.shape
    C = text.shape[0]
    dev = feats.device
    rect = isinstance(size, (tuple, list))
    if rect:
        if len(size) != 2:
            raise ValueError(f"segment: size must be an int or (height, width), got {size!r}")
        H, W = int(size[0]), int(size[1])
    else:
        H = W = model.geo.image_resolution if size is None else int(size)
    scale = float(model.logit_scale.detach().exp()) if temperature is None else float(temperature)
    probs = torch.empty(B, C, g, g, device=dev, dtype=torch.float32)
    labels = torch.empty(B, H, W, device=dev, dtype=torch.uint8)
    conf = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    if B > 0:
        ops.dense_class_probs(feats.view(B * g * g, E), text, scale, g * g, probs.view(B, C, g * g))
        if rect:
            _stretch_maps(probs, labels, conf, min_conf)
        else:
            ops.dense_label_map(probs, H, labels, conf, min_conf=min_conf)
    return DenseResult(probs=probs, labels=labels, conf=conf, class_names=names, min_conf=float(min_conf))


# ---- whole photos: sliding windows, stitched ---------------------------------------------------
def _device_boxes(boxes: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32)).to(dev)


def _overlay_inputs(alpha, palette, n_classes, photo, shape, dev):
    """(palette on the device, photo on the device or None, a8) of an overlay of `shape` = ([B,] H, W, 3), checked"""
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"overlay: alpha must lie in [0, 1], got {alpha}")
    pal = default_palette(n_classes) if palette is None else palette
    if not isinstance(pal, torch.Tensor) or pal.dtype != torch.uint8 or tuple(pal.shape) != (256, 3):
        raise ValueError("overlay: palette must be a uint8 [256, 3] tensor")
    if photo is not None:
        if isinstance(photo, np.ndarray):
            photo = torch.from_numpy(np.ascontiguousarray(photo))
        if not isinstance(photo, torch.Tensor) or photo.dtype != torch.uint8:
            raise ValueError(f"overlay: photo must be a uint8 tensor {list(shape)}")
        if len(shape) == 4 and photo.dim() == 3:
            photo = photo.unsqueeze(0).expand(shape[0], -1, -1, -1)
        if tuple(photo.shape) != tuple(shape):
            raise ValueError(f"overlay: photo must be {list(shape)} (resize it to the map first), got {tuple(photo.shape)}")
        photo = photo.to(dev).contiguous()
    return pal.to(dev).contiguous(), photo, int(round(256 * alpha))


def _stretch_maps(probs, labels, conf, min_conf, overlay=None, palette=None, photo=None, alpha8=256) -> None:
    """probs [B, C, g, g] stretched over labels / conf [B, H, W] (and overlay / photo [B, H, W, 3]), each axis with its own scale:
    one ops.dense_stitch launch per image, one window covering the map."""
    B, H, W = labels.shape
    box = _device_boxes(np.array([[0, 0, W, H]]), probs.device)
    for b in range(B):
        ops.dense_stitch(probs[b:b + 1], box, H, W, labels[b], conf[b], min_conf=min_conf, overlay=None if overlay is None else overlay[b],
                         palette=palette, photo=None if photo is None else photo[b], alpha8=alpha8)


def _plan_one(width: int, height: int, window: int, stride: Optional[int]) -> np.ndarray:
    if int(window) != window or window < 2:
        raise ValueError(f"plan_windows: window must be an integer >= 2, got {window}")
    window = int(window)
    stride = window // 2 if stride is None else stride
    if int(stride) != stride or stride < 1:
        raise ValueError(f"plan_windows: stride must be an integer >= 1, got {stride}")
    if stride > window:
        raise ValueError(f"plan_windows: stride {stride} exceeds window {window}: pixels between two windows would be covered by none")
    side = min(window, width, height)
    step = min(int(stride), side)                 # a window clipped to a small photo keeps the lattice free of holes

    def starts(length):
        last = length - side
        s = list(range(0, last + 1, step))
        if s[-1] != last:
            s.append(last)                        # the last row / column, shifted back flush with the edge
        return s

    xs, ys = starts(width), starts(height)
    return np.array([[x, y, x + side, y + side] for y in ys for x in xs], dtype=np.int64).reshape(-1, 4)


def plan_windows(width: int, height: int, window, stride=None) -> np.ndarray:
    """int64 [K, 4] (x0, y0, x1, y1): square windows of side min(window, width, height) on a `stride` lattice (default
    window // 2; never more than the side), row-major, the last row and column shifted back flush with the photo's edge
    (MMSegmentation's "slide" mode): every pixel is covered and no window leaves the photo.  `window` may be a sequence of sizes
    (a multi-scale ensemble): the lists are concatenated in the order given, and `stride` is then a sequence of the same length
    or None.  ValueError: window < 2, stride < 1, stride > window (holes), an empty photo."""
    if int(width) != width or int(height) != height or width < 1 or height < 1:
        raise ValueError(f"plan_windows: the photo must be at least 1 x 1, got {width} x {height}")
    width, height = int(width), int(height)
    if isinstance(window, (list, tuple, np.ndarray)):
        wins = list(window)
        if not wins:
            raise ValueError("plan_windows: no window size given")
        if stride is None:
            strides = [None] * len(wins)
        elif isinstance(stride, (list, tuple, np.ndarray)) and len(stride) == len(wins):
            strides = list(stride)
        else:
            raise ValueError(f"plan_windows: with {len(wins)} window sizes, stride must be None or a sequence of {len(wins)}, got {stride!r}")
        return np.concatenate([_plan_one(width, height, w, s) for w, s in zip(wins, strides)], axis=0)
    if isinstance(stride, (list, tuple, np.ndarray)):
        raise ValueError(f"plan_windows: one window size takes one stride, got {stride!r}")
    return _plan_one(width, height, window, stride)


def label_boxes(labels, c: int, min_area: int = 1) -> List[Tuple[int, int, int, int]]:
    """(x0, y0, x1, y1) of every 4-connected component of label `c` in the [H, W] map with at least min_area pixels, in the order
    of each component's first pixel (row-major).  Host side, numpy only: the runs of `c` in every row, joined to the runs they
    touch in the row above by union-find."""
    lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if lab.ndim != 2:
        raise ValueError(f"class_boxes: labels must be [H, W], got {lab.shape}")
    H, W = lab.shape
    parent: List[int] = []
    runs = []                                      # (y, x0, x1) per run id

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prev: List[int] = []
    for y in range(H):
        m = np.concatenate(([0], (lab[y] == c).astype(np.int8), [0]))
        d = np.diff(m)
        cur = []
        for x0, x1 in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
            i = len(parent)
            parent.append(i)
            runs.append((y, x0, x1))
            for j in prev:
                if runs[j][1] < x1 and x0 < runs[j][2]:                      # share a column: 4-connected
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)                        # the root is the component's first run
            cur.append(i)
        prev = cur
    comps = {}
    for i, (y, x0, x1) in enumerate(runs):
        r = find(i)
        bx = comps.get(r)
        comps[r] = [x0, y, x1, y + 1, x1 - x0] if bx is None else [min(bx[0], x0), bx[1], max(bx[2], x1), y + 1, bx[4] + x1 - x0]
    return [(b[0], b[1], b[2], b[3]) for _, b in sorted(comps.items()) if b[4] >= min_area]


# ---- instances: connected components on the device ----------------------------------------------
@dataclass
class ComponentsResult:
    """The connected components of a label map (`label_components`).  Component i is numbered in the order of its first pixel
    (image by image, row-major), which is the order `label_boxes` returns boxes in."""
    ids: torch.Tensor                    # int32, the labels' shape: the component number of every pixel, -1 = none
    root: torch.Tensor                   # int32, the labels' shape: the flat index of the component's first pixel, -1 = none
    n: int
    label: torch.Tensor                  # uint8 [n] (CPU): the class
    image: torch.Tensor                  # int32 [n] (CPU): the batch index
    first: torch.Tensor                  # int32 [n] (CPU): the flat index of the first pixel
    area: torch.Tensor                   # int32 [n] (CPU): pixels
    boxes: torch.Tensor                  # int32 [n, 4] (CPU): (x0, y0, x1, y1), half-open, in the image's own coordinates
    score: Optional[torch.Tensor]        # fp64 [n] (CPU): the mean confidence, None without conf
    qsum: Optional[torch.Tensor] = None  # int64 [n] (CPU): the sum of the 16.16 fixed-point confidences behind `score`
    connectivity: int = 4

    def boxes_of(self, c: int, min_area: int = 1, image: int = 0) -> List[Tuple[int, int, int, int]]:
        """the boxes of class c's components in one image with at least min_area pixels: what label_boxes(labels[image], c,
        min_area) returns for connectivity 4, in the same order"""
        keep = (self.label == c) & (self.image == image) & (self.area >= min_area)
        return [tuple(b) for b in self.boxes[keep].tolist()]

    def mask(self, i: int) -> torch.Tensor:
        """bool map of the ids' shape (on the device): the pixels of component i"""
        if not 0 <= i < self.n:
            raise IndexError(f"mask: component {i} of {self.n}")
        return self.ids == i

    def instances(self, min_area: int = 1, min_score: float = 0.0, classes: Optional[Sequence[int]] = None,
                  class_names: Optional[Sequence[str]] = None) -> List[dict]:
        """one dict {"image", "class", "name", "box", "area", "score"} per component with at least min_area pixels, a mean
        confidence of at least min_score (not applied when there is no conf) and a class in `classes` (None: any), in id order.
        name is class_names[class], None without names; score is None without conf."""
        want = None if classes is None else {int(c) for c in classes}
        out = []
        for i in range(self.n):
            c, area = int(self.label[i]), int(self.area[i])
            score = None if self.score is None else float(self.score[i])
            if area < min_area or (want is not None and c not in want) or (score is not None and score < min_score):
                continue
            out.append({"image": int(self.image[i]), "class": c, "name": None if class_names is None else class_names[c],
                        "box": tuple(self.boxes[i].tolist()), "area": area, "score": score})
        return out


def label_components(labels: torch.Tensor, conf: Optional[torch.Tensor] = None, *, connectivity: int = 4) -> ComponentsResult:
    """The connected components of a label map, on the device (csrc/label_components.hip): labels uint8 [H, W] or [B, H, W], 255 =
    none; pixels of equal label that are 4-neighbours (or 8-neighbours) inside one image belong together.  With conf (fp32, the
    labels' shape) every component also gets its mean confidence, an exact integer sum of 16.16 fixed-point values divided
    once in fp64.  ops.label_components, ONE device -> host read (the count, which sizes the statistics), ops.component_stats;
    the per-component statistics come back as CPU tensors.  HIP only: a CPU tensor raises."""
    fname = "label_components"
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise ValueError(f"{fname}: labels must be a cuda tensor, got {getattr(labels, 'device', type(labels))} (no CPU path)")
    if labels.dim() not in (2, 3):
        raise ValueError(f"{fname}: labels must be [H, W] or [B, H, W], got {tuple(labels.shape)}")
    if conf is not None and (not isinstance(conf, torch.Tensor) or tuple(conf.shape) != tuple(labels.shape)):
        raise ValueError(f"{fname}: conf must be a tensor of the labels' shape {list(labels.shape)}, got {tuple(getattr(conf, 'shape', ()))}")
    shape = labels.shape
    lab3 = labels.reshape(-1, shape[-2], shape[-1]) if labels.dim() == 2 else labels
    conf3 = None if conf is None else conf.reshape(lab3.shape)
    dev = labels.device
    root = torch.empty(lab3.shape, device=dev, dtype=torch.int32)
    ids = torch.empty(lab3.shape, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    workspace = torch.empty(max(1, (lab3.numel() + ops.COMPONENTS_GROUP - 1) // ops.COMPONENTS_GROUP), device=dev, dtype=torch.int32)
    ops.label_components(lab3, connectivity, root, ids, count, workspace)
    n = int(count.item())                                                     # the one read that sizes what follows
    label = torch.empty(n, device=dev, dtype=torch.uint8)
    image, first, area = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(3))
    box = torch.empty(n, 4, device=dev, dtype=torch.int32)
    qsum = None if conf3 is None else torch.empty(n, device=dev, dtype=torch.int64)
    ops.component_stats(lab3, root, ids, n, label, image, first, area, box, conf=conf3, qsum=qsum)
    area_c = area.cpu()
    qsum_c = None if qsum is None else qsum.cpu()
    score = None if qsum_c is None else qsum_c.double() / (65536.0 * area_c.double())
    return ComponentsResult(ids=ids.reshape(shape), root=root.reshape(shape), n=n, label=label.cpu(), image=image.cpu(),
                            first=first.cpu(), area=area_c, boxes=box.cpu(), score=score, qsum=qsum_c, connectivity=int(connectivity))


@dataclass
class PhotoDenseResult(_LabelledResult):
    probs: torch.Tensor                  # fp32 [K, C, g, g]: the class maps of every window
    boxes: torch.Tensor                  # int64 [K, 4] (CPU): the windows, (x0, y0, x1, y1) in photo pixels
    labels: torch.Tensor                 # uint8 [H, W]; 255 = none
    conf: torch.Tensor                   # fp32 [H, W]
    cover: torch.Tensor                  # uint8 [H, W]: windows per pixel (saturating at 255)
    class_names: Optional[List[str]]
    min_conf: float = 0.0

    @property
    def n_classes(self) -> int:
        return self.probs.shape[1]

    def overlay(self, photo=None, alpha: float = 0.5, palette: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [H, W, 3]: the palette colour of every pixel's label, over `photo` (the uint8 [H, W, 3] photo itself) with weight
        round(256 alpha) / 256 when one is given.  Re-runs the stitch launch, as DenseResult.overlay re-runs its own."""
        H, W = self.labels.shape
        dev = self.probs.device
        pal, photo, a8 = _overlay_inputs(alpha, palette, self.n_classes, photo, (H, W, 3), dev)
        out = torch.empty(H, W, 3, device=dev, dtype=torch.uint8)
        ops.dense_stitch(self.probs, _device_boxes(self.boxes.numpy(), dev), H, W, torch.empty_like(self.labels),
                         torch.empty_like(self.conf), min_conf=self.min_conf, overlay=out, palette=pal, photo=photo, alpha8=a8)
        return out

    def class_boxes(self, c: int, min_area: int = 1) -> List[Tuple[int, int, int, int]]:
        """bounding boxes (x0, y0, x1, y1) of the 4-connected components of label c (`label_boxes`): what classify_regions takes"""
        return label_boxes(self.labels, c, min_area)

    def refine(self, photo, *, dilations: Sequence[int] = ops.REFINE_DEFAULT_DILATIONS, iterations: int = 10,
               min_conf: Optional[float] = None) -> "RefinedDenseResult":
        """Snap the stitched class maps to the photo's edges: ops.dense_stitch_maps over all windows, `refine_maps` under `photo`
        (the uint8 [H, W, 3] photo itself, as overlay(photo=) takes it), ops.dense_maps_label.  Pixels that no window covers
        enter as zeros and may receive a class from their neighbours.  min_conf: default this result's.  Memory: two
        C x H x W fp32 buffers plus 16 bytes per pixel - about 0.9 GB for 12 megapixels and nine classes; label a smaller
        picture (segment_images.py --max-side) when that is too much."""
        H, W = self.labels.shape
        dev = self.probs.device
        guide = _refine_guide(photo, (H, W, 3), dev)
        maps = torch.empty(1, self.n_classes, H, W, device=dev, dtype=torch.float32)
        ops.dense_stitch_maps(self.probs, _device_boxes(self.boxes.numpy(), dev), H, W, maps[0])
        return _refined(maps, guide[None], (H, W), self.class_names, self.min_conf if min_conf is None else min_conf, dilations,
                        iterations)


REFINE_MAX_ITERATIONS = 64


def _iterations(fname: str, iterations) -> int:
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= iterations <= REFINE_MAX_ITERATIONS:
        raise ValueError(f"{fname}: iterations must be an integer in [1, {REFINE_MAX_ITERATIONS}], got {iterations!r}")
    return int(iterations)


def _refine_guide(photo, shape, dev) -> torch.Tensor:
    """the photo of refine(photo): checked as overlay(photo=) checks its own, on the device"""
    if photo is None:
        raise ValueError(f"overlay: photo must be a uint8 tensor {list(shape)}")
    return _overlay_inputs(0.0, None, 0, photo, shape, dev)[1]


def refine_maps(maps: torch.Tensor, guide: torch.Tensor, *, dilations: Sequence[int] = ops.REFINE_DEFAULT_DILATIONS,
                iterations: int = 10) -> torch.Tensor:
    """Pixel-adaptive mask refinement of class maps at the output size: maps fp32 [B, C, H, W] or [C, H, W], guide uint8
    [B, H, W, 3] or [H, W, 3] (the photo at the same size) -> refined maps of the same shape, a new tensor.  Each of the
    `iterations` (1 .. 64) steps replaces a pixel's class values by a weighted mean over its 8 neighbours at every dilation (1
    to 6 of them, each 1 .. 24, coordinates clamped to the image); the weights are a softmax of minus the colour difference to
    the neighbour over a tenth of the local standard deviation, so values spread inside a region of like colour and stop at an
    edge.  Rows of weights sum to 1: a constant map stays constant and maps that sum to 1 over the classes keep doing so, up to
    rounding.  One ops.dense_refine_prepare launch, then one ops.dense_refine_step per iteration between two buffers.  HIP only."""
    fname = "refine_maps"
    if not isinstance(maps, torch.Tensor) or maps.dim() not in (3, 4) or maps.dtype != torch.float32:
        raise ValueError(f"{fname}: maps must be an fp32 [B, C, H, W] or [C, H, W] tensor, got "
                         f"{getattr(maps, 'dtype', type(maps))} {tuple(getattr(maps, 'shape', ()))}")
    if not isinstance(guide, torch.Tensor) or guide.dtype != torch.uint8 or guide.dim() != maps.dim():
        raise ValueError(f"{fname}: guide must be a uint8 tensor {'[B, H, W, 3]' if maps.dim() == 4 else '[H, W, 3]'}, got "
                         f"{getattr(guide, 'dtype', type(guide))} {tuple(getattr(guide, 'shape', ()))}")
    m4 = maps if maps.dim() == 4 else maps.unsqueeze(0)
    g4 = guide if guide.dim() == 4 else guide.unsqueeze(0)
    B, C, H, W = m4.shape
    if tuple(g4.shape) != (B, H, W, 3):
        raise ValueError(f"{fname}: guide must be {[B, H, W, 3] if maps.dim() == 4 else [H, W, 3]} for maps {tuple(maps.shape)}, "
                         f"got {tuple(guide.shape)}")
    ds = ops.refine_dilations(fname, dilations)
    iterations = _iterations(fname, iterations)
    if not maps.is_cuda:
        raise ValueError(f"{fname}: maps must be a cuda tensor, got {maps.device} (no CPU path)")
    return _refine_run(m4, g4.to(maps.device), ds, iterations, own=False).view(maps.shape)


def _refine_run(m4: torch.Tensor, g4: torch.Tensor, ds, iterations: int, own: bool) -> torch.Tensor:
    """prepare, then `iterations` steps between two buffers.  own: m4 may serve as the second buffer (it is overwritten);
    otherwise the caller's tensor is read once and two buffers are made."""
    mc, g4 = m4.contiguous(), g4.contiguous()
    own = own or mc is not m4
    key = torch.empty(*g4.shape[:3], 4, device=mc.device, dtype=torch.float32)
    ops.dense_refine_prepare(g4, ds, key)
    cur = torch.empty_like(mc)
    ops.dense_refine_step(mc, cur, g4, key, ds)
    nxt = (mc if own else torch.empty_like(mc)) if iterations > 1 else None
    for _ in range(iterations - 1):
        ops.dense_refine_step(cur, nxt, g4, key, ds)
        cur, nxt = nxt, cur
    return cur


@dataclass
class RefinedDenseResult(_LabelledResult):
    """Class maps refined under a photo (`DenseResult.refine`, `PhotoDenseResult.refine`) and what they label."""
    maps: torch.Tensor                   # fp32 [B, C, H, W], or [C, H, W] from a PhotoDenseResult
    labels: torch.Tensor                 # uint8 [B, H, W] / [H, W]; 255 = none (conf < min_conf)
    conf: torch.Tensor                   # fp32, the labels' shape
    class_names: Optional[List[str]]
    min_conf: float = 0.0
    dilations: Tuple[int, ...] = ops.REFINE_DEFAULT_DILATIONS
    iterations: int = 10

    @property
    def n_classes(self) -> int:
        return self.maps.shape[-3]

    def _maps4(self) -> torch.Tensor:
        return self.maps if self.maps.dim() == 4 else self.maps.unsqueeze(0)

    def overlay(self, photo=None, alpha: float = 0.5, palette: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8, the labels' shape + [3]: the palette colour of every pixel's label, blended over `photo` (at the map's size) as
        the other results' overlays are.  Re-runs ops.dense_maps_label."""
        dev = self.maps.device
        shape = (*self.labels.shape, 3)
        pal, photo, a8 = _overlay_inputs(alpha, palette, self.n_classes, photo, shape, dev)
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
        m4 = self._maps4()
        pic = (m4.shape[0], *shape[-3:])
        ops.dense_maps_label(m4, torch.empty_like(self.labels).view(pic[:3]), torch.empty_like(self.conf).view(pic[:3]),
                             min_conf=self.min_conf, overlay=out.view(pic), palette=pal, photo=None if photo is None else photo.view(pic),
                             alpha8=a8)
        return out


def _refined(maps, guide, shape, class_names, min_conf, dilations, iterations) -> RefinedDenseResult:
    """refine maps [B, C, H, W] under guide [B, H, W, 3] and label them; `shape` = (H, W) gives a single photo's result"""
    ds = ops.refine_dilations("refine", dilations)
    iterations = _iterations("refine", iterations)
    out = _refine_run(maps, guide, ds, iterations, own=True)          # `maps` is this module's own buffer: the second of the two
    B, C, H, W = out.shape
    labels = torch.empty(B, H, W, device=out.device, dtype=torch.uint8)
    conf = torch.empty(B, H, W, device=out.device, dtype=torch.float32)
    ops.dense_maps_label(out, labels, conf, min_conf=min_conf)
    if shape is not None:
        out, labels, conf = out[0], labels[0], conf[0]
    return RefinedDenseResult(maps=out, labels=labels, conf=conf, class_names=class_names, min_conf=float(min_conf),
                              dilations=ds, iterations=iterations)


def segment_photo(model, image, classes: Union[torch.Tensor, Sequence[str]], *, window=None, stride=None, mode: str = "value",
                  min_conf: float = 0.0, temperature: Optional[float] = None, batch: int = 64, preprocess=None,
                  tokenize: Optional[Callable] = None) -> PhotoDenseResult:
    """Label every pixel of one photo of ANY size (a PIL RGB image or a uint8 HWC array / tensor) by sliding-window inference:
    `plan_windows(width, height, window, stride)` (window: default the model's input resolution; a sequence = multi-scale),
    `DevicePreprocess.regions` for all K crops in one upload, `encode_image_dense` in chunks of `batch` windows, one
    ops.dense_class_probs per chunk into one [K, C, g, g] buffer, and ONE ops.dense_stitch at the photo's H x W.  A window that
    the region kernels cannot reduce (check_downscale) is a ValueError that names its size.  Results are not promised to be
    bitwise independent of `batch` (the GEMM tile choice may follow the row count)."""
    from .preprocess_device import DevicePreprocess, check_downscale
    dev = model.logit_scale.device
    R = model.geo.image_resolution
    pre = DevicePreprocess(R, dev) if preprocess is None else preprocess
    if not isinstance(pre, DevicePreprocess) or pre.n_px != R:
        raise ValueError(f"segment_photo: preprocess must be a DevicePreprocess of the model's resolution {R}")
    if int(batch) != batch or batch < 1:
        raise ValueError(f"segment_photo: batch must be an integer >= 1, got {batch}")
    arr = DevicePreprocess._pixels(image)
    if arr is None:
        raise ValueError(f"segment_photo: a PIL image must have mode RGB, got {image.mode} (convert it first)")
    H, W = int(arr.shape[0]), int(arr.shape[1])
    boxes = plan_windows(W, H, R if window is None else window, stride)
    check_downscale(boxes, R)
    text, names = class_features(model, classes, tokenize)
    C, K = text.shape[0], boxes.shape[0]
    scale = float(model.logit_scale.detach().exp()) if temperature is None else float(temperature)
    crops = pre.regions(arr, boxes)                                           # [K, 3, R, R], one upload
    probs = None
    for i in range(0, K, int(batch)):
        feats = dense_features(model, crops[i:i + batch], mode)
        b, g, _, E = feats.shape
        if probs is None:
            probs = torch.empty(K, C, g, g, device=dev, dtype=torch.float32)
        ops.dense_class_probs(feats.view(b * g * g, E), text, scale, g * g, probs[i:i + b].view(b, C, g * g))
    labels = torch.empty(H, W, device=dev, dtype=torch.uint8)
    conf = torch.empty(H, W, device=dev, dtype=torch.float32)
    cover = torch.empty(H, W, device=dev, dtype=torch.uint8)
    ops.dense_stitch(probs, _device_boxes(boxes, dev), H, W, labels, conf, min_conf=min_conf, cover=cover)
    return PhotoDenseResult(probs=probs, boxes=torch.from_numpy(boxes), labels=labels, conf=conf, cover=cover, class_names=names,
                            min_conf=float(min_conf))


# ---- evaluation: mean IoU and boundary IoU against ground-truth masks --------------------------------
def _mean_defined(values) -> float:
    """the mean of the values that are not NaN (math.fsum: the exactly rounded sum, whatever the order); NaN over none"""
    keep = [float(v) for v in values if v == v]
    return math.fsum(keep) / len(keep) if keep else float("nan")


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in float64, NaN where den == 0 (integer tensors in)"""
    out = torch.full(num.shape, float("nan"), dtype=torch.float64)
    ok = den != 0
    out[ok] = num[ok].double() / den[ok].double()
    return out


class SegmentationScores:
    """The scores of label maps against ground truth, from integer counts (`evaluate_labels`; or from count tensors directly).

    confusion: int64 [C, C + 1], or [B, C, C + 1] per image: confusion[g, p] pixels of ground-truth class g labelled p; the last
    column is "none" (255) and counts against the ground-truth class (a false negative of g, a false positive of nobody).
    bands: None, or int64 [C, 3] / [B, C, 3] = (|G_c|, |P_c|, |G_c n P_c|) of the boundary band of half-width `band` pixels.
    All arithmetic is float64 on the host.  A class with an empty union has IoU NaN and is left out of the means; a mean over
    no class is NaN.  Without bands the boundary scores are None.  a + b and a += b add the counts (dataset-level scores over
    photos of any sizes); both must agree on C, band and shape."""

    def __init__(self, confusion: torch.Tensor, bands: Optional[torch.Tensor] = None, band: int = 0,
                 class_names: Optional[Sequence[str]] = None):
        confusion = torch.as_tensor(confusion)
        if confusion.dtype != torch.int64 or confusion.dim() not in (2, 3) or confusion.shape[-1] != confusion.shape[-2] + 1:
            raise ValueError(f"SegmentationScores: confusion must be int64 [C, C + 1] or [B, C, C + 1], got {confusion.dtype} "
                             f"{tuple(confusion.shape)}")
        C = confusion.shape[-2]
        if bands is not None:
            bands = torch.as_tensor(bands)
            if bands.dtype != torch.int64 or tuple(bands.shape) != (*confusion.shape[:-2], C, 3):
                raise ValueError(f"SegmentationScores: bands must be int64 {[*confusion.shape[:-2], C, 3]}, got {bands.dtype} "
                                 f"{tuple(bands.shape)}")
        if isinstance(band, bool) or int(band) != band or band < 0 or (band > 0) != (bands is not None):
            raise ValueError(f"SegmentationScores: band must be a positive integer with bands and 0 without, got {band!r}")
        if class_names is not None and len(class_names) != C:
            raise ValueError(f"SegmentationScores: {len(class_names)} class names for {C} classes")
        self.confusion = confusion.detach().cpu().clone()
        self.bands = None if bands is None else bands.detach().cpu().clone()
        self.band = int(band)
        self.class_names = None if class_names is None else [str(n) for n in class_names]

    # -- counts ----
    @property
    def n_classes(self) -> int:
        return self.confusion.shape[-2]

    @property
    def per_image(self) -> bool:
        return self.confusion.dim() == 3

    def _tp(self):
        return torch.diagonal(self.confusion[..., :, :-1], dim1=-2, dim2=-1)

    def _gt(self):
        return self.confusion.sum(dim=-1)                                       # "none" included

    def _pred(self):
        return self.confusion[..., :, :-1].sum(dim=-2)

    def _rows(self, per_class: torch.Tensor, fn):
        """fn over the class vector of every image ([B] of floats), or of the one result (a float)"""
        if self.per_image:
            return torch.tensor([fn(r) for r in per_class], dtype=torch.float64)
        return fn(per_class)

    # -- scores ----
    @property
    def iou(self) -> torch.Tensor:
        tp = self._tp()
        return _ratio(tp, self._gt() + self._pred() - tp)

    @property
    def miou(self):
        return self._rows(self.iou, _mean_defined)

    @property
    def class_accuracy(self) -> torch.Tensor:
        return _ratio(self._tp(), self._gt())

    @property
    def precision(self) -> torch.Tensor:
        return _ratio(self._tp(), self._pred())

    @property
    def pixel_accuracy(self):
        r = _ratio(self._tp().sum(dim=-1), self.confusion.sum(dim=(-2, -1)))
        return r if self.per_image else float(r)

    @property
    def none_fraction(self):
        r = _ratio(self.confusion[..., -1].sum(dim=-1), self.confusion.sum(dim=(-2, -1)))
        return r if self.per_image else float(r)

    @property
    def fw_iou(self):
        """the IoUs weighted by each class's share of the ground-truth pixels (classes without ground truth carry no weight)"""
        gt, iou = self._gt().double(), self.iou

        def one(i):
            g, u = (gt, iou) if i is None else (gt[i], iou[i])
            total = float(g.sum())
            if total == 0:
                return float("nan")
            return math.fsum(float(a) * float(b) for a, b in zip(g, u) if a > 0) / total
        if self.per_image:
            return torch.tensor([one(i) for i in range(gt.shape[0])], dtype=torch.float64)
        return one(None)

    @property
    def boundary_iou(self) -> Optional[torch.Tensor]:
        if self.bands is None:
            return None
        g, p, i = self.bands[..., 0], self.bands[..., 1], self.bands[..., 2]
        return _ratio(i, g + p - i)

    @property
    def mean_boundary_iou(self):
        return None if self.bands is None else self._rows(self.boundary_iou, _mean_defined)

    # -- sums ----
    def _check_same(self, other) -> None:
        if not isinstance(other, SegmentationScores):
            raise TypeError(f"SegmentationScores: cannot add {type(other).__name__}")
        if other.n_classes != self.n_classes:
            raise ValueError(f"SegmentationScores: {self.n_classes} classes against {other.n_classes}")
        if other.band != self.band:
            raise ValueError(f"SegmentationScores: band {self.band} against band {other.band}")
        if other.confusion.shape != self.confusion.shape:
            raise ValueError(f"SegmentationScores: counts {tuple(self.confusion.shape)} against {tuple(other.confusion.shape)} "
                             f"(take .total() of per-image results first)")

    def __add__(self, other) -> "SegmentationScores":
        self._check_same(other)
        return SegmentationScores(self.confusion + other.confusion, None if self.bands is None else self.bands + other.bands,
                                  self.band, self.class_names if self.class_names is not None else other.class_names)

    def __iadd__(self, other) -> "SegmentationScores":
        self._check_same(other)
        self.confusion += other.confusion
        if self.bands is not None:
            self.bands += other.bands
        if self.class_names is None:
            self.class_names = other.class_names
        return self

    def total(self) -> "SegmentationScores":
        """the counts summed over the images of a per-image result (a pooled result is returned as a copy)"""
        if not self.per_image:
            return SegmentationScores(self.confusion, self.bands, self.band, self.class_names)
        return SegmentationScores(self.confusion.sum(dim=0), None if self.bands is None else self.bands.sum(dim=0), self.band,
                                  self.class_names)

    def as_dict(self) -> dict:
        """plain floats and lists, ready for json.dumps: NaN (nothing to score) becomes None"""
        def plain(v):
            if v is None:
                return None
            if isinstance(v, torch.Tensor):
                return [plain(x) for x in v.tolist()] if v.dim() else plain(v.item())
            if isinstance(v, list):
                return [plain(x) for x in v]
            return None if v != v else float(v)
        out = {"n_classes": self.n_classes, "band": self.band, "class_names": self.class_names,
               "pixels": self.confusion.sum(dim=(-2, -1)).tolist()}
        for k in ("miou", "pixel_accuracy", "fw_iou", "none_fraction", "mean_boundary_iou", "iou", "class_accuracy", "precision",
                  "boundary_iou"):
            out[k] = plain(getattr(self, k))
        return out


def default_band(height: int, width: int) -> int:
    """the band half-width of Boundary IoU's 2 % of the image diagonal: round(0.02 sqrt(H^2 + W^2)) clipped to [1, 32]"""
    return max(1, min(ops.AGREEMENT_MAX_BAND, int(round(0.02 * math.sqrt(height * height + width * width)))))


def evaluate_labels(pred: torch.Tensor, gt: torch.Tensor, n_classes: int, *, band: Optional[int] = None, per_image: bool = False,
                    class_names: Optional[Sequence[str]] = None) -> SegmentationScores:
    """Score label maps against ground truth on the device (csrc/label_agreement.hip): pred and gt uint8 [H, W] or [B, H, W] of
    equal shape, class indices below n_classes; 255 in gt = ignore the pixel, 255 in pred = "none" (counts against the
    ground-truth class).  band: the half-width in pixels of the boundary band of Boundary IoU (Cheng et al., CVPR 2021), 1 .. 32;
    None = `default_band` (2 % of the diagonal, capped), kept on the result; 0 skips the boundary scores.  per_image: one row of
    counts per image instead of one for the batch.  A label in [n_classes, 254] in either map is a ValueError that says in
    which map and how many pixels.  One ops.label_agreement launch and one device -> host read of the counts.  HIP only."""
    fname = "evaluate_labels"
    for t, name in ((pred, "pred"), (gt, "gt")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{fname}: {name} must be a cuda tensor, got {getattr(t, 'device', type(t))} (no CPU path)")
        if t.dtype != torch.uint8:
            raise ValueError(f"{fname}: {name} must be torch.uint8, got {t.dtype}")
    if pred.dim() not in (2, 3) or min(pred.shape) < 1:
        raise ValueError(f"{fname}: pred must be [H, W] or [B, H, W] with no empty dimension, got {tuple(pred.shape)}")
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"{fname}: gt must have pred's shape {list(pred.shape)}, got {list(gt.shape)}")
    H, W = pred.shape[-2:]
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= NONE_LABEL:
        raise ValueError(f"{fname}: n_classes must be an integer in [1, {NONE_LABEL}] (label 255 means none), got {n_classes!r}")
    d = default_band(H, W) if band is None else band
    if isinstance(d, bool) or int(d) != d or not 0 <= d <= ops.AGREEMENT_MAX_BAND:
        raise ValueError(f"{fname}: band must be None or an integer in [0, {ops.AGREEMENT_MAX_BAND}], got {band!r}")
    C, d = int(n_classes), int(d)
    if class_names is not None and len(class_names) != C:
        raise ValueError(f"{fname}: {len(class_names)} class names for {C} classes")
    p3, g3 = pred.reshape(-1, H, W).contiguous(), gt.reshape(-1, H, W).to(pred.device).contiguous()
    B, dev = p3.shape[0], pred.device
    R = B if per_image else 1
    confusion = torch.empty(R, C, C + 1, device=dev, dtype=torch.int64)
    bad = torch.empty(R, 2, device=dev, dtype=torch.int64)
    bands = torch.empty(R, C, 3, device=dev, dtype=torch.int64) if d > 0 else None
    ops.label_agreement(p3, g3, C, d, confusion, bad, bands, per_image=per_image)
    nbad = bad.cpu().sum(dim=0).tolist()                                               # the one read; the counts follow it
    if nbad[0] or nbad[1]:
        what = [f"{n} pixels of {name} hold a label in [{C}, 254]" for n, name in zip(nbad, ("gt", "pred")) if n]
        raise ValueError(f"{fname}: {' and '.join(what)} (n_classes = {C}; 255 = ignore in gt, none in pred)")
    conf_c, bands_c = confusion.cpu(), None if bands is None else bands.cpu()
    if not per_image:
        conf_c, bands_c = conf_c[0], None if bands_c is None else bands_c[0]
    return SegmentationScores(conf_c, bands_c, int(d), class_names)
