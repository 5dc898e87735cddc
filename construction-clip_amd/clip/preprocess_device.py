"""Device-side `preprocess`: the resize / crop / normalise part of openai/CLIP's `_transform(n_px)` on
the GPU, bit-identical to the PIL + numpy pipeline of clip.clip._Transform (which stays the host fallback).

Host side (this file): PIL's resampling windows and integer coefficients restated from its published algorithm
(libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc; bicubic a = -0.5; 8-bit fixed point with 22 fraction
bits) - a few hundred numbers per image size, cached.  Device side: csrc/preprocess.hip (two launches per image).
JPEG decoding stays on the host (PIL), as in the reference's DataLoader workers.
"""
from __future__ import annotations

import functools
import math
from typing import Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def resample_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """(bounds int32 [out, 2] = (first input index, count), coefficients int32 [out, ksize], ksize) of PIL's BICUBIC resampler."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)            # C cast: truncation
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = np.array([_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)], dtype=np.float64)
        ww = 0.0
        for v in w:                                   # sequential double sum, as the C loop
            ww += v
        if ww != 0.0:
            w = w / ww
        kq = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        kk[xx, :xmax] = kq
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def resized_size(w: int, h: int, n: int) -> Tuple[int, int]:
    """torchvision Resize(n) on the shorter side (what clip.clip._Transform does)."""
    if (w <= h and w == n) or (h <= w and h == n):
        return w, h
    if w < h:
        return n, int(n * h / w)
    return int(n * w / h), n


def plan(w: int, h: int, n: int):
    """Everything the two launches need for a w x h image: crop offsets, the horizontal windows of the n surviving columns,
    the vertical windows of the n surviving rows and the input-row range those touch."""
    nw, nh = resized_size(w, h, n)
    left, top = int(round((nw - n) / 2.0)), int(round((nh - n) / 2.0))
    bh, kh, ksh = resample_coeffs(w, nw)
    bv, kv, ksv = resample_coeffs(h, nh)
    bh, kh = np.ascontiguousarray(bh[left:left + n]), np.ascontiguousarray(kh[left:left + n])
    bv, kv = np.ascontiguousarray(bv[top:top + n]), np.ascontiguousarray(kv[top:top + n])
    row0 = int(bv[:, 0].min())
    row1 = int((bv[:, 0] + bv[:, 1]).max())
    return dict(bh=bh, kh=kh, ksh=ksh, bv=bv, kv=kv, ksv=ksv, row0=row0, rows=row1 - row0)


def reference_numpy(img_u8: np.ndarray, n: int) -> np.ndarray:
    """The same two integer passes in numpy (host check of the coefficient restatement against PIL; tests only)."""
    h, w, _ = img_u8.shape
    p = plan(w, h, n)
    src = img_u8[p["row0"]:p["row0"] + p["rows"]].astype(np.int64)
    tmp = np.zeros((p["rows"], n, 3), dtype=np.uint8)
    for xx in range(n):
        x0, cnt = p["bh"][xx]
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, x0:x0 + cnt, :], p["kh"][xx, :cnt].astype(np.int64), axes=([1], [0]))
        tmp[:, xx, :] = np.clip(s >> PRECISION_BITS, 0, 255)
    out = np.zeros((n, n, 3), dtype=np.uint8)
    t64 = tmp.astype(np.int64)
    for yy in range(n):
        y0, cnt = p["bv"][yy]
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(p["kv"][yy, :cnt].astype(np.int64), t64[y0 - p["row0"]:y0 - p["row0"] + cnt], axes=([0], [0]))
        out[yy] = np.clip(s >> PRECISION_BITS, 0, 255)
    return out


# ---- regions: many boxes per call (csrc/preprocess_rois.hip) ----------------------------------------------------------
# The host part is O(1) per box in vectorised float64 numpy: no loop over output samples or taps, the tables are built on
# the device.  ROI_FIELDS names the columns of the int64 descriptor (cclip_roi_desc in include/cclip_hip.h).
ROI_FIELDS = ("src_off", "src_ld", "tmp_off", "w", "h", "nw", "nh", "left", "top", "row0", "rows")
MAX_DOWNSCALE = 64                        # per axis; a window then has 2 * ceil(2 * 64) + 1 = 257 taps, the kernels' limit
MAX_KSIZE = 2 * 2 * MAX_DOWNSCALE + 1


def normalize_boxes(boxes, width: int, height: int) -> np.ndarray:
    """[K, 4] (x0, y0, x1, y1) boxes, ints or floats -> int64 [K, 4] inside a width x height image.  Floats (detector output)
    grow to the enclosing pixel box: floor(x0), floor(y0), ceil(x1), ceil(y1).  Every box is clipped to the image; one that is
    then narrower or lower than 2 pixels (one entirely outside the image has no pixels at all) is a ValueError."""
    b = np.asarray(boxes)
    if b.size == 0:
        return np.zeros((0, 4), dtype=np.int64)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes: expected [K, 4] as (x0, y0, x1, y1), got shape {b.shape}")
    if b.dtype.kind == "f":
        if not np.isfinite(b).all():
            raise ValueError(f"box {int(np.argwhere(~np.isfinite(b).all(axis=1))[0, 0])} has a non-finite coordinate")
        b = np.concatenate([np.floor(b[:, :2]), np.ceil(b[:, 2:])], axis=1)
    elif b.dtype.kind not in "iu":
        raise ValueError(f"boxes: expected integer or floating-point coordinates, got {b.dtype}")
    b = np.clip(b, 0, [width, height, width, height]).astype(np.int64)
    small = (b[:, 2] - b[:, 0] < 2) | (b[:, 3] - b[:, 1] < 2)
    if small.any():
        i = int(np.argmax(small))
        raise ValueError(f"box {i} {np.asarray(boxes)[i].tolist()} covers {max(int(b[i, 2] - b[i, 0]), 0)} x {max(int(b[i, 3] - b[i, 1]), 0)} "
                         f"pixels of the {width} x {height} image after rounding and clipping; a region needs at least 2 x 2")
    return b


def resized_sizes(w: np.ndarray, h: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """resized_size for int64 arrays of widths and heights."""
    keep = ((w <= h) & (w == n)) | ((h <= w) & (h == n))
    portrait = w < h
    long_w = ((n * w).astype(np.float64) / h.astype(np.float64)).astype(np.int64)      # int(n * w / h): true division, truncation
    long_h = ((n * h).astype(np.float64) / w.astype(np.float64)).astype(np.int64)
    nw = np.where(keep, w, np.where(portrait, n, long_w))
    nh = np.where(keep, h, np.where(portrait, long_h, n))
    return nw, nh


def _window_edges(in_size: np.ndarray, out_size: np.ndarray, first: np.ndarray, last: np.ndarray):
    """(start of output sample `first`'s window, end of output sample `last`'s window, ksize) - the two bound formulas of
    resample_coeffs, in its operation order; window starts and ends do not decrease with the sample index."""
    scale = in_size.astype(np.float64) / out_size.astype(np.float64)
    support = 2.0 * np.maximum(scale, 1.0)
    lo = np.maximum(((first + 0.5) * scale - support + 0.5).astype(np.int64), 0)           # astype truncates, as the C cast
    hi = np.minimum(((last + 0.5) * scale + support + 0.5).astype(np.int64), in_size)
    return lo, hi, np.ceil(support).astype(np.int64) * 2 + 1


def _roi_geometry(boxes: np.ndarray, n: int):
    """per box: (w, h, nw, nh, left, top, row0, rows, ksize); ValueError for a box past the downscale limit"""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    nw, nh = resized_sizes(w, h, n)
    left = np.rint((nw - n) / 2.0).astype(np.int64)                                        # round(): half to even, as np.rint
    top = np.rint((nh - n) / 2.0).astype(np.int64)
    ksh = _window_edges(w, nw, left, left + n - 1)[2]
    row0, row1, ksv = _window_edges(h, nh, top, top + n - 1)
    ks = np.maximum(ksh, ksv)
    if ks.size and int(ks.max()) > MAX_KSIZE:
        i = int(np.argmax(ks > MAX_KSIZE))
        raise ValueError(f"box {i} ({int(w[i])} x {int(h[i])} pixels) is reduced by a factor of {max(w[i] / nw[i], h[i] / nh[i]):.1f} "
                         f"at n = {n}; the region kernels take a downscale factor of at most {MAX_DOWNSCALE} per axis")
    return w, h, nw, nh, left, top, row0, row1 - row0, ks


def check_downscale(boxes: np.ndarray, n: int) -> None:
    """ValueError naming the first of the int64 boxes [K, 4] that n x n output would reduce by more than MAX_DOWNSCALE."""
    _roi_geometry(np.asarray(boxes, dtype=np.int64).reshape(-1, 4), n)


def roi_descriptors(boxes: np.ndarray, photo_off: np.ndarray, photo_ld: np.ndarray, n: int):
    """int64 boxes [K, 4] of photos that start at byte `photo_off` [K] of the source buffer with row stride `photo_ld` [K]
    -> (descriptors int64 [K, len(ROI_FIELDS)], ksize_max, bytes of the 8-bit intermediate)."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    x0, y0 = boxes[:, 0], boxes[:, 1]
    w, h, nw, nh, left, top, row0, rows, ks = _roi_geometry(boxes, n)
    tmp = rows * n * 3
    tmp_off = np.cumsum(tmp) - tmp
    photo_off, photo_ld = np.asarray(photo_off, dtype=np.int64), np.asarray(photo_ld, dtype=np.int64)
    desc = np.stack([photo_off + y0 * photo_ld + x0 * 3, np.broadcast_to(photo_ld, w.shape), tmp_off, w, h, nw, nh, left, top, row0, rows],
                    axis=1).astype(np.int64)
    return np.ascontiguousarray(desc), (int(ks.max()) if ks.size else 0), int(tmp.sum())


class DevicePreprocess:
    """Callable with the semantics of clip's `preprocess` but producing a CUDA tensor: PIL image (mode RGB) or uint8 HWC
    array / tensor -> fp32 [3, n, n] on `device`.  Non-RGB PIL images go through the host pipeline (the reference converts
    to RGB only AFTER resizing, which an RGB-first device path would not reproduce bit for bit).

    `regions(image, boxes)` and `many(images, boxes=None)` produce many rows per call - boxes of one photo, or photos (and
    their boxes) of mixed sizes - with one upload and three launches, each row bit-identical to `_transform(n)(image.crop(box))`."""

    def __init__(self, n_px: int, device="cuda"):
        self.n_px, self.device = n_px, torch.device(device)
        self._plans = {}

    @staticmethod
    def _pixels(image):
        """uint8 HWC tensor of a PIL RGB image / array / tensor; None for a PIL image of another mode (host pipeline)."""
        if isinstance(getattr(image, "mode", None), str):       # PIL (a torch tensor has a `mode` method)
            if image.mode != "RGB":
                return None
            return torch.from_numpy(np.asarray(image, dtype=np.uint8).copy())
        if isinstance(image, np.ndarray) and not image.flags.writeable:
            image = image.copy()                        # torch refuses to wrap read-only memory quietly
        arr = torch.as_tensor(image)
        assert arr.dtype == torch.uint8 and arr.dim() == 3 and arr.shape[2] == 3, "expected a uint8 HWC RGB image"
        return arr

    def _host_regions(self, image, boxes: np.ndarray) -> torch.Tensor:
        from .clip import _Transform
        t = _Transform(self.n_px)
        return torch.stack([t(image.crop(tuple(int(v) for v in b))) for b in boxes]).to(self.device)

    def _run_regions(self, src: torch.Tensor, boxes: np.ndarray, photo_off, photo_ld) -> torch.Tensor:
        """src: flat uint8 tensor holding every photo; boxes int64 [K, 4], each relative to its photo.  One upload of the pixels,
        one of the descriptors, three launches, no read-back."""
        from cclip_hip import ops
        n, K = self.n_px, boxes.shape[0]
        out = torch.empty(K, 3, n, n, device=self.device, dtype=torch.float32)
        if K == 0:
            return out
        desc_np, ksize_max, tmp_bytes = roi_descriptors(boxes, photo_off, photo_ld, n)
        desc_host = torch.from_numpy(desc_np)
        src = src.to(self.device, non_blocking=True).contiguous()
        desc = desc_host.to(self.device, non_blocking=True)
        bounds = torch.empty(K, 2, n, 2, device=self.device, dtype=torch.int32)
        kk = torch.empty(K, 2, n, ksize_max, device=self.device, dtype=torch.int32)
        tmp = torch.empty(tmp_bytes, device=self.device, dtype=torch.uint8)
        ops.roi_coeffs(desc_host, desc, n, ksize_max, bounds, kk)
        ops.roi_resample_h(src, desc_host, desc, n, ksize_max, bounds, kk, tmp)
        ops.roi_resample_v_norm(tmp, desc_host, desc, n, ksize_max, bounds, kk, MEAN, STD, out)
        return out

    def regions(self, image, boxes) -> torch.Tensor:
        """fp32 [K, 3, n, n]: row k is `_transform(n)(image.crop(boxes[k]))`, bit for bit.  image: PIL image or uint8 HWC
        array / tensor, uploaded once; boxes [K, 4] as (x0, y0, x1, y1), see normalize_boxes for rounding and errors."""
        arr = self._pixels(image)
        if arr is None:                                 # non-RGB PIL image: the host pipeline per box, as __call__
            return self._host_regions(image, normalize_boxes(boxes, *image.size))
        h, w, _ = arr.shape
        b = normalize_boxes(boxes, w, h)
        return self._run_regions(arr.contiguous().reshape(-1), b, np.zeros(len(b), dtype=np.int64), np.full(len(b), 3 * w, dtype=np.int64))

    def many(self, images: Sequence, boxes=None) -> torch.Tensor:
        """fp32 [N, 3, n, n] from photos of mixed sizes packed into one upload: the whole photo each (what `batch` returns), or,
        with boxes = one [K_i, 4] array per photo, the boxes of photo 0, then those of photo 1, ..."""
        if boxes is not None and len(boxes) != len(images):
            raise ValueError(f"many: {len(boxes)} box lists for {len(images)} images")
        flat, per_box, off, ld, host, dev_rows = [], [], [], [], [], []   # host: (first output row, image, its boxes) of non-RGB images
        cursor = rows = 0
        for i, im in enumerate(images):
            arr = self._pixels(im)
            w, h = im.size if arr is None else (arr.shape[1], arr.shape[0])
            try:
                b = np.array([[0, 0, w, h]], dtype=np.int64) if boxes is None else normalize_boxes(boxes[i], w, h)
                if arr is not None:
                    check_downscale(b, self.n_px)       # here, so that the error names the box within its image
            except ValueError as e:
                raise ValueError(f"image {i}: {e}") from None
            if arr is None:
                host.append((rows, im, b))
            else:
                flat.append(arr.contiguous().reshape(-1))
                per_box.append(b)
                off.append(np.full(len(b), cursor, dtype=np.int64))
                ld.append(np.full(len(b), 3 * w, dtype=np.int64))
                cursor += arr.numel()
                dev_rows.extend(range(rows, rows + len(b)))
            rows += len(b)
        dev = (self._run_regions(torch.cat(flat), np.concatenate(per_box), np.concatenate(off), np.concatenate(ld)) if flat
               else torch.empty(0, 3, self.n_px, self.n_px, device=self.device, dtype=torch.float32))
        if not host:
            return dev
        out = torch.empty(rows, 3, self.n_px, self.n_px, device=self.device, dtype=torch.float32)
        for r, im, b in host:
            out[r:r + len(b)] = self._host_regions(im, b)
        if dev_rows:                                    # the row numbers are known here: an index copy, no mask and no sync
            out.index_copy_(0, torch.tensor(dev_rows, dtype=torch.long).to(self.device, non_blocking=True), dev)
        return out

    def _device_plan(self, w, h):
        key = (w, h)
        if key not in self._plans:
            p = plan(w, h, self.n_px)
            dev = {k: torch.from_numpy(p[k]).to(self.device) for k in ("bh", "kh", "bv", "kv")}
            dev.update(ksh=p["ksh"], ksv=p["ksv"], row0=p["row0"], rows=p["rows"])
            self._plans[key] = dev
        return self._plans[key]

    def __call__(self, image) -> torch.Tensor:
        from cclip_hip import ops
        if hasattr(image, "mode"):                      # PIL
            if image.mode != "RGB":
                from .clip import _Transform
                return _Transform(self.n_px)(image).to(self.device)
            arr = torch.from_numpy(np.asarray(image, dtype=np.uint8).copy())
        else:
            arr = torch.as_tensor(image)
        assert arr.dtype == torch.uint8 and arr.dim() == 3 and arr.shape[2] == 3, "expected a uint8 HWC RGB image"
        h, w, _ = arr.shape
        p = self._device_plan(w, h)
        src = arr.to(self.device, non_blocking=True).contiguous()
        n = self.n_px
        tmp = torch.empty(p["rows"], n, 3, device=self.device, dtype=torch.uint8)
        out = torch.empty(3, n, n, device=self.device, dtype=torch.float32)
        ops.resample_h_u8(src[p["row0"]:p["row0"] + p["rows"]], p["bh"], p["kh"], p["ksh"], tmp)
        ops.resample_v_norm(tmp, p["row0"], p["bv"], p["kv"], p["ksv"], MEAN, STD, out)
        return out

    def batch(self, images: Sequence) -> torch.Tensor:
        return torch.stack([self(im) for im in images])
