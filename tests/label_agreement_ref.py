"""Host reference of the label-agreement counts (csrc/label_agreement.hip, include/cclip_hip.h: cclip_label_agreement) and of the
scores made from them (clip.SegmentationScores), in numpy with explicit index arithmetic, plus the shared case table.

Counts.  For pred, gt uint8 [B, H, W], C classes and the band half-width d:
  confusion [R, C, C + 1]  confusion[r, g, p]: pixels with gt == g < C and pred == p; column C is pred == 255; gt == 255 is ignored
  bad       [R, 2]         pixels with gt in [C, 254]; pixels with gt < C and pred in [C, 254]; they enter no other count
  bands     [R, C, 3]      (|G_c|, |P_c|, |G_c n P_c|), None when d == 0
A pixel p = (y, x) is in the band of a map m when some q = (y + dy, x + dx), |dy| <= d, |dx| <= d, lies outside the image or
has m[q] != m[p] (raw bytes).  `band_mask` walks the (2d + 1)^2 offsets one by one; for the offset (dy, dx) the pixels whose q
lies inside the image are the rectangle y in [max(0, -dy), min(H, H - dy)), x in [max(0, -dx), min(W, W - dx)), and a pixel has a
q outside the image exactly when y < d, y > H - 1 - d, x < d or x > W - 1 - d.  No pooling call, no padding.

Scores.  float64, one division each; means by math.fsum (the exactly rounded sum) over the classes that are not NaN."""
from __future__ import annotations

import math

import numpy as np

NONE = 255
TILE = 64                     # the kernel's tile side
HIST_CELLS = 2048             # C (C + 1) up to here: the kernel's LDS histogram (C <= 44); above: the wave combine


def band_mask(m: np.ndarray, d: int) -> np.ndarray:
    """bool [H, W]: the pixels of m [H, W] that are in its band of half-width d"""
    H, W = m.shape
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    inb = (ys < d) | (ys > H - 1 - d) | (xs < d) | (xs > W - 1 - d)             # some q lies outside the image
    inb = np.broadcast_to(inb, (H, W)).copy()
    for dy in range(-d, d + 1):
        ya, yb = max(0, -dy), min(H, H - dy)
        if ya >= yb:
            continue
        for dx in range(-d, d + 1):
            xa, xb = max(0, -dx), min(W, W - dx)
            if xa >= xb:
                continue
            inb[ya:yb, xa:xb] |= m[ya + dy:yb + dy, xa + dx:xb + dx] != m[ya:yb, xa:xb]
    return inb


def counts(pred: np.ndarray, gt: np.ndarray, C: int, d: int, per_image: bool = False) -> dict:
    """the three outputs as int64 arrays (bands None for d == 0) of pred, gt uint8 [B, H, W]"""
    assert pred.shape == gt.shape and pred.ndim == 3 and pred.dtype == np.uint8 and gt.dtype == np.uint8
    B = pred.shape[0]
    R = B if per_image else 1
    confusion = np.zeros((R, C, C + 1), dtype=np.int64)
    bad = np.zeros((R, 2), dtype=np.int64)
    bands = np.zeros((R, C, 3), dtype=np.int64) if d > 0 else None
    for b in range(B):
        r = b if per_image else 0
        g, p = gt[b].astype(np.int64), pred[b].astype(np.int64)
        bad_g = (g >= C) & (g != NONE)
        bad_p = (g < C) & (p >= C) & (p != NONE)
        bad[r, 0] += int(bad_g.sum())
        bad[r, 1] += int(bad_p.sum())
        use = (g < C) & ~bad_p
        col = np.where(p == NONE, C, p)
        np.add.at(confusion[r], (g[use], col[use]), 1)
        if d > 0:
            ing, inp = band_mask(gt[b], d), band_mask(pred[b], d)
            for c in range(C):
                G = use & (g == c) & ing
                P = use & (p == c) & inp
                bands[r, c, 0] += int(G.sum())
                bands[r, c, 1] += int(P.sum())
                bands[r, c, 2] += int((G & P).sum())
    return {"confusion": confusion, "bad": bad, "bands": bands}


# ---- scores ---------------------------------------------------------------------------------------
def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    out = np.full(num.shape, np.nan, dtype=np.float64)
    ok = den != 0
    out[ok] = num[ok].astype(np.float64) / den[ok].astype(np.float64)
    return out


def _mean_defined(v) -> float:
    keep = [float(x) for x in v if x == x]
    return math.fsum(keep) / len(keep) if keep else float("nan")


def scores(confusion: np.ndarray, bands=None) -> dict:
    """the scores of ONE row of counts: confusion [C, C + 1], bands [C, 3] or None"""
    C = confusion.shape[0]
    tp = np.diagonal(confusion[:, :C])
    gt = confusion.sum(axis=1)
    pr = confusion[:, :C].sum(axis=0)
    total = int(confusion.sum())
    iou = _ratio(tp, gt + pr - tp)
    out = {"iou": iou, "miou": _mean_defined(iou), "class_accuracy": _ratio(tp, gt), "precision": _ratio(tp, pr),
           "pixel_accuracy": float(_ratio(tp.sum(), total)), "none_fraction": float(_ratio(confusion[:, C].sum(), total)),
           "fw_iou": math.fsum(float(a) * float(b) for a, b in zip(gt, iou) if a > 0) / total if total else float("nan"),
           "boundary_iou": None, "mean_boundary_iou": None}
    if bands is not None:
        out["boundary_iou"] = _ratio(bands[:, 2], bands[:, 0] + bands[:, 1] - bands[:, 2])
        out["mean_boundary_iou"] = _mean_defined(out["boundary_iou"])
    return out


def default_band(H: int, W: int) -> int:
    return max(1, min(32, int(round(0.02 * math.sqrt(H * H + W * W)))))


# ---- the case table -------------------------------------------------------------------------------
def blocky(B, H, W, C, seed, block=8, none=0.03, shift=(3, 5), noise=0.05):
    """(pred, gt): gt takes a random class per block x block cell and a few strips of 255; pred is gt moved by `shift` (the last
    rows / columns repeated), with a share `noise` of random pixels and a share `none` of 255"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, C, (B, (H + block - 1) // block, (W + block - 1) // block), dtype=np.int64)
    gt = np.repeat(np.repeat(cells, block, axis=1), block, axis=2)[:, :H, :W].astype(np.uint8)
    yy = np.clip(np.arange(H) - shift[0], 0, H - 1)
    xx = np.clip(np.arange(W) - shift[1], 0, W - 1)
    pred = gt[:, yy][:, :, xx].copy()
    flip = rng.random((B, H, W)) < noise
    pred[flip] = rng.integers(0, C, int(flip.sum()), dtype=np.int64).astype(np.uint8)
    pred[rng.random((B, H, W)) < none] = NONE
    gt = gt.copy()
    if H > 2:
        gt[:, H // 3] = NONE                                  # a strip of ignored pixels across the image
    if W > 6:
        gt[:, :, W - 3] = NONE
    return pred, gt


def stairs(H, W, d):
    """(pred, gt, C = 16): class boundaries exactly on the tile border (x = 64, y = 64) and d and d + 1 pixels past it in each axis;
    pred is gt moved one pixel right and down"""
    def steps(n):
        i = np.arange(n)
        return (i >= TILE).astype(np.int64) + (i >= TILE + d) + (i >= TILE + d + 1)
    gt = (4 * steps(H)[:, None] + steps(W)[None, :]).astype(np.uint8)
    yy, xx = np.clip(np.arange(H) - 1, 0, H - 1), np.clip(np.arange(W) - 1, 0, W - 1)
    return gt[yy][:, xx][None].copy(), gt[None].copy(), 16


def all_pairs(C, H=48, W=48):
    """every (g, p) pair of C classes, p == 255 included, at least once: H W >= C (C + 1)"""
    assert H * W >= C * (C + 1)
    i = np.arange(H * W)
    g = (i // (C + 1)) % C
    p = i % (C + 1)
    return np.where(p == C, NONE, p).astype(np.uint8).reshape(1, H, W), g.astype(np.uint8).reshape(1, H, W)


def batch_same_class_across_images(H=40, W=70):
    """B = 3: image b ends in the class that image b + 1 starts in (its first and last rows are uniform)"""
    gt = np.zeros((3, H, W), dtype=np.uint8)
    for b in range(3):
        gt[b, :H // 2] = b
        gt[b, H // 2:] = (b + 1) % 3
    pred = gt.copy()
    pred[:, :, W // 2:] = np.minimum(pred[:, :, W // 2:] + 1, 2) % 3
    pred[1, 5:9, 3:40] = NONE
    return pred, gt


def _cases():
    out = {}
    out["1x1x1_C1_d1"] = (np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8), 1, 1)
    for d in (1, 32):
        p, g = blocky(1, 5, 7, 3, seed=1, block=2)
        out[f"1x5x7_C3_d{d}"] = (p, g, 3, d)
    for H in (63, 64, 65):
        for W in (63, 64, 65):
            for d in (1, 2, 32):
                p, g = blocky(1, H, W, 5, seed=H * 100 + W + d)
                out[f"side_{H}x{W}_d{d}"] = (p, g, 5, d)
    for d in (1, 2, 32):
        p, g, C = stairs(131, 135, d)
        out[f"stairs_131x135_d{d}"] = (p, g, C, d)
    out["uniform_130x130_d32"] = (np.zeros((1, 130, 130), np.uint8), np.zeros((1, 130, 130), np.uint8), 2, 32)
    p, g = batch_same_class_across_images()
    out["batch_3x40x70_d2"] = (p, g, 3, 2)
    p, g = blocky(2, 33, 70, 4, seed=7)
    p[0, 3:6, 10:30] = 4                                       # labels in [C, 254] in either map: `bad` and nothing else
    p[1, 20, :] = 254
    g[0, 10:12, 40:60] = 200
    g[1, 0, 0] = 4
    out["bad_2x33x70_d2"] = (p, g, 4, 2)
    for C in (43, 44, 45):                                     # one below, at and one past the LDS-histogram switch
        assert (C * (C + 1) <= HIST_CELLS) == (C <= 44)
        p, g = all_pairs(C)
        out[f"pairs_C{C}_d1"] = (p, g, C, 1)
    i = np.arange(20 * 67)
    out["C255_20x67_d2"] = (((i * 7) % 256).astype(np.uint8).reshape(1, 20, 67), (i % 255).astype(np.uint8).reshape(1, 20, 67), 255, 2)
    p, g = blocky(1, 30, 41, 1, seed=9, none=0.2)
    out["C1_30x41_d1"] = (p, g, 1, 1)
    return out


CASES = _cases()              # name -> (pred [B, H, W], gt [B, H, W], C, d)
