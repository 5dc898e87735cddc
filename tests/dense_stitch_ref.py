"""float64 reference of the window stitch (csrc/dense_stitch.hip, ops.dense_stitch), written with index arithmetic of its own on
the `_axis` form of tests/dense_ref.py - not with F.interpolate, which tests/test_dense_stitch_ref_cpu.py holds it against - the
seeded cases the CPU and GPU tests share, and the planted faults the label comparison must see.

Per window k in ascending order: the window-local bilinear sample of every class map (align_corners=False, the y axis over the
box's height, the x axis over its width) is added to float64 sums where the box lies inside the picture, and an integer count is
raised there; u = sums / count, conf = max_c u, label = the lowest arg-max, 255 below min_conf and where no window covers the
pixel (conf 0 there).  A box with a side outside [1, 16384] covers nothing.  The label comparison is dense_ref.compare_labels with
its FRAGILE = 1e-5 and CONF_TOL = 1e-6: the stitched value is a mean of samples <= 1, its fp32 error no larger than one sample's
plus the adds' (test_dense_stitch_gpu.py works the figure out)."""
from __future__ import annotations

import torch

from dense_ref import CONF_TOL, FRAGILE, NONE_LABEL, _axis, compare_labels  # noqa: F401  (re-exported for the tests)

MAX_SIDE = 16384
FAULTS = ("global", "nodiv", "rowcount", "x1incl")


def upsample_hw(maps: torch.Tensor, h: int, w: int, rows=None, cols=None) -> torch.Tensor:
    """[..., g, g] -> float64 [..., h, w] (or only the output rows / columns in the slices `rows`, `cols`): bilinear, half-pixel
    centres, source index clamped at 0, each axis with its own scale g / h, g / w."""
    m = maps.double()
    g = m.shape[-1]
    y0, y1, wy = (t[rows if rows is not None else slice(None)] for t in _axis(h, g))
    x0, x1, wx = (t[cols if cols is not None else slice(None)] for t in _axis(w, g))
    r = m[..., y0, :] * (1 - wy)[:, None] + m[..., y1, :] * wy[:, None]
    return r[..., :, x0] * (1 - wx) + r[..., :, x1] * wx


def _valid(x0, y0, x1, y1) -> bool:
    return 1 <= x1 - x0 <= MAX_SIDE and 1 <= y1 - y0 <= MAX_SIDE


def stitch_ref(probs: torch.Tensor, boxes, H: int, W: int, min_conf: float = 0.0, fault: str = None) -> dict:
    """probs [K, C, g, g], boxes [K, 4] (x0, y0, x1, y1) -> the dict compare_labels takes (labels, conf, arg, second, margin,
    min_conf) plus cover int64 [H, W] and up float64 [C, H, W].  `fault` plants one of FAULTS (CPU test only)."""
    assert fault is None or fault in FAULTS
    K, C, g, _ = probs.shape
    sums = torch.zeros(C, H, W, dtype=torch.float64)
    count = torch.zeros(H, W, dtype=torch.int64)
    for k in range(K):
        x0, y0, x1, y1 = (int(v) for v in boxes[k])
        if fault == "x1incl":
            x1 += 1
        if not _valid(x0, y0, x1, y1):
            continue
        xa, xb, ya, yb = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
        if xa >= xb or ya >= yb:
            continue
        if fault == "global":                                   # the map stretched over the picture, not over its window
            up = upsample_hw(probs[k], H, W, slice(ya, yb), slice(xa, xb))
        else:
            up = upsample_hw(probs[k], y1 - y0, x1 - x0, slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))
        sums[:, ya:yb, xa:xb] += up
        if fault == "rowcount":
            count[ya:yb, :] += 1
        else:
            count[ya:yb, xa:xb] += 1
    covered = count > 0
    u = sums if fault == "nodiv" else sums / count.clamp_min(1).double()
    conf, arg = u.max(dim=0)
    if C > 1:
        masked = u.scatter(0, arg[None], float("-inf"))
        second_v, second = masked.max(dim=0)
        margin = conf - second_v
    else:
        second, margin = arg.clone(), torch.full_like(conf, float("inf"))
    none = torch.full_like(arg, NONE_LABEL)
    conf = torch.where(covered, conf, torch.zeros_like(conf))
    arg, second = torch.where(covered, arg, none), torch.where(covered, second, none)       # an uncovered pixel has no class
    margin = torch.where(covered, margin, torch.full_like(margin, float("inf")))
    labels = torch.where(conf < min_conf, none, arg)
    return dict(labels=labels, conf=conf, arg=arg, second=second, margin=margin, min_conf=float(min_conf), up=u, cover=count)


def conf_ok(got_conf: torch.Tensor, ref: dict, tol: float = CONF_TOL) -> bool:
    return (got_conf.double().cpu() - ref["conf"]).abs().max().item() <= tol


def fragile_share(ref: dict, fragile: float = FRAGILE, conf_tol: float = CONF_TOL) -> float:
    """the reference's own share of pixels where fp32 may decide either way: margin in (0, fragile), or conf near min_conf"""
    frag = (ref["margin"] > 0) & (ref["margin"] < fragile)
    near = (ref["conf"] - ref["min_conf"]).abs() < conf_tol
    if ref["min_conf"] == 0.0:
        near = near & (ref["cover"] > 0)                        # conf 0 of an uncovered pixel is exact, not near a threshold
    return float((frag | near).double().mean())


# (W, H, window, stride, g, C): odd widths and widths that are no multiple of 4 (row starts mid-dword), a partial last group
STITCH_CASES = [(37, 23, 16, 8, 2, 3), (50, 31, 20, 10, 3, 2), (97, 64, 32, 16, 7, 5), (13, 9, 9, 4, 1, 4), (160, 100, 48, 32, 24, 9)]


def stitch_maps(K: int, C: int, g: int, seed: int = 0) -> torch.Tensor:
    """fp32 [K, C, g, g]: a softmax over classes of 3 * randn, generator seed 3000 + seed"""
    gen = torch.Generator().manual_seed(3000 + seed)
    return (3.0 * torch.randn(K, C, g, g, generator=gen)).softmax(dim=1).contiguous()


def stitch_case(case, seed: int = None):
    """(probs fp32 [K, C, g, g], boxes int64 tensor [K, 4], H, W) of one of STITCH_CASES; the seed defaults to its index"""
    from clip.dense import plan_windows
    W, H, window, stride, g, C = case
    boxes = torch.from_numpy(plan_windows(W, H, window, stride))
    seed = STITCH_CASES.index(tuple(case)) if seed is None else seed
    return stitch_maps(boxes.shape[0], C, g, seed), boxes, H, W
