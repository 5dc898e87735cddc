"""Host reference of csrc/label_components.hip: connected components of uint8 label maps by plain breadth-first flood fill, in
numpy / Python.  It shares no code with clip.label_boxes (row runs + union-find), which the CPU tests compare it with.

components(labels [B, H, W] or [H, W], conf=None, connectivity=4) -> dict of numpy arrays
    root  int32, the labels' shape: the flat index (b H + y) W + x of the component's first pixel in row-major order, -1 at 255
    ids   int32, the labels' shape: 0 .. n - 1 in ascending order of root, -1 at 255
    n, label uint8 [n], image int32 [n], first int32 [n], area int32 [n], boxes int32 [n, 4] (x0, y0, x1, y1 half-open, image
    coordinates), qsum uint64 [n] (None without conf): the sum of q(conf) over the pixels,
    q(v) = (v >= 0) ? min(65536, (uint32)(v * 65536.0f + 0.5f)) : 0, NaN -> 0, every operation in np.float32.

Pixels are visited in row-major order and a fill starts at the first pixel not yet reached, so components come out in ascending
order of their first pixel: the visiting order IS the numbering.

Also the maps of the tests (MAPS: name -> uint8 [H, W]; BATCHES: name -> uint8 [B, H, W]), the smallest at which each mechanism of
the kernels (32 x 32 tiles, four pixels per thread, groups of 1024 flat pixels) can go wrong.
"""
from __future__ import annotations

from collections import deque

import numpy as np

NONE = 255
NEIGHBOURS = {4: ((0, -1), (0, 1), (-1, 0), (1, 0)),
              8: ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def quantise(conf) -> np.ndarray:
    """q(v) of the header, elementwise, as uint64"""
    v = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(65536.0) + np.float32(0.5)                # two fp32 operations, each rounded once
        assert t.dtype == np.float32
        t = np.minimum(t, np.float32(65536.0))                      # the min, before the cast (every value past it truncates to it)
        ok = v >= np.float32(0.0)                                    # False for NaN
    return np.where(ok, np.where(ok, t, np.float32(0.0)).astype(np.uint64), np.uint64(0))


def components(labels, conf=None, connectivity: int = 4) -> dict:
    lab = np.asarray(labels)
    assert lab.dtype == np.uint8 and lab.ndim in (2, 3) and connectivity in NEIGHBOURS
    shape = lab.shape
    lab3 = lab.reshape((-1,) + shape[-2:])
    B, H, W = lab3.shape
    q = None if conf is None else quantise(conf).reshape(lab3.shape)
    root = np.full((B, H, W), -1, dtype=np.int32)
    ids = np.full((B, H, W), -1, dtype=np.int32)
    label, image, first, area, boxes, qsum = [], [], [], [], [], []
    steps = NEIGHBOURS[connectivity]
    for b in range(B):
        img = lab3[b]
        for y in range(H):
            for x in range(W):
                c = img[y, x]
                if c == NONE or ids[b, y, x] >= 0:
                    continue
                i, start = len(label), (b * H + y) * W + x
                ids[b, y, x] = i
                queue = deque([(y, x)])
                n, x0, y0, x1, y1, s = 0, x, y, x + 1, y + 1, 0
                while queue:
                    py, px = queue.popleft()
                    root[b, py, px] = start
                    n += 1
                    x0, y0, x1, y1 = min(x0, px), min(y0, py), max(x1, px + 1), max(y1, py + 1)
                    if q is not None:
                        s += int(q[b, py, px])
                    for dy, dx in steps:
                        ny, nx = py + dy, px + dx
                        if 0 <= ny < H and 0 <= nx < W and img[ny, nx] == c and ids[b, ny, nx] < 0:
                            ids[b, ny, nx] = i
                            queue.append((ny, nx))
                label.append(c); image.append(b); first.append(start); area.append(n); boxes.append((x0, y0, x1, y1)); qsum.append(s)
    return dict(root=root.reshape(shape), ids=ids.reshape(shape), n=len(label), label=np.array(label, dtype=np.uint8),
                image=np.array(image, dtype=np.int32), first=np.array(first, dtype=np.int32), area=np.array(area, dtype=np.int32),
                boxes=np.array(boxes, dtype=np.int32).reshape(-1, 4), qsum=None if q is None else np.array(qsum, dtype=np.uint64))


def boxes_of(ref: dict, c: int, min_area: int = 1, image: int = 0):
    """the reference's boxes of class c in one image, as clip.label_boxes lists them"""
    keep = (ref["label"] == c) & (ref["image"] == image) & (ref["area"] >= min_area)
    return [tuple(int(v) for v in b) for b in ref["boxes"][keep]]


def instances(ref: dict, class_names=None, min_area: int = 1, min_score: float = 0.0):
    """the records ComponentsResult.instances makes, from the reference (score = qsum / (65536 area) in fp64)"""
    out = []
    for i in range(ref["n"]):
        score = None if ref["qsum"] is None else float(np.float64(ref["qsum"][i]) / (65536.0 * np.float64(ref["area"][i])))
        if ref["area"][i] < min_area or (score is not None and score < min_score):
            continue
        c = int(ref["label"][i])
        out.append({"image": int(ref["image"][i]), "class": c, "name": None if class_names is None else class_names[c],
                    "box": tuple(int(v) for v in ref["boxes"][i]), "area": int(ref["area"][i]), "score": score})
    return out


# ---- the maps --------------------------------------------------------------------------------------
def _random(H, W, values, seed, p=None):
    return np.random.RandomState(seed).choice(np.array(values, dtype=np.uint8), size=(H, W), p=p).astype(np.uint8)


def spiral(H, W, inside=0, outside=NONE):
    """a one-pixel-wide rectangular spiral of `inside` from the top-left corner inwards, its turns two pixels apart"""
    m = np.full((H, W), outside, dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = inside
    while True:
        steps = 0
        while True:                               # straight on until the edge, or until the cell after the next is the spiral itself
            ny, nx = y + dy, x + dx
            if not (0 <= ny < H and 0 <= nx < W):
                break
            ay, ax = ny + dy, nx + dx
            if 0 <= ay < H and 0 <= ax < W and m[ay, ax] == inside:
                break
            y, x = ny, nx
            m[y, x] = inside
            steps += 1
        if steps == 0:
            return m
        dy, dx = dx, -dy                          # turn right


def arms(H=70, W=70):
    """two vertical arms of label 0 joined only along the bottom row, the right arm starting higher than the left: the root of the
    whole is the right arm's top, which the left arm's pixels learn of late"""
    m = np.full((H, W), NONE, dtype=np.uint8)
    m[20:, 5] = 0
    m[3:, 60] = 0
    m[H - 1, 5:61] = 0
    return m


def nested(H=50, W=75):
    """a label-1 region enclosing a label-0 island enclosing label 255, on a label-2 ground"""
    m = np.full((H, W), 2, dtype=np.uint8)
    m[4:46, 6:70] = 1
    m[12:40, 20:60] = 0
    m[20:30, 30:50] = NONE
    return m


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) & 1).astype(np.uint8)


MAPS = {
    "pixel_1x1": np.zeros((1, 1), dtype=np.uint8),
    "row_1x70": _random(1, 70, [0, 1, NONE], 1),
    "column_70x1": _random(70, 1, [0, 1, NONE], 2),
    "edge_33x65": _random(33, 65, [0, 1, NONE], 3),
    "edge_31x32": _random(31, 32, [0, 1, NONE], 4),
    "edge_64x97": _random(64, 97, [0, 1, NONE], 5),
    "one_class_97x130": np.full((97, 130), 3, dtype=np.uint8),
    "checkerboard_66x70": checkerboard(66, 70),
    "spiral_129x129": spiral(129, 129),
    "arms_70x70": arms(),
    "percolation_130x257": _random(130, 257, [0, NONE], 6, p=[0.6, 0.4]),
    "three_class_130x257": _random(130, 257, [0, 1, 2], 7),
    "nested_50x75": nested(),
}
RANDOM_MAPS = ("edge_33x65", "edge_31x32", "edge_64x97", "percolation_130x257", "three_class_130x257")


def _three_different():
    a = _random(33, 65, [0, 1, NONE], 8)
    b = _random(33, 65, [0, 1, NONE], 9)
    c = _random(33, 65, [0, 1, NONE], 10)
    a[-1, :] = 1; b[0, :] = 1                     # the last row of an image and the first of the next share a label on purpose
    b[-1, :] = 0; c[0, :] = 0
    return np.stack([a, b, c])


def _three_same():
    a = MAPS["edge_33x65"].copy()
    a[-1, :] = 1; a[0, :] = 1
    return np.stack([a, a, a])


BATCHES = {"same_3x33x65": _three_same(), "different_3x33x65": _three_different()}


def confidences(shape, seed=0) -> np.ndarray:
    """fp32 in [0, 1] with the values that sit on the edges of q() planted at fixed places"""
    conf = np.random.RandomState(100 + seed).random_sample(shape).astype(np.float32)
    flat = conf.reshape(-1)
    special = [0.0, 1.0, 0.5 - 2.0 ** -25, 1.0 + 1e-3, -0.25, np.nan, np.inf, 2.0 ** -17, 1.0 - 2.0 ** -24]
    for k, v in enumerate(special):
        flat[(k * 7) % flat.size] = np.float32(v)
    return conf
