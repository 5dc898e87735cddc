"""Host reference of cclip_dense_prototypes (include/cclip_hip.h): masked average pooling of per-patch features into class
prototypes, restated in numpy with explicit index arithmetic.  Counts are integers, the weight is the one fp32 division of the
contract restated bit for bit (np.float32(count) / np.float32(area)), the sums are float64.  `reference` also returns what the
tests' bounds need (sum of w |f^| per element, sum of w per class) and can plant one fault at a time (`fault=`), so that the CPU
test can show the bounds trip on each.  CASES holds the case table the GPU test runs."""
from __future__ import annotations

import numpy as np

MAX_SIDE = 16384                 # CCLIP_OVERLAY_MAX_SIDE
SLAB = 64                        # CCLIP_PROTOTYPES_SLAB
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FAULTS = ("drop_cell", "floor_rule", "strict", "no_area", "slab_twice")


def valid_window(box, b, B) -> bool:
    x0, y0, x1, y1 = (int(v) for v in box)                 # Python integers: no overflow
    return 1 <= x1 - x0 <= MAX_SIDE and 1 <= y1 - y0 <= MAX_SIDE and 0 <= int(b) < B


def cell_of(u: np.ndarray, side: int, g: int, fault=None) -> np.ndarray:
    """the cell of pixel offsets u along a side of `side` pixels: the pixel-centre rule"""
    u = u.astype(np.int64)
    if fault == "floor_rule":
        return (u * g) // side
    return ((2 * u + 1) * g) // (2 * side)


def reference(feat, masks, boxes, g, C, min_share8, image=None, fault=None) -> dict:
    """feat fp32 [K g g, E], masks uint8 [B, H, W], boxes int [K, 4], image int [K] or None -> dict of
    sums float64 [C, E], weight float64 [C], patches / pixels int64 [C], bad int64 [1], mag float64 [C, E] = sum of w |f^|."""
    feat = np.asarray(feat, dtype=np.float32)
    K, E = feat.shape[0] // (g * g), feat.shape[1]
    B, H, W = masks.shape
    out = dict(sums=np.zeros((C, E)), weight=np.zeros(C), patches=np.zeros(C, np.int64), pixels=np.zeros(C, np.int64),
               bad=np.zeros(1, np.int64), mag=np.zeros((C, E)))
    f64 = feat.astype(np.float64)
    norm = np.sqrt((f64 * f64).sum(axis=1))
    unit = np.where(norm[:, None] > 0, f64 / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
    dropped = False
    for k in range(K):
        b = 0 if image is None else int(image[k])
        if not valid_window(boxes[k], b, B):
            continue
        x0, y0, x1, y1 = (int(v) for v in boxes[k])
        w, h = x1 - x0, y1 - y0
        cj, ci = cell_of(np.arange(w), w, g, fault), cell_of(np.arange(h), h, g, fault)
        area = np.outer(np.bincount(ci, minlength=g), np.bincount(cj, minlength=g)).astype(np.int64)      # [i][j], box pixels
        xs, ys = x0 + np.arange(w, dtype=np.int64), y0 + np.arange(h, dtype=np.int64)
        inx, iny = (xs >= 0) & (xs < W), (ys >= 0) & (ys < H)
        count = np.zeros((g * g, 256), np.int64)
        if inx.any() and iny.any():
            sub = masks[b][np.ix_(ys[iny], xs[inx])].astype(np.int64)
            cell = ci[iny][:, None] * g + cj[inx][None, :]
            count = np.bincount((cell * 256 + sub).ravel(), minlength=g * g * 256).reshape(g * g, 256)
        out["bad"][0] += count[:, C:255].sum()
        out["pixels"] += count[:, :C].sum(axis=0)
        for p in range(g * g):
            a = int(area[p // g, p % g])
            if a == 0:
                continue
            row = k * g * g + p
            for c in np.flatnonzero(count[p, :C]):
                n = int(count[p, c])
                passes = 256 * n > min_share8 * a if fault == "strict" else 256 * n >= min_share8 * a
                if not passes:
                    continue
                if fault == "drop_cell" and not dropped:
                    dropped = True
                    continue
                wt = float(n) if fault == "no_area" else float(np.float32(n) / np.float32(a))
                times = 2 if fault == "slab_twice" and row < SLAB else 1
                out["sums"][c] += times * wt * unit[row]
                out["mag"][c] += wt * np.abs(unit[row])
                out["weight"][c] += times * wt
                out["patches"][c] += 1
    return out


def sums_bound(ref, n=None) -> np.ndarray:
    """[C, E]: 2^-24 (n_c + E / 2 + 8) sum_p w |f^| + 1e-30 - n_c summation roundings, E / 2 for the sum of squares under the root,
    8 for the weight, reciprocal, product and one accumulate add"""
    n = ref["patches"] if n is None else n
    E = ref["sums"].shape[1]
    return 2.0 ** -24 * (n[:, None] + E / 2 + 8) * ref["mag"] + 1e-30


def weight_bound(ref, n=None) -> np.ndarray:
    n = ref["patches"] if n is None else n
    return 2.0 ** -24 * (n + 2) * ref["weight"]


def within(got_sums, got_weight, ref, n=None) -> bool:
    return bool((np.abs(got_sums.astype(np.float64) - ref["sums"]) <= sums_bound(ref, n)).all() and
                (np.abs(got_weight.astype(np.float64) - ref["weight"]) <= weight_bound(ref, n)).all())


# ---- the case table -----------------------------------------------------------------------------------
def _feat(rng, rows, E):
    return rng.standard_normal((rows, E)).astype(np.float32)


def _blocky(rng, B, H, W, C, block=3, ignore=0.1):
    """a mask of small blocks of classes with some ignored pixels"""
    m = rng.integers(0, C, size=(B, -(-H // block), -(-W // block)))
    m = np.repeat(np.repeat(m, block, axis=1), block, axis=2)[:, :H, :W].astype(np.uint8)
    m[rng.random((B, H, W)) < ignore] = 255
    return np.ascontiguousarray(m)


def _case(seed, g, C, E, masks, boxes, min_share8=128, image=None, ldf_pad=0, feat=None):
    rng = np.random.default_rng(seed)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    feat = _feat(rng, boxes.shape[0] * g * g, E) if feat is None else feat
    return dict(feat=feat, masks=masks, boxes=boxes, g=g, C=C, min_share8=min_share8, ldf_pad=ldf_pad,
                image=None if image is None else np.asarray(image, dtype=np.int64))


def _threshold_mask():
    """an 8 x 8 box at g = 2: four cells of area 16"""
    m = np.zeros((1, 8, 8), np.uint8)
    m[0, :4, :4] = np.array([0] * 8 + [1] * 8, np.uint8).reshape(4, 4)                  # count 8 of 16, twice
    m[0, :4, 4:] = 0
    m[0, 1, 6] = 1                                                                       # one stray pixel
    m[0, 4:, :4] = np.array([0] * 4 + [1] * 9 + [2] * 3, np.uint8).reshape(4, 4)         # 4, 9 and 3 of 16
    m[0, 4:, 4:] = 2
    return m


def _build_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    m12 = _blocky(rng, 1, 13, 15, 3)                                                     # odd W
    for side in (10, 3, 2, 1):
        cases[f"g3_side{side}"] = _case(side, 3, 3, 8, m12, [[2, 1, 2 + side, 1 + side]], min_share8=64)
    cases["g3_box10x7"] = _case(5, 3, 3, 8, m12, [[3, 2, 13, 9]], min_share8=64)
    cases["g1_side9"] = _case(6, 1, 3, 8, m12, [[1, 1, 10, 10]], min_share8=0)
    m230 = _blocky(rng, 1, 231, 233, 4, block=11)
    cases["g7_side224"] = _case(7, 7, 4, 16, m230, [[3, 2, 227, 226]])
    cases["g7_side225"] = _case(8, 7, 4, 16, m230, [[3, 2, 228, 227]])
    edge = [[-4, 2, 6, 12], [9, 2, 19, 12], [2, -5, 12, 5], [2, 8, 12, 18],              # over the left, right, top, bottom edge
            [40, 40, 50, 50], [-30, -30, -20, -20],                                      # wholly outside
            [3, 3, 3, 9], [8, 8, 4, 12],                                                 # empty, inverted
            [0, 0, MAX_SIDE + 1, 5], [0, 0, 5, MAX_SIDE + 1],                            # a side one past the cap
            [I32_MIN, I32_MIN, I32_MAX, I32_MAX], [I32_MAX, 0, I32_MIN, 4],              # sides that overflow 32 bits (the second wraps to 1)
            [I32_MAX - 5, 0, I32_MAX, 5], [I32_MIN, 0, I32_MIN + 4, 4], [-5, -5, I32_MAX, 3],
            [1, 1, 12, 11]]
    cases["boxes_edges"] = _case(9, 3, 3, 8, m12, edge, min_share8=32)
    cases["mask_values"] = _case(10, 3, 4, 8, np.ascontiguousarray(
        np.array([0, 1, 4, 254, 255, 3, 2, 200], np.uint8)[rng.integers(0, 8, size=(1, 11, 13))]), [[0, 0, 13, 11], [1, 2, 10, 11]], min_share8=16)
    cases["mask_all_ignore"] = _case(11, 3, 3, 8, np.full((1, 9, 11), 255, np.uint8), [[0, 0, 11, 9]], min_share8=0)
    for s8 in (128, 129, 0, 256, 64):
        cases[f"threshold_{s8}"] = _case(12, 2, 3, 8, _threshold_mask(), [[0, 0, 8, 8]], min_share8=s8)
    cases["C1"] = _case(13, 3, 1, 8, _blocky(rng, 1, 10, 11, 1), [[0, 0, 11, 10]])
    m255 = np.full((1, 12, 12), 255, np.uint8)
    m255[0, :4], m255[0, 4:8], m255[0, 8:, :6] = 0, 128, 254
    cases["C255"] = _case(14, 3, 255, 12, m255, [[0, 0, 12, 12]])
    for E in (4, 260, 512, 1024):
        cases[f"E{E}"] = _case(15 + E, 3, 3, E, m12, [[1, 1, 12, 11], [0, 2, 15, 13]], min_share8=64)
    cases["ldf_pad4"] = _case(16, 3, 3, 20, m12, [[1, 1, 12, 11]], min_share8=64, ldf_pad=4)
    m40 = _blocky(rng, 1, 41, 43, 3, block=2)
    cases["cells_63"] = _case(17, 3, 3, 8, m40, [[i, 2 * i, i + 12, 2 * i + 13] for i in range(7)], min_share8=64)
    cases["cells_64"] = _case(18, 8, 3, 8, m40, [[1, 2, 41, 40]], min_share8=64)
    cases["cells_65"] = _case(19, 1, 3, 8, m40, [[i % 13 * 3, i // 13 * 7, i % 13 * 3 + 4, i // 13 * 7 + 5] for i in range(65)], min_share8=64)
    last = np.zeros((1, 28, 28), np.uint8)
    last[0, :14] = 1
    last[0, 26:, 26:] = 2                                                                # class 2: the last cell of the last slab only
    cases["slabs_4_last_cell"] = _case(20, 14, 3, 8, last, [[0, 0, 28, 28]])
    cases["large_cell"] = _case(21, 2, 3, 8, _blocky(rng, 1, 305, 310, 3, block=37), [[4, 3, 304, 303]], min_share8=32)
    m2 = _blocky(rng, 2, 13, 15, 3)
    cases["batch_image_101"] = _case(22, 3, 3, 8, m2, [[1, 1, 12, 11], [0, 0, 15, 13], [4, 3, 13, 12]], image=[1, 0, 1], min_share8=64)
    cases["batch_image_bad"] = _case(23, 3, 3, 8, m2, [[1, 1, 12, 11], [0, 0, 15, 13], [4, 3, 13, 12]], image=[-1, 1, 2], min_share8=64)
    fz = _feat(np.random.default_rng(24), 9, 8)
    fz[4] = 0.0                                                                          # the centre cell's row
    cases["zero_row"] = _case(24, 3, 3, 8, m12, [[1, 1, 13, 13]], min_share8=0, feat=fz)
    cases["accumulate"] = _case(25, 3, 3, 12, m12, [[0, 0, 15, 13], [1, 1, 12, 11], [-3, 2, 9, 14], [5, 0, 14, 9], [2, 2, 8, 8], [7, 5, 15, 13]],
                                min_share8=64)
    return cases


CASES = _build_cases()
