"""CPU: the host reference of the label-agreement counts (tests/label_agreement_ref.py) pinned to cases that can be counted by
hand, the arithmetic of clip.SegmentationScores from hand-written count tensors, and the declarations the feature adds (header,
ops constant, library symbol, clip's names, the script's options)."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import label_agreement_ref as AR  # noqa: E402

N = AR.NONE


# ---- the reference ----------------------------------------------------------------------------------
def test_equal_maps_give_a_diagonal_and_ious_of_one():
    rng = np.random.default_rng(0)
    gt = rng.integers(0, 4, (2, 17, 23)).astype(np.uint8)
    for per_image in (False, True):
        c = AR.counts(gt, gt, 4, 2, per_image)
        for r in range(c["confusion"].shape[0]):
            conf, bands = c["confusion"][r], c["bands"][r]
            assert np.array_equal(conf[:, :4], np.diag(np.diagonal(conf))) and not conf[:, 4].any()
            assert np.array_equal(bands[:, 0], bands[:, 1]) and np.array_equal(bands[:, 0], bands[:, 2])
            s = AR.scores(conf, bands)
            assert s["iou"].tolist() == [1.0] * 4 and s["boundary_iou"].tolist() == [1.0] * 4
            assert s["miou"] == 1.0 and s["mean_boundary_iou"] == 1.0 and s["pixel_accuracy"] == 1.0 and s["fw_iou"] == 1.0
        assert int(c["confusion"].sum()) == gt.size and not c["bad"].any()


GT_4x4 = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [N, 0, 0, 1]], dtype=np.uint8)
PRED_4x4 = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, N], [0, 0, 0, 1]], dtype=np.uint8)


def test_a_written_out_4x4_case():
    """d = 1: the twelve frame pixels are in both bands; of the inner four, gt's band holds (2, 1) (the 255 at (3, 0) is in its
    window) and (2, 2) (the 1 at (3, 3)), pred's band all four.  Counted by hand:
      gt == 0: 14 pixels, labelled 0 / 1 / none 9 / 4 / 1 times; gt == 1: one pixel, labelled 1; (3, 0) is ignored
      G_0 = 14 - 2 = 12, P_0 = 10 - 1 (ignored) = 9, I_0 = 9 - 1 ((1, 1) is not in G) = 8; G_1, P_1, I_1 = 1, 5, 1"""
    assert AR.band_mask(GT_4x4, 1).tolist() == [[True] * 4, [True, False, False, True], [True] * 4, [True] * 4]
    assert AR.band_mask(PRED_4x4, 1).all()
    c = AR.counts(PRED_4x4[None], GT_4x4[None], 2, 1)
    assert c["confusion"].tolist() == [[[9, 4, 1], [0, 1, 0]]]
    assert c["bands"].tolist() == [[[12, 9, 8], [1, 5, 1]]]
    assert c["bad"].tolist() == [[0, 0]]
    s = AR.scores(c["confusion"][0], c["bands"][0])
    assert s["iou"].tolist() == [9 / 14, 1 / 5] and s["boundary_iou"].tolist() == [8 / 13, 1 / 5]
    assert s["pixel_accuracy"] == 10 / 15 and s["none_fraction"] == 1 / 15
    assert s["class_accuracy"].tolist() == [9 / 14, 1.0] and s["precision"].tolist() == [1.0, 1 / 5]
    assert s["miou"] == math.fsum([9 / 14, 1 / 5]) / 2
    assert s["fw_iou"] == math.fsum([14 * (9 / 14), 1 * (1 / 5)]) / 15
    assert AR.counts(PRED_4x4[None], GT_4x4[None], 2, 0)["bands"] is None


def test_a_band_as_wide_as_the_image_holds_every_pixel():
    pred, gt = AR.blocky(1, 9, 13, 3, seed=3, block=4)
    for d in (13, 32):
        c = AR.counts(pred, gt, 3, d)
        conf, bands = c["confusion"][0], c["bands"][0]
        assert np.array_equal(bands[:, 0], conf.sum(axis=1))                   # G_c: the row sum
        assert np.array_equal(bands[:, 1], conf[:, :3].sum(axis=0))            # P_c: the valid column sum
        assert np.array_equal(bands[:, 2], np.diagonal(conf[:, :3]))           # I_c: the diagonal
    assert AR.band_mask(gt[0], 13).all()


def test_one_class_has_the_one_pixel_frame_as_its_band():
    m = np.full((7, 11), 2, dtype=np.uint8)
    want = np.ones((7, 11), dtype=bool)
    want[1:-1, 1:-1] = False
    assert np.array_equal(AR.band_mask(m, 1), want)
    c = AR.counts(m[None], m[None], 3, 1)
    assert c["bands"][0].tolist() == [[0, 0, 0], [0, 0, 0], [32, 32, 32]] and c["confusion"][0, 2, 2] == 77
    u = AR.counts(np.zeros((1, 130, 130), np.uint8), np.zeros((1, 130, 130), np.uint8), 2, 32)
    assert u["bands"][0, 0].tolist() == [130 * 130 - 66 * 66] * 3


def test_ignored_none_and_out_of_range_pixels_land_where_the_definition_says():
    gt = np.array([[0, 1, N, 5, 0, 1]], dtype=np.uint8)[None]
    pred = np.array([[N, 1, 0, 0, 7, 254]], dtype=np.uint8)[None]
    c = AR.counts(pred, gt, 2, 1)
    assert c["confusion"].tolist() == [[[0, 0, 1], [0, 1, 0]]]                  # (gt 0, none) and (gt 1, pred 1)
    assert c["bad"].tolist() == [[1, 2]]                                        # gt 5; pred 7 and 254 under a valid gt
    assert c["bands"].tolist() == [[[1, 0, 0], [1, 1, 1]]]                      # every pixel of a 1 x 6 image is in the band
    both = AR.counts(np.concatenate([pred, pred]), np.concatenate([gt, gt]), 2, 1, per_image=True)
    assert both["confusion"].shape == (2, 2, 3) and np.array_equal(both["confusion"].sum(axis=0), 2 * c["confusion"][0])


def test_the_case_table_is_what_the_gpu_test_expects():
    assert len(AR.CASES) == 1 + 2 + 27 + 3 + 1 + 1 + 1 + 3 + 1 + 1
    for name, (pred, gt, C, d) in AR.CASES.items():
        assert pred.shape == gt.shape and pred.ndim == 3 and pred.dtype == np.uint8 and gt.dtype == np.uint8, name
        assert 1 <= C <= 255 and 0 <= d <= 32
    for C in (43, 44, 45):
        c = AR.counts(*AR.CASES[f"pairs_C{C}_d1"][:2], C, 0)
        assert (c["confusion"] > 0).all() and not c["bad"].any()
    p, g, C, d = AR.CASES["C255_20x67_d2"]
    assert set(np.unique(g).tolist()) == set(range(255)) and set(np.unique(p).tolist()) == set(range(256))
    p, g, C, d = AR.CASES["bad_2x33x70_d2"]
    assert (AR.counts(p, g, C, 0)["bad"] > 0).all()
    p, g, C, d = AR.CASES["stairs_131x135_d32"]
    assert g[0, 0, 63] != g[0, 0, 64] and g[0, 0, 95] != g[0, 0, 96] and g[0, 0, 96] != g[0, 0, 97] and g[0, 63, 0] != g[0, 64, 0]
    p, g, _, _ = AR.CASES["batch_3x40x70_d2"]
    assert all((g[b, -1] == g[b + 1, 0]).all() for b in range(2))
    assert AR.default_band(1080, 1920) == 32 and AR.default_band(64, 96) == 2 and AR.default_band(5, 7) == 1 and AR.default_band(224, 224) == 6


# ---- SegmentationScores -------------------------------------------------------------------------------
def _t(x):
    return torch.tensor(x, dtype=torch.int64)


def test_scores_from_hand_written_counts():
    import clip
    s = clip.SegmentationScores(_t([[9, 4, 1], [0, 1, 0]]), _t([[12, 9, 8], [1, 5, 1]]), band=1, class_names=["a", "b"])
    assert s.n_classes == 2 and not s.per_image and s.band == 1 and s.class_names == ["a", "b"]
    assert s.iou.dtype == torch.float64 and s.iou.tolist() == [9 / 14, 1 / 5]
    assert s.boundary_iou.tolist() == [8 / 13, 1 / 5] and s.mean_boundary_iou == math.fsum([8 / 13, 1 / 5]) / 2
    assert s.miou == math.fsum([9 / 14, 1 / 5]) / 2 and s.pixel_accuracy == 10 / 15 and s.none_fraction == 1 / 15
    assert s.class_accuracy.tolist() == [9 / 14, 1.0] and s.precision.tolist() == [1.0, 1 / 5]
    assert s.fw_iou == math.fsum([14 * (9 / 14), 1 / 5]) / 15
    ref = AR.scores(np.array([[9, 4, 1], [0, 1, 0]]), np.array([[12, 9, 8], [1, 5, 1]]))
    for k, v in ref.items():
        got = getattr(s, k)
        assert (got.tolist() if isinstance(got, torch.Tensor) else got) == (v.tolist() if isinstance(v, np.ndarray) else v), k


def test_nan_rules():
    import clip
    s = clip.SegmentationScores(_t([[5, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 3]]), _t([[2, 2, 2], [0, 0, 0], [1, 0, 0]]), band=3)
    iou = s.iou.tolist()
    assert iou[0] == 1.0 and math.isnan(iou[1]) and iou[2] == 0.0              # class 1: empty union -> NaN, left out of the mean
    assert s.miou == 0.5 and s.pixel_accuracy == 5 / 8 and s.none_fraction == 3 / 8
    assert math.isnan(s.class_accuracy[1]) and math.isnan(s.precision[1]) and math.isnan(s.precision[2])
    b = s.boundary_iou.tolist()
    assert b[0] == 1.0 and math.isnan(b[1]) and b[2] == 0.0 and s.mean_boundary_iou == 0.5
    assert s.fw_iou == (5 * 1.0 + 3 * 0.0) / 8
    empty = clip.SegmentationScores(torch.zeros(2, 3, dtype=torch.int64))
    assert math.isnan(empty.miou) and math.isnan(empty.pixel_accuracy) and math.isnan(empty.fw_iou) and math.isnan(empty.none_fraction)
    assert empty.boundary_iou is None and empty.mean_boundary_iou is None and empty.bands is None and empty.band == 0
    d = s.as_dict()
    assert d["iou"] == [1.0, None, 0.0] and d["miou"] == 0.5 and d["band"] == 3 and d["n_classes"] == 3 and d["pixels"] == 8
    assert json.loads(json.dumps(d)) == d and all(isinstance(v, (float, int, list, type(None))) for v in d.values())
    assert empty.as_dict()["miou"] is None and empty.as_dict()["boundary_iou"] is None


def test_sums_totals_and_mismatches():
    import clip
    a = clip.SegmentationScores(_t([[9, 4, 1], [0, 1, 0]]), _t([[12, 9, 8], [1, 5, 1]]), band=1)
    b = clip.SegmentationScores(_t([[1, 0, 0], [2, 3, 4]]), _t([[1, 1, 1], [4, 3, 2]]), band=1, class_names=["x", "y"])
    c = a + b
    assert c.confusion.tolist() == [[10, 4, 1], [2, 4, 4]] and c.bands.tolist() == [[13, 10, 9], [5, 8, 3]] and c.class_names == ["x", "y"]
    assert a.confusion.tolist() == [[9, 4, 1], [0, 1, 0]]                       # + leaves its operands
    assert c.iou.tolist() == [10 / (15 + 12 - 10), 4 / (10 + 8 - 4)]
    a2 = clip.SegmentationScores(a.confusion, a.bands, 1)
    a2 += b
    assert a2.confusion.tolist() == c.confusion.tolist() and a2.bands.tolist() == c.bands.tolist()
    per = clip.SegmentationScores(torch.stack([a.confusion, b.confusion]), torch.stack([a.bands, b.bands]), band=1)
    assert per.per_image and per.iou.shape == (2, 2) and per.miou.shape == (2,) and per.pixel_accuracy.shape == (2,)
    assert per.iou[0].tolist() == a.iou.tolist() and float(per.miou[1]) == b.miou and float(per.fw_iou[0]) == a.fw_iou
    assert float(per.mean_boundary_iou[1]) == b.mean_boundary_iou and per.boundary_iou[1].tolist() == b.boundary_iou.tolist()
    tot = per.total()
    assert not tot.per_image and tot.confusion.tolist() == c.confusion.tolist() and tot.bands.tolist() == c.bands.tolist()
    assert per.as_dict()["miou"] == [a.miou, b.miou] and per.as_dict()["pixels"] == [15, 10]
    for other, match in ((clip.SegmentationScores(torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), 1), "2 classes against 3"),
                         (clip.SegmentationScores(a.confusion, a.bands, 2), "band 1 against band 2"),
                         (clip.SegmentationScores(a.confusion), "band 1 against band 0"),
                         (per, "take .total")):
        with pytest.raises(ValueError, match=match):
            a + other
        with pytest.raises(ValueError, match=match):
            a2 += other
    for bad in (lambda: clip.SegmentationScores(torch.zeros(2, 2, dtype=torch.int64)),
                lambda: clip.SegmentationScores(torch.zeros(2, 3)),
                lambda: clip.SegmentationScores(a.confusion, a.bands),                       # bands without a band
                lambda: clip.SegmentationScores(a.confusion, None, 2),
                lambda: clip.SegmentationScores(a.confusion, torch.zeros(3, 3, dtype=torch.int64), 1),
                lambda: clip.SegmentationScores(a.confusion, class_names=["one"])):
        with pytest.raises(ValueError, match="SegmentationScores"):
            bad()


# ---- declarations -------------------------------------------------------------------------------------
def test_header_ops_library_and_names():
    text = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    assert re.search(r"#define\s+CCLIP_ABI_VERSION\s+3\b", text)
    assert re.search(r"\bint\s+cclip_label_agreement\s*\(const uint8_t\*\s*pred,\s*const uint8_t\*\s*gt,", text)
    band = re.search(r"#define\s+CCLIP_AGREEMENT_MAX_BAND\s+(\d+)", text)
    cells = re.search(r"#define\s+CCLIP_AGREEMENT_HIST_CELLS\s+(\d+)", text)
    import clip
    import cclip_hip
    from cclip_hip import ops
    from cclip_hip._lib import ABI_VERSION
    assert ABI_VERSION == 3 and int(band.group(1)) == ops.AGREEMENT_MAX_BAND == 32
    assert int(cells.group(1)) == ops.AGREEMENT_HIST_CELLS == AR.HIST_CELLS
    assert hasattr(cclip_hip.load_library(), "cclip_label_agreement")
    assert callable(clip.evaluate_labels) and isinstance(clip.SegmentationScores, type) and callable(ops.label_agreement)
    for cls in (clip.DenseResult, clip.PhotoDenseResult, clip.RefinedDenseResult):
        assert callable(cls.evaluate)
    import clip.dense as D
    for hw in ((1080, 1920), (64, 96), (5, 7), (224, 224), (1, 1), (3024, 4032)):
        assert D.default_band(*hw) == AR.default_band(*hw)


def test_cpu_tensors_are_refused():
    import clip
    from cclip_hip import ops
    lab = torch.zeros(1, 4, 5, dtype=torch.uint8)
    out = torch.zeros(1, 2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="label_agreement: pred must be a cuda tensor"):
        ops.label_agreement(lab, lab, 2, 0, out, torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="evaluate_labels: pred must be a cuda tensor"):
        clip.evaluate_labels(lab, lab, 2)


def test_script_options_parse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_segmentation.py"), "--synthetic", "--help"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    for opt in ("--images", "--masks", "--classes", "--mode", "--window", "--stride", "--max-side", "--min-conf", "--band", "--refine",
                "--synthetic"):
        assert opt in r.stdout, opt
