"""CPU: the float64 reference of the window stitch (tests/dense_stitch_ref.py) against F.interpolate pasted and averaged,
`clip.plan_windows`, the planted faults the label comparison and the conf bound must see, the reference's own fragile share on
the shared cases, and the host-side functions of clip/dense.py that need no device."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_stitch_ref as SR  # noqa: E402

FRAGILE_CAP = 1e-3


def _pasted(probs, boxes, H, W):
    """F.interpolate of every window's maps to its own (h, w), pasted into float64 sums and averaged (boxes inside the picture)"""
    C = probs.shape[1]
    sums, count = torch.zeros(C, H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.float64)
    for k, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        up = F.interpolate(probs[k].double()[None], size=(y1 - y0, x1 - x0), mode="bilinear", align_corners=False)[0]
        sums[:, y0:y1, x0:x1] += up
        count[y0:y1, x0:x1] += 1
    return sums / count, count


@pytest.mark.parametrize("case", SR.STITCH_CASES)
def test_stitch_ref_is_interpolate_pasted_and_averaged(case):
    probs, boxes, H, W = SR.stitch_case(case)
    ref = SR.stitch_ref(probs, boxes, H, W)
    want, count = _pasted(probs, boxes, H, W)
    assert (ref["up"] - want).abs().max() < 1e-12
    assert torch.equal(ref["cover"], count.long()) and int(ref["cover"].min()) >= 1
    assert torch.equal(ref["labels"], want.argmax(dim=0))
    assert (ref["conf"] - want.max(dim=0).values).abs().max() < 1e-12
    assert SR.compare_labels(ref["labels"], ref)[0] == 0 and SR.conf_ok(ref["conf"], ref)


def test_stitch_ref_rectangles_holes_and_bad_boxes():
    probs = SR.stitch_maps(5, 3, 3, seed=7)
    # one rectangle over a non-square picture is F.interpolate to (H, W)
    ref = SR.stitch_ref(probs[:1], torch.tensor([[0, 0, 11, 6]]), 6, 11)
    want = F.interpolate(probs[:1].double(), size=(6, 11), mode="bilinear", align_corners=False)[0]
    assert (ref["up"] - want).abs().max() < 1e-12
    # a box hanging over the edge shows the part of its upsampled maps that lies inside; bad boxes change nothing
    boxes = torch.tensor([[-3, -2, 5, 4], [4, 1, 4, 5], [6, 5, 2, 1], [0, 0, 16385, 3], [7, 2, 13, 9]])
    ref = SR.stitch_ref(probs, boxes, 6, 11)
    up0 = F.interpolate(probs[0].double()[None], size=(6, 8), mode="bilinear", align_corners=False)[0]
    assert (ref["up"][:, 0:4, 0:5] - up0[:, 2:6, 3:8]).abs().max() < 1e-12
    assert torch.equal(ref["cover"], SR.stitch_ref(probs[[0, 4]], boxes[[0, 4]], 6, 11)["cover"])
    hole = ref["cover"] == 0
    assert hole.any() and (ref["labels"][hole] == SR.NONE_LABEL).all() and (ref["conf"][hole] == 0).all()
    assert SR.compare_labels(ref["labels"], ref)[0] == 0
    assert SR.compare_labels(torch.where(hole, torch.zeros_like(ref["labels"]), ref["labels"]), ref)[0] == int(hole.sum())


@pytest.mark.parametrize("fault", SR.FAULTS)
def test_planted_faults_are_seen(fault):
    """each fault fails the label comparison or the conf bound on at least one shared case"""
    seen = []
    for case in SR.STITCH_CASES:
        probs, boxes, H, W = SR.stitch_case(case)
        ref = SR.stitch_ref(probs, boxes, H, W)
        bad = SR.stitch_ref(probs, boxes, H, W, fault=fault)
        wrong = SR.compare_labels(bad["labels"], ref)[0]
        seen.append(wrong > 0 or not SR.conf_ok(bad["conf"], ref))
        print(f"fault {fault} {case}: wrong labels {wrong}, max |dconf| {(bad['conf'] - ref['conf']).abs().max().item():.3e}")
    assert any(seen), fault


@pytest.mark.parametrize("case", SR.STITCH_CASES)
def test_reference_fragile_share_is_capped(case):
    """the cap is a condition on the shared inputs, not a measurement: 0, 0, 0, 0 and 1.25e-4 on the five cases"""
    probs, boxes, H, W = SR.stitch_case(case)
    share = SR.fragile_share(SR.stitch_ref(probs, boxes, H, W))
    print(f"fragile share {case}: {share:.3e}")
    assert share <= FRAGILE_CAP


# ---- plan_windows ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,window,stride", [(37, 23, 16, 8), (50, 31, 20, 10), (97, 64, 32, 16), (13, 9, 9, 4), (160, 100, 48, 32),
                                                (4032, 3024, 224, None), (64, 72, 224, 112), (350, 100, 224, 112), (5, 5, 2, 1),
                                                (224, 224, 224, None)])
def test_plan_windows_covers_every_pixel_inside_the_photo(W, H, window, stride):
    import clip
    b = clip.plan_windows(W, H, window, stride)
    assert b.dtype == np.int64 and b.ndim == 2 and b.shape[1] == 4
    side = min(window, W, H)
    assert (b[:, 2] - b[:, 0] == side).all() and (b[:, 3] - b[:, 1] == side).all()          # squares
    assert b[:, :2].min() >= 0 and b[:, 2].max() == W and b[:, 3].max() == H                # inside, edge windows flush
    assert b[:, 0].min() == 0 and b[:, 1].min() == 0
    cover = np.zeros((H, W), dtype=np.int64)
    if H * W <= 1 << 16:
        for x0, y0, x1, y1 in b.tolist():
            cover[y0:y1, x0:x1] += 1
        assert cover.min() >= 1
    else:                                                                                    # separable: columns and rows
        cx, cy = np.zeros(W, dtype=bool), np.zeros(H, dtype=bool)
        for x0, y0, x1, y1 in b.tolist():
            cx[x0:x1], cy[y0:y1] = True, True
        assert cx.all() and cy.all()
        xs, ys = sorted(set(b[:, 0].tolist())), sorted(set(b[:, 1].tolist()))
        assert len(b) == len(xs) * len(ys)                                                   # the full product of the two lattices
    order = [(y0, x0) for x0, y0, _, _ in b.tolist()]
    assert order == sorted(order) and len(set(order)) == len(order)                          # row-major, no duplicates
    assert np.array_equal(b, clip.plan_windows(W, H, window, stride))                        # deterministic
    st = min(window // 2 if stride is None else stride, side)
    xs = sorted(set(b[:, 0].tolist()))
    assert all(d == st for d in np.diff(xs)[:-1]) and (len(xs) < 2 or 0 < xs[-1] - xs[-2] <= st)


def test_plan_windows_first_case_is_the_issues_table_row():
    import clip
    b = clip.plan_windows(37, 23, 16, 8)
    assert len(b) == 8
    assert b[:4, 0].tolist() == [0, 8, 16, 21] and sorted(set(b[:, 1].tolist())) == [0, 7]
    cover = np.zeros((23, 37), dtype=np.int64)
    for x0, y0, x1, y1 in b.tolist():
        cover[y0:y1, x0:x1] += 1
    assert cover.min() == 1 and cover.max() == 6


def test_plan_windows_multi_scale_and_errors():
    import clip
    a, b = clip.plan_windows(100, 60, 32, 16), clip.plan_windows(100, 60, 48, 12)
    both = clip.plan_windows(100, 60, (32, 48), (16, 12))
    assert np.array_equal(both, np.concatenate([a, b]))
    assert np.array_equal(clip.plan_windows(100, 60, [48, 32]), np.concatenate([clip.plan_windows(100, 60, 48), clip.plan_windows(100, 60, 32)]))
    with pytest.raises(ValueError, match="stride must be an integer >= 1"):
        clip.plan_windows(100, 60, 32, 0)
    with pytest.raises(ValueError, match="exceeds window"):
        clip.plan_windows(100, 60, 32, 33)
    with pytest.raises(ValueError, match="window must be an integer >= 2"):
        clip.plan_windows(100, 60, 1)
    with pytest.raises(ValueError, match="sequence of 2"):
        clip.plan_windows(100, 60, (32, 48), 16)
    with pytest.raises(ValueError, match="one window size takes one stride"):
        clip.plan_windows(100, 60, 32, (16, 8))
    with pytest.raises(ValueError, match="at least 1 x 1"):
        clip.plan_windows(0, 60, 32)


# ---- pure host functions -----------------------------------------------------------------------
def _result(labels, C=3):
    import clip
    H, W = labels.shape
    return clip.PhotoDenseResult(probs=torch.zeros(1, C, 1, 1), boxes=torch.tensor([[0, 0, W, H]]), labels=labels,
                                 conf=torch.zeros(H, W), cover=torch.ones(H, W, dtype=torch.uint8), class_names=None)


def test_class_boxes_on_hand_made_maps():
    lab = torch.tensor([[1, 1, 0, 0, 1],
                        [0, 1, 0, 1, 1],
                        [0, 0, 0, 0, 0],
                        [1, 0, 1, 0, 2],
                        [1, 1, 1, 0, 2]], dtype=torch.uint8)
    res = _result(lab)
    assert res.class_boxes(1) == [(0, 0, 2, 2), (3, 0, 5, 2), (0, 3, 3, 5)]     # diagonal neighbours do not join; a U joins late
    assert res.class_boxes(1, min_area=4) == [(0, 3, 3, 5)]
    assert res.class_boxes(2) == [(4, 3, 5, 5)] and res.class_boxes(7) == []
    assert res.class_boxes(0) == [(0, 0, 5, 5)]                                  # one component through the middle row
    spiral = torch.tensor([[1, 1, 1, 1],
                           [0, 0, 0, 1],
                           [1, 1, 0, 1],
                           [1, 0, 0, 1],
                           [1, 1, 1, 1]], dtype=torch.uint8)
    assert _result(spiral).class_boxes(1) == [(0, 0, 4, 5)]                      # two arms that meet only in the last row
    import clip
    assert clip.label_boxes(np.zeros((2, 3), dtype=np.uint8), 0) == [(0, 0, 3, 2)]


def test_photo_result_area_fractions_sum_to_one():
    lab = torch.tensor([[0, 0, 2, 2], [255, 2, 2, 1], [0, 1, 255, 255]], dtype=torch.uint8)
    res = _result(lab)
    fr = res.area_fractions()
    assert fr.dtype == torch.float64 and fr.shape == (4,)
    assert torch.equal(fr, torch.tensor([3, 2, 4, 3], dtype=torch.float64) / 12) and abs(float(fr.sum()) - 1.0) < 1e-15
    assert res.top_class() == 2 and res.n_classes == 3
    assert _result(torch.full((2, 2), 255, dtype=torch.uint8)).top_class() is None


def test_stitch_surface_exists_and_refuses_cpu_tensors():
    import clip
    from cclip_hip import ops
    for name in ("segment_photo", "plan_windows", "PhotoDenseResult", "label_boxes"):
        assert hasattr(clip, name), name
    with pytest.raises(ValueError, match="dense_stitch: probs must be a cuda tensor"):
        ops.dense_stitch(torch.zeros(1, 2, 2, 2), torch.zeros(1, 4, dtype=torch.int32), 4, 4, torch.zeros(4, 4, dtype=torch.uint8),
                         torch.zeros(4, 4))
