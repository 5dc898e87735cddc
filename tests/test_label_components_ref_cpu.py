"""The host reference of the connected-components kernels (label_components_ref.py: flood fill) against the host statement the
project already has (clip.label_boxes: row runs + union-find), which share no code; the C header; and the refusals of the new
entry points for CPU tensors.  No GPU needed."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import label_components_ref as LR  # noqa: E402

ALL_MAPS = dict(LR.MAPS, **{f"{k}[{b}]": v[b] for k, v in LR.BATCHES.items() for b in range(v.shape[0])})


@pytest.fixture(scope="module")
def refs4():
    return {name: LR.components(m, connectivity=4) for name, m in ALL_MAPS.items()}


@pytest.mark.parametrize("name", sorted(ALL_MAPS))
def test_reference_boxes_are_label_boxes(name, refs4):
    import clip
    m, ref = ALL_MAPS[name], refs4[name]
    classes = sorted(set(np.unique(m).tolist()) - {LR.NONE}) + [7]            # 7: a class no map has
    for c in classes:
        for min_area in (1, 5):
            assert LR.boxes_of(ref, c, min_area) == clip.label_boxes(m, c, min_area), (name, c, min_area)
    assert LR.NONE not in ref["label"]                                        # "none" is never a component


@pytest.mark.parametrize("name", sorted(LR.MAPS))
def test_reference_is_consistent(name, refs4):
    m, ref = LR.MAPS[name], refs4[name]
    H, W = m.shape
    live = m != LR.NONE
    assert np.array_equal(ref["root"] >= 0, live) and np.array_equal(ref["ids"] >= 0, live)
    assert ref["n"] == len(ref["first"]) and np.all(np.diff(ref["first"]) > 0)            # numbered in ascending order of root
    assert int(ref["area"].sum()) == int(live.sum())
    flat_root, flat_ids = ref["root"].reshape(-1), ref["ids"].reshape(-1)
    for i in range(ref["n"]):
        f = int(ref["first"][i])
        assert flat_root[f] == f and flat_ids[f] == i and m.reshape(-1)[f] == ref["label"][i]
    assert np.array_equal(flat_root[live.reshape(-1)], ref["first"][flat_ids[live.reshape(-1)]])
    assert np.all(flat_root[live.reshape(-1)] <= np.flatnonzero(live.reshape(-1)))        # the root is the FIRST pixel


def test_known_counts():
    cb = LR.MAPS["checkerboard_66x70"]
    assert LR.components(cb, connectivity=4)["n"] == 66 * 70
    r8 = LR.components(cb, connectivity=8)
    assert r8["n"] == 2 and r8["area"].tolist() == [66 * 70 // 2, 66 * 70 // 2]
    assert r8["boxes"].tolist() == [[0, 0, 70, 66], [0, 0, 70, 66]]
    assert LR.components(LR.checkerboard(1, 9), connectivity=8)["n"] == 9                  # 1 x N: no diagonal to join along, so
    assert LR.components(LR.checkerboard(1, 1), connectivity=8)["n"] == 1                  # two only from 2 x 2 on; 1 x 1 has one
    one = LR.components(LR.MAPS["one_class_97x130"])
    assert one["n"] == 1 and one["area"].tolist() == [97 * 130] and one["boxes"].tolist() == [[0, 0, 130, 97]] and one["label"].tolist() == [3]
    sp = LR.components(LR.MAPS["spiral_129x129"])
    assert sp["n"] == 1 and sp["first"].tolist() == [0] and sp["area"][0] > 129 * 129 // 2 - 200
    arms = LR.components(LR.MAPS["arms_70x70"])
    assert arms["n"] == 1 and arms["first"].tolist() == [3 * 70 + 60]
    nest = LR.components(LR.MAPS["nested_50x75"])
    assert nest["label"].tolist() == [2, 1, 0] and nest["n"] == 3
    for name, b in LR.BATCHES.items():                                                     # nothing crosses the image boundary
        whole = LR.components(b)
        parts = [LR.components(b[i]) for i in range(b.shape[0])]
        assert whole["n"] == sum(p["n"] for p in parts), name
        assert whole["image"].tolist() == [i for i, p in enumerate(parts) for _ in range(p["n"])]
        assert np.array_equal(whole["boxes"], np.concatenate([p["boxes"] for p in parts]))


def test_quantise_edges():
    v = np.array([0.0, 1.0, 0.5 - 2.0 ** -25, 1.0 + 1e-3, -0.25, np.nan, np.inf, -np.inf, 2.0 ** -17, 0.25, 1.0 - 2.0 ** -24, -0.0], dtype=np.float32)
    assert LR.quantise(v).tolist() == [0, 65536, 32768, 65536, 0, 0, 65536, 0, 1, 16384, 65536, 0]
    conf = LR.confidences((33, 65))
    ref = LR.components(LR.MAPS["edge_33x65"], conf)
    assert int(ref["qsum"].sum()) == int(LR.quantise(conf)[LR.MAPS["edge_33x65"] != LR.NONE].sum())


def test_header_declares_the_entry_points_and_keeps_the_abi():
    text = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    assert re.search(r"#define\s+CCLIP_ABI_VERSION\s+3\b", text)
    assert re.search(r"\bint\s+cclip_label_components\s*\(const uint8_t\*\s*labels,", text)
    assert re.search(r"\bint\s+cclip_component_stats\s*\(const uint8_t\*\s*labels,", text)
    group = re.search(r"#define\s+CCLIP_COMPONENTS_GROUP\s+(\d+)", text)
    from cclip_hip import ops
    from cclip_hip._lib import ABI_VERSION
    assert ABI_VERSION == 3 and group and int(group.group(1)) == ops.COMPONENTS_GROUP


def test_cpu_tensors_are_refused():
    import clip
    from cclip_hip import ops
    lab = torch.zeros(1, 4, 5, dtype=torch.uint8)
    i32 = torch.zeros(1, 4, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"label_components: labels must be a cuda tensor, got cpu \(no CPU path\)"):
        ops.label_components(lab, 4, i32, i32.clone(), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"component_stats: labels must be a cuda tensor, got cpu \(no CPU path\)"):
        ops.component_stats(lab, i32, i32.clone(), 0, torch.zeros(0, dtype=torch.uint8), *(torch.zeros(0, dtype=torch.int32) for _ in range(3)),
                            torch.zeros(0, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"label_components: labels must be a cuda tensor, got cpu \(no CPU path\)"):
        clip.label_components(lab[0])
    with pytest.raises(ValueError, match=r"label_components: labels must be a cuda tensor"):
        clip.label_components(lab[0].numpy())
