"""CPU: the float64 references of the dense zero-shot maps (tests/dense_ref.py) against plain torch on float64, the label
comparison against planted faults, the seeded inputs' fragile shares, and the host logic of clip/dense.py and
BlockStack.forward(layers=) that needs no device."""
import inspect
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_ref as R  # noqa: E402

# the error of the plain fp32 restatement (class_probs_fp32) against float64 on PROBS_CASES, measured here; the kernel test's
# bound is 4 x this (tests/test_dense_gpu.py)
PROBS_FP32_WORST = 1.79e-6


@pytest.mark.parametrize("case", R.PROBS_CASES)
def test_class_probs_ref_is_normalize_matmul_softmax(case):
    B, g, C, E = case
    feat, text, scale = R.probs_case(B, g, C, E)
    probs, logits = R.class_probs_ref(feat, text, scale, g * g)
    lg = scale * F.normalize(feat.double(), dim=1) @ F.normalize(text.double(), dim=1).t()
    want = lg.softmax(dim=1).view(B, g * g, C).permute(0, 2, 1)
    assert probs.shape == (B, C, g * g) and probs.dtype == torch.float64
    assert (probs - want).abs().max() < 1e-13
    assert (logits - lg.view(B, g * g, C).permute(0, 2, 1)).abs().max() < 1e-11
    assert (probs.sum(dim=1) - 1).abs().max() < 1e-13


def test_class_probs_ref_zero_row_is_uniform_and_text_length_is_ignored():
    feat, text, scale = R.probs_case(2, 2, 3, 32)
    feat[5] = 0
    probs, _ = R.class_probs_ref(feat, text, scale, 4)
    assert torch.equal(probs[1, :, 1], torch.full((3,), 1 / 3, dtype=torch.float64))
    again, _ = R.class_probs_ref(feat, F.normalize(text.double(), dim=1), scale, 4)
    assert (probs - again).abs().max() < 1e-12


def test_fp32_restatement_error_is_what_the_kernel_bound_was_made_from():
    worst = 0.0
    for B, g, C, E in R.PROBS_CASES:
        feat, text, scale = R.probs_case(B, g, C, E)
        ref, _ = R.class_probs_ref(feat, text, scale, g * g)
        worst = max(worst, (R.class_probs_fp32(feat, text, scale, g * g).double() - ref).abs().max().item())
    print(f"fp32 restatement, worst |dp| over PROBS_CASES: {worst:.3e}")
    # recorded to three digits; the summation order of a BLAS may move the last one
    assert 0.5 * PROBS_FP32_WORST < worst < 1.5 * PROBS_FP32_WORST, worst


@pytest.mark.parametrize("case", R.LABEL_CASES)
def test_label_map_ref_is_interpolate_argmax(case):
    g, S, C, B = case
    probs = R.label_case(g, S, C, B)
    ref = R.label_map_ref(probs, S)
    up = F.interpolate(probs.double(), size=(S, S), mode="bilinear", align_corners=False)
    assert (ref["up"] - up).abs().max() < 1e-14
    assert torch.equal(ref["labels"], up.argmax(dim=1))
    assert (ref["conf"] - up.max(dim=1).values).abs().max() < 1e-14
    wrong, share = R.compare_labels(ref["labels"], ref)
    assert wrong == 0
    if B * S * S >= 10000:                        # the seeds of the big cases keep the reference alone under the 1 % cap
        assert share < 0.01, share


def test_label_map_ref_threshold_and_ties():
    probs = R.label_case(3, 17, 2, 2)
    ref = R.label_map_ref(probs, 17, min_conf=0.8)
    low = ref["conf"] < 0.8
    assert low.any() and (~low).any()
    assert (ref["labels"][low] == R.NONE_LABEL).all() and (ref["labels"][~low] < 2).all()
    twin = torch.stack([probs[:, 0], probs[:, 0], torch.zeros_like(probs[:, 1])], dim=1)       # classes 0 and 1 identical, both win
    ref = R.label_map_ref(twin, 17)
    assert (ref["labels"] == 0).all() and (ref["margin"] == 0).all()


def test_compare_labels_flags_planted_faults():
    g, S, C, B = 7, 56, 5, 2
    probs = R.label_case(g, S, C, B, seed=3)
    ref = R.label_map_ref(probs, S)
    assert R.compare_labels(ref["labels"], ref)[0] == 0
    # align_corners=True
    bad = F.interpolate(probs.double(), size=(S, S), mode="bilinear", align_corners=True).argmax(dim=1)
    assert R.compare_labels(bad, ref)[0] > 0
    # probabilities written patch-major ([B, P, C] bytes read as [B, C, g, g])
    pm = probs.view(B, C, g * g).permute(0, 2, 1).contiguous().view(B, C, g, g)
    assert R.compare_labels(R.label_map_ref(pm, S)["labels"], ref)[0] > 0
    # a wrong tie rule: two identical winning maps, the HIGHER index taken
    twin = torch.stack([probs[:, 0], probs[:, 0], torch.zeros_like(probs[:, 1])], dim=1)
    tref = R.label_map_ref(twin, S)
    assert R.compare_labels(torch.ones_like(tref["labels"]), tref)[0] == B * S * S
    # a fragile pixel may take the runner-up, nothing else
    tref["margin"][0, 0, 0] = 1e-7
    flipped = tref["labels"].clone()
    flipped[0, 0, 0] = tref["second"][0, 0, 0]
    assert R.compare_labels(flipped, tref)[0] == 0
    flipped[0, 0, 0] = 2
    assert R.compare_labels(flipped, tref)[0] == 1


def _toy_sd(grid=2):
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)
    return geo, init_state_dict(geo, 11)


@pytest.mark.parametrize("mode", ("value", "qq", "kk"))
def test_dense_tail_ref_is_maskclips_tail(mode):
    """a direct restatement with torch's own layer_norm / linear / scaled_dot_product_attention on a toy state dict"""
    geo, sd = _toy_sd(3)
    D, H, T = geo.vision_width, geo.vision_heads, geo.vision_tokens
    x = torch.randn(2, T, D, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    p = "visual.transformer.resblocks.1."
    xn = F.layer_norm(x, (D,), sd[p + "ln_1.weight"].double(), sd[p + "ln_1.bias"].double(), 1e-5)
    qkv = F.linear(xn, sd[p + "attn.in_proj_weight"].double(), sd[p + "attn.in_proj_bias"].double())
    q, k, v = qkv.split(D, dim=-1)
    if mode == "value":
        a = v
    else:
        s = q if mode == "qq" else k
        heads = lambda t: t.view(2, T, H, D // H).transpose(1, 2)       # noqa: E731
        a = F.scaled_dot_product_attention(heads(s), heads(s), heads(v)).transpose(1, 2).reshape(2, T, D)
    want = F.linear(a, sd[p + "attn.out_proj.weight"].double(), sd[p + "attn.out_proj.bias"].double())
    got = R.dense_tail_ref(sd, x, mode)
    assert got.dtype == torch.float64 and (got - want).abs().max() < 1e-12
    # no residual: the result does not move with a constant added to x's rows beyond what ln_1 sees (it removes the mean)
    assert (R.dense_tail_ref(sd, x + 3.0, mode) - got).abs().max() < 1e-9


def test_dense_features_ref_prefix_is_the_oracles_tower_and_the_class_row_matters():
    from clip.weights import synthetic_images
    from oracle import clip_oracle as O
    geo, sd = _toy_sd(3)
    img = synthetic_images(2, geo, 4)
    # the prefix plus the oracle's own last block, pooled, is the oracle's encode_image
    x = R.tower_prefix_ref(sd, img)
    full = O.residual_block(x, "visual.transformer.resblocks.1.", sd, geo.vision_heads, None)
    pooled = O._layer_norm(full[:, 0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"].float()
    assert torch.allclose(pooled, O.encode_image(sd, img), rtol=0, atol=1e-6)
    feats = R.dense_features_ref(sd, img)
    assert feats.shape == (2, 3, 3, geo.embed_dim) and feats.dtype == torch.float64
    # the class row not dropped: the label map of the shifted features is flagged
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(6))
    good, _ = R.class_probs_ref(feats.reshape(18, -1), text, 100.0, 9)
    shifted, _ = R.class_probs_ref(R.dense_features_ref(sd, img, drop_class_row=False).reshape(18, -1), text, 100.0, 9)
    ref = R.label_map_ref(good.view(2, 4, 3, 3), 24)
    assert R.compare_labels(R.label_map_ref(shifted.view(2, 4, 3, 3), 24)["labels"], ref)[0] > 0


def test_overlay_ref_integer_blend():
    lab = torch.tensor([[[0, 1], [255, 1]]], dtype=torch.uint8)
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    pal[0], pal[1], pal[255] = torch.tensor([255, 0, 0]), torch.tensor([0, 200, 0]), torch.tensor([9, 9, 9])
    photo = torch.full((1, 2, 2, 3), 100, dtype=torch.uint8)
    assert torch.equal(R.overlay_ref(lab, pal)[0, 1, 0], torch.tensor([9, 9, 9], dtype=torch.uint8))
    assert torch.equal(R.overlay_ref(lab, pal, photo, 0), photo)
    assert torch.equal(R.overlay_ref(lab, pal, photo, 256), R.overlay_ref(lab, pal))
    assert R.overlay_ref(lab, pal, photo, 128)[0, 0, 0].tolist() == [(100 * 128 + 255 * 128 + 128) >> 8, 50, 50]


# ---- host logic (fails on a tree without the feature) ------------------------------------------
def test_public_surface_exists():
    import clip
    from cclip_hip import ops
    from cclip_hip.stack import BlockStack
    for name in ("segment", "dense_features", "DenseResult", "default_palette"):
        assert hasattr(clip, name), name
    assert hasattr(clip.CLIP, "encode_image_dense")
    assert hasattr(ops, "dense_class_probs") and hasattr(ops, "dense_label_map")
    assert "layers" in inspect.signature(BlockStack.forward).parameters
    assert inspect.signature(BlockStack.forward).parameters["layers"].default is None
    assert hasattr(BlockStack, "dense_tail")


def test_default_palette_is_deterministic():
    import clip
    a, b = clip.default_palette(9), clip.default_palette(9)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (256, 3) and torch.equal(a, b)
    assert len({tuple(r) for r in a[:9].tolist()}) == 9                         # nine different colours
    assert torch.equal(a[9:], torch.full((247, 3), 96, dtype=torch.uint8))      # the rest, "none" among them, one grey
    assert torch.equal(clip.default_palette(3)[:3], a[:3])                      # a class keeps its colour when the list grows
    with pytest.raises(ValueError):
        clip.default_palette(256)


def test_area_fractions_are_integer_counts():
    import clip
    labels = torch.tensor([[[0, 0, 2], [255, 2, 2], [0, 1, 255]]], dtype=torch.uint8)
    res = clip.DenseResult(probs=torch.zeros(1, 3, 1, 1), labels=labels, conf=torch.zeros(1, 3, 3), class_names=["a", "b", "c"])
    fr = res.area_fractions()
    assert fr.shape == (1, 4) and torch.equal(fr, torch.tensor([[3, 1, 3, 2]], dtype=torch.float64) / 9)
    assert res.top_class() == [0]


def test_dense_calls_refuse_cpu_tensors_and_bad_modes():
    import clip
    from cclip_hip import ops
    from cclip_hip.stack import BlockStack, Scratch, StackGeometry
    with pytest.raises(ValueError, match="dense_class_probs: feat must be a cuda tensor"):
        ops.dense_class_probs(torch.zeros(4, 8), torch.zeros(2, 8), 1.0, 4, torch.zeros(1, 2, 4))
    with pytest.raises(ValueError, match="dense_label_map: probs must be a cuda tensor"):
        ops.dense_label_map(torch.zeros(1, 2, 2, 2), 4, torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4))
    geo, sd = _toy_sd()
    model = clip.build_model(sd)
    with pytest.raises(RuntimeError, match="encode_image_dense"):
        model.encode_image_dense(torch.zeros(1, 3, 64, 64))
    st = BlockStack(StackGeometry(128, 4, 5, True, ops.ACT_QUICKGELU, False, head_dim=32), [], Scratch("cpu"))
    with pytest.raises(RuntimeError, match="64-wide heads"):
        st.dense_tail(torch.zeros(5, 128), 1)
    with pytest.raises(ValueError, match="mode"):
        st.dense_tail(torch.zeros(5, 128), 1, mode="vv")
