"""GPU: the dense zero-shot maps on the MI355X against the float64 references of tests/dense_ref.py.

Bounds.
  dense_class_probs   |p - p64| <= PROBS_BOUND = 7.2e-6 = 4 x 1.79e-6, the worst error of the plain fp32 torch restatement
                      (F.normalize, matmul, softmax) against float64 on the same fp32 inputs, measured on the CPU
                      (tests/test_dense_ref_cpu.py keeps that figure honest); the factor 4 is for the different summation orders.
                      logits_out: |logit - logit64| <= LOGIT_BOUND = scale x 16 x 2^-24 = 9.6e-5 at scale 100 - a cosine is a
                      dot product of E <= 768 terms whose error grows like sqrt(E) roundings of its own size, times two inverse
                      norms and the scale: sixteen roundings of a value <= 1 cover it with room.
  dense_label_map     labels equal outside the fragile set (float64 top-two margin in (0, 1e-5): either class; share capped at 1 %
                      for >= 10 000 pixels), conf within 1e-6; overlay bytes exactly the integer formula on the returned labels.
  encode_image_dense  rel L2 against tower_prefix_ref + dense_tail_ref + ln_post + proj: 1.2e-2 with bf16 operands, 1e-3 with
                      fp16 - the feature bounds of tests/test_clip_parity_gpu.py (the same GEMM chain, one block shorter)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dense_ref as R  # noqa: E402

PROBS_BOUND = 4 * 1.79e-6
LOGIT_BOUND = 100.0 * 16 * 2.0 ** -24
FEAT_TOL = {torch.bfloat16: 1.2e-2, torch.float16: 1.0e-3}
GUARD = 64


def _ops():
    from cclip_hip import ops
    return ops


def _guarded(shape, dtype, fill):
    """(flat buffer, the view of `shape` in its middle) with GUARD elements of `fill` on either side"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _run_probs(feat, text, scale, P, want_logits=False):
    B, C = feat.shape[0] // P, text.shape[0]
    buf, probs = _guarded((B, C, P), torch.float32, -7.0)
    lg = torch.empty(B, C, P, device="cuda") if want_logits else None
    _ops().dense_class_probs(feat, text.cuda(), scale, P, probs, lg)
    torch.cuda.synchronize()
    assert _guards_intact(buf, -7.0)
    return probs, lg


# ---- dense_class_probs -------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PROBS_CASES)
def test_class_probs_against_float64(case):
    B, g, C, E = case
    feat, text, scale = R.probs_case(B, g, C, E)
    ref, ref_lg = R.class_probs_ref(feat, text, scale, g * g)
    probs, lg = _run_probs(feat.cuda(), text, scale, g * g, want_logits=True)
    err = (probs.double().cpu() - ref).abs().max().item()
    lerr = (lg.double().cpu() - ref_lg).abs().max().item()
    print(f"dense_class_probs {case}: max |dp| {err:.3e} (bound {PROBS_BOUND:.2e}), max |dlogit| {lerr:.3e}")
    assert err <= PROBS_BOUND
    assert lerr <= LOGIT_BOUND
    if C == 1:
        assert torch.equal(probs, torch.ones_like(probs))
    again, _ = _run_probs(feat.cuda(), text, scale, g * g)
    assert torch.equal(again, probs)                                         # two calls, equal bytes (with and without logits_out)


def test_class_probs_strided_zero_row_and_unnormalised_text():
    B, g, C, E = 2, 7, 5, 512
    feat, text, scale = R.probs_case(B, g, C, E)
    feat[17] = 0.0
    ref, _ = R.class_probs_ref(feat, text, scale, g * g)
    wide = torch.full((B * g * g, E + 12), 3.0, device="cuda")
    wide[:, 4:4 + E] = feat.cuda()
    probs, _ = _run_probs(wide[:, 4:4 + E], text, scale, g * g)              # row stride E + 12, 16-byte aligned start
    assert (probs.double().cpu() - ref).abs().max().item() <= PROBS_BOUND
    assert torch.equal(probs, _run_probs(feat.cuda(), text, scale, g * g)[0])
    row = probs[0, :, 17]
    assert (row.double().cpu() - 1.0 / C).abs().max().item() <= PROBS_BOUND and bool((row == row[0]).all())
    unit = torch.nn.functional.normalize(text.double(), dim=1).float()
    pn, _ = _run_probs(feat.cuda(), unit, scale, g * g)
    assert (pn.double().cpu() - ref).abs().max().item() <= PROBS_BOUND       # a text row's length does not matter


def test_class_probs_argument_errors():
    ops = _ops()
    feat, text = torch.randn(8, 32, device="cuda"), torch.randn(3, 32, device="cuda")
    probs = torch.empty(2, 3, 4, device="cuda")
    ops.dense_class_probs(feat, text, 10.0, 4, probs)
    with pytest.raises(ValueError, match="256 classes"):
        ops.dense_class_probs(feat, torch.randn(256, 32, device="cuda"), 10.0, 4, torch.empty(2, 256, 4, device="cuda"))
    with pytest.raises(ValueError, match="width 6"):
        ops.dense_class_probs(torch.randn(8, 6, device="cuda"), torch.randn(3, 6, device="cuda"), 10.0, 4, probs)
    with pytest.raises(ValueError, match="width 1028"):
        ops.dense_class_probs(torch.randn(8, 1028, device="cuda"), torch.randn(3, 1028, device="cuda"), 10.0, 4, probs)
    with pytest.raises(ValueError, match="text must be a cuda tensor"):
        ops.dense_class_probs(feat, text.cpu(), 10.0, 4, probs)
    with pytest.raises(ValueError, match="feat must be torch.float32"):
        ops.dense_class_probs(feat.half(), text, 10.0, 4, probs)
    with pytest.raises(ValueError, match="text must be contiguous"):
        ops.dense_class_probs(feat, torch.randn(32, 3, device="cuda").t(), 10.0, 4, probs)
    with pytest.raises(ValueError, match="multiple of patches"):
        ops.dense_class_probs(feat, text, 10.0, 3, probs)
    with pytest.raises(ValueError, match="probs must be"):
        ops.dense_class_probs(feat, text, 10.0, 4, torch.empty(2, 4, 3, device="cuda"))
    with pytest.raises(ValueError, match="text must be \\[C, 32\\]"):
        ops.dense_class_probs(feat, torch.randn(3, 16, device="cuda"), 10.0, 4, probs)


# ---- dense_label_map ---------------------------------------------------------------------------
def _run_labels(probs, S, min_conf=0.0, overlay=False, palette=None, photo=None, alpha8=256):
    B = probs.shape[0]
    lbuf, labels = _guarded((B, S, S), torch.uint8, 77)
    cbuf, conf = _guarded((B, S, S), torch.float32, -7.0)
    obuf, out = _guarded((B, S, S, 3), torch.uint8, 77) if overlay else (None, None)
    _ops().dense_label_map(probs, S, labels, conf, min_conf=min_conf, overlay=out, palette=palette, photo=photo, alpha8=alpha8)
    torch.cuda.synchronize()
    assert _guards_intact(lbuf, 77) and _guards_intact(cbuf, -7.0) and (obuf is None or _guards_intact(obuf, 77))
    return labels, conf, out


@pytest.mark.parametrize("case", R.LABEL_CASES)
def test_label_map_against_float64(case):
    import clip
    g, S, C, B = case
    probs = R.label_case(g, S, C, B)
    ref = R.label_map_ref(probs, S)
    pal = clip.default_palette(C).cuda()
    labels, conf, out = _run_labels(probs.cuda(), S, overlay=True, palette=pal)
    wrong, share = R.compare_labels(labels, ref)
    cerr = (conf.double().cpu() - ref["conf"]).abs().max().item()
    print(f"dense_label_map {case}: wrong {wrong}, fragile share {share:.2e}, max |dconf| {cerr:.3e}")
    assert wrong == 0
    if B * S * S >= 10000:
        assert share < 0.01
    assert cerr <= R.CONF_TOL
    assert torch.equal(out.cpu(), R.overlay_ref(labels, pal))
    l2, c2, o2 = _run_labels(probs.cuda(), S, overlay=True, palette=pal)
    assert torch.equal(l2, labels) and torch.equal(c2, conf) and torch.equal(o2, out)
    l3, c3, _ = _run_labels(probs.cuda(), S)                                  # the picture changes neither
    assert torch.equal(l3, labels) and torch.equal(c3, conf)


def test_label_map_ties_threshold_and_overlay_bytes():
    g, S, B = 3, 17, 2
    base = R.label_case(g, S, 2, B)
    twin = torch.stack([base[:, 0], base[:, 0], torch.zeros_like(base[:, 0])], dim=1).contiguous()
    labels, _, _ = _run_labels(twin.cuda(), S)
    assert bool((labels == 0).all())                                          # two identical winners: the lower index
    twin2 = torch.stack([torch.zeros_like(base[:, 0]), base[:, 1], base[:, 1]], dim=1).contiguous()
    assert bool((_run_labels(twin2.cuda(), S)[0] == 1).all())

    ref = R.label_map_ref(base, S, min_conf=0.8)
    gen = torch.Generator().manual_seed(9)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()       # a custom palette
    photo = torch.randint(0, 256, (B, S, S, 3), generator=gen, dtype=torch.uint8).cuda()
    labels, conf, out = _run_labels(base.cuda(), S, min_conf=0.8, overlay=True, palette=pal)
    assert R.compare_labels(labels, ref)[0] == 0
    assert bool((labels == 255).any()) and bool((labels < 2).any())
    assert bool((labels[conf < 0.8] == 255).all()) and bool((labels[conf >= 0.8] < 2).all())
    assert torch.equal(out.cpu(), R.overlay_ref(labels, pal))
    for a8 in (0, 1, 77, 128, 256):
        l2, _, o2 = _run_labels(base.cuda(), S, min_conf=0.8, overlay=True, palette=pal, photo=photo, alpha8=a8)
        assert torch.equal(l2, labels)
        assert torch.equal(o2.cpu(), R.overlay_ref(labels, pal, photo, a8)), a8
    assert torch.equal(_run_labels(base.cuda(), S, min_conf=0.8, overlay=True, palette=pal, photo=photo, alpha8=0)[2], photo)


def test_label_map_misaligned_buffers():
    """labels / overlay / photo that start one byte off a dword: the element-wise store path gives the same bytes"""
    g, S, C, B = 2, 5, 3, 3
    probs = R.label_case(g, S, C, B).cuda()
    gen = torch.Generator().manual_seed(4)
    pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
    photo = torch.randint(0, 256, (B, S, S, 3), generator=gen, dtype=torch.uint8).cuda()
    labels, conf, out = _run_labels(probs, S, overlay=True, palette=pal, photo=photo, alpha8=100)
    n = B * S * S
    lb = torch.full((n + 9,), 77, device="cuda", dtype=torch.uint8)
    ob = torch.full((3 * n + 9,), 77, device="cuda", dtype=torch.uint8)
    pb = torch.zeros(3 * n + 3, device="cuda", dtype=torch.uint8)
    pb[3:] = photo.flatten()
    cb = torch.full((n + 5,), -7.0, device="cuda")
    _ops().dense_label_map(probs, S, lb[1:1 + n].view(B, S, S), cb[1:1 + n].view(B, S, S), overlay=ob[1:1 + 3 * n].view(B, S, S, 3),
                           palette=pal, photo=pb[3:].view(B, S, S, 3), alpha8=100)
    assert torch.equal(lb[1:1 + n].view(B, S, S), labels) and torch.equal(ob[1:1 + 3 * n].view(B, S, S, 3), out)
    assert torch.equal(cb[1:1 + n].view(B, S, S), conf)
    assert lb[0] == 77 and bool((lb[1 + n:] == 77).all()) and ob[0] == 77 and bool((ob[1 + 3 * n:] == 77).all())
    assert cb[0] == -7.0 and bool((cb[1 + n:] == -7.0).all())


def test_label_map_argument_errors():
    ops = _ops()
    probs = R.label_case(2, 5, 3, 1).cuda()
    lab, conf = torch.empty(1, 5, 5, device="cuda", dtype=torch.uint8), torch.empty(1, 5, 5, device="cuda")
    pal = torch.zeros(256, 3, device="cuda", dtype=torch.uint8)
    ov = torch.empty(1, 5, 5, 3, device="cuda", dtype=torch.uint8)
    ops.dense_label_map(probs, 5, lab, conf, overlay=ov, palette=pal)
    with pytest.raises(ValueError, match="labels must be torch.uint8"):
        ops.dense_label_map(probs, 5, lab.int(), conf)
    with pytest.raises(ValueError, match="probs must be a cuda tensor"):
        ops.dense_label_map(probs.cpu(), 5, lab, conf)
    with pytest.raises(ValueError, match="probs must be \\[B, C, g, g\\]"):
        ops.dense_label_map(probs[:, :, :1].contiguous(), 5, lab, conf)
    with pytest.raises(ValueError, match="conf must be"):
        ops.dense_label_map(probs, 5, lab, torch.empty(1, 5, 4, device="cuda"))
    with pytest.raises(ValueError, match="size 0"):
        ops.dense_label_map(probs, 0, lab, conf)
    with pytest.raises(ValueError, match="palette must be uint8 \\[256, 3\\]"):
        ops.dense_label_map(probs, 5, lab, conf, overlay=ov)
    with pytest.raises(ValueError, match="give overlay too"):
        ops.dense_label_map(probs, 5, lab, conf, palette=pal)
    with pytest.raises(ValueError, match="photo must be"):
        ops.dense_label_map(probs, 5, lab, conf, overlay=ov, palette=pal, photo=torch.zeros(1, 4, 4, 3, device="cuda", dtype=torch.uint8))
    with pytest.raises(ValueError, match="alpha8"):
        ops.dense_label_map(probs, 5, lab, conf, overlay=ov, palette=pal, alpha8=257)
    with pytest.raises(ValueError, match="256 classes"):
        ops.dense_label_map(torch.rand(1, 256, 2, 2, device="cuda"), 5, lab, conf)
    with pytest.raises(ValueError, match="overlay must be contiguous"):
        ops.dense_label_map(probs, 5, lab, conf, overlay=torch.empty(1, 5, 3, 5, device="cuda", dtype=torch.uint8).transpose(2, 3), palette=pal)


# ---- encode_image_dense ------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _toy(grid, dtype, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)       # width 128, 2 heads of 64, 2 layers
    sd = init_state_dict(geo, seed)
    return geo, sd, clip.build_model(sd, dtype).cuda().eval()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("grid,B", [(2, 1), (3, 3)])
def test_encode_image_dense_toy_against_float64(grid, B, dtype):
    from clip.weights import synthetic_images
    geo, sd, model = _toy(grid, dtype)
    img = synthetic_images(B, geo, 4)
    before = model.encode_image(img.cuda())
    outs, refs = {}, {}
    for mode in ("value", "qq", "kk"):
        got = model.encode_image_dense(img.cuda(), mode=mode)
        assert got.shape == (B, grid, grid, geo.embed_dim) and got.dtype == torch.float32
        refs[mode] = R.dense_features_ref(sd, img, mode)
        e = rel(got, refs[mode])
        print(f"encode_image_dense grid {grid} B {B} {dtype} {mode}: rel L2 {e:.3e} (bound {FEAT_TOL[dtype]:.1e})")
        assert e < FEAT_TOL[dtype]
        outs[mode] = got
    # three different heads, not one: they differ, and by what the references differ (a self-self attention of 64-wide heads
    # is close to the identity, so the distances are small; each side of the triangle is within the feature bound)
    for a, b in (("value", "qq"), ("value", "kk"), ("qq", "kk")):
        d_ref, d_got = rel(refs[a], refs[b]), rel(outs[a], outs[b])
        print(f"  {a} vs {b}: rel L2 {d_got:.3e} (float64 {d_ref:.3e})")
        assert d_ref > 0 and not torch.equal(outs[a], outs[b]), (a, b)
        assert abs(d_got - d_ref) < 2 * FEAT_TOL[dtype], (a, b)
    assert torch.equal(model.encode_image(img.cuda()), before)               # no state left behind
    assert model.encode_image_dense(img[:0].cuda()).shape == (0, grid, grid, geo.embed_dim)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encode_image_dense_vit_b32(dtype):
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_images
    g = torch.load(os.path.join(HERE, "golden", "clip_vit_b32.pt"), weights_only=True)
    geo = MODELS[g["model"]]
    sd = init_state_dict(geo, g["seed"])
    model = clip.build_model(sd, dtype).cuda().eval()
    img = synthetic_images(2, geo, g["seed"] + 1)
    got = model.encode_image_dense(img.cuda())
    e = rel(got, R.dense_features_ref(sd, img))
    print(f"encode_image_dense ViT-B/32 B 2 {dtype}: rel L2 {e:.3e} (bound {FEAT_TOL[dtype]:.1e})")
    assert got.shape == (2, 7, 7, 512) and e < FEAT_TOL[dtype]


def test_value_mode_is_patch_local_and_layers_none_is_the_default_call():
    from clip.weights import synthetic_images
    geo, sd, model = _toy(3, torch.bfloat16)
    img = synthetic_images(2, geo, 4).cuda()
    model.encode_image(img)                                                   # builds the runtime
    st = model._rt["vis"]
    T, D = geo.vision_tokens, geo.vision_width
    x0 = torch.randn(2 * T, D, device="cuda")
    a = st.forward(x0.clone(), 2)
    b = st.forward(x0.clone(), 2, layers=None)
    assert torch.equal(a, b)
    assert torch.equal(st.forward(x0.clone(), 2, layers=0), x0)
    x = st.forward(x0.clone(), 2, layers=len(st.blocks) - 1)
    assert not torch.equal(x, a) and not torch.equal(x, x0)
    y = st.dense_tail(x, 2, "value")
    j = T + 4                                                                 # a patch row of the second image
    xp = x.clone()
    xp[j] += torch.randn(D, device="cuda")                                   # (not a constant: ln_1 removes a row's mean)
    yp = st.dense_tail(xp, 2, "value")
    others = torch.ones(2 * T, dtype=torch.bool, device="cuda")
    others[j] = False
    assert rel(yp[others], y[others]) < FEAT_TOL[torch.bfloat16]              # (row-local launches: in fact the same bytes)
    assert rel(yp[j], y[j]) > 10 * FEAT_TOL[torch.bfloat16]


def test_dense_after_fp8_projections_raises():
    from clip.weights import synthetic_images
    geo, sd, model = _toy(2, torch.bfloat16)
    img = synthetic_images(1, geo, 4).cuda()
    model.fp8_projections()
    with pytest.raises(RuntimeError, match="fp8"):
        model.encode_image_dense(img)
    model.fp8_projections(False)
    assert model.encode_image_dense(img).shape == (1, 2, 2, geo.embed_dim)


# ---- end to end --------------------------------------------------------------------------------
def test_segment_is_the_composition_of_the_two_ops():
    import clip
    from clip.weights import synthetic_images
    geo, sd, model = _toy(3, torch.bfloat16)
    img = synthetic_images(2, geo, 4).cuda()
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    res = clip.segment(model, img, text, size=40, min_conf=0.3)
    feats = clip.dense_features(model, img)
    scale = float(model.logit_scale.detach().exp())
    probs = torch.empty(2, 4, 9, device="cuda")
    _ops().dense_class_probs(feats.view(18, -1), text, scale, 9, probs)
    labels, conf = torch.empty(2, 40, 40, device="cuda", dtype=torch.uint8), torch.empty(2, 40, 40, device="cuda")
    _ops().dense_label_map(probs.view(2, 4, 3, 3), 40, labels, conf, min_conf=0.3)
    assert torch.equal(res.probs, probs.view(2, 4, 3, 3)) and torch.equal(res.labels, labels) and torch.equal(res.conf, conf)
    assert res.class_names is None and res.n_classes == 4
    fr = res.area_fractions()
    assert fr.shape == (2, 5) and (fr.sum(dim=1) - 1).abs().max().item() < 1e-12
    assert torch.equal((fr * 1600).round().long().sum(dim=1).cpu(), torch.tensor([1600, 1600]))
    pal = clip.default_palette(4)
    assert torch.equal(res.overlay().cpu(), R.overlay_ref(labels, pal))
    photo = torch.randint(0, 256, (2, 40, 40, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    assert torch.equal(res.overlay(photo=photo, alpha=0.25).cpu(), R.overlay_ref(labels, pal, photo, 64))
    cool = clip.segment(model, img, text, size=40, temperature=1.0)          # a flat softmax: nothing reaches 0.3
    assert float(cool.conf.max()) < 0.5 and not torch.equal(cool.probs, res.probs)
    by_name = clip.segment(model, img, ["ab", "cd"], size=8, tokenize=lambda names: _tokens(names, geo))
    assert by_name.class_names == ["ab", "cd"] and by_name.labels.shape == (2, 8, 8)


def _tokens(names, geo):
    from clip.weights import synthetic_text
    return synthetic_text(len(names), geo, 7)


def test_segment_images_script(tmp_path):
    out = tmp_path / "maps"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "segment_images.py"), "--synthetic", "--n_images", "2", "--size", "40",
                        "--png", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    from PIL import Image
    for line in lines:
        assert abs(sum(line["area"]) - 1.0) < 1e-5 and len(line["area"]) == len(line["classes"]) + 1
        assert line["top_class"] in line["classes"]
        assert Image.open(line["png"]).size == (40, 40)
    assert len(os.listdir(out)) == 2
