"""clip.relevance_overlay on the MI355X against the float64 oracle of tests/overlay_ref.py (every pixel outside the fragile set
equal, the fragile ones within 5 levels, the fragile share capped), its map output, degenerate inputs, a custom colour table,
the bytes around the output buffer, determinism and argument errors; Captioner.explain against the composition of the public
pieces; scripts/explain_images.py end to end."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.dirname(os.path.abspath(__file__))]

import overlay_ref as OR  # noqa: E402

# (grid, resolution, size, maps, one shared image) - the smallest shapes at which the kernel can go wrong:
CASES = [(7, 224, 224, 1, False),      # the reference's own case (ViT-B/32 at 224)
         (2, 5, 5, 3, False),          # fewer pixels than threads; 75-byte overlays start unaligned; vector-store tail
         (3, 32, 17, 2, False),        # image resampled down, odd size
         (7, 64, 224, 2, False),       # image resampled up
         (24, 336, 336, 2, False),     # many loop trips per thread (ViT-L/14@336px)
         (7, 224, 224, 3, True)]       # one image [1, 3, R, R] under 3 maps


@functools.lru_cache(maxsize=None)
def _inputs(i):
    g, R, S, N, shared = CASES[i]
    gen = torch.Generator().manual_seed(100 + i)
    return torch.rand(N, g * g, generator=gen), torch.randn(1 if shared else N, 3, R, R, generator=gen), S


@functools.lru_cache(maxsize=None)
def _ref(i):
    """the float64 oracle of case i with the default table: computed once, shared, never modified"""
    import clip
    rel, images, S = _inputs(i)
    return OR.overlay_ref(rel, images, clip.jet_table(), S)


def _check(got, ref, what):
    fragile, pixels, bad, worst = OR.compare(got, ref)
    print(f"{what}: {pixels} pixels, {fragile} fragile ({100 * fragile / pixels:.2f} %), {bad} mismatches outside the fragile set, "
          f"worst fragile difference {worst}")
    assert bad == 0 and worst <= OR.FRAGILE_LEVELS, (what, fragile, pixels, bad, worst)
    return fragile, pixels


@pytest.mark.parametrize("i", range(len(CASES)))
def test_overlay_matches_the_float64_oracle(i):
    import clip
    rel, images, S = _inputs(i)
    got = clip.relevance_overlay(rel.cuda(), images.cuda(), size=S)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (rel.shape[0], S, S, 3)
    fragile, pixels = _check(got, _ref(i), str(CASES[i]))
    if pixels >= 10000:
        assert fragile <= 0.01 * pixels, (CASES[i], fragile, pixels)


def test_fragile_share_of_the_cases_pooled():
    """the rule lets a fragile pixel differ, so the fragile set has to stay small: <= 1 % over the table of cases (the 25-pixel
    case alone exceeds it through its exact-0 and exact-255 pixels, hence pooled)"""
    fragile = pixels = 0
    for i in range(len(CASES)):
        _, m255, c255 = _ref(i)
        mask = OR.fragile_mask(m255, c255)
        fragile += int(mask.sum())
        pixels += mask.numel()
    print(f"pooled: {fragile} of {pixels} pixels fragile ({100 * fragile / pixels:.2f} %)")
    assert fragile <= 0.01 * pixels, (fragile, pixels)


def test_shared_image_equals_separate_calls():
    import clip
    rel, images, S = _inputs(5)
    rel, images = rel.cuda(), images.cuda()
    assert images.shape[0] == 1 and rel.shape[0] == 3
    got = clip.relevance_overlay(rel, images, size=S)
    for n in range(3):
        assert torch.equal(got[n], clip.relevance_overlay(rel[n], images[0], size=S))
    assert torch.equal(got, clip.relevance_overlay(rel, images.expand(3, -1, -1, -1).contiguous(), size=S))


@pytest.mark.parametrize("i", [0, 1, 2])
def test_return_map_is_image_relevance_map(i):
    """1e-6 absolute: values in [0, 1] from under ten fp32 roundings.  That count holds where the rounding of the source
    coordinate itself (half an ulp of a value below the grid side) stays far below 1e-6: the grids of 7 and fewer here."""
    import clip
    rel, images, S = _inputs(i)
    out, m = clip.relevance_overlay(rel.cuda(), images.cuda(), size=S, return_map=True)
    want = clip.image_relevance_map(rel.cuda(), S)
    assert m.dtype == torch.float32 and m.shape == want.shape
    err = float((m - want).abs().max())
    print(f"{CASES[i]}: max |map - image_relevance_map| = {err:.3g}")
    assert err <= 1e-6
    assert float(m.min()) == 0.0 and float(m.max()) == 1.0
    assert torch.equal(out, clip.relevance_overlay(rel.cuda(), images.cuda(), size=S))      # the map output changes no byte
    o1, m1 = clip.relevance_overlay(rel[0].cuda(), images[0].cuda(), size=S, return_map=True)
    assert o1.shape == (S, S, 3) and m1.shape == (S, S) and torch.equal(o1, out[0]) and torch.equal(m1, m[0])


def test_degenerate_inputs():
    import clip
    lut = clip.jet_table()
    gen = torch.Generator().manual_seed(7)
    rel, img = torch.rand(2, 9, generator=gen), torch.randn(2, 3, 12, 12, generator=gen)
    flat_rel, flat_img = torch.full((2, 9), 0.25), torch.full((2, 3, 12, 12), -0.5)
    S = 19
    # a constant relevance vector: the map is 0, so every pixel takes table row 0
    out, m = clip.relevance_overlay(flat_rel.cuda(), img.cuda(), size=S, return_map=True)
    assert torch.equal(m, torch.zeros_like(m))
    _check(out, OR.overlay_ref(flat_rel, img, lut, S), "constant relevance")
    # a constant image: xn = 0, the picture is the scaled heat map alone
    out = clip.relevance_overlay(rel.cuda(), flat_img.cuda(), size=S)
    _check(out, OR.overlay_ref(rel, flat_img, lut, S), "constant image")
    # both: cam = table row 0 = (0, 0, 0.5) everywhere, M = 0.5
    out, m = clip.relevance_overlay(flat_rel.cuda(), flat_img.cuda(), size=S, return_map=True)
    assert torch.isfinite(m).all()
    assert torch.equal(out.cpu(), torch.tensor([0, 0, 255], dtype=torch.uint8).expand(2, S, S, 3))
    # an all-zero table under a constant image: cam = 0 everywhere, M = 0 - zeros, not a division by zero
    for r in (rel, flat_rel):
        out, m = clip.relevance_overlay(r.cuda(), flat_img.cuda(), size=S, lut=torch.zeros(256, 3), return_map=True)
        assert int(out.max()) == 0 and torch.isfinite(m).all()


def test_custom_table_is_read():
    import clip
    rel, images, S = _inputs(3)
    grey = (torch.arange(256, dtype=torch.float32) / 255)[:, None].expand(256, 3).contiguous()
    got = clip.relevance_overlay(rel.cuda(), images.cuda(), size=S, lut=grey.cuda())
    _check(got, OR.overlay_ref(rel, images, grey, S), "grey ramp")
    assert not torch.equal(got, clip.relevance_overlay(rel.cuda(), images.cuda(), size=S))
    assert torch.equal(got, clip.relevance_overlay(rel.cuda(), images.cuda(), size=S, lut=grey))   # a host table is moved over


def test_bytes_around_the_output_stay_untouched():
    """ops level, S = 5, N = 3: the 3 x 75 bytes sit at an odd address inside a buffer filled with 0xA5, one spare overlay behind"""
    import clip
    from cclip_hip import ops
    rel, images, S = _inputs(1)
    rel, images, lut = rel.cuda(), images.cuda(), clip.jet_table().cuda()
    want = clip.relevance_overlay(rel, images, size=S)
    one = 3 * S * S
    for lead in (0, 1, 2, 3):
        buf = torch.full((lead + 4 * one,), 0xA5, device="cuda", dtype=torch.uint8)
        out = buf[lead:].view(4, S, S, 3)
        ops.relevance_overlay(rel, images, lut, S, out)
        assert torch.equal(out[:3], want), lead
        assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + 3 * one:] == 0xA5).all()), lead


def test_two_calls_give_equal_bytes():
    import clip
    for i in (0, 2):
        rel, images, S = _inputs(i)
        rel, images = rel.cuda(), images.cuda()
        a, ma = clip.relevance_overlay(rel, images, size=S, return_map=True)
        b, mb = clip.relevance_overlay(rel, images, size=S, return_map=True)
        assert torch.equal(a, b) and torch.equal(ma, mb)


def test_argument_errors():
    import clip
    from cclip_hip import ops
    rel, images, S = _inputs(3)
    rel, images = rel.cuda(), images.cuda()
    with pytest.raises(ValueError, match="no CPU path"):
        clip.relevance_overlay(rel.cpu(), images.cpu(), size=S)
    with pytest.raises(ValueError, match="cuda"):
        clip.relevance_overlay(rel, images.cpu(), size=S)
    with pytest.raises(ValueError, match="contiguous"):
        clip.relevance_overlay(rel, images.transpose(2, 3), size=S)
    with pytest.raises(ValueError, match="float32"):
        clip.relevance_overlay(rel, images.half(), size=S)
    with pytest.raises(ValueError, match="float32"):
        clip.relevance_overlay(rel.double(), images, size=S)
    with pytest.raises(ValueError, match="square"):
        clip.relevance_overlay(torch.rand(2, 50, device="cuda"), images, size=S)
    with pytest.raises(ValueError, match="2 images for 3 maps"):
        clip.relevance_overlay(torch.rand(3, 49, device="cuda"), images, size=S)
    with pytest.raises(ValueError, match="out must be"):
        ops.relevance_overlay(rel, images, clip.jet_table().cuda(), S, torch.empty(1, S, S, 3, device="cuda", dtype=torch.uint8))


# ---- Captioner.explain (the tiny models of tests/test_captioner_gpu.py) -------------------------------------------------

TYPES = {"s": "a", "v": "b"}
VIOS = ["c", "d", "e", "f", "g", "h", "i", "j", "k"]


@functools.lru_cache(maxsize=None)
def _setup():
    import _common as C
    import clip
    from clip.weights import MODELS, init_state_dict, synthetic_images
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    clip_model = clip.build_model(init_state_dict(MODELS["test-tiny"], 3)).cuda().eval().half()
    other = clip.build_model(init_state_dict(MODELS["test-tiny"], 19)).cuda().eval().half()
    geo = GPT2_MODELS["test-tiny"]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval().half()
    cap = Captioner(clip_model, model, C.ByteCaptionTokenizer(geo.vocab_size), clip_tokenize=C.get_tokenize(clip_model),
                    caption_types=TYPES, violation_types=VIOS, prefix_length=geo.prefix_length, attribute_length=geo.attribute_length)
    return cap, clip_model, other, synthetic_images(3, clip_model.geo, 4).cuda()


KW = dict(beam_size=3, entry_length=10, temperature=0.5, stop_token=102)


def test_explain_extends_the_records_of_describe():
    import clip
    cap, clip_model, _, images = _setup()
    want = cap.describe(images, **KW)
    got = cap.explain(images, size=48, **KW)
    assert len(got) == 3
    tokens = cap.clip_tokenize([r["prediction"] for r in want]).cuda()
    r_text, r_image = clip.interpret_rows(images, tokens, clip_model)
    overlays = clip.relevance_overlay(r_image.contiguous(), images, size=48)
    scores = clip.text_row_scores(r_text, tokens)
    for i, (g, w) in enumerate(zip(got, want)):
        assert {k: g[k] for k in w} == w                                # prediction, caption_type, violation_type, ... as describe
        assert set(g) - set(w) == {"overlay", "image_relevance", "token_scores", "clip_tokens"}
        assert g["overlay"].shape == (48, 48, 3) and g["overlay"].dtype.name == "uint8"
        assert torch.equal(torch.from_numpy(g["overlay"]), overlays[i].cpu())
        assert g["image_relevance"].dtype == torch.float32 and torch.equal(g["image_relevance"], r_image[i])
        assert g["token_scores"].dtype == torch.float32 and torch.equal(g["token_scores"], scores[i])
        assert torch.equal(g["clip_tokens"], tokens[i])
        eot = int(tokens[i].argmax())
        assert g["token_scores"].shape == (eot - 1,)


def test_explain_with_a_second_relevance_model():
    cap, _, other, images = _setup()
    base = cap.explain(images, size=48, **KW)
    got = cap.explain(images, size=48, relevance_model=other, **KW)
    for g, b in zip(got, base):
        assert g["prediction"] == b["prediction"] and g["caption_type"] == b["caption_type"] and g["violation_type"] == b["violation_type"]
        assert torch.equal(g["clip_tokens"], b["clip_tokens"])
    assert any(not torch.equal(g["image_relevance"], b["image_relevance"]) for g, b in zip(got, base))
    assert any((g["overlay"] != b["overlay"]).any() for g, b in zip(got, base))


def test_explain_images_script(tmp_path):
    from PIL import Image
    out = tmp_path / "explained"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "explain_images.py"), "--synthetic", "--n_images", "3", "--size", "40",
                        "--entry_length", "10", "--out-dir", str(out), "--html"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    recs = [l for l in lines if "png" in l]
    assert len(recs) == 3
    for rec in recs:
        assert set(rec) == {"file", "caption_type", "violation_type", "prediction", "top_patch", "png"}
        assert rec["caption_type"] in ("a", "b") and rec["violation_type"] in VIOS and 0 <= rec["top_patch"] < 4
        im = Image.open(rec["png"])
        im.load()
        assert im.size == (40, 40) and im.mode == "RGB"
    page = (out / "explained.html").read_text(encoding="utf-8")
    assert page.count("<img") == 3 and page.count('class="text-heat"') == 3
