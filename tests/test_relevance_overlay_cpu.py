"""CPU: the host side of the relevance overlays - the default colour table, the float64 oracle of tests/overlay_ref.py pinned to
the reference's own lines (F.interpolate + attention.py:77-96 with the colour table substituted), clip.text_heat_html, and
the argument checks clip.relevance_overlay makes before it touches the device."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts"), os.path.dirname(os.path.abspath(__file__))]

import overlay_ref as OR  # noqa: E402

# (grid, resolution, size, maps, one shared image): the shapes of tests/test_relevance_overlay_gpu.py
CASES = [(7, 224, 224, 1, False), (2, 5, 5, 3, False), (3, 32, 17, 2, False), (7, 64, 224, 2, False), (24, 336, 336, 2, False),
         (7, 224, 224, 3, True)]


def _inputs(i):
    g, R, S, N, shared = CASES[i]
    gen = torch.Generator().manual_seed(100 + i)
    return torch.rand(N, g * g, generator=gen), torch.randn(1 if shared else N, 3, R, R, generator=gen), S


def test_jet_table_is_the_ramp_of_explain_clip():
    import clip
    import explain_clip
    lut = clip.jet_table()
    assert lut.shape == (256, 3) and lut.dtype == torch.float32
    want = explain_clip._jet(np.arange(256, dtype=np.float64) / 255)
    assert np.array_equal(lut.numpy(), want.astype(np.float32))
    assert lut[0, 2] > lut[0, 0] and lut[0, 2] > lut[0, 1]            # row 0 blue-ish
    assert lut[255, 0] > lut[255, 1] and lut[255, 0] > lut[255, 2]    # row 255 red-ish
    assert float(lut.min()) == 0.0 and float(lut.max()) == 1.0


def _reference_lines(rel, image, lut, S):
    """attention.py:88-96 and show_cam_on_image (77-82) for one map, fp32 as there; `lut[np.uint8(255 * mask)]` in the place of
    cv2.applyColorMap(...) / 255, and the image brought to S x S by the same F.interpolate (the reference's is 224 already)"""
    dim = int(rel.numel() ** 0.5)
    m = F.interpolate(rel.reshape(1, 1, dim, dim), size=S, mode="bilinear").reshape(S, S).numpy()
    m = (m - m.min()) / (m.max() - m.min())
    if image.shape[-1] != S:
        image = F.interpolate(image[None], size=S, mode="bilinear")[0]
    img = image.permute(1, 2, 0).numpy()
    img = (img - img.min()) / (img.max() - img.min())
    heatmap = lut.numpy()[np.uint8(255 * m)]
    cam = heatmap + np.float32(img)
    cam = cam / np.max(cam)
    return torch.from_numpy(np.uint8(255 * cam))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_oracle_reproduces_the_reference_lines(dtype):
    """the oracle (float64, and run in fp32) against F.interpolate + the reference's numpy lines, under the comparison rule of
    overlay_ref.compare with the fragile set taken from the float64 oracle"""
    import clip
    lut = clip.jet_table()
    fragile = pixels = 0
    for i in range(len(CASES)):
        rel, images, S = _inputs(i)
        N = rel.shape[0]
        ref64 = OR.overlay_ref(rel, images, lut, S)
        want = torch.stack([_reference_lines(rel[n], images[n if images.shape[0] > 1 else 0], lut, S) for n in range(N)])
        for got in (want, OR.overlay_ref(rel, images, lut, S, dtype=dtype)[0]):
            f, p, bad, worst = OR.compare(got, ref64)
            assert bad == 0 and worst <= OR.FRAGILE_LEVELS, (CASES[i], f, p, bad, worst)
        fragile += f
        pixels += p
        if p >= 10000:
            assert f <= 0.01 * p, (CASES[i], f, p)
    assert fragile <= 0.01 * pixels, (fragile, pixels)


def test_oracle_identity_and_degenerate_ranges():
    import clip
    lut = clip.jet_table()
    x = torch.randn(2, 3, 6, 6, dtype=torch.float64)
    assert torch.equal(OR.bil(x, 6), x)                                # L == S is the identity
    out, m255, c255 = OR.overlay_ref(torch.full((1, 4), 0.3), torch.full((1, 3, 5, 5), -1.0), lut, 5)
    assert torch.equal(m255, torch.zeros(1, 5, 5, dtype=torch.float64))
    assert torch.equal(out, torch.tensor([0, 0, 255], dtype=torch.uint8).expand(1, 5, 5, 3))
    out, _, _ = OR.overlay_ref(torch.rand(1, 4), torch.full((1, 3, 5, 5), 2.0), torch.zeros(256, 3), 5)
    assert int(out.max()) == 0


def test_text_heat_html():
    import clip
    page = clip.text_heat_html(["a<b", "&", "ok"], torch.tensor([0.25, 0.5, 0.0]))
    assert page.count("<span") == 3 and page.count("</span>") == 3
    assert "a&lt;b" in page and "&amp;" in page and "a<b" not in page
    alphas = [float(a) for a in re.findall(r"rgba\(255, 0, 0, ([0-9.]+)\)", page)]
    assert alphas == [0.5, 1.0, 0.0]
    empty = clip.text_heat_html([], [])
    assert isinstance(empty, str) and "<span" not in empty
    assert clip.text_heat_html(["x"], [0.0]).count("<span") == 1      # no division by a zero maximum
    with pytest.raises(ValueError):
        clip.text_heat_html(["x", "y"], [1.0])


def test_argument_checks_before_any_device_call():
    import clip
    rel, img = torch.rand(3, 49), torch.randn(3, 3, 8, 8)
    with pytest.raises(ValueError, match="square"):
        clip.relevance_overlay(torch.rand(3, 50), img)
    with pytest.raises(ValueError, match="2 images for 3 maps"):
        clip.relevance_overlay(rel, img[:2])
    with pytest.raises(ValueError, match="lut"):
        clip.relevance_overlay(rel, img, lut=torch.zeros(255, 3))
    with pytest.raises(ValueError, match="image must be"):
        clip.relevance_overlay(rel, torch.randn(3, 1, 8, 8))
    with pytest.raises(ValueError, match="no CPU path"):              # well-formed, but on the host: an error, not a fall-back
        clip.relevance_overlay(rel, img)
    with pytest.raises(ValueError, match="no CPU path"):
        clip.relevance_overlay(rel[0], img[0], size=16, return_map=True)
