"""The arithmetic of clip.relevance_overlay (include/cclip_hip.h, cclip_relevance_overlay) restated with torch on the CPU, in
float64 unless another dtype is asked for, and the rule by which an 8-bit overlay is compared with it.

overlay_ref returns the picture and the two quantities that are floored on the way to it - 255 m (the colour-table row) and
255 cam / M (the byte) - so that a comparison can tell the pixels at which a floor may legitimately land on either side in fp32.
"""
import torch

DELTA = 5e-4          # "fragile": a floored quantity within DELTA of an integer.  The fp32 error of both quantities is below 1e-4
#                       levels (fewer than ten roundings of values <= 2, scaled by 255); DELTA is five times that.
FRAGILE_LEVELS = 5    # a fragile pixel may differ by one table step (a channel moves by at most 4/255 per row) plus one floor


def _axis(L, S, dtype):
    """bilinear, align_corners=False, no antialiasing: s = max((i + 0.5) L / S - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, L - 1)"""
    i = torch.arange(S, dtype=dtype)
    s = ((i + 0.5) * L / S - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=L - 1)
    i1 = (i0 + 1).clamp(max=L - 1)
    return i0, i1, s - i0.to(dtype)


def bil(src, S):
    """src [..., L, L] -> [..., S, S]"""
    i0, i1, w = _axis(src.shape[-1], S, src.dtype)
    rows = src[..., i0, :] * (1 - w)[:, None] + src[..., i1, :] * w[:, None]
    return rows[..., i0] * (1 - w) + rows[..., i1] * w


def _minmax01(x, dims):
    lo = x.amin(dim=dims, keepdim=True)
    rng = x.amax(dim=dims, keepdim=True) - lo
    return torch.where(rng > 0, (x - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(x))


def overlay_ref(rel, images, lut, size, dtype=torch.float64):
    """rel [N, g*g], images [N or 1, 3, R, R], lut [256, 3] -> (overlay uint8 [N, S, S, 3], 255 m [N, S, S], 255 cam / M
    [N, S, S, 3] unfloored), computed in `dtype`."""
    rel, images, lut = rel.detach().cpu().to(dtype), images.detach().cpu().to(dtype), lut.detach().cpu().to(dtype)
    N = rel.shape[0]
    g = int(round(rel.shape[1] ** 0.5))
    assert g * g == rel.shape[1]
    if images.shape[0] == 1:
        images = images.expand(N, -1, -1, -1)
    m = _minmax01(bil(rel.reshape(N, g, g), size), (1, 2))
    xn = _minmax01(bil(images, size), (1, 2, 3)).permute(0, 2, 3, 1)
    m255 = 255 * m
    k = m255.floor().long().clamp(max=255)
    cam = lut[k] + xn
    M = cam.amax(dim=(1, 2, 3), keepdim=True)
    c255 = torch.where(M != 0, 255 * cam / torch.where(M != 0, M, torch.ones_like(M)), torch.zeros_like(cam))
    return c255.floor().clamp(0, 255).to(torch.uint8), m255, c255


def fragile_mask(m255, c255):
    """[N, S, S] bool: the table row or one of the three bytes comes from a floor within DELTA of an integer"""
    near = lambda x: (x - x.round()).abs() <= DELTA
    return near(m255) | near(c255).any(dim=-1)


def compare(got, ref):
    """`got` uint8 [N, S, S, 3] against overlay_ref's triple: every non-fragile pixel equal, every fragile pixel within
    FRAGILE_LEVELS.  Returns (fragile pixels, pixels, mismatches outside the fragile set, worst fragile difference)."""
    want, m255, c255 = ref
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == torch.uint8, (got.shape, got.dtype, want.shape)
    frag = fragile_mask(m255, c255)
    diff = (got.int() - want.int()).abs().amax(dim=-1)
    bad = int((diff[~frag] != 0).sum())
    worst = int(diff[frag].max()) if frag.any() else 0
    return int(frag.sum()), frag.numel(), bad, worst
