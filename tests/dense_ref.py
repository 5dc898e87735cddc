"""float64 references of the dense zero-shot maps (clip/dense.py, csrc/dense_classes.hip, BlockStack.dense_tail), written with
index arithmetic of their own - not with F.normalize / F.interpolate, which tests/test_dense_ref_cpu.py holds them against - and
the seeded inputs the CPU and the GPU tests share.

The label comparison.  A label is an arg-max over upsampled fp32 probabilities: where the float64 best and runner-up are closer
than FRAGILE (1e-5: at most eight fp32 roundings on values <= 1 stay below 1e-6; ten times that) fp32 cannot decide, and either
of the two classes is accepted.  An EXACT float64 tie (margin 0: identical class maps) is not fragile - the kernel's samples of
two identical maps are identical too, and the lower index must win.  The same width applies around min_conf."""
from __future__ import annotations

import torch

FRAGILE = 1e-5
CONF_TOL = 1e-6
NONE_LABEL = 255


# ---- class probabilities -----------------------------------------------------------------------
def class_probs_ref(feat: torch.Tensor, text: torch.Tensor, scale: float, patches: int):
    """(probs, logits) float64 [B, C, patches] from feat [B * patches, E] and text [C, E] as given (fp32 values, exact in float64):
    cosine with inverse norms taken as 0 for a zero row, times scale, softmax over the classes."""
    f, t = feat.double(), text.double()
    fn, tn = f.pow(2).sum(1).sqrt(), t.pow(2).sum(1).sqrt()
    fi = torch.where(fn > 0, 1.0 / fn.clamp_min(1e-300), torch.zeros_like(fn))
    ti = torch.where(tn > 0, 1.0 / tn.clamp_min(1e-300), torch.zeros_like(tn))
    logits = float(scale) * (f @ t.t()) * fi[:, None] * ti[None, :]            # [M, C]
    z = logits - logits.max(dim=1, keepdim=True).values
    e = z.exp()
    probs = e / e.sum(dim=1, keepdim=True)
    B = f.shape[0] // patches
    to_maps = lambda a: a.view(B, patches, -1).permute(0, 2, 1).contiguous()   # noqa: E731
    return to_maps(probs), to_maps(logits)


def probs_case(B: int, g: int, C: int, E: int, seed: int = 0):
    """fp32 (feat [B g^2, E], text [C, E], scale): unnormalised rows of mixed length, CLIP's largest logit scale."""
    gen = torch.Generator().manual_seed(1000 + seed)
    feat = torch.randn(B * g * g, E, generator=gen) * (0.5 + 2.0 * torch.rand(B * g * g, 1, generator=gen))
    text = torch.randn(C, E, generator=gen) * (0.5 + 2.0 * torch.rand(C, 1, generator=gen))
    return feat, text, 100.0


PROBS_CASES = [(1, 1, 1, 4), (2, 2, 3, 32), (3, 3, 255, 48), (2, 7, 5, 512), (1, 24, 9, 768)]     # (B, g, C, E)


def class_probs_fp32(feat, text, scale, patches):
    """the same arithmetic as plain fp32 torch ops (what the error bound of the kernel test is measured on)"""
    import torch.nn.functional as F
    logits = float(scale) * F.normalize(feat.float(), dim=1) @ F.normalize(text.float(), dim=1).t()
    probs = logits.softmax(dim=1)
    B = feat.shape[0] // patches
    return probs.view(B, patches, -1).permute(0, 2, 1).contiguous()


# ---- label map ---------------------------------------------------------------------------------
def _axis(S: int, g: int):
    i = torch.arange(S, dtype=torch.float64)
    s = ((i + 0.5) * (g / S) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(g - 1)
    i1 = (i0 + 1).clamp_max(g - 1)
    return i0, i1, s - i0.double()


def upsample_ref(maps: torch.Tensor, S: int) -> torch.Tensor:
    """[..., g, g] -> float64 [..., S, S]: bilinear, half-pixel centres, source index clamped at 0 (align_corners=False)."""
    m = maps.double()
    g = m.shape[-1]
    i0, i1, w = _axis(S, g)
    rows = m[..., i0, :] * (1 - w)[:, None] + m[..., i1, :] * w[:, None]
    return rows[..., :, i0] * (1 - w) + rows[..., :, i1] * w


def label_map_ref(probs: torch.Tensor, S: int, min_conf: float = 0.0) -> dict:
    """probs [B, C, g, g] -> labels int64 [B, S, S] (lowest arg-max; 255 below min_conf), conf float64, and for compare_labels the
    arg-max before thresholding, the runner-up class and the top-two margin."""
    up = upsample_ref(probs, S)                                  # [B, C, S, S]
    conf, arg = up.max(dim=1)                                    # torch.max returns the first maximum
    C = up.shape[1]
    if C > 1:
        masked = up.scatter(1, arg[:, None], float("-inf"))
        second_v, second = masked.max(dim=1)
        margin = conf - second_v
    else:
        second, margin = arg.clone(), torch.full_like(conf, float("inf"))
    labels = torch.where(conf < min_conf, torch.full_like(arg, NONE_LABEL), arg)
    return dict(labels=labels, conf=conf, arg=arg, second=second, margin=margin, min_conf=float(min_conf), up=up)


def compare_labels(got: torch.Tensor, ref: dict, fragile: float = FRAGILE, conf_tol: float = CONF_TOL):
    """(number of wrong pixels, share of fragile pixels).  A pixel is right when it carries the reference's class; or, where
    0 < margin < fragile, the runner-up; or, where conf is within conf_tol of min_conf, 255 or either admissible class."""
    got = got.long().cpu()
    arg, second, margin, conf = ref["arg"], ref["second"], ref["margin"], ref["conf"]
    frag = (margin > 0) & (margin < fragile)
    near_thr = (conf - ref["min_conf"]).abs() < conf_tol
    below = conf < ref["min_conf"]
    cls_ok = (got == arg) | (frag & (got == second))
    ok = torch.where(near_thr, cls_ok | (got == NONE_LABEL), torch.where(below, got == NONE_LABEL, cls_ok))
    return int((~ok).sum()), float((frag | near_thr).double().mean())


def label_case(g: int, S: int, C: int, B: int, seed: int = 0) -> torch.Tensor:
    """fp32 probs [B, C, g, g]: a softmax over classes of smooth-ish random logits (regions, not salt and pepper)"""
    gen = torch.Generator().manual_seed(2000 + seed)
    return (3.0 * torch.randn(B, C, g, g, generator=gen)).softmax(dim=1).contiguous()


LABEL_CASES = [(7, 224, 5, 1), (2, 5, 3, 3), (3, 17, 2, 2), (24, 336, 4, 1), (1, 9, 3, 1)]        # (g, S, C, B)


def overlay_ref(labels: torch.Tensor, palette: torch.Tensor, photo=None, a8: int = 256) -> torch.Tensor:
    """uint8 [B, S, S, 3] from uint8 labels: palette[label], or (photo (256 - a8) + palette[label] a8 + 128) >> 8"""
    col = palette.cpu().long()[labels.cpu().long()]
    if photo is None:
        return col.to(torch.uint8)
    return ((photo.cpu().long() * (256 - a8) + col * a8 + 128) >> 8).to(torch.uint8)


# ---- the tower side ----------------------------------------------------------------------------
def _ln64(x, w, b):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    return (x - mu) / (var + 1e-5).sqrt() * w.double() + b.double()


def dense_tail_ref(sd: dict, x: torch.Tensor, mode: str = "value", prefix: str = None, heads: int = None) -> torch.Tensor:
    """The last image block as dense CLIP runs it, float64: x [B, T, D] (the stream entering it) -> [B, T, D].
    xn = ln_1(x); v = xn W_v^T + b_v; "value": a = v; "qq" / "kk": a = softmax(s s^T / 8) v per 64-wide head with s = q or k;
    result a W_o^T + b_o - no residual, no MLP."""
    from oracle import clip_oracle as O
    cfg = O.infer_config(sd)
    p = prefix or f"visual.transformer.resblocks.{cfg['vision_layers'] - 1}."
    H = heads or cfg["vision_heads"]
    B, T, D = x.shape
    xn = _ln64(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
    W, b = sd[p + "attn.in_proj_weight"].double(), sd[p + "attn.in_proj_bias"].double()
    v = xn @ W[2 * D:].t() + b[2 * D:]
    if mode == "value":
        a = v
    else:
        r0 = 0 if mode == "qq" else D
        s = xn @ W[r0:r0 + D].t() + b[r0:r0 + D]
        dh = D // H
        sh, vh = s.view(B, T, H, dh).transpose(1, 2), v.view(B, T, H, dh).transpose(1, 2)
        att = torch.softmax(sh @ sh.transpose(-1, -2) * dh ** -0.5, dim=-1)
        a = (att @ vh).transpose(1, 2).reshape(B, T, D)
    return a @ sd[p + "attn.out_proj.weight"].double().t() + sd[p + "attn.out_proj.bias"].double()


def tower_prefix_ref(sd: dict, image: torch.Tensor) -> torch.Tensor:
    """The stream entering the LAST image block, [B, T, D], from the oracle's own tower pieces (conv1, class / positional
    embedding, ln_pre, residual_block 0 .. L-2; fp32, as every golden feature of this suite is)."""
    import torch.nn.functional as F
    from oracle import clip_oracle as O
    cfg = O.infer_config(sd)
    x = F.conv2d(image.float(), sd["visual.conv1.weight"].float(), stride=cfg["vision_patch_size"])
    n, w = x.shape[0], x.shape[1]
    x = x.reshape(n, w, -1).permute(0, 2, 1)
    x = torch.cat([sd["visual.class_embedding"].float().expand(n, 1, w), x], dim=1) + sd["visual.positional_embedding"].float()
    x = O._layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
    for i in range(cfg["vision_layers"] - 1):
        x = O.residual_block(x, f"visual.transformer.resblocks.{i}.", sd, cfg["vision_heads"], None)
    return x


def dense_features_ref(sd: dict, image: torch.Tensor, mode: str = "value", drop_class_row: bool = True) -> torch.Tensor:
    """float64 [B, g, g, E]: tower_prefix_ref, dense_tail_ref, the class row dropped, ln_post and visual.proj on every patch row.
    drop_class_row=False is the planted fault of the CPU test (rows 0 .. P-1 instead of 1 .. P)."""
    x = tower_prefix_ref(sd, image)
    y = dense_tail_ref(sd, x.double(), mode)
    B, T, _ = y.shape
    g = round((T - 1) ** 0.5)
    y = y[:, 1:] if drop_class_row else y[:, :T - 1]
    f = _ln64(y, sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"].double()
    return f.view(B, g, g, -1)
