"""Relevance maps: the reference's `interpret()` and its two display helpers (attention.py:14-69, 88-92,
115-117) on the MI355X `clip` package.

The reference keeps a second copy of CLIP that saves every block's attention probabilities and asks autograd for their
gradient.  Here CLIP.relevance() runs one training-shaped forward of both towers and a gradient-only backward in which a fused
HIP kernel (csrc/attention_relevance.hip) forms each block's map from the block's saved q / k / v / log-sum-exp and its
attention-output gradient; the probabilities and their gradient never reach memory.  Blocks expose no `attn_probs` and there
is no autograd through them.

interpret() forms the whole T x T matrices and so ends at 128 tokens (ViT-B/32).  interpret_rows() returns exactly the rows the
reference's callers read - the class-token row of the image tower and each caption's EOT row - through a streaming row kernel
(csrc/attention_relevance_row.hip) at any sequence length: ViT-B/16, ViT-L/14, ViT-L/14@336px.

relevance_overlay() is show_image_relevance's picture (attention.py:77-96): the upsampled, normalised map through a colour
table, added to the min-max normalised image and rescaled to 8 bits, for N maps in one launch (csrc/relevance_overlay.hip).
text_heat_html() is a dependency-free stand-in for show_heatmap_on_text's captum record (attention.py:113-143).
"""
from __future__ import annotations

import html
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from cclip_hip import ops


def interpret(image: torch.Tensor, texts: torch.Tensor, model, device=None, start_layer: int = -1,
              start_layer_text: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Chefer et al. relevance of each (image, text) pair for its own score logits_per_image[i, i].

    image: [1, 3, R, R] (repeated over the N texts, as in the reference) or [N, 3, R, R] (pair i = image i, text i);
    texts: [N, context_length] token ids.  start_layer / start_layer_text: -1 = the last block only; any other value v keeps
    the blocks i >= v (the reference's rule).  Returns (text_relevance fp32 [N, T_txt, T_txt], image_relevance fp32
    [N, T_img - 1]) on the model's device.  Sequences of more than 128 tokens (ViT-B/16, ViT-L/14) raise NotImplementedError:
    use interpret_rows, which returns the rows of these matrices that the display helpers read, at any length."""
    image, texts = _pairs(image, texts, device, "interpret")
    r_img, r_txt = model.relevance(image, texts, start_layer=start_layer, start_layer_text=start_layer_text)
    return r_txt, r_img[:, 0, 1:]


def interpret_rows(image: torch.Tensor, texts: torch.Tensor, model, device=None, start_layer: int = -1,
                   start_layer_text: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """interpret() for towers of any length: the same arguments, pairing and start-layer rule.  Returns (text_relevance fp32
    [N, T_txt], image_relevance fp32 [N, T_img - 1]): image_relevance is what interpret returns second, text_relevance[b] is
    row eot_b (caption b's EOT position) of what it returns first - the row text_row_scores reads."""
    image, texts = _pairs(image, texts, device, "interpret_rows")
    r_img, r_txt = model.relevance_rows(image, texts, start_layer=start_layer, start_layer_text=start_layer_text)
    return r_txt, r_img[:, 1:]


def _pairs(image, texts, device, what):
    """one image is repeated over the N texts (as in the reference); N images pair with the N texts"""
    if device is not None:
        image, texts = image.to(device), texts.to(device)
    N = texts.shape[0]
    if image.shape[0] == 1 and N != 1:
        image = image.expand(N, *image.shape[1:])
    elif image.shape[0] != N:
        raise ValueError(f"{what}: {image.shape[0]} images for {N} texts (give one image, or one per text)")
    return image, texts


def image_relevance_map(image_relevance: torch.Tensor, size: int = 224) -> torch.Tensor:
    """attention.py:88-92: the patch relevance [grid*grid] (or [N, grid*grid]) as a grid, bilinearly upsampled to
    size x size, min-max normalised to [0, 1] (per map; a constant map gives zeros).  Returns [size, size] (or [N, size, size])."""
    x = image_relevance.detach().float()
    single = x.dim() == 1
    x = x.reshape(-1, x.shape[-1])
    dim = int(round(x.shape[1] ** 0.5))
    if dim * dim != x.shape[1]:
        raise ValueError(f"image_relevance_map: {x.shape[1]} patches do not form a square grid")
    m = F.interpolate(x.reshape(-1, 1, dim, dim), size=size, mode="bilinear").reshape(-1, size, size)
    lo = m.amin(dim=(1, 2), keepdim=True)
    rng = m.amax(dim=(1, 2), keepdim=True) - lo
    m = torch.where(rng > 0, (m - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))
    return m[0] if single else m


def text_token_scores(text_relevance: torch.Tensor, tokens: torch.Tensor) -> Union[torch.Tensor, List[torch.Tensor]]:
    """attention.py:115-117: the EOT row's relevance of the caption tokens 1 .. EOT-1, normalised to sum 1.
    text_relevance [T, T] with tokens [T] gives one tensor; [N, T, T] with [N, T] gives a list of N."""
    if text_relevance.dim() == 3:
        return [text_token_scores(r, t) for r, t in zip(text_relevance, tokens)]
    eot = int(tokens.argmax(dim=-1))
    r = text_relevance[eot, 1:eot].float()
    return r / r.sum()


def text_row_scores(text_relevance_row: torch.Tensor, tokens: torch.Tensor) -> Union[torch.Tensor, List[torch.Tensor]]:
    """text_token_scores on interpret_rows' output: the EOT row itself, [T] with tokens [T] (one tensor) or [N, T] with [N, T]
    (a list of N).  row[1:eot] / row[1:eot].sum() - the values text_token_scores gives on the full matrix."""
    if text_relevance_row.dim() == 2:
        return [text_row_scores(r, t) for r, t in zip(text_relevance_row, tokens)]
    eot = int(tokens.argmax(dim=-1))
    r = text_relevance_row[1:eot].float()
    return r / r.sum()


def jet_table() -> torch.Tensor:
    """The default colour table of relevance_overlay: fp32 [256, 3], row k = the blue-cyan-yellow-red ramp at t = k / 255,
    r = clip(1.5 - |4t - 3|, 0, 1), g = clip(1.5 - |4t - 2|, 0, 1), b = clip(1.5 - |4t - 1|, 0, 1), channel order RGB (row 0 is
    blue, row 255 red).  It stands in for cv2.COLORMAP_JET: cv2 is not a dependency of this package.  cv2's own table - or any
    other [256, 3] table with values in [0, 1] - can be passed as `lut=`; reverse its last axis first, cv2 tables are BGR.  The
    reference adds the BGR heat map to the RGB image and swaps the sum once more (attention.py:78-80, 97), so its hot patches
    come out blue; that accident is not reproduced: hot is red here."""
    t = torch.arange(256, dtype=torch.float64) / 255
    return torch.stack([(1.5 - (4 * t - c).abs()).clamp(0, 1) for c in (3, 2, 1)], dim=1).float()


_JET = {}


def relevance_overlay(image_relevance: torch.Tensor, image: torch.Tensor, size: int = 224, lut: Optional[torch.Tensor] = None,
                      return_map: bool = False):
    """attention.py:77-96 (show_image_relevance without the matplotlib figure) on the device: image_relevance fp32 [N, grid*grid]
    as a grid, bilinearly upsampled to size x size and min-max normalised (image_relevance_map), looked up in the colour table
    (row min(floor(255 m), 255)), added to the image - fp32 [N, 3, R, R], or [1, 3, R, R] under all N maps - resampled to
    size x size and min-max normalised, and the sum scaled by its maximum to 8 bits.  Returns uint8 [N, size, size, 3] (HWC, RGB:
    `Image.fromarray(overlay[i].cpu().numpy())`) on the device of the inputs; with return_map also the fp32 [N, size, size]
    normalised maps.  image_relevance [grid*grid] with image [3, R, R] gives one [size, size, 3] (and [size, size]).
    lut: fp32 [256, 3] with values in [0, 1]; default jet_table().  One launch for all N; the map, the normalised image and the
    blend are never stored.  The inputs must be contiguous float32 cuda tensors."""
    single = image_relevance.dim() == 1
    rel = image_relevance.detach()
    img = image.detach()
    if single:
        rel = rel.unsqueeze(0)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if rel.dim() != 2 or rel.shape[0] < 1:
        raise ValueError(f"relevance_overlay: image_relevance must be [grid*grid] or [N, grid*grid], got {tuple(image_relevance.shape)}")
    N, P = rel.shape
    dim = int(round(P ** 0.5))
    if dim < 1 or dim * dim != P:
        raise ValueError(f"relevance_overlay: {P} patches do not form a square grid")
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise ValueError(f"relevance_overlay: image must be [3, R, R] or [N, 3, R, R], got {tuple(image.shape)}")
    if img.shape[0] not in (1, N):
        raise ValueError(f"relevance_overlay: {img.shape[0]} images for {N} maps (give one image, or one per map)")
    if lut is not None and tuple(lut.shape) != (256, 3):
        raise ValueError(f"relevance_overlay: lut must be [256, 3], got {tuple(lut.shape)}")
    dev = rel.device
    if lut is None:
        if dev not in _JET:
            _JET[dev] = jet_table().to(dev)
        lut = _JET[dev]
    else:
        lut = lut.detach().to(device=dev, dtype=torch.float32).contiguous()
    if not rel.is_cuda:
        raise ValueError(f"relevance_overlay: expected cuda tensors, got {dev} (no CPU path)")
    out = torch.empty(N, size, size, 3, device=dev, dtype=torch.uint8)
    m = torch.empty(N, size, size, device=dev, dtype=torch.float32) if return_map else None
    ops.relevance_overlay(rel, img, lut, size, out, m)
    if single:
        out, m = out[0], (m[0] if return_map else None)
    return (out, m) if return_map else out


def text_heat_html(pieces: Sequence[str], scores) -> str:
    """Host-only stand-in for show_heatmap_on_text's captum record (attention.py:113-143): one <span> per piece of the caption on a
    red background whose alpha is the piece's score over the largest score (scores <= 0 stay transparent), the text HTML-escaped.
    pieces: the caption's tokens (or characters); scores: as many numbers (a tensor, an array or a list) - text_row_scores of the
    caption, or its sums per piece."""
    vals = [float(s) for s in (scores.tolist() if hasattr(scores, "tolist") else scores)]
    pieces = list(pieces)
    if len(vals) != len(pieces):
        raise ValueError(f"text_heat_html: {len(pieces)} pieces, {len(vals)} scores")
    top = max(vals, default=0.0)
    spans = []
    for piece, v in zip(pieces, vals):
        alpha = min(max(v / top, 0.0), 1.0) if top > 0 and v == v else 0.0
        spans.append(f'<span style="background-color: rgba(255, 0, 0, {alpha:.3f})" title="{v:.4f}">{html.escape(str(piece))}</span>')
    return '<div class="text-heat" style="font-family: sans-serif; line-height: 1.8">' + "".join(spans) + "</div>"
