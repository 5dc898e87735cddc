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
"""
from __future__ import annotations

from typing import List, Tuple, Union

import torch
import torch.nn.functional as F


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
