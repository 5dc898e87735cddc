"""CLIPScore and RefCLIPScore (Hessel et al., EMNLP 2021): how well a caption matches its photo, without ground truth.

    CLIPScore(c, v)       = w max(cos(c, v), 0),  w = 2.5
    RefCLIPScore(c, R, v) = harmonic mean of CLIPScore(c, v) and max(max_{r in R} cos(c, r), 0)

The reference project measures captions with a character-level BLEU only (CLIP_prefix_caption/score.py, whose rouge() is a
stub); that needs ground-truth captions and never looks at the photo.  Here the two towers' outputs go straight into one
kernel launch (csrc/caption_select.hip) that scores every (image, candidate) pair, ranks the K candidates of each image and
names the best; nothing is read by the host between the towers and the answer.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from cclip_hip import ops

from .loss import unique_texts


class ClipScores(NamedTuple):
    """cos, clip_score and ref_clip_score (None without references) fp32 [N, K]; order int32 [N, K], the candidates of every
    image by (score descending, index ascending); best int32 [N] = order[:, 0].  All on the device."""
    cos: torch.Tensor
    clip_score: torch.Tensor
    ref_clip_score: Optional[torch.Tensor]
    order: torch.Tensor
    best: torch.Tensor


def _rows(features: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_floating_point():
        shape = tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__
        raise ValueError(f"{name} must be a 2-D float tensor of features, got {shape}")
    return features.detach().float().contiguous()


def csr_offsets(counts: Sequence[int]) -> list:
    """CSR offsets [N + 1] of per-image reference counts"""
    off = [0]
    for c in counts:
        if c < 0:
            raise ValueError(f"a reference count is negative: {list(counts)}")
        off.append(off[-1] + int(c))
    return off


@torch.no_grad()
def clip_score_features(image_features: torch.Tensor, text_features: torch.Tensor, w: float = 2.5,
                        reference_features: Optional[torch.Tensor] = None, reference_offsets: Optional[Sequence[int]] = None,
                        lm_mean: Optional[torch.Tensor] = None, lm_weight: float = 0.0, return_score: bool = False):
    """clip_score on features that are already computed: image_features [N, E], text_features [N * K, E] (row n * K + k =
    candidate k of image n; K is taken from the row counts), both raw tower outputs of any float dtype.  reference_features
    [Rtot, E] with reference_offsets, N + 1 CSR offsets on the host (image n's references are rows off[n] .. off[n + 1] - 1,
    possibly none).  lm_mean [N * K] with lm_weight adds the captioner's mean token log-probability to the ranking score
    (score = cos + lm_weight lm_mean); return_score: (ClipScores, score [N, K])."""
    img, txt = _rows(image_features, "image_features"), _rows(text_features, "text_features")
    N = img.shape[0]
    if N < 1:
        raise ValueError("need at least one image")
    if txt.shape[0] < N or txt.shape[0] % N:
        raise ValueError(f"text_features has {txt.shape[0]} rows for {N} images: need K rows per image, K >= 1")
    if txt.shape[1] != img.shape[1]:
        raise ValueError(f"image_features has {img.shape[1]} columns, text_features has {txt.shape[1]}")
    K = txt.shape[0] // N
    if (reference_features is None) != (reference_offsets is None):
        raise ValueError("give both reference_features and reference_offsets, or neither")
    ref = None if reference_features is None else _rows(reference_features, "reference_features")
    if lm_mean is not None:
        lm_mean = lm_mean.detach().float().reshape(-1).contiguous()
    cos, cs, rs, score, order, best = ops.caption_select(img, txt, K, lm_mean=lm_mean, ref=ref, ref_off=reference_offsets, w=float(w),
                                                         lm_weight=float(lm_weight))
    out = ClipScores(cos, cs, rs, order, best)
    return (out, score) if return_score else out


def candidate_tokens(tokens: torch.Tensor, N: int) -> Tuple[torch.Tensor, int]:
    """tokens [N, L] (one caption per image) or [N, K, L] -> (rows [N * K, L], K)"""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() not in (2, 3) or tokens.is_floating_point():
        shape = tuple(tokens.shape) if isinstance(tokens, torch.Tensor) else type(tokens).__name__
        raise ValueError(f"tokens must be an integer tensor [N, L] or [N, K, L], got {shape}")
    if tokens.shape[0] != N:
        raise ValueError(f"tokens are for {tokens.shape[0]} images, there are {N}")
    K = 1 if tokens.dim() == 2 else tokens.shape[1]
    if K < 1:
        raise ValueError("tokens hold no candidate (K = 0)")
    if K > ops.CAPTION_SELECT_MAX_K:
        raise NotImplementedError(f"K = {K} candidates per image; the kernel ranks at most {ops.CAPTION_SELECT_MAX_K}")
    return tokens.reshape(N * K, tokens.shape[-1]), K


def encode_distinct_texts(model, tokens: torch.Tensor, batch_size: int = 256) -> torch.Tensor:
    """fp32 [M, E] text features of the token rows [M, L]: every distinct row goes through the text tower once
    (clip.unique_texts) and its features are scattered back, so equal captions get equal bits.  (torch.unique learns the
    number of distinct rows on the host: the one wait, before the tower is enqueued.)"""
    uniq, inverse = unique_texts(tokens)
    feat = torch.cat([model.encode_text(uniq[s:s + batch_size]).float() for s in range(0, uniq.shape[0], batch_size)])
    return feat[inverse.long()].contiguous()


@torch.no_grad()
def clip_score(model, images: torch.Tensor, tokens: torch.Tensor, w: float = 2.5, references: Optional[Sequence[torch.Tensor]] = None,
               batch_size: int = 256) -> ClipScores:
    """CLIPScore of captions against their photos.  images: preprocessed [N, 3, R, R], or image features [N, E].  tokens:
    CLIP token rows [N, L] (one caption per image) or [N, K, L] (K candidates, which are also ranked: `order`, `best`).
    references: N token tensors [R_n, L], the ground-truth captions of each image (R_n may be 0) - adds RefCLIPScore.
    Identical token rows (candidates and references alike) are encoded once, so duplicate candidates tie exactly and the
    lower index wins.  The results stay on the device."""
    dev = model.logit_scale.device
    if not isinstance(images, torch.Tensor) or images.dim() not in (2, 4):
        shape = tuple(images.shape) if isinstance(images, torch.Tensor) else type(images).__name__
        raise ValueError(f"images must be [N, 3, R, R] or features [N, E], got {shape}")
    N = images.shape[0]
    rows, K = candidate_tokens(tokens, N)
    L = rows.shape[1]
    off = None
    if references is not None:
        if len(references) != N:
            raise ValueError(f"references: need one tensor per image ({N}), got {len(references)}")
        for r in references:
            if not isinstance(r, torch.Tensor) or r.dim() != 2 or r.shape[1] != L:
                shape = tuple(r.shape) if isinstance(r, torch.Tensor) else type(r).__name__
                raise ValueError(f"references: every entry must be [R_n, {L}] token rows, got {shape}")
        off = csr_offsets([r.shape[0] for r in references])
        rows = torch.cat([rows.to(dev)] + [r.to(device=dev, dtype=rows.dtype) for r in references])
    images = images.to(dev)
    if images.dim() == 4:
        img = torch.cat([model.encode_image(images[s:s + batch_size]).float() for s in range(0, N, batch_size)])
    else:
        img = images.float()
    feat = encode_distinct_texts(model, rows.to(dev), batch_size)
    txt, ref = feat[:N * K], (None if off is None else feat[N * K:])
    return clip_score_features(img, txt, w=w, reference_features=ref, reference_offsets=off)
