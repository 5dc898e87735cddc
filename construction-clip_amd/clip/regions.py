"""Region-level entry points: embed or zero-shot-classify every box of a photo.  The reference's service already has the
boxes (application.py:51-70 runs a detector and `/detect`, :248, returns {"boxes", "scores", "labels"}) but never shows them
to CLIP; here one `DevicePreprocess.regions` call turns all of them into model inputs (one upload, three launches, each row
bit-identical to `preprocess(image.crop(box))`) and the towers run on the result.

An `EmbeddingIndex` takes the features as they are: `index.add(encode_regions(model, image, boxes), metadata=[(file, box), ...])`
makes boxes searchable by text (`search_text`) or by another region.  `clip_caption.Captioner.describe` accepts preprocessed
tensors, so `captioner.describe(pre.regions(image, boxes))` captions every box."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .preprocess_device import DevicePreprocess


def _preprocess_for(model, preprocess: Optional[DevicePreprocess]) -> DevicePreprocess:
    if preprocess is not None:
        return preprocess
    return DevicePreprocess(model.visual.input_resolution, device=model.logit_scale.device)


@torch.no_grad()
def encode_regions(model, image, boxes, preprocess: Optional[DevicePreprocess] = None, chunk: int = 256) -> torch.Tensor:
    """Image features [K, D] of the K boxes of `image` (PIL image or uint8 HWC array / tensor; boxes [K, 4] as (x0, y0, x1, y1),
    ints or floats - see clip.preprocess_device.normalize_boxes): `model.encode_image` of `preprocess.regions(image, boxes)`,
    `chunk` boxes per encode.  `preprocess` defaults to a DevicePreprocess at the model's input resolution."""
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    x = _preprocess_for(model, preprocess).regions(image, boxes)
    if x.shape[0] <= chunk:
        return model.encode_image(x)
    return torch.cat([model.encode_image(x[s:s + chunk]) for s in range(0, x.shape[0], chunk)])


@torch.no_grad()
def classify_regions(classifier, image, boxes, preprocess: Optional[DevicePreprocess] = None,
                     chunk: int = 256) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
    """`ZeroShotClassifier.__call__` per box: (similarity [K, P] softmax, indices [K], labels list), with the classifier's
    cached text features.  Pass the features of one `encode_regions` call to several classifiers through their
    `image_features=` argument to encode the boxes once."""
    features = encode_regions(classifier.model, image, boxes, preprocess=preprocess, chunk=chunk)
    return classifier(image_features=features)
