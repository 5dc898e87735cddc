"""Shared pieces of the entry-point scripts: path setup, an offline stand-in tokenizer, and synthetic fixtures (annotation
JSON + generated images, an embedding pickle) so that every script runs end to end on a box with no network, no dataset, no
BPE vocabulary and no pretrained weights (`--synthetic`).  The scripts themselves are this repo's own statement of the
loops of CLIP/train.py, CLIP/predict.py and CLIP_prefix_caption/train.py on top of the MI355X `clip` / `clip_caption` packages."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SOT, EOT = 49406, 49407


def byte_tokenize(texts, context_length: int = 77, vocab_size: int = 49408) -> torch.Tensor:
    """Stand-in for clip.tokenize when the BPE vocabulary (bpe_simple_vocab_16e6.txt.gz) is not on disk: [SOT] + one id per
    UTF-8 byte + [EOT], zero padded, over-long texts cut (the real tokenizer raises instead).  SOT / EOT are the model's two
    largest ids (49406 / 49407 for the real vocabulary), so EOT stays the largest id of a row - all encode_text relies on."""
    if isinstance(texts, str):
        texts = [texts]
    sot, eot = vocab_size - 2, vocab_size - 1
    out = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, t in enumerate(texts):
        ids = [sot] + [1 + b % (vocab_size - 3) for b in t.encode("utf-8")][: context_length - 2] + [eot]
        out[i, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


def get_tokenize(model=None):
    """clip.tokenize when a vocabulary file is configured (CCLIP_BPE_PATH), the byte stand-in otherwise; sized for `model`."""
    import functools
    ctx = getattr(model, "context_length", 77)
    if os.environ.get("CCLIP_BPE_PATH"):
        import clip
        return functools.partial(clip.tokenize, context_length=ctx)
    return functools.partial(byte_tokenize, context_length=ctx, vocab_size=getattr(model, "vocab_size", 49408))


class ByteCaptionTokenizer:
    """Stand-in for AutoTokenizer.from_pretrained(<gpt2 type>) in --synthetic runs: ids 1 + byte (mod vocab), decode inverts it."""

    def __init__(self, vocab_size: int):
        self.vocab_size = vocab_size

    def encode(self, text: str):
        return [1 + (b % (self.vocab_size - 1)) for b in text.encode("utf-8")]

    def decode(self, ids):
        return bytes(max(0, int(i) - 1) % 256 for i in ids if int(i) > 0).decode("utf-8", errors="replace")


CLASSES = ["fall", "machine", "material", "shock", "gear", "puncture", "blast", "site", "carry"]


def make_synthetic_annotations(out_dir: str, per_class: int = 12, size: int = 96, seed: int = 567) -> str:
    """`<out_dir>/all.json` in the reference's annotation layout ({"annotations": [{id, caption_type, violation_type,
    violation_list, caption, file_name}]}) plus one generated RGB image per annotation (class-tinted noise)."""
    from PIL import Image
    os.makedirs(os.path.join(out_dir, "images"), exist_ok=True)
    rng = np.random.RandomState(seed)
    anns = []
    for c, name in enumerate(CLASSES):
        tint = rng.randint(40, 215, size=3)
        for j in range(per_class):
            fn = f"images/{name}_{j:03d}.png"
            px = np.clip(rng.normal(0, 40, size=(size + 8 * (j % 3), size, 3)) + tint, 0, 255).astype(np.uint8)
            Image.fromarray(px).save(os.path.join(out_dir, fn))
            anns.append({"id": len(anns), "caption_type": "violation" if j % 2 else "status", "violation_type": name,
                         "violation_list": f"{name} hazard {j % 4}", "caption": f"worker near {name} zone {j}", "file_name": fn})
    path = os.path.join(out_dir, "all.json")
    with open(path, "w") as f:
        json.dump({"type": "synthetic", "annotations": anns}, f)
    return path


def log_line(**kw) -> None:
    print(json.dumps(kw), flush=True)


# ---- the fine-tuning options of the two training scripts (clip.optim.AdamW's groups, clipping, EMA; WiSE-FT) ----
def add_optim_args(ap) -> None:
    ap.add_argument("--weight-decay", type=float, default=0.0, help="decoupled weight decay; biases, LayerNorms, logit_scale and the "
                    "learned positional / class embeddings are left out of it (see --decay-all)")
    ap.add_argument("--decay-all", action="store_true", help="one parameter group: --weight-decay on every parameter")
    ap.add_argument("--layer-decay", type=float, default=None, help="layer-wise learning-rate decay: lr * this ** (depth from the top)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, help="clip the total gradient norm to this")
    ap.add_argument("--skip-nonfinite", action="store_true", help="skip a step whose gradient norm is inf or NaN")
    ap.add_argument("--ema-decay", type=float, default=None, help="keep an EMA of the weights (with warm-up) and save it next to every "
                    "checkpoint as <checkpoint>_ema.pt")
    ap.add_argument("--wise-ft", type=float, default=None, metavar="ALPHA", help="at the end write (1 - ALPHA) * final + ALPHA * initial "
                    "weights as <last checkpoint>_wise.pt")


def make_optimizer(model, args):
    """clip.optim.AdamW for the options of add_optim_args; without any of them it is AdamW(model, lr), today's path"""
    from clip import optim as coptim
    kw = {}
    if args.layer_decay is not None:
        kw["param_groups"] = coptim.layer_decay_groups(model, args.layer_decay, 0.0 if args.decay_all else args.weight_decay)
        if args.decay_all:
            kw["weight_decay"] = args.weight_decay
            for g in kw["param_groups"]:
                del g["weight_decay"]
    elif args.weight_decay > 0 and not args.decay_all:
        kw["param_groups"] = coptim.no_decay_groups(model, args.weight_decay)
    elif args.weight_decay > 0:
        kw["weight_decay"] = args.weight_decay
    if args.clip_grad_norm is not None:
        kw["max_grad_norm"] = args.clip_grad_norm
    if args.skip_nonfinite:
        kw["skip_nonfinite"] = True
    if args.ema_decay is not None:
        kw.update(ema_decay=args.ema_decay, ema_warmup=True)
    return coptim.AdamW(model, lr=args.lr, **kw)


def optim_log(opt) -> dict:
    """the gradient norm and the skipped steps for a log line (one read-back each, where the optimiser keeps them)"""
    out = {}
    if opt.last_grad_norm is not None:
        out["grad_norm"] = round(float(opt.last_grad_norm), 6)
    if opt.skipped_steps is not None and opt.skip_nonfinite:
        out["skipped_steps"] = int(opt.skipped_steps)
    return out


def save_side_weights(opt, model, path: str, initial=None, alpha=None) -> None:
    """<path>_ema.pt for an optimiser that keeps an EMA; with `initial` and alpha, <path>_wise.pt: the WiSE-FT interpolation,
    written without disturbing the model (its masters are put back)"""
    from clip import optim as coptim
    if opt.ema_decay is not None and opt._ema is not None:
        torch.save({k: v.cpu() for k, v in opt.ema_state_dict().items()}, path[:-3] + "_ema.pt")
        log_line(saved=path[:-3] + "_ema.pt")
    if initial is not None and alpha is not None:
        final = {k: v.detach().clone() for k, v in model.state_dict().items()}
        coptim.interpolate_weights(model, initial, alpha)
        torch.save({k: v.cpu() for k, v in model.state_dict().items()}, path[:-3] + "_wise.pt")
        coptim.interpolate_weights(model, final, 1.0)
        log_line(saved=path[:-3] + "_wise.pt", wise_ft_alpha=alpha)
