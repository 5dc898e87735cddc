#!/usr/bin/env python3
"""Contrastive fine-tune of CLIP on (image, label) groups - the loop of /root/reference/CLIP/train.py:101-217 on the MI355X
`clip` package: class-balanced K-way groups (ClipPairDataset), `model(image, text)`, symmetric cross-entropy, HF-AdamW with
linear warm-up, per-epoch evaluation, periodic state_dict checkpoints in the OpenAI key layout.

    python scripts/train_clip.py --json all.json --image-path data/ --key violation_type --combination-num 9
    python scripts/train_clip.py --synthetic --model test-small --epochs 1 --max-steps 3        # offline smoke run

Differences from the reference script, on purpose: constants became flags; TensorBoard (not installed) became one JSON line per
step on stdout; `--fused-loss` uses clip.contrastive_loss (fused logits + CE, the data-parallel form under torchrun).

`--class-aware` (implies the fused loss) is where `--batch-size G > 1` becomes meaningful: G groups of the same K labels hold
every text G times, and the pairwise loss pushes each image away from the G-1 copies of its own text.  With the flag the batch's
distinct texts are encoded once (clip.unique_texts), every text of an image's class is its positive (clip.contrastive_loss with
labels= / text_labels=), and the logged accuracy counts an arg-max on the image's class as a hit.

`--loss sigmoid` (implies the fused path) swaps the objective for SigLIP's pairwise sigmoid loss (clip.SigmoidLoss): every
(image, text) cell is scored on its own against a learnable `logit_bias` (`--logit-bias-init`, SigLIP's -10), which suits the
small batches of this loop.  It composes with `--class-aware` (distinct texts once, every text of the class a positive).  The
bias is not a CLIP weight: it has an AdamW of its own at `--lr` under the same warm-up, it is logged with the loss, and it is
saved next to each checkpoint as `<checkpoint>_logit_bias.pt` - the checkpoint itself stays a pure OpenAI-layout state_dict.

`--distill-from {pretrained|PATH}` (implies the fused path) adds `--distill-weight` times clip.distill_loss to whichever hard
loss the run chose: a second, frozen model from clip.load - `pretrained`: the named model (`--distill-arch`, default `--model`)
as clip.load gives it, i.e. what the run started from; PATH: a state_dict checkpoint - encodes exactly the image and text
tensors the student encodes (under `--class-aware` the distinct texts, once), in eval mode under no_grad, and the student's
similarity rows are pulled towards the teacher's (KL, both directions).  A few thousand pairs otherwise make the towers forget
what zero-shot heads and free-text search rely on.  The teacher is never handed to the optimiser; its input resolution and
token layout must be the student's.  The step log gains `distill` (the KL term) and `agree` (the share of images whose
arg-max text is the teacher's)."""
from __future__ import annotations

import argparse
import os
import tempfile

import _common as C  # noqa: F401  (path setup)
import torch
from torch.utils.data import DataLoader


def build_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="state_dict to start from (train.py:108-111)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--image-path", default="")
    ap.add_argument("--key", default="violation_type")
    ap.add_argument("--combination-num", type=int, default=9)
    ap.add_argument("--train-ratio", type=float, default=0.8)
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=1, help="groups per step (train.py:138: 1 group of K pairs)")
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--warmup-steps", type=int, default=5000)
    ap.add_argument("--save-every", type=int, default=100)
    ap.add_argument("--out-dir", default="models")
    ap.add_argument("--name", default="clip_balance")
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many optimiser steps (0: run all epochs)")
    ap.add_argument("--fused-loss", action="store_true")
    ap.add_argument("--class-aware", action="store_true",
                    help="same-text pairs are positives: encode each distinct text once, class-aware fused loss (for --batch-size > 1)")
    ap.add_argument("--loss", choices=("softmax", "sigmoid"), default="softmax",
                    help="sigmoid: SigLIP's pairwise sigmoid loss with a learnable logit bias (implies the fused path)")
    ap.add_argument("--logit-bias-init", type=float, default=-10.0, help="initial logit bias of --loss sigmoid")
    ap.add_argument("--distill-from", default=None, metavar="{pretrained|PATH}",
                    help="distil from a frozen teacher: 'pretrained' (clip.load of --distill-arch) or a state_dict checkpoint "
                         "(implies the fused path)")
    ap.add_argument("--distill-arch", default=None, metavar="NAME", help="model name of '--distill-from pretrained' (default: --model)")
    ap.add_argument("--distill-weight", type=float, default=1.0, help="total = hard + this * distill")
    ap.add_argument("--synthetic", action="store_true", help="generated images + labels, seeded weights, byte tokenizer")
    ap.add_argument("--seed", type=int, default=567)
    C.add_optim_args(ap)
    return ap


def check_teacher(model, teacher) -> None:
    """The teacher encodes the very tensors the student encodes: refuse one that wants other pixels or other tokens."""
    a, b = model.visual.input_resolution, teacher.visual.input_resolution
    if a != b:
        raise ValueError(f"--distill-from: the teacher's input resolution is {b}, the student's {a}; both encode the same "
                         "preprocessed images")
    for what in ("context_length", "vocab_size"):
        a, b = getattr(model, what), getattr(teacher, what)
        if a != b:
            raise ValueError(f"--distill-from: the teacher's {what} is {b}, the student's {a}; both encode the same token rows")


def load_teacher(args, model, device):
    """(frozen teacher in eval mode, clip.DistillLoss holding its scale) of --distill-from, or (None, None)"""
    if args.distill_from is None:
        return None, None
    import clip
    if args.distill_from == "pretrained":
        name = args.distill_arch or args.model
    elif os.path.isfile(args.distill_from):
        name = args.distill_from
    else:
        raise ValueError(f"--distill-from: {args.distill_from!r} is neither 'pretrained' nor a checkpoint file")
    teacher, _ = clip.load(name, device=device, jit=False)
    check_teacher(model, teacher)
    teacher.eval()
    teacher.requires_grad_(False)
    return teacher, clip.DistillLoss(teacher.logit_scale.detach().exp()).to(device)


def evaluate(model, loader, device):
    """train.py:191-207: accuracy of arg-max(logits_per_image) against arange over the test groups"""
    model.eval()
    hit = tot = 0
    with torch.no_grad():
        for image, text in loader:
            image, text = image.to(device).flatten(0, 1), text.to(device).flatten(0, 1)
            logits_i, _ = model(image, text)
            label = torch.arange(image.shape[0], device=device)
            hit += int((logits_i.argmax(1) == label).sum())
            tot += image.shape[0]
    model.train()
    return hit / max(tot, 1)


def main(argv=None):
    args = build_args().parse_args(argv)
    import clip
    from clip import optim as coptim
    from clip.data import ClipPairDataset
    torch.manual_seed(args.seed)
    device = torch.device("cuda:0")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        args.json, args.image_path = C.make_synthetic_annotations(tmp.name), tmp.name
    model, preprocess = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    teacher, distill = load_teacher(args, model, device)
    tokenize = C.get_tokenize(model)
    mk = lambda split: ClipPairDataset(preprocess, args.json, args.image_path, args.train_ratio, args.key, split,   # noqa: E731
                                       args.combination_num, tokenize=tokenize)
    train_ds, test_ds = mk("train"), mk("test")
    train_dl = DataLoader(train_ds, batch_size=args.batch_size, shuffle=True, num_workers=args.workers)
    test_dl = DataLoader(test_ds, batch_size=args.batch_size, shuffle=False, num_workers=args.workers)
    model.train()
    opt = C.make_optimizer(model, args)                                                     # train.py:143 (+ groups, clipping, EMA)
    initial = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()} if args.wise_ft is not None else None
    sched = coptim.get_linear_schedule_with_warmup(opt, args.warmup_steps, args.epochs * len(train_dl))   # train.py:145-147
    ce = torch.nn.CrossEntropyLoss()
    sig = bias_opt = bias_sched = None
    if args.loss == "sigmoid":
        sig = clip.SigmoidLoss(init_bias=args.logit_bias_init).to(device)
        bias_opt = torch.optim.AdamW(sig.parameters(), lr=args.lr, weight_decay=0.0)
        bias_sched = coptim.get_linear_schedule_with_warmup(bias_opt, args.warmup_steps, args.epochs * len(train_dl))
    os.makedirs(args.out_dir, exist_ok=True)
    step = 0
    for epoch in range(1, args.epochs + 1):
        for image, text in train_dl:                                                        # train.py:157
            image, text = image.to(device).flatten(0, 1), text.to(device).flatten(0, 1)     # [G, K, ...] -> [G*K, ...]
            opt.zero_grad()
            if bias_opt is not None:
                bias_opt.zero_grad()
            label = torch.arange(image.shape[0], device=device)
            encoded = text                                                                  # the token rows the text tower sees
            if args.class_aware:
                text_u, inverse = clip.unique_texts(text)                                   # [U, 77], text == text_u[inverse]
                fi, ft = model.encode_image_text(image, text_u)                             # the text tower sees U rows, not G*K
                encoded = text_u
                text_ids = torch.arange(text_u.shape[0], device=device)
                if sig is not None:
                    loss, stats = sig(fi, ft, model.logit_scale, labels=inverse, text_labels=text_ids)
                else:
                    loss, stats = clip.contrastive_loss(fi, ft, model.logit_scale, None, labels=inverse, text_labels=text_ids)
                acc = float(stats[1]) / image.shape[0]
            elif sig is not None:
                fi, ft = model.encode_image_text(image, text)
                loss, stats = sig(fi, ft, model.logit_scale)
                acc = float(stats[1]) / image.shape[0]
            elif args.fused_loss or teacher is not None:
                fi, ft = model.encode_image_text(image, text)
                loss, stats = clip.contrastive_loss(fi, ft, model.logit_scale, None)
                acc = float(stats[1]) / image.shape[0] if len(stats) > 1 else float("nan")
            else:
                logits_i, logits_t = model(image, text)                                     # train.py:161
                loss = (ce(logits_i, label) + ce(logits_t, label)) / 2                      # train.py:164-166
                acc = float((logits_i.argmax(1) == label).float().mean())                   # train.py:173
            extra = {}
            if teacher is not None:
                with torch.no_grad():
                    tfi, tft = teacher.encode_image_text(image, encoded)                    # the tensors the student encoded
                hard = loss
                soft, dstats = distill(fi, ft, model.logit_scale, tfi, tft)
                loss = hard + args.distill_weight * soft
                extra = dict(hard=round(float(hard.detach()), 6), distill=round(float(dstats[0]), 6),
                             agree=round(float(dstats[1]) / image.shape[0], 4))
            loss.backward()
            opt.step()
            sched.step()
            if sig is not None:
                bias_opt.step()
                bias_sched.step()
                extra.update(logit_bias=round(float(sig.logit_bias.detach()), 6))
            step += 1
            C.log_line(epoch=epoch, step=step, loss=round(float(loss.detach()), 6), accuracy=round(acc, 4), lr=sched.get_last_lr()[0],
                       **C.optim_log(opt), **extra)
            if args.max_steps and step >= args.max_steps:
                break
        test_acc = evaluate(model, test_dl, device)
        C.log_line(epoch=epoch, testing_accuracy=round(test_acc, 4))
        if epoch % args.save_every == 0 or (args.max_steps and step >= args.max_steps) or epoch == args.epochs:
            path = os.path.join(args.out_dir, f"{args.name}_comb{args.combination_num}_{epoch}.pt")
            torch.save(model.state_dict(), path)                                            # train.py:211-217
            C.log_line(saved=path)
            if sig is not None:
                side = path[:-3] + "_logit_bias.pt"
                torch.save(sig.logit_bias.detach().cpu(), side)
                C.log_line(saved=side)
            last = args.epochs == epoch or bool(args.max_steps and step >= args.max_steps)
            C.save_side_weights(opt, model, path, initial if last else None, args.wise_ft)
        if args.max_steps and step >= args.max_steps:
            break
    if tmp is not None:
        tmp.cleanup()
    return step


if __name__ == "__main__":
    main()
