#!/usr/bin/env python3
"""Say in words what is in every photo of an embedding pickle (scripts/extract_embeddings.py; CLIP_prefix_caption/parse_coco.py's
layout): encode a vocabulary file (one word or phrase per line) once with the text tower of `--model` / `--checkpoint`, and
write every stored embedding as a sparse, non-negative combination of those text rows (`clip.decompose`: SpLiCE, a fixed number
of FISTA iterations inside one launch of csrc/concept_codes.hip).  One JSON line per photo: {row, file_name, concepts: the `--top`
largest [name, weight], cosine, nnz, kkt} - `kkt` is the row's distance from the optimum, so a large one says `--iters` was too
few - then one summary line.

`--group-key violation_type` reads that key of every caption record and adds, before the summary, one line per value:
{group, size, top: the concepts with the largest mean weight in the group, distinctive: those whose group mean most exceeds
the overall mean} (`clip.concept_profile`, `clip.distinctive`); rows with an empty value are left out of the groups.
`--center` is SpLiCE's answer to the modality gap: the vocabulary's mean is taken off the text rows and the photos' own mean off
the photos.  `--template "a photo of {}"` wraps every vocabulary entry before it is tokenised.

    python scripts/explain_concepts.py --index embeddings.pkl --checkpoint clip.pt --vocab words.txt --center --group-key violation_type
    python scripts/explain_concepts.py --synthetic                                              # offline smoke run
"""
from __future__ import annotations

import argparse

import _common as C
import torch

SYNTHETIC_WORDS = ["worker", "helmet", "scaffold", "ladder", "crane", "guard rail", "exposed rebar"]


def synthetic_pickle(dictionary, per_class: int = 6, seed: int = 567):
    """Seeded stand-in for an embedding pickle, planted in the dictionary's own frame: photo j of class a is
    normalise(0.7 c_a + 0.5 c_b + a little noise), c_a the row of the class name and c_b that of one of SYNTHETIC_WORDS; every
    record carries its class as `violation_type`.  Returns (features fp32 [9 per_class, D], captions, pairs [rows, 2])."""
    g = torch.Generator().manual_seed(seed)
    c = dictionary.rows.float().cpu()
    n_cls, D = len(C.CLASSES), c.shape[1]
    cls = torch.arange(n_cls).repeat_interleave(per_class)
    other = n_cls + torch.arange(cls.numel()) % len(SYNTHETIC_WORDS)
    feats = 0.7 * c[cls] + 0.5 * c[other] + 0.05 / D ** 0.5 * torch.randn(cls.numel(), D, generator=g)
    caps = [{"file_name": f"images/{C.CLASSES[int(a)]}_{j:05d}.png", "clip_embedding": j, "caption": f"photo {j}",
             "violation_type": C.CLASSES[int(a)]} for j, a in enumerate(cls)]
    return torch.nn.functional.normalize(feats, dim=1), caps, torch.stack([cls, other], dim=1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", default=None, help="embedding pickle of scripts/extract_embeddings.py")
    ap.add_argument("--vocab", default=None, metavar="FILE", help="the concept vocabulary: one word or phrase per line")
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--checkpoint", default=None, help="fine-tuned state_dict (CLIP/train.py's clip.pt)")
    ap.add_argument("--template", default="{}", help="text around every vocabulary entry, e.g. 'a photo of {}'")
    ap.add_argument("--l1", type=float, default=0.1, help="sparsity weight: larger, fewer concepts per photo")
    ap.add_argument("--iters", type=int, default=200, help="FISTA iterations (fixed; read kkt)")
    ap.add_argument("--top", type=int, default=8, help="concepts printed per photo and per group")
    ap.add_argument("--max-terms", type=int, default=32, help="concepts kept per photo")
    ap.add_argument("--center", action="store_true", help="take the vocabulary's mean off the text rows and the photos' mean off the photos")
    ap.add_argument("--group-key", default=None, help="caption key whose values group the photos, e.g. violation_type")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--synthetic", action="store_true")
    args = ap.parse_args(argv)
    if not args.synthetic and (args.index is None or args.vocab is None):
        ap.error("--index and --vocab are required (or --synthetic)")
    if args.top < 1 or args.max_terms < args.top or args.iters < 0 or not args.l1 >= 0.0:
        ap.error("--top >= 1, --max-terms >= --top, --iters >= 0 and --l1 >= 0")
    if "{}" not in args.template:
        ap.error("--template must hold {}")
    if args.synthetic:
        args.model, args.center = "test-tiny", True
        if args.group_key is None:
            args.group_key = "violation_type"
    return args


def main(argv=None):
    args = parse_args(argv)
    import clip
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    device = torch.device("cuda:0")
    if args.synthetic:
        words = C.CLASSES + SYNTHETIC_WORDS
    else:
        words = [ln.strip() for ln in open(args.vocab) if ln.strip()]
        if not words:
            raise SystemExit(f"{args.vocab}: no vocabulary entry")
    model, _ = clip.load(args.model, device=device, jit=False)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model.eval()
    tokens = C.get_tokenize(model)([args.template.format(w) for w in words])
    dictionary = clip.ConceptDictionary.from_texts(model, tokens, names=words, dtype=dtype, center="mean" if args.center else None)
    del model
    if args.synthetic:
        feats, captions, _ = synthetic_pickle(dictionary)                  # planted in the (centred) frame of the dictionary
        index, center = clip.EmbeddingIndex(feats, dtype=dtype, metadata=captions), None
    else:
        index, center = clip.EmbeddingIndex.from_pickle(args.index, dtype=dtype), "mean" if args.center else None
        captions = index.metadata

    def field(row, key):
        cap = captions[row]
        return cap.get(key) if isinstance(cap, dict) else None

    N = len(index)
    dec = index.decompose(dictionary, l1=args.l1, iters=args.iters, max_terms=args.max_terms, center=center)
    idx, wts = dec.indices[:, :args.top].tolist(), dec.weights[:, :args.top].tolist()
    cosine, nnz, kkt = dec.cosine.tolist(), dec.nnz.tolist(), dec.kkt.tolist()
    lines = []
    for r in range(N):
        line = dict(row=r, file_name=field(r, "file_name"), concepts=[[dictionary.name(v), w] for v, w in zip(idx[r], wts[r]) if v >= 0],
                    cosine=cosine[r], nnz=nnz[r], kkt=kkt[r])
        lines.append(line)
        C.log_line(**line)
    groups = []
    if args.group_key:
        values = [field(r, args.group_key) for r in range(N)]
        names = sorted({v for v in values if v})
        slot = {v: i for i, v in enumerate(names)}
        profile = clip.concept_profile(dec, [slot[v] if v else -1 for v in values])
        apart = clip.distinctive(profile, args.top)
        top, at = torch.topk(profile.mean, min(args.top, len(dictionary)), dim=1)
        for gid, size, row_at, row_top in zip(profile.groups.tolist(), profile.counts.tolist(), at.tolist(), top.tolist()):
            line = dict(group=names[gid], size=size, top=[[dictionary.name(v), w] for v, w in zip(row_at, row_top) if w > 0],
                        distinctive=[[n, e] for n, e in apart[gid]])
            groups.append(line)
            C.log_line(**line)
    summary = dict(rows=N, vocabulary=len(dictionary), l1=args.l1, iters=args.iters, centred=bool(args.center), L=dictionary.L,
                   mean_nnz=sum(nnz) / N, truncated=int(dec.truncated.sum()), mean_cosine=sum(cosine) / N, worst_kkt=max(kkt),
                   groups=len(groups))
    C.log_line(summary=summary)
    return lines, groups, summary, dec


if __name__ == "__main__":
    main()
