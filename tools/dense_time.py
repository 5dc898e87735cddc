#!/usr/bin/env python3
"""Milliseconds and peak device memory of the dense-map head (after the features: clip.segment's two launches,
csrc/dense_classes.hip, plus DenseResult.overlay's third) against the same arithmetic as torch ops on the device:
F.normalize of both sides, matmul, softmax, F.interpolate(bilinear) of every class map to the picture size, max / argmax,
the threshold and the palette gather.  Shapes: ViT-B/32 (grid 7, E 512, 224 x 224) and ViT-L/14@336px (grid 24, E 768,
336 x 336), B images, C classes.  Device events around every call after `--warmup` calls, the median of `--reps`; the two
alternate in one process.  Peak memory is torch's allocator peak over one call, above what was live before it.  Also checks
that the two label maps agree on at least 99.9 % of the pixels.  Prints one JSON line per shape and a markdown table.

    python tools/dense_time.py [--reps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def hip_head(feat, text, scale, g, S, pal):
    from cclip_hip import ops
    B, C = feat.shape[0] // (g * g), text.shape[0]
    probs = torch.empty(B, C, g * g, device=feat.device)
    ops.dense_class_probs(feat, text, scale, g * g, probs)
    labels = torch.empty(B, S, S, device=feat.device, dtype=torch.uint8)
    conf = torch.empty(B, S, S, device=feat.device)
    out = torch.empty(B, S, S, 3, device=feat.device, dtype=torch.uint8)
    ops.dense_label_map(probs.view(B, C, g, g), S, labels, conf, min_conf=0.2, overlay=out, palette=pal)
    return labels, out


def torch_head(feat, text, scale, g, S, pal):
    B, C = feat.shape[0] // (g * g), text.shape[0]
    logits = scale * F.normalize(feat, dim=1) @ F.normalize(text, dim=1).t()
    probs = logits.softmax(dim=1).view(B, g, g, C).permute(0, 3, 1, 2)
    up = F.interpolate(probs, size=(S, S), mode="bilinear", align_corners=False)
    conf, arg = up.max(dim=1)
    labels = torch.where(conf < 0.2, torch.full_like(arg, 255), arg).to(torch.uint8)
    return labels, pal[labels.long()]


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    import clip
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, g, E, S, B, C in (("ViT-B/32", 7, 512, 224, 1, 9), ("ViT-B/32", 7, 512, 224, 64, 9), ("ViT-B/32", 7, 512, 224, 64, 128),
                                ("ViT-L/14@336px", 24, 768, 336, 16, 9)):
        feat = torch.randn(B * g * g, E, device="cuda", generator=gen)
        text = torch.randn(C, E, device="cuda", generator=gen)
        pal = clip.default_palette(C).cuda()
        fns = dict(hip=lambda: hip_head(feat, text, 100.0, g, S, pal), torch=lambda: torch_head(feat, text, 100.0, g, S, pal))
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        same = float((fns["hip"]()[0] == fns["torch"]()[0]).float().mean())
        assert same >= 0.999, f"kernel and torch restatement agree on only {same:.5f} of the labels"
        times = dict(hip=[], torch=[])
        for _ in range(args.reps):
            for k, fn in fns.items():
                times[k].append(_event_ms(fn))
        line = dict(model=name, B=B, C=C, grid=g, E=E, size=S, reps=args.reps, labels_equal=round(same, 6),
                    ms={k: round(statistics.median(v), 4) for k, v in times.items()},
                    peak_mb={k: round(_peak_mb(fn), 2) for k, fn in fns.items()})
        print(json.dumps(line))
        rows.append(line)
    print("| model | B | C | HIP (ms) | torch ops (ms) | HIP peak (MB) | torch peak (MB) |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['model']} | {r['B']} | {r['C']} | {r['ms']['hip']} | {r['ms']['torch']} | {r['peak_mb']['hip']} | {r['peak_mb']['torch']} |")


if __name__ == "__main__":
    main()
