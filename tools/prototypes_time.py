#!/usr/bin/env python3
"""Milliseconds and allocator peak of ONE `DensePrototypes.add_features` call (csrc/dense_prototypes.hip: a zeroing launch when it
sets, the pooling launch, the slab-combine launch) at a realistic size - one 12-megapixel mask (4032 x 3024), the default window
plan of a ViT-B/16 tower (224-pixel windows on a 112-pixel lattice: 910 windows of 14 x 14 cells, E = 512), 9 classes - against
the torch composition of the same arithmetic: one-hot planes [C, H, W], a pooled share per window
(`F.adaptive_avg_pool2d(planes[:, y0:y1, x0:x1], g)`: with sides that are multiples of g its bins are the kernel's cells),
the threshold, and an einsum with the unit features.  The features are random (the tower is not part of either side).

The method of tools/dense_stitch_time.py: device events around every call after `--warmup` calls, the median of `--reps`
alternating calls in one process; the allocator peak is torch.cuda.max_memory_allocated() above what is live with the inputs
only.  Asserts equal patch counts and sums that agree to 1e-4 relative to the largest entry.  Prints one JSON line and a
markdown table.

    python tools/prototypes_time.py [--reps 5] [--warmup 1] [--size 4032x3024] [--window 224] [--grid 14] [--embed 512] [--classes 9]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from agreement_time import _peak  # noqa: E402
from dense_time import _event_ms  # noqa: E402


def make_mask(H: int, W: int, C: int) -> torch.Tensor:
    """random cells of 48 x 48 pixels (not a multiple of the 16-pixel patch cells: many cells are mixed), 3 % ignored"""
    rng = np.random.RandomState(0)
    cells = rng.randint(0, C, size=((H + 47) // 48, (W + 47) // 48)).astype(np.uint8)
    m = torch.from_numpy(np.ascontiguousarray(np.kron(cells, np.ones((48, 48), dtype=np.uint8))[:H, :W])).cuda()
    m[torch.rand(H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.03] = 255
    return m


def torch_prototypes(feat, mask, boxes, g: int, C: int, min_share8: int):
    """(sums [C, E], patches [C]) by one-hot planes, a pooled share per window and an einsum"""
    planes = (mask[None] == torch.arange(C, device=mask.device, dtype=torch.uint8)[:, None, None]).float()      # [C, H, W]
    share = torch.stack([F.adaptive_avg_pool2d(planes[:, y0:y1, x0:x1], g) for x0, y0, x1, y1 in boxes])     # [K, C, g, g]
    w = torch.where((share > 0) & (share * 256 >= min_share8), share, torch.zeros_like(share)).flatten(2)       # [K, C, P]
    unit = F.normalize(feat, dim=1).view(len(boxes), g * g, -1)
    return torch.einsum("kcp,kpe->ce", w, unit), (w > 0).sum(dim=(0, 2))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", default="4032x3024")
    ap.add_argument("--window", type=int, default=224)
    ap.add_argument("--grid", type=int, default=14)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--min-share", type=float, default=0.5)
    args = ap.parse_args(argv)
    import clip
    from cclip_hip import ops
    W, H = (int(v) for v in args.size.split("x"))
    g, E, C = args.grid, args.embed, args.classes
    boxes = clip.plan_windows(W, H, args.window)
    K = len(boxes)
    mask = make_mask(H, W, C)
    feat = torch.randn(K * g * g, E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    dev_boxes = torch.from_numpy(boxes.astype(np.int32)).cuda()
    box_list = [tuple(int(v) for v in b) for b in boxes]
    protos = clip.DensePrototypes(C, E, min_share=args.min_share)

    def hip():
        protos.add_features(feat, mask[None], dev_boxes, g)

    def ref():
        return torch_prototypes(feat, mask, box_list, g, C, protos.min_share8)

    hip()
    sums, patches = ref()
    assert torch.equal(protos.patches, patches), "patch counts differ"
    err = float((protos.sums - sums).abs().max() / sums.abs().max())
    assert err <= 1e-4, f"sums differ: {err:.3e} of the largest entry"
    again = clip.DensePrototypes(C, E, min_share=args.min_share)
    again.add_features(feat, mask[None], dev_boxes, g)
    assert torch.equal(again.sums, protos.sums) and torch.equal(again.weight, protos.weight), "two fresh calls differ"
    for _ in range(args.warmup):
        hip(), ref()
    hip_ms, ref_ms = [], []
    for _ in range(args.reps):
        hip_ms.append(_event_ms(hip))
        ref_ms.append(_event_ms(ref))
    line = dict(width=W, height=H, windows=K, grid=g, embed=E, classes=C, min_share8=protos.min_share8, reps=args.reps,
                hip_ms=round(statistics.median(hip_ms), 3), torch_ms=round(statistics.median(ref_ms), 3),
                hip_peak_mib=round(_peak(hip), 2), torch_peak_mib=round(_peak(ref), 1),
                workspace_mib=round(ops.dense_prototypes_workspace(K, g, C, E) / 2 ** 20, 2), rel_err=float(f"{err:.3e}"))
    print(json.dumps(line), flush=True)
    print("| mask | windows | C | add_features (ms) | torch composition (ms) | add_features peak (MiB) | torch peak (MiB) |\n|---|---|---|---|---|---|---|")
    print(f"| {W}x{H} | {K} | {C} | {line['hip_ms']} | {line['torch_ms']} | {line['hip_peak_mib']} | {line['torch_peak_mib']} |")


if __name__ == "__main__":
    main()
