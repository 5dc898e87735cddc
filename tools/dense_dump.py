"""Bit-identity check of the dense-map kernels across a change that must not alter their results (a refactor of
csrc/dense_stitch.hip, dense_classes.hip, dense_refine.hip, label_pixels.h or bilinear.h, a compiler update): seeded inputs, one
SHA-256 per output tensor (dtype, shape and raw bytes), one line per tensor.

    python tools/dense_dump.py > before.txt        # on the build to compare against
    python tools/dense_dump.py > after.txt         # on the new build; then: diff before.txt after.txt

dense_stitch on every STITCH_CASES input of tests/dense_stitch_ref.py and on the three path cases (40 windows on a pixel: the
recompute loop; K = 300 small windows: the LDS list; K = 600 columns: the walk of all K boxes), each at min_conf 0 and at the
median of its own conf, without a picture, with a palette, and with a palette over a photo (alpha8 77), cover included;
dense_stitch_maps with and without cover; dense_maps_label on those maps with and without cover, at both thresholds, with and
without the picture.  dense_refine_prepare and 1 (long cases: 1, 2, 10) dense_refine_step on every case and guide of
tests/dense_refine_ref.py.  The last line counts cases and tensors.  Runs every launch twice and fails if a repeat differs."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "tests")]
from cclip_hip import ops  # noqa: E402
import dense_refine_ref as RR  # noqa: E402
import dense_stitch_ref as SR  # noqa: E402


def path_case(name):
    """the path cases of tests/test_dense_stitch_gpu.py, generators and seeds as there"""
    if name == "forty":
        H, W, g, C = 30, 41, 3, 4
        rng = np.random.default_rng(15)
        boxes = np.array([[rng.integers(0, 15), rng.integers(0, 10), rng.integers(26, 42), rng.integers(20, 31)] for _ in range(40)])
        return SR.stitch_maps(40, C, g, seed=15), boxes, H, W
    K = {"small": 300, "columns": 600}[name]
    H, W, g, C = 48, 64, 2, 3
    rng = np.random.default_rng(16)
    if name == "small":
        x0, y0 = rng.integers(-3, W - 2, K), rng.integers(-3, H - 2, K)
        boxes = np.stack([x0, y0, x0 + rng.integers(4, 13, K), y0 + rng.integers(4, 13, K)], axis=1)
    else:
        x0 = rng.integers(0, W - 1, K)
        boxes = np.stack([x0, np.zeros(K, dtype=np.int64), x0 + rng.integers(1, 3, K), np.full(K, H)], axis=1)
    return SR.stitch_maps(K, C, g, seed=16), boxes, H, W


def stitch_cases():
    for i, case in enumerate(SR.STITCH_CASES):
        yield f"case{i}", SR.stitch_case(case)
    for name in ("forty", "small", "columns"):
        yield name, path_case(name)


def empty(*shape, dtype=torch.uint8):
    return torch.empty(*shape, device="cuda", dtype=dtype)


def cases():
    """(name, {tensor name: tensor}) of every launch, in a fixed order"""
    for name, (probs, boxes, H, W) in stitch_cases():
        p = probs.cuda()
        bx = torch.as_tensor(np.asarray(boxes), dtype=torch.int32).reshape(-1, 4).cuda()
        C = p.shape[1]
        gen = torch.Generator().manual_seed(5)
        pal = torch.randint(0, 256, (256, 3), generator=gen, dtype=torch.uint8).cuda()
        photo = torch.randint(0, 256, (H, W, 3), generator=gen, dtype=torch.uint8).cuda()
        conf0 = empty(H, W, dtype=torch.float32)
        ops.dense_stitch(p, bx, H, W, empty(H, W), conf0)
        pictures = (("plain", None, None, 256), ("palette", pal, None, 256), ("photo", pal, photo, 77))
        for ttag, thr in (("t0", 0.0), ("tmed", float(conf0.median()))):
            for ptag, pl, ph, a8 in pictures:
                out = dict(labels=empty(H, W), conf=empty(H, W, dtype=torch.float32), cover=empty(H, W))
                if pl is not None:
                    out["overlay"] = empty(H, W, 3)
                ops.dense_stitch(p, bx, H, W, out["labels"], out["conf"], min_conf=thr, cover=out["cover"], overlay=out.get("overlay"),
                                 palette=pl, photo=ph, alpha8=a8)
                yield f"stitch/{name}/{ttag}/{ptag}", out
        maps, cover = empty(C, H, W, dtype=torch.float32), empty(H, W)
        ops.dense_stitch_maps(p, bx, H, W, maps, cover=cover)
        yield f"stitch_maps/{name}/cover", dict(maps=maps, cover=cover)
        maps2 = empty(C, H, W, dtype=torch.float32)
        ops.dense_stitch_maps(p, bx, H, W, maps2)
        yield f"stitch_maps/{name}/no_cover", dict(maps=maps2)
        for ttag, thr in (("t0", 0.0), ("tmed", float(conf0.median()))):
            for ctag, cv in (("cover", cover[None]), ("no_cover", None)):
                for ptag, pl, ph, a8 in pictures:
                    out = dict(labels=empty(1, H, W), conf=empty(1, H, W, dtype=torch.float32))
                    if pl is not None:
                        out["overlay"] = empty(1, H, W, 3)
                    ops.dense_maps_label(maps[None], out["labels"], out["conf"], min_conf=thr, cover=cv, overlay=out.get("overlay"),
                                         palette=pl, photo=None if ph is None else ph[None], alpha8=a8)
                    yield f"maps_label/{name}/{ttag}/{ctag}/{ptag}", out
    for i in range(len(RR.CASES)):
        for kind in RR.GUIDES:
            maps, guide, ds = RR.case_inputs(i, kind)
            m, g = maps.cuda(), guide.cuda()
            key = empty(*g.shape[:3], 4, dtype=torch.float32)
            ops.dense_refine_prepare(g, ds, key)
            out = dict(key=key)
            ts = (1,) + (tuple(RR.LONG_T) if i in RR.LONG_CASES else ())
            for t in range(1, max(ts) + 1):
                nxt = torch.empty_like(m)
                ops.dense_refine_step(m, nxt, g, key, ds)
                m = nxt
                if t in ts:
                    out[f"step{t}"] = m
            yield f"refine/case{i}/{kind}", out


def digests(tensors):
    out = {}
    for key, t in tensors.items():
        raw = t.detach().contiguous().cpu().view(torch.int8).numpy().tobytes()
        out[key] = f"{str(t.dtype)[6:]} {list(t.shape)} {hashlib.sha256(raw).hexdigest()[:32]}"
    return out


def main():
    n_cases = n = 0
    for (name, first), (_, second) in zip(cases(), cases()):
        a, b = digests(first), digests(second)
        if a != b:
            print(f"NOT REPEATABLE  {name}", flush=True)
            sys.exit(1)
        for key, d in a.items():
            print(f"{name}:{key}  {d}", flush=True)
            n += 1
        n_cases += 1
    print(f"{n_cases} cases, {n} tensors, every launch repeated with equal bytes")


if __name__ == "__main__":
    main()
