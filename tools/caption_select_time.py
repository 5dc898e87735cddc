"""Timing of the caption-selection path: python tools/caption_select_time.py [--skip-describe]

1. clip.clip_score_features (one cclip_caption_select launch) against the same arithmetic as torch ops - F.normalize, bmm,
   clamp, a stable argsort - at (N, K, E) = (16, 8, 512), (1, 64, 512) and (4096, 1, 512): the median of 100 calls, each
   bracketed by device events, after 20 warm-up calls, the two alternating.
2. Captioner.describe(best_of=8) against Captioner.describe() with beam 3 at ViT-B/32 + gpt2-base-chinese geometry (seeded
   weights, 16 images, entry_length 20): the median of 7 host-clock timings around calls that end in the read-back."""
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "construction-clip_amd"), os.path.join(ROOT, "scripts")]
import clip  # noqa: E402


def torch_select(img, txt, K, w=2.5):
    N, E = img.shape
    cos = torch.bmm(F.normalize(txt, dim=1).view(N, K, E), F.normalize(img, dim=1).unsqueeze(2)).squeeze(2)
    order = cos.argsort(dim=1, descending=True, stable=True)
    return cos, w * cos.clamp(min=0), order, order[:, 0]


def event_median_us(fns, warm=20, reps=100):
    """per function the median device time of one call; the functions alternate inside every repetition"""
    for _ in range(warm):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) * 1e3)
    return [statistics.median(t) for t in times]


def kernel_part():
    for N, K, E in ((16, 8, 512), (1, 64, 512), (4096, 1, 512)):
        g = torch.Generator(device="cuda").manual_seed(1)
        img = torch.randn(N, E, device="cuda", generator=g)
        txt = torch.randn(N * K, E, device="cuda", generator=g) + 0.5 * img.repeat_interleave(K, 0)
        res = clip.clip_score_features(img, txt)
        cos, cs, order, best = torch_select(img, txt, K)
        err = (res.cos - cos).abs().max().item()
        same = (res.order.long() == order).float().mean().item()
        hip, ref = event_median_us([lambda: clip.clip_score_features(img, txt), lambda: torch_select(img, txt, K)])
        print(f"N={N:5d} K={K:3d} E={E}: clip_score_features {hip:8.1f} us   torch ops {ref:8.1f} us   ratio {ref / hip:5.2f}x   "
              f"max |dcos| {err:.2e}   order agreement {same:.4f}", flush=True)


def describe_part():
    import _common as C
    from clip.weights import MODELS, init_state_dict, synthetic_images
    from clip_caption import Captioner, ClipCaptionModel, GPT2_MODELS, init_caption_state_dict
    clip_model = clip.build_model(init_state_dict(MODELS["ViT-B/32"], 3)).cuda().eval().half()
    geo = GPT2_MODELS["ckiplab/gpt2-base-chinese"]
    model = ClipCaptionModel(geo.prefix_length, prefix_size=geo.prefix_size, gpt2_type=geo)
    model.load_state_dict(init_caption_state_dict(geo, 31))
    model = model.cuda().eval().half()
    cap = Captioner(clip_model, model, C.ByteCaptionTokenizer(geo.vocab_size), clip_tokenize=C.get_tokenize(clip_model),
                    prefix_length=geo.prefix_length, attribute_length=geo.attribute_length)
    images = synthetic_images(16, clip_model.geo, 4).cuda()
    gen = torch.Generator(device="cuda").manual_seed(2)
    calls = {"describe() beam 3": lambda: cap.describe(images, beam_size=3, entry_length=20),
             "describe(best_of=8)": lambda: cap.describe(images, best_of=8, entry_length=20, temperature=1.0, generator=gen)}
    times = {k: [] for k in calls}
    for rep in range(2 + 7):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
    for k, t in times.items():
        print(f"16 images, entry_length 20, {k:20s}: median {statistics.median(t):8.1f} ms  (min {min(t):.1f}, max {max(t):.1f})", flush=True)


if __name__ == "__main__":
    kernel_part()
    if "--skip-describe" not in sys.argv:
        describe_part()
