"""float64 reference of the image-guided refinement (csrc/dense_refine.hip, ops.dense_refine_prepare / dense_refine_step,
clip.refine_maps), written from the formulas of include/cclip_hip.h with explicit clamped index arithmetic - no padding, no
unfold, no code of the kernels' - plus a plain fp32 torch restatement (replicate pad and shifted slices) that is used ONLY to size
the bounds, the cases the CPU and GPU tests share, and the label comparison (dense_ref.compare_labels).

Bounds.  The project's rule: a kernel may be 4 x as far from float64 as the same arithmetic in plain fp32 torch ops
on the same inputs.  BOUNDS holds, per case and guide, 4 x the restatement's worst error as tests/test_dense_refine_ref_cpu.py
measures and prints it: the key's factors (relative: a flat neighbourhood gives 1e8), L (absolute), the maps after one step and
after T = 2 and T = 10 (absolute).  FRAGILE_T10 is twice the largest map bound at T = 10, no smaller than the project's 1e-5."""
from __future__ import annotations

import torch

from dense_ref import FRAGILE, NONE_LABEL, compare_labels  # noqa: F401  (re-exported for the tests)

OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))     # (dy, dx), the order of n = 8 j + e
DEFAULT_DILATIONS = (1, 2, 4, 8, 12, 24)


# ---- float64, from the definition ----------------------------------------------------------------
def neighbours(H: int, W: int, dilations):
    """(qy, qx) int64 [N, H, W]: the clamped coordinates of neighbour n = 8 j + e of every pixel"""
    ys = torch.arange(H)[:, None].expand(H, W)
    xs = torch.arange(W)[None, :].expand(H, W)
    qy, qx = [], []
    for d in dilations:
        for oy, ox in OFFSETS:
            qy.append((ys + d * oy).clamp(0, H - 1))
            qx.append((xs + d * ox).clamp(0, W - 1))
    return torch.stack(qy), torch.stack(qx)


def weights_ref(guide: torch.Tensor, dilations) -> dict:
    """guide uint8 [B, H, W, 3] -> float64 factors [B, H, W, 3], L [B, H, W], a and w [B, N, H, W]"""
    B, H, W, _ = guide.shape
    D = len(dilations)
    qy, qx = neighbours(H, W, dilations)
    x = guide.double().permute(0, 3, 1, 2) / 255.0                        # [B, 3, H, W]
    nb = x[:, :, qy, qx]                                                  # [B, 3, N, H, W]
    xb = guide.long().permute(0, 3, 1, 2)                                 # the bytes: their sums are exact integers, so that
    taps = torch.cat([xb[:, :, qy, qx], xb[:, :, None].expand(B, 3, D, H, W)], dim=2)      # a flat neighbourhood has sigma = 0
    n = taps.shape[2]                                                     # 9 D taps: the centre once per dilation
    num = n * taps.pow(2).sum(dim=2) - taps.sum(dim=2).pow(2)             # n (n - 1) x the unbiased variance of the bytes
    sigma = (num.double() / (n * (n - 1))).sqrt() / 255.0                 # [B, 3, H, W]
    f = 1.0 / (1e-8 + 0.1 * sigma)
    a = -((x[:, :, None] - nb).abs() * f[:, :, None]).sum(dim=1) / 3.0    # [B, N, H, W]
    mx = a.max(dim=1).values
    L = mx + (a - mx[:, None]).exp().sum(dim=1).log()
    return dict(factors=f.permute(0, 2, 3, 1), L=L, a=a, w=(a - L[:, None]).exp(), qy=qy, qx=qx)


def step_ref(maps: torch.Tensor, wr: dict) -> torch.Tensor:
    """one iteration on float64 maps [B, C, H, W], summed in ascending n"""
    w, qy, qx = wr["w"], wr["qy"], wr["qx"]
    out = torch.zeros_like(maps)
    for n in range(w.shape[1]):
        out = out + w[:, None, n] * maps[:, :, qy[n], qx[n]]
    return out


def refine_ref(maps: torch.Tensor, guide: torch.Tensor, dilations, iterations: int, keep=()) -> dict:
    """float64: {"key": weights_ref, t: maps after t iterations for t in keep and t = iterations}"""
    wr = weights_ref(guide, dilations)
    m = maps.double()
    out = {"key": wr}
    for t in range(1, iterations + 1):
        m = step_ref(m, wr)
        if t in keep or t == iterations:
            out[t] = m
    return out


def label_ref(maps64: torch.Tensor, min_conf: float = 0.0) -> dict:
    """the dict dense_ref.compare_labels takes, of float64 maps [B, C, H, W]"""
    conf, arg = maps64.max(dim=1)
    if maps64.shape[1] > 1:
        masked = maps64.scatter(1, arg[:, None], float("-inf"))
        second_v, second = masked.max(dim=1)
        margin = conf - second_v
    else:
        second, margin = arg.clone(), torch.full_like(conf, float("inf"))
    labels = torch.where(conf < min_conf, torch.full_like(arg, NONE_LABEL), arg)
    return dict(labels=labels, conf=conf, arg=arg, second=second, margin=margin, min_conf=float(min_conf))


def fragile_share(ref: dict, fragile: float) -> float:
    """the share of pixels whose float64 top-two margin lies in (0, fragile)"""
    return float(((ref["margin"] > 0) & (ref["margin"] < fragile)).double().mean())


# ---- the same arithmetic as plain fp32 torch ops (sizes the bounds, nothing else) ----------------
def _shifted(x: torch.Tensor, dilations):
    """x [..., H, W] -> the N replicate-padded shifted copies, in the order of n"""
    import torch.nn.functional as F
    H, W = x.shape[-2:]
    p = max(dilations)
    lead = x.shape[:-2]
    xp = F.pad(x.reshape(1, -1, H, W), (p, p, p, p), mode="replicate").reshape(*lead, H + 2 * p, W + 2 * p)
    return [xp[..., p + d * oy:p + d * oy + H, p + d * ox:p + d * ox + W] for d in dilations for oy, ox in OFFSETS]


def weights_fp32(guide: torch.Tensor, dilations) -> dict:
    x = guide.float().permute(0, 3, 1, 2) / 255.0
    nb = torch.stack(_shifted(x, dilations), dim=2)                       # [B, 3, N, H, W]
    taps = torch.cat([nb, x[:, :, None].expand(-1, -1, len(dilations), -1, -1)], dim=2)
    f = 1.0 / (1e-8 + 0.1 * taps.std(dim=2, unbiased=True))
    a = -((x[:, :, None] - nb).abs() * f[:, :, None]).sum(dim=1) / 3.0
    L = torch.logsumexp(a, dim=1)
    return dict(factors=f.permute(0, 2, 3, 1), L=L, w=(a - L[:, None]).exp())     # the weights as the kernels form them


def step_fp32(maps: torch.Tensor, w: torch.Tensor, dilations) -> torch.Tensor:
    out = None
    for n, s in enumerate(_shifted(maps, dilations)):
        out = w[:, None, n] * s if out is None else out + w[:, None, n] * s
    return out


def refine_fp32(maps: torch.Tensor, guide: torch.Tensor, dilations, iterations: int, keep=()) -> dict:
    wr = weights_fp32(guide, dilations)
    m = maps.float()
    out = {"key": wr}
    for t in range(1, iterations + 1):
        m = step_fp32(m, wr["w"], dilations)
        if t in keep or t == iterations:
            out[t] = m
    return out


def errors(got: dict, ref: dict, ts) -> dict:
    """worst errors of a result dict (refine_fp32's, or the device's in the same form) against refine_ref's"""
    e = {"factor": ((got["key"]["factors"].double() - ref["key"]["factors"]).abs() / ref["key"]["factors"]).max().item(),
         "L": (got["key"]["L"].double() - ref["key"]["L"]).abs().max().item()}
    for t in ts:
        e[t] = (got[t].double() - ref[t]).abs().max().item()
    return e


# ---- shared cases ----------------------------------------------------------------------------------
# (B, C, H, W, dilations): one pixel; all clamping; one past a 32-tile in both axes with two images; several tiles with the
# default dilations; one dilation that is no power of two on a picture narrower than a tile; the class limit under the largest dilation
CASES = [(1, 1, 1, 1, (1,)), (1, 3, 5, 7, DEFAULT_DILATIONS), (2, 3, 33, 65, (1, 2)), (1, 9, 70, 97, DEFAULT_DILATIONS),
         (1, 2, 40, 31, (3,)), (1, 255, 9, 9, (24,))]
GUIDES = ("noise", "flat", "edge", "gradient")
LONG_CASES = (2, 3)                                                      # T = 2 and T = 10 run on these
LONG_T = (2, 10)
SEEDS = (0, 1, 2, 5, 4, 6)                                               # chosen on the CPU so that the float64 results of the
#                                                                          long cases have a fragile share <= 1e-3 under every guide


def make_guide(kind: str, B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """uint8 [B, H, W, 3]: seeded noise; one flat colour; two colours either side of a vertical edge; a gradient whose bytes
    step by one from column to column (small sigma)"""
    gen = torch.Generator().manual_seed(4000 + seed)
    if kind == "noise":
        return torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8)
    if kind == "flat":
        return torch.tensor([37, 200, 111], dtype=torch.uint8).expand(B, H, W, 3).contiguous()
    if kind == "edge":
        g = torch.tensor([30, 60, 200], dtype=torch.uint8).expand(B, H, W, 3).clone()
        g[:, :, (W + 1) // 2:] = torch.tensor([220, 180, 40], dtype=torch.uint8)
        return g
    if kind == "gradient":
        col = (torch.arange(W) + 40).remainder(256).to(torch.uint8)
        row = (torch.arange(H) + 90).remainder(256).to(torch.uint8)
        g = torch.empty(B, H, W, 3, dtype=torch.uint8)
        g[..., 0] = col[None, None, :]
        g[..., 1] = row[None, :, None]
        g[..., 2] = 128
        return g
    raise ValueError(kind)


def make_maps(B: int, C: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """fp32 [B, C, H, W]: a softmax over classes of a coarse random grid stretched over the picture (regions, as class maps are)
    plus a little per-pixel noise; sums to 1 over the classes"""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(5000 + seed)
    gh, gw = max(1, (H + 15) // 16), max(1, (W + 15) // 16)
    coarse = 3.0 * torch.randn(B, C, gh, gw, generator=gen)
    logits = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False) if (gh, gw) != (H, W) else coarse
    logits = logits + 0.3 * torch.randn(B, C, H, W, generator=gen)
    return logits.softmax(dim=1).contiguous()


def case_inputs(i: int, kind: str):
    """(maps fp32 [B, C, H, W], guide uint8 [B, H, W, 3], dilations) of CASES[i] under guide `kind`"""
    B, C, H, W, ds = CASES[i]
    return make_maps(B, C, H, W, seed=SEEDS[i]), make_guide(kind, B, H, W, seed=SEEDS[i]), ds


# ---- bounds: 4 x the fp32 restatement's error, per (case, guide) -----------------------------------
# rows: (case index, guide) -> {"factor": relative, "L": absolute, 1: |dm| after one step, 2 / 10: after T steps (LONG_CASES)}
# as printed by tests/test_dense_refine_ref_cpu.py::test_fp32_restatement_sizes_the_bounds (values are 4 x the measured error)
BOUNDS = {
    (0, 'noise'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 8.882e-16},
    (0, 'flat'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 8.882e-16},
    (0, 'edge'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 8.882e-16},
    (0, 'gradient'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 8.882e-16},
    (1, 'noise'): {'factor': 4.697e-07, 'L': 2.846e-06, 1: 1.733e-06},
    (1, 'flat'): {'factor': 0.000e+00, 'L': 1.098e-07, 1: 1.495e-06},
    (1, 'edge'): {'factor': 3.332e-07, 'L': 3.323e-07, 1: 1.874e-06},
    (1, 'gradient'): {'factor': 4.553e-07, 'L': 1.098e-06, 1: 1.724e-06},
    (2, 'noise'): {'factor': 7.241e-07, 'L': 6.177e-06, 1: 2.291e-06, 2: 3.742e-06, 10: 1.449e-05},
    (2, 'flat'): {'factor': 0.000e+00, 'L': 3.047e-08, 1: 7.153e-07, 2: 1.005e-06, 10: 7.835e-07},
    (2, 'edge'): {'factor': 2.326e-07, 'L': 3.336e-07, 1: 7.153e-07, 2: 1.005e-06, 10: 9.393e-07},
    (2, 'gradient'): {'factor': 4.771e-06, 'L': 5.458e-06, 1: 1.925e-06, 2: 2.828e-06, 10: 1.066e-05},
    (3, 'noise'): {'factor': 7.341e-07, 'L': 3.916e-06, 1: 1.817e-06, 2: 2.420e-06, 10: 8.286e-06},
    (3, 'flat'): {'factor': 0.000e+00, 'L': 1.098e-07, 1: 1.226e-06, 2: 9.999e-07, 10: 1.490e-06},
    (3, 'edge'): {'factor': 3.332e-07, 'L': 3.522e-07, 1: 1.226e-06, 2: 9.983e-07, 10: 1.788e-06},
    (3, 'gradient'): {'factor': 1.498e-06, 'L': 7.583e-06, 1: 1.976e-06, 2: 2.194e-06, 10: 4.289e-06},
    (4, 'noise'): {'factor': 7.742e-07, 'L': 6.953e-06, 1: 1.994e-06},
    (4, 'flat'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 4.172e-07},
    (4, 'edge'): {'factor': 4.542e-07, 'L': 1.153e-07, 1: 5.247e-07},
    (4, 'gradient'): {'factor': 1.013e-05, 'L': 1.210e-05, 1: 1.936e-06},
    (5, 'noise'): {'factor': 5.825e-07, 'L': 4.830e-06, 1: 5.287e-07},
    (5, 'flat'): {'factor': 0.000e+00, 'L': 2.286e-08, 1: 8.941e-08},
    (5, 'edge'): {'factor': 4.542e-07, 'L': 1.153e-07, 1: 1.188e-07},
    (5, 'gradient'): {'factor': 2.526e-07, 'L': 1.665e-06, 1: 2.335e-07},
}

FRAGILE_T10 = max([FRAGILE] + [2.0 * b[10] for b in BOUNDS.values() if 10 in b])


# ---- the behavioural case: a diagonal edge against a blurred vertical band -------------------------
def diagonal_case():
    """(maps fp32 [1, 2, 64, 96], guide uint8 [1, 64, 96, 3], truth int64 [64, 96]): two flat colours split by the diagonal
    x / 96 < y / 64 (truth = the colour region), and two class maps stretched from a 4 x 6 grid whose left three columns favour
    class 1 and right three class 0 - a blurred vertical band where the photo has a diagonal"""
    import torch.nn.functional as F
    H, W = 64, 96
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    truth = ((2 * xs + 1) * H < (2 * ys + 1) * W).long()                 # 1 below / left of the diagonal
    guide = torch.where(truth[..., None] == 1, torch.tensor([200, 60, 40]), torch.tensor([40, 90, 210])).to(torch.uint8)[None]
    p1 = torch.tensor([0.9, 0.8, 0.6, 0.4, 0.2, 0.1]).expand(4, 6)
    grid = torch.stack([1.0 - p1, p1])[None].contiguous()                 # [1, 2, 4, 6]
    maps = F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False).contiguous()
    return maps, guide.contiguous(), truth


def agreement(labels: torch.Tensor, truth: torch.Tensor) -> float:
    return float((labels.long().cpu().reshape(truth.shape) == truth).double().mean())


# measured on the float64 reference (test_dense_refine_ref_cpu.py::test_diagonal_case_margin prints both): the share of pixels
# whose label matches their colour region before and after 10 default iterations
DIAGONAL_BEFORE = 0.75                                                   # exactly: the band splits the picture at x = 48
DIAGONAL_AFTER = 0.849                                                   # 0.84928 on the float64 reference
DIAGONAL_MARGIN = 0.09                                                   # what a refined result must gain at least
