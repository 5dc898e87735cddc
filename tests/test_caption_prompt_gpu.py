"""cclip_caption_prompt (csrc/caption_prompt.hip) on the MI355X against the float64 statement of its formula
(prompt_reference64, pinned against ZeroShotClassifier's arithmetic in tests/test_caption_prompt_cpu.py).

Relative L2 error of `probs` per head against float64, measured on one MI355X over E in {64, 128, 512, 768}, head layouts
(2, 9), (1,), (3, 4, 2), (9, 2), N in {1, 7, 512}, logit scales 100 and 1 / 0.07 and a strided `feat`:
  largest seen 3.6e-7 (E = 768, heads (3, 4, 2), N = 1, scale 100; typical 5e-8 .. 2.5e-7); PROBS_TOL is about twice that.
The arithmetic is fp32 (dot products of 64 - 768 terms, expf), so the expectation was around 1e-6.
The arg-max equals the float64 arg-max wherever the float64 top-2 logit gap exceeds GAP = 1e-3; the share of (row, head) cases
left out on that ground is a property of the inputs alone: 0 % at scale 100 and for every N = 1 / N = 7 case, at most 0.49 %
(E = 512, heads (9, 2), N = 512, scale 1 / 0.07); the test asserts it stays within 1 % and prints it.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_caption_prompt_cpu import prompt_reference64  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED_MAX = 3.6e-7
PROBS_TOL = 8e-7
GAP = 1e-3
MAX_EXCLUDED = 0.01
SCALES = [math.log(100.0), math.log(1 / 0.07)]
LAYOUTS = [(2, 9), (1,), (3, 4, 2), (9, 2)]
A = 5


def _inputs(E, heads):
    g = torch.Generator().manual_seed(567)
    feat = torch.randn(512, E, generator=g)
    prompts = torch.cat([torch.randn(k, E, generator=g) for k in heads])
    head_start = [0]
    for k in heads:
        head_start.append(head_start[-1] + k)
    rows = math.prod(heads)
    table = torch.randint(0, 30000, (rows, A), generator=g, dtype=torch.int32)
    return feat, prompts, head_start, table


def _launch(feat_dev, prompts, head_start, log_scale, table):
    from cclip_hip import ops
    N, K, G = feat_dev.shape[0], prompts.shape[0], len(head_start) - 1
    probs = torch.full((N, K), -1.0, device="cuda", dtype=torch.float32)
    index = torch.full((N, G), -1, device="cuda", dtype=torch.int32)
    ids = torch.full((N, table.shape[1]), -1, device="cuda", dtype=torch.int32)
    ls = torch.full((1,), log_scale, device="cuda", dtype=torch.float32)
    ops.caption_prompt(feat_dev, prompts.cuda(), head_start, ls, table.cuda(), probs, index, ids)
    return probs, index, ids


def _check(feat, feat_dev, prompts, head_start, log_scale, table, tag):
    probs, index, ids = _launch(feat_dev, prompts, head_start, log_scale, table)
    ls32 = float(torch.tensor(log_scale, dtype=torch.float32))                 # the scalar the kernel reads is fp32
    rp, ri, rids, gap = prompt_reference64(feat, prompts, head_start, ls32, table)
    worst = 0.0
    for g, (k0, k1) in enumerate(zip(head_start[:-1], head_start[1:])):
        err = ((probs[:, k0:k1].double().cpu() - rp[:, k0:k1]).norm() / rp[:, k0:k1].norm()).item()
        worst = max(worst, err)
    clear = gap > GAP
    excluded = 1.0 - clear.double().mean().item()
    print(f"caption_prompt {tag}: probs rel L2 {worst:.3e}  excluded {100 * excluded:.2f} %  min gap {gap.min().item():.3e}")
    assert worst < PROBS_TOL, (tag, worst)
    assert excluded <= MAX_EXCLUDED, (tag, excluded)
    idx = index.long().cpu()
    assert torch.equal(idx[clear], ri[clear]), tag
    # ids: exactly the table row of the combination the kernel itself reports, for every row
    comb = torch.zeros(idx.shape[0], dtype=torch.int64)
    for g, (k0, k1) in enumerate(zip(head_start[:-1], head_start[1:])):
        assert int(idx[:, g].min()) >= 0 and int(idx[:, g].max()) < k1 - k0
        comb = comb * (k1 - k0) + idx[:, g]
    assert torch.equal(ids.long().cpu(), table.long()[comb]), tag
    return worst


@pytest.mark.parametrize("E", [64, 128, 512, 768])
@pytest.mark.parametrize("heads", LAYOUTS)
def test_kernel_against_float64(E, heads):
    feat, prompts, head_start, table = _inputs(E, heads)
    for N in (1, 7, 512):
        for ls in SCALES:
            _check(feat[:N], feat[:N].cuda(), prompts, head_start, ls, table, f"E={E} heads={heads} N={N} scale={math.exp(ls):.2f}")


@pytest.mark.parametrize("E", [64, 512])
def test_strided_feature_rows(E):
    feat, prompts, head_start, table = _inputs(E, (2, 9))
    wide = torch.zeros(512, E + 12, device="cuda")
    wide[:, 4:4 + E] = feat.cuda()
    view = wide[:, 4:4 + E]                                                   # row stride E + 12, rows 16-byte aligned
    assert not view.is_contiguous()
    a = _launch(view, prompts, head_start, SCALES[0], table)
    b = _launch(feat.cuda(), prompts, head_start, SCALES[0], table)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _check(feat, view, prompts, head_start, SCALES[1], table, f"E={E} strided")


def test_exact_ties_report_the_lower_index():
    feat, prompts, head_start, table = _inputs(512, (3, 4, 2))
    p2 = prompts.clone()
    p2[6] = p2[4]                                                             # head 1: its rows 1 and 3 are the same prompt
    _, index, ids = _launch(feat.cuda(), p2, head_start, SCALES[0], table)
    _, ri, rids, _ = prompt_reference64(feat, p2, head_start, float(torch.tensor(SCALES[0], dtype=torch.float32)), table)
    idx = index.long().cpu()
    assert (idx[:, 1] != 3).all() and (idx[:, 1] == 1).any()                  # the duplicate never wins; the original does
    assert (idx[:, 1] == ri[:, 1]).double().mean() >= 0.99                   # (all but float64 near-ties between OTHER prompts)
    comb = (idx[:, 0] * 4 + idx[:, 1]) * 2 + idx[:, 2]
    assert torch.equal(ids.long().cpu(), table.long()[comb])
    # a head whose prompts are ALL the same row: every logit ties, index 0, uniform probabilities
    p3 = prompts.clone()
    p3[3:7] = p3[3]
    probs, index, _ = _launch(feat.cuda(), p3, head_start, SCALES[0], table)
    assert (index[:, 1] == 0).all() and torch.equal(probs[:, 3:7], torch.full_like(probs[:, 3:7], 0.25))


def test_two_launches_are_bitwise_equal():
    feat, prompts, head_start, table = _inputs(768, (2, 9))
    a = _launch(feat.cuda(), prompts, head_start, SCALES[0], table)
    b = _launch(feat.cuda(), prompts, head_start, SCALES[0], table)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = _launch(feat[:7].cuda(), prompts, head_start, SCALES[0], table)       # a row's result does not depend on N either
    for x, y in zip(a, c):
        assert torch.equal(x[:7], y)


def test_bad_arguments_are_refused():
    from cclip_hip import load_library, ops
    feat, prompts, head_start, table = _inputs(64, (2, 9))
    fd, pd, td = feat.cuda(), prompts.cuda(), table.cuda()
    ls = torch.full((1,), SCALES[0], device="cuda")

    def outs(N=512, K=11, G=2):
        return (torch.zeros(N, K, device="cuda"), torch.zeros(N, G, device="cuda", dtype=torch.int32),
                torch.zeros(N, A, device="cuda", dtype=torch.int32))

    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # a head with no prompts
        ops.caption_prompt(fd, pd, [0, 0, 11], ls, td, *outs())
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # heads do not cover the prompt rows
        ops.caption_prompt(fd, pd, [0, 2, 10], ls, td[:16], *outs())
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # table rows != 2 * 9
        ops.caption_prompt(fd, pd, head_start, ls, td[:17], *outs())
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # E % 4
        ops.caption_prompt(torch.zeros(8, 66, device="cuda"), torch.ones(11, 66, device="cuda"), head_start, ls, td, *outs(N=8))
    buf = torch.zeros(8 * 64 + 4, device="cuda")
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # rows not 16-byte aligned
        ops.caption_prompt(buf[1:1 + 8 * 64].view(8, 64), pd, head_start, ls, td, *outs(N=8))
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # more heads than the launcher takes
        ops.caption_prompt(fd, torch.ones(17, 64, device="cuda"), list(range(18)), ls, torch.zeros(1, A, device="cuda", dtype=torch.int32),
                           *outs(K=17, G=17))
    with pytest.raises(RuntimeError, match="cclip_caption_prompt.*status 1"):           # prompt rows beyond what LDS holds
        ops.caption_prompt(torch.zeros(8, 1024, device="cuda"), torch.ones(20, 1024, device="cuda"), [0, 20], ls,
                           torch.zeros(20, A, device="cuda", dtype=torch.int32), *outs(N=8, K=20, G=1))
    # the C entry itself: null pointers and non-positive sizes return CCLIP_ERR_ARG (1) and launch nothing
    lib = load_library()
    hs = (ctypes.c_int32 * 3)(0, 2, 11)
    p, i, d = outs()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    good = [P(fd), ctypes.c_int64(64), ctypes.c_int32(512), ctypes.c_int32(64), P(pd), ctypes.c_int32(11), hs, ctypes.c_int32(2),
            P(ls), P(td), ctypes.c_int32(18), ctypes.c_int32(A), P(p), P(i), P(d), ctypes.c_void_p(0)]
    for pos in (0, 4, 6, 8, 9, 12, 13, 14):
        bad = list(good)
        bad[pos] = ctypes.c_void_p(0) if pos != 6 else None
        assert lib.cclip_caption_prompt(*bad) == 1, pos
    for pos in (2, 3, 5, 7, 11):
        bad = list(good)
        bad[pos] = ctypes.c_int32(0)
        assert lib.cclip_caption_prompt(*bad) == 1, pos
    torch.cuda.synchronize()
    assert float(p.abs().sum()) == 0.0                                        # nothing was launched
