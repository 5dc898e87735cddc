"""The fp8 reference (tests/fp8_ref.py) checked against independent statements of the same facts: torch's own float8_e4m3fn
conversion, a numpy-fp32 transcription of the kernels' E8M0 rule, and the block-scale layout written out by hand.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp8_ref as R  # noqa: E402

F64 = torch.float64


def test_decode_table_is_torch_e4m3fn():
    b = torch.arange(256, dtype=torch.uint8)
    want = b.view(torch.float8_e4m3fn).float().double()
    nan = torch.isnan(want)
    assert nan.tolist() == [i in (0x7F, 0xFF) for i in range(256)]
    assert torch.equal(torch.isnan(R.E4M3), nan)
    assert torch.equal(R.E4M3[~nan], want[~nan])
    assert torch.equal(torch.signbit(R.E4M3[~nan]), torch.signbit(want[~nan]))          # 0x80 is -0
    assert torch.equal(R.decode(b)[~nan], want[~nan])


def test_encode_rne_is_torch_e4m3fn():
    """every finite byte round-trips; random values and every midpoint of two neighbours round as torch rounds them"""
    b = torch.tensor([i for i in range(256) if i not in (0x7F, 0xFF)], dtype=torch.uint8)
    assert torch.equal(R.encode_rne(R.decode(b)), b)
    g = torch.Generator().manual_seed(0)
    x = ((torch.rand(10000, generator=g) * 2 - 1) * 448).float()
    x = torch.cat([x, x * 2.0 ** -9, x * 2.0 ** -15])
    pos = R.E4M3[:0x7F]
    mid = ((pos[1:] + pos[:-1]) / 2).float()                 # exact in fp32
    x = torch.cat([x, mid, -mid])
    want = x.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(R.encode_rne(x.double()), want)
    assert R.encode_rne(torch.tensor([1e9, -1e9, 449.0, 17.0, 27.0], dtype=F64)).tolist() == [0x7E, 0xFE] + R.encode_rne(
        torch.tensor([448.0, 16.0, 28.0], dtype=F64)).tolist()


def _e8m0_kernel_rule(amax32):
    """e8m0_of (csrc/gemm_bf16_fp8ops.hip) in numpy fp32"""
    s = (amax32.astype(np.float32) * (np.float32(1.0) / np.float32(448.0))).astype(np.float32)
    b = s.view(np.uint32)
    e = (b >> 23).astype(np.int64) + ((b & 0x7FFFFF) != 0)
    return np.clip(e, 1, 253)


def test_e8m0_exact_equals_the_kernel_rule_on_the_dyadic_grid():
    m = np.array(R.DYADIC_M, dtype=np.float64)
    k = np.arange(-20, 21, dtype=np.float64)
    amax = (m[:, None] * 2.0 ** k[None, :]).reshape(-1)
    want = _e8m0_kernel_rule(amax.astype(np.float32))
    got = R.e8m0_exact(torch.from_numpy(amax)).numpy()
    assert np.array_equal(got, want)
    # m in (224, 448] shares one exponent, 2^(e - 127) = 2^k; m = 224 = 448 / 2 sits exactly on the next lower one
    assert np.array_equal(got.reshape(len(m), -1), 127 + k.astype(np.int64)[None, :] - (m == 224).astype(np.int64)[:, None])
    # and the definition itself: amax / 2^(e - 127) <= 448 < amax / 2^(e - 128), off the grid too
    g = torch.Generator().manual_seed(1)
    a = torch.exp2(torch.rand(5000, generator=g, dtype=F64) * 60 - 30)
    e = R.e8m0_exact(a).double()
    assert bool((a / torch.exp2(e - 127) <= 448).all() and (a / torch.exp2(e - 128) > 448).all())
    assert R.e8m0_exact(torch.tensor([0.0, 1e-300, 1e300], dtype=F64)).tolist() == [1, 1, 253]


def test_quant_step_bounds_the_conversion_and_is_attained_at_ties():
    g = torch.Generator().manual_seed(2)
    x = ((torch.rand(10000, generator=g) * 2 - 1) * 448).float()
    x = torch.cat([x, x * 2.0 ** -7, x * 2.0 ** -12])          # the subnormal range too
    err = (x.double() - x.to(torch.float8_e4m3fn).float().double()).abs()
    step = R.quant_step(x.double(), 1.0)
    assert bool((err <= step).all())
    assert (err / step).max().item() > 0.99                     # not slack: random values come close to it
    pos = R.E4M3[:0x7F]
    mid = (pos[1:] + pos[:-1]) / 2
    errm = (mid - mid.float().to(torch.float8_e4m3fn).float().double()).abs()
    assert torch.equal(errm, R.quant_step(mid, 1.0))            # attained at every tie
    assert torch.equal(R.quant_step(mid * 0.25, 0.25), errm * 0.25)
    assert R.quant_step(torch.tensor([0.0, 2.0 ** -7, 300.0, 448.0], dtype=F64), 1.0).tolist() == [2.0 ** -10, 2.0 ** -10, 16.0, 16.0]
    assert bool(R.near_tie(mid[1:]).all()) and not bool(R.near_tie(pos[1:]).any())


@pytest.mark.parametrize("C", [32, 96, 128, 192, 1024])
def test_scale_layout_round_trips(C):
    Rr, pad = 5, 2
    e = (torch.arange(Rr * (C // 32)).view(Rr, C // 32) % 250 + 1).to(torch.uint8)
    buf = R.mx_put(R.mx_buffer(Rr, C, rows_pad=pad, fill=0), e)
    assert tuple(buf.shape) == ((C + 127) // 128, Rr + pad, 4)
    for r in range(Rr):
        for b in range(C // 32):
            assert buf[b >> 2, r, b & 3] == e[r, b]             # the layout as the kernels state it
    assert torch.equal(R.mx_rows(buf, Rr, C), e)
    mask = R.mx_written_mask(buf, Rr, C)
    assert int(mask.sum()) == Rr * (C // 32) and bool((buf[~mask] == 0).all()) and bool((buf[mask] != 0).all())
    q = torch.full((Rr, C), 0x38, dtype=torch.uint8)            # 1.0
    want = torch.exp2(e.double() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(R.dequant_mx(q, buf), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_generators(dtype):
    q, v = R.int_operand(7, 48, -8, 8, 3)
    assert q.dtype == torch.uint8 and torch.equal(R.decode(q), v) and v.abs().max() <= 8 and bool((v == v.round()).all())
    x, m, k = R.dyadic_amax_rows(9, 160, dtype, 4, block=32)
    amax = x.double().abs().view(9, 5, 32).amax(2)
    assert torch.equal(amax, m.double() * torch.exp2(k.double()))
    assert torch.equal(R.e8m0_exact(amax), 127 + k - (m == 224).long())
    assert len(set(zip(m.view(-1).tolist(), k.view(-1).tolist()))) > 20      # neighbours differ
    e, qb = R.quantize_mx_ref(x.double())
    assert torch.equal(e, R.e8m0_exact(amax))
    buf = R.mx_put(R.mx_buffer(9, 160), e)
    assert bool(((R.dequant_mx(qb, buf) - x.double()).abs() <= R.quant_step(x.double(), torch.exp2(e.double() - 127).repeat_interleave(32, dim=1))).all())
    xr, mr, kr = R.dyadic_amax_rows(6, 24, dtype, 5)
    assert tuple(mr.shape) == (6, 1) and torch.equal(xr.double().abs().amax(1, keepdim=True), mr.double() * torch.exp2(kr.double()))
    s = R.rows_scale_ref(xr.float().abs().amax(1))
    assert torch.equal(s[mr[:, 0] == 448], torch.exp2(kr[mr[:, 0] == 448, 0].float()))   # amax = 448 * 2^k: the scale is 2^k exactly
    assert R.rows_scale_ref(torch.zeros(1)).item() == 1.0
