"""A plain float64 reference of what the fp8 kernels compute (csrc/gemm_bf16_fp8ops.hip: quantize_rows_fp8, quantize_mx_fp8,
ln_fwd_fp8, gemm_fp8_kernel; csrc/attention.hip: attn_store_mx): the OCP e4m3fn number format (decode table, round-to-nearest-
even encoding, spacing), the E8M0 block-scale rule and the block-scale buffer layout, plus generators of operands on which the
kernels' answers are determined exactly.  Helper module of tests/test_fp8_ref_cpu.py (which checks this reference itself) and
tests/test_fp8_edges_gpu.py; torch on the CPU only, tensors of any device are accepted and answered on the same device.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN, largest finite 448 = 1.75 * 2^8;
subnormals m * 2^-9 below 2^-6.  E8M0: a biased power-of-two exponent byte, scale = 2^(e - 127); the kernels write e in [1, 253].
"""
import math

import torch

F64 = torch.float64
E4M3_MAX = 448.0
DYADIC_M = (448, 416, 384, 352, 320, 288, 256, 240, 224)     # block amax mantissas m (amax = m * 2^k): 2^(e - 127) = 2^k for 224 < m <= 448, 2^(k - 1) for m = 224 = 448 / 2


def _decode_table():
    t = []
    for b in range(256):
        s = -1.0 if b & 0x80 else 1.0
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            t.append(float("nan"))
        elif e == 0:
            t.append(s * m * 2.0 ** -9)
        else:
            t.append(s * (1 + m / 8.0) * 2.0 ** (e - 7))
    return torch.tensor(t, dtype=F64)


E4M3 = _decode_table()                                       # byte -> value
_POS = E4M3[:0x7F].clone()                                   # the 127 non-negative finite values, ascending (byte = index)


def decode(q8):
    """uint8 e4m3 bytes -> float64"""
    return E4M3.to(q8.device)[q8.long()]


def _floor_log2(a):
    """floor(log2(a)) for a > 0 in float64, exactly (frexp: a = f * 2^x, f in [0.5, 1))"""
    return torch.frexp(a)[1].to(F64) - 1


def spacing(a):
    """distance between the e4m3 values around magnitude a (float64, 0 <= a): 2^-9 below 2^-6, 32 in the top binade [256, 448]"""
    a = a.to(F64).abs().clamp(max=E4M3_MAX)
    e = torch.where(a > 0, _floor_log2(a.clamp_min(2.0 ** -1000)), torch.full_like(a, -6.0)).clamp(-6.0, 8.0)
    return torch.exp2(e - 3)


def encode_rne(y):
    """float64 -> e4m3 byte, round to nearest even, saturating at +-448 (the kernels clamp before they convert); the sign bit is
    the sign of y, also where the magnitude rounds to zero (IEEE)."""
    y = y.to(F64)
    a = y.abs().clamp(max=E4M3_MAX)
    sp = spacing(a)
    v = torch.round(a / sp) * sp                             # (torch.round: half to even; a / sp is exact, sp a power of two)
    code = torch.searchsorted(_POS.to(y.device), v.contiguous())
    assert bool((_POS.to(y.device)[code] == v).all())
    return (code + 128 * torch.signbit(y).long()).to(torch.uint8)


def quant_step(y, scale):
    """The largest error of rounding y / scale to e4m3 and scaling back: half the e4m3 spacing at |y| / scale, times scale.
    Attained at ties.  (A magnitude just below a power of two gets the finer spacing of its own binade.)"""
    y, scale = y.to(F64), torch.as_tensor(scale, dtype=F64, device=y.device)
    return 0.5 * spacing(y.abs() / scale) * scale


def near_tie(y, rel=2.0 ** -20):
    """True where y is within rel * |y| of the midpoint of two neighbouring e4m3 values (or beyond 448 by less): there an
    fp32 evaluation of y may round the other way than the float64 one."""
    a = y.to(F64).abs()
    sp = spacing(a)
    fr = a / sp - torch.floor(a / sp)
    return (((fr - 0.5).abs() * sp) <= rel * a) & (a < E4M3_MAX * (1 + rel))


# ---- block scales --------------------------------------------------------------------------------------------------------------
def e8m0_exact(amax):
    """The smallest e in [1, 253] with amax / 2^(e - 127) <= 448, decided exactly: amax = f * 2^x with f in [0.5, 1), and
    448 = 0.875 * 2^9, so e - 127 = x - 9 (+ 1 if f > 0.875).  An all-zero block: 1."""
    amax = amax.to(F64)
    f, x = torch.frexp(amax)
    e = x.to(torch.int64) - 9 + 127 + (f > 0.875).long()
    return torch.where(amax > 0, e.clamp(1, 253), torch.ones_like(e))


def mx_buffer(R, C, rows_pad=0, fill=0):
    """block-scale buffer of a [R, C] operand: uint8 [ceil(C / 128), R + rows_pad, 4], filled with `fill`"""
    return torch.full(((C + 127) // 128, R + rows_pad, 4), fill, dtype=torch.uint8)


def mx_rows(e8, R, C):
    """block-scale buffer [ceil(C/128), >= R, 4] (K-tile major: the byte of (row r, block b) at [b >> 2, r, b & 3]) -> [R, C // 32]"""
    return e8[:, :R].permute(1, 0, 2).reshape(R, -1)[:, :C // 32]


def mx_put(e8, e_rows):
    """write exponents [R, C // 32] into a block-scale buffer (the inverse of mx_rows); bytes it does not name are left alone"""
    R, nb = e_rows.shape
    for b in range(nb):
        e8[b >> 2, :R, b & 3] = e_rows[:, b].to(torch.uint8)
    return e8


def mx_written_mask(e8, R, C):
    """bool mask over a block-scale buffer: the bytes a [R, C] operand owns"""
    m = torch.zeros(e8.shape, dtype=torch.bool, device=e8.device)
    for b in range(C // 32):
        m[b >> 2, :R, b & 3] = True
    return m


def dequant_rows(q8, scale):
    """e4m3 bytes [R, C] + per-row fp32 scales [R] -> float64"""
    return decode(q8) * scale.to(F64)[:, None]


def dequant_mx(q8, e8):
    """e4m3 bytes [R, C] (C % 32 == 0) + block-scale buffer -> float64"""
    R, C = q8.shape
    s = torch.exp2(mx_rows(e8, R, C).to(F64) - 127.0).repeat_interleave(32, dim=1)
    return decode(q8) * s


def quantize_mx_ref(x):
    """float64 [R, C] -> (exponents [R, C // 32] int64, bytes [R, C] uint8): each 32-block on its own exact E8M0 exponent"""
    R, C = x.shape
    e = e8m0_exact(x.abs().view(R, C // 32, 32).amax(2))
    s = torch.exp2(e.to(F64) - 127.0).repeat_interleave(32, dim=1)
    return e, encode_rne(x.to(F64) / s)


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_operand(R, C, lo, hi, seed):
    """small-integer e4m3 operand: (bytes uint8 [R, C], values float64 [R, C]), integers uniform in [lo, hi] (|.| <= 16: exact in e4m3)"""
    assert -16 <= lo <= hi <= 16
    v = torch.randint(lo, hi + 1, (R, C), generator=_gen(seed)).to(F64)
    q = encode_rne(v)
    assert bool((decode(q) == v).all())
    return q, v


def dyadic_amax_rows(R, C, dtype, seed, block=None, kmin=-6, kmax=6):
    """16-bit rows [R, C] in which every `block` consecutive columns (default: the whole row) have amax exactly m * 2^k, m from
    DYADIC_M and k in [kmin, kmax], both cycling with (row, block) so that neighbours differ; the amax sits at a random column with
    a random sign, the other elements are random 16-bit values below it (a few exact zeros among them).  Returns (x, m, k) with m, k
    int64 [R, C // block].  For these amax the kernels' fp32 rule (amax * (1.0f / 448.0f), exponent + 1 if the mantissa is not
    zero) and e8m0_exact agree (tests/test_fp8_ref_cpu.py)."""
    block = C if block is None else block
    assert C % block == 0
    nb = C // block
    g = _gen(seed)
    idx = torch.arange(R)[:, None] * 5 + torch.arange(nb)[None, :] * 3 + seed
    m = torch.tensor(DYADIC_M)[idx % len(DYADIC_M)]
    k = kmin + (idx * 7 + idx // 9) % (kmax - kmin + 1)
    amax = m.to(F64) * torch.exp2(k.to(F64))
    body = (torch.rand(R, nb, block, generator=g, dtype=F64) * 2 - 1) * 0.97 * amax[:, :, None]
    body = torch.where(torch.rand(R, nb, block, generator=g) < 0.05, torch.zeros_like(body), body)
    body = body.to(dtype).to(F64)                              # (rounding to 16 bits moves a value by < 2^-8 of itself: still below amax)
    pos = torch.randint(0, block, (R, nb, 1), generator=g)
    sign = torch.randint(0, 2, (R, nb, 1), generator=g).to(F64) * 2 - 1
    body.scatter_(2, pos, sign * amax[:, :, None])
    x = body.view(R, C).to(dtype)
    assert bool((x.to(F64).abs().view(R, nb, block).amax(2) == amax).all()), "amax not representable in the 16-bit type"
    return x, m, k


def rows_scale_ref(amax32):
    """the row quantiser's scale, the fp32 product fp32(amax) * fp32(1 / 448) (1 for an all-zero row); amax32 fp32 on any device"""
    c = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)
    return torch.where(amax32 > 0, amax32 * c.to(amax32.device), torch.ones_like(amax32))


def layernorm_ref(x, gamma, beta, eps=1e-5):
    """float64 LayerNorm over the last dimension (biased variance)"""
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def quickgelu_ref(v):
    return v * torch.sigmoid(1.702 * v)


assert math.isnan(E4M3[0x7F].item()) and E4M3[0x7E].item() == E4M3_MAX
