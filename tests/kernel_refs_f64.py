"""Float64 references of the fp32 glue kernels (csrc/layernorm.hip, loss.hip, embed.hip, optim.hip, gemm_f32.hip), written out
by hand - no autograd inside - and, next to every result, the per-element error bound an fp32 evaluation of the same
expression may reach.  Plain torch on whatever device the operands live on; tests/test_kernel_refs_f64_cpu.py pins every
function against torch's own float64 operators, tests/test_kernels_f32_gpu.py compares the HIP kernels with them.

Bound forms (E = 2^-24, the fp32 unit roundoff; nothing is ever scaled by a tensor-wide maximum):
  * element-wise expressions: k * E * (sum of the magnitudes of the terms), k = the number of roundings on the path, counted in
    the comment next to each bound;
  * a reduction of n terms: RED(n) = C_RED * E * sqrt(n) times the sum of |terms|, plus E * |ref| for the final rounding.
    C_RED = 2.  The kernels sum a row as (a few sequential adds per lane) + (a 6-level butterfly), and a column over rows as
    (a few sequential visits) + (4 waves) + (a blocked tree): the depth of every one of those trees at the shapes the tests use
    is below 2 sqrt(n) (D = 1024: 15 + 6 <= 64; D = 4: 3 <= 4), so for them C_RED * sqrt(n) is also a worst-case bound.  The
    embedding-gradient runs (up to 64 sequential rows) and the fp32 GEMM's K-ordered fma chain are deeper than 2 sqrt(n): there
    the form is the usual probabilistic one, with the factor two over it that tests/test_kernels_f16_gpu.py uses (C_ACC);
  * __expf / __logf (xent_rows): exp(a) is formed as exp2(a * log2 e), so its relative error grows like (|a| + 1) * 2^-23;
    EXP_F = 4 over that, at the largest |logit - lse| of the row (`xent`).
The constants were fixed from these derivations before the first GPU run."""
import math

import torch

E32 = 2.0 ** -24
C_RED = 2.0
EXP_F = 4.0
FLT_MIN = 2.0 ** -126          # results below the smallest normal may be flushed


def red(n):
    """C_RED * E * sqrt(n); n a number or a tensor of term counts"""
    if torch.is_tensor(n):
        return C_RED * E32 * n.double().clamp_min(1.0).sqrt()
    return C_RED * E32 * math.sqrt(max(n, 1))


def f32(v: float) -> float:
    """the value a C `float` argument holds"""
    return torch.tensor(v, dtype=torch.float32).item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rejects(got, wrong, bound) -> bool:
    """True when `bound` tells `got` apart from the planted-error reference `wrong` in at least one element"""
    return bool(((got.double() - wrong).abs() > bound).any())


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps=1e-5, row_index=None, short_mean_row=None):
    """y = (x - mean) * rstd * gamma + beta per row (biased variance, two passes), rows gathered through row_index.
    short_mean_row: plant an error - that (output) row's sum for the mean leaves out its last 4 columns (one lane's group).
    Returns (dict y / mean / rstd / xhat, dict of bounds y / mean / rstd)."""
    x = x.double()
    if row_index is not None:
        x = x[row_index.long()]
    g, b = gamma.double(), beta.double()
    D = x.shape[1]
    mean = x.sum(1, keepdim=True) / D
    if short_mean_row is not None:
        mean = mean.clone()
        mean[short_mean_row] = x[short_mean_row, :D - 4].sum() / D
    xc = x - mean
    var = (xc * xc).sum(1, keepdim=True) / D
    rstd = 1.0 / (var + eps).sqrt()
    xh = xc * rstd
    y = xh * g + b
    B = red(D)
    d_mean = B * x.abs().sum(1, keepdim=True) / D + E32 * mean.abs()            # the sum; one rounding of the mean itself
    d_xc = d_mean + E32 * xc.abs()                                               # the subtraction
    d_var = 2 * (xc.abs() * d_xc).sum(1, keepdim=True) / D + (B + 4 * E32) * var  # squares (2E), their sum, * 1/D (2E)
    d_rstd = rstd * (0.5 * d_var / (var + eps) + 4 * E32)                        # + eps, rsqrtf (2E)
    d_xh = d_xc * rstd + xc.abs() * d_rstd + E32 * xh.abs()
    d_y = g.abs() * d_xh + E32 * (xh * g).abs() + E32 * y.abs()
    return (dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], xhat=xh),
            dict(y=d_y, mean=d_mean[:, 0], rstd=d_rstd[:, 0]))


def ln_bwd(dy, x, gamma, mean, rstd, row_index=None, dx_res=None, dgamma0=None, dbeta0=None):
    """The kernel's contract, with mean / rstd AS GIVEN (the saved fp32 statistics are operands, not recomputed):
      xhat = (x - mean) rstd; d = dy gamma; dx = rstd (d - mean_D(d) - xhat mean_D(d xhat)) (+ dx_res);
      dgamma = sum_rows dy xhat (+ dgamma0); dbeta = sum_rows dy (+ dbeta0).
    dx / dx_res are [rows, D] in OUTPUT-row order (row r belongs to input row row_index[r]).
    Returns (dict dx / dgamma / dbeta, dict of bounds)."""
    dy, g = dy.double(), gamma.double()
    xs = x.double() if row_index is None else x.double()[row_index.long()]
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    rows, D = dy.shape
    xh = (xs - mean) * rstd
    d = dy * g
    c1 = d.sum(1, keepdim=True) / D
    c2 = (d * xh).sum(1, keepdim=True) / D
    dx = rstd * (d - c1 - xh * c2)
    res = torch.zeros_like(dx) if dx_res is None else dx_res.double()
    dx = dx + res
    t_g = dy * xh
    dgamma, dbeta = t_g.sum(0), dy.sum(0)
    g0 = torch.zeros_like(dgamma) if dgamma0 is None else dgamma0.double()
    b0 = torch.zeros_like(dbeta) if dbeta0 is None else dbeta0.double()
    dgamma, dbeta = dgamma + g0, dbeta + b0
    B = red(D)
    # roundings on the path to dx (xhat: 2E, d: E, the two row means: B + 3E and B + 6E, products, two subtractions, * rstd):
    # at most B + 12E on each of |d|, mean|d| and |xhat| mean|d xhat|
    mag = d.abs() + d.abs().sum(1, keepdim=True) / D + xh.abs() * (d * xh).abs().sum(1, keepdim=True) / D
    b_dx = rstd * (B + 12 * E32) * mag + E32 * (res.abs() + dx.abs())
    b_dg = (red(rows) + 4 * E32) * t_g.abs().sum(0) + E32 * (g0.abs() + dgamma.abs())      # term: xhat 2E, product E
    b_db = red(rows) * dy.abs().sum(0) + E32 * (b0.abs() + dbeta.abs())
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta), dict(dx=b_dx, dgamma=b_dg, dbeta=b_db)


def vit_x0(patch, cls, pos, T):
    """x0 = (patch + positional[r % T]) + class_embedding at r % T == 0: fp32 adds in the kernel's order (each add is correctly
    rounded, so fp32 torch IS the exact reference of this part); vit_embed_ln's LayerNorm is ln_fwd(x0)."""
    rows = patch.shape[0]
    t = torch.arange(rows, device=patch.device) % T
    x0 = patch.float() + pos.float()[t]
    first = t == 0
    x0[first] = x0[first] + cls.float()
    return x0


# ---------------------------------------------------------------------------------------------------------------------------
# embeddings: one fp32 add per element -> exact references in fp32
# ---------------------------------------------------------------------------------------------------------------------------
def text_embed(ids, emb, pos, L):
    V = emb.shape[0]
    x = emb.float()[ids.long().clamp(0, V - 1)]
    if pos is not None:
        x = x + pos.float()[torch.arange(ids.numel(), device=ids.device) % L]
    return x


def caption_embed(prefix, ids, wte, wpe, B, P, Lt):
    """x[b, s] = (s < P ? prefix[b, s] : wte[clamp(ids[b, s - P])]) + wpe[s], rows b * (P + Lt) + s"""
    V, D = wte.shape
    parts = []
    if P:
        parts.append(prefix.float().reshape(B, P, D))
    if Lt:
        parts.append(wte.float()[ids.long().clamp(0, V - 1)].reshape(B, Lt, D))
    x = torch.cat(parts, 1) + wpe.float()[:P + Lt]
    return x.reshape(B * (P + Lt), D)


def add_positional(emb, wpe, S):
    rows = emb.shape[0]
    return emb.float() + wpe.float()[torch.arange(rows, device=emb.device) % S]


def embed_grad(ids, dx, demb0, keep=None, L=None, seq_stride=None, seq_off=0, drop_first_chunk_of=None):
    """demb[clamp(ids[r])] += dx[(r // L) * seq_stride + seq_off + r % L] over the kept rows, as a 0/1 matrix product in fp64.
    drop_first_chunk_of: plant an error - the first 64 kept rows of that id are left out.
    Bound per element: RED(run length of the id) * sum|dx| of the run + E (|demb0| + |ref|)."""
    rows = ids.numel()
    V, D = demb0.shape
    L = rows if L is None else L
    seq_stride = L if seq_stride is None else seq_stride
    r = torch.arange(rows, device=ids.device)
    tok = ids.long().clamp(0, V - 1)
    M = torch.zeros(V, rows, dtype=torch.float64, device=ids.device)
    M[tok, r] = 1.0 if keep is None else keep.double()
    run = M.sum(1)
    d = dx.double()[(r // L) * seq_stride + seq_off + r % L]
    absd = M @ d.abs()
    if drop_first_chunk_of is not None:
        first = M[drop_first_chunk_of].nonzero().flatten()[:64]
        M = M.clone()
        M[drop_first_chunk_of, first] = 0.0
    ref = demb0.double() + M @ d
    bound = red(run)[:, None] * absd + E32 * (demb0.double().abs() + ref.abs())
    return ref, bound


def colsum(x, out0=None, drop=None):
    """out[c] = (out0[c] +) sum_r x[r, c].  drop = (row, c0, c1): plant an error - that row's columns [c0, c1) are left out."""
    xv = x.double()
    R = xv.shape[0]
    o0 = torch.zeros(xv.shape[1], dtype=torch.float64, device=x.device) if out0 is None else out0.double()
    s = xv.sum(0)
    if drop is not None:
        r, c0, c1 = drop
        s = s.clone()
        s[c0:c1] -= xv[r, c0:c1]
    ref = o0 + s
    return ref, red(R) * xv.abs().sum(0) + E32 * (o0.abs() + ref.abs())


# ---------------------------------------------------------------------------------------------------------------------------
# loss side
# ---------------------------------------------------------------------------------------------------------------------------
def l2norm_fwd(x):
    """y = x / |x|, inv = 1 / |x|.  sum of squares: positive terms, relative error RED(D) + E; rsqrtf 2E; the product E."""
    x = x.double()
    D = x.shape[1]
    inv = 1.0 / (x * x).sum(1, keepdim=True).sqrt()
    y = x * inv
    rel = 0.5 * (red(D) + E32)
    return dict(y=y, inv=inv[:, 0]), dict(y=y.abs() * (rel + 4 * E32), inv=inv[:, 0] * (rel + 3 * E32))


def l2norm_bwd(dy, y, inv, mul=1.0):
    """dx = (dy - y <y, dy>) inv mul, y and inv as given"""
    dy, y, inv = dy.double(), y.double(), inv.double()[:, None]
    D = y.shape[1]
    s = (y * dy).sum(1, keepdim=True)
    dx = (dy - y * s) * inv * mul
    d_s = (red(D) + E32) * (y * dy).abs().sum(1, keepdim=True)
    # y s (E), the subtraction (E), inv * mul (E), the last product (E)
    bound = (inv * mul).abs() * (y.abs() * d_s + 4 * E32 * (dy.abs() + (y * s).abs()))
    return dx, bound


def xent(logits, labels, ignore_index=-100, grad_scale=1.0):
    """Row cross-entropy: lse, loss (0 on an ignored row: label == ignore_index, label < 0 or label >= C), pred = the LOWEST
    index holding the row maximum, dlogits = (softmax - onehot) grad_scale (an ignored row: zeros), rowdot = sum dlogits logits.
    Bounds from EPS = EXP_F (a + 1) 2^-23 with a = the largest finite |logit - lse| of the row (the largest exponent argument):
      lse:     EPS (the exps behind the sum: the arguments of a term's rescale chain add up to at most a) + RED(C) (the sum)
               + 4E (1 + |lse| + |max|) (__logf, the two additions)
      softmax: p (EPS + E a + d_lse)   (its own __expf, the rounding of logit - lse, and the error of lse)
    """
    z = logits.double()
    R, C = z.shape
    dev = z.device
    m = z.max(1).values
    s = torch.exp(z - m[:, None]).sum(1)
    lse = m + torch.log(s)
    cols = torch.arange(C, device=dev)[None, :].expand(R, C)
    pred = torch.where(z == m[:, None], cols, torch.full_like(cols, C)).min(1).values
    lab = labels.long()
    ign = (lab == ignore_index) | (lab < 0) | (lab >= C)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    p = torch.exp(z - lse[:, None])
    oh = torch.zeros_like(p)
    oh[torch.arange(R, device=dev), safe] = 1.0
    oh = oh * (~ign)[:, None]
    gs = torch.where(ign, torch.zeros_like(lse), torch.full_like(lse, f32(grad_scale)))
    d = (p - oh) * gs[:, None]
    z_lab = z.gather(1, safe[:, None])[:, 0]
    loss = torch.where(ign, torch.zeros_like(lse), lse - z_lab)
    dz = torch.where(d == 0, torch.zeros_like(d), d * z)                 # 0 * -inf: nothing
    rowdot = dz.sum(1)
    a = (z - lse[:, None]).abs()
    a_max = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max(1).values
    eps = EXP_F * (a_max + 1.0) * 2.0 ** -23
    B = red(C)
    d_lse = eps + B + 4 * E32 * (1.0 + lse.abs() + m.abs())
    d_p = p * (eps + E32 * a_max + d_lse)[:, None]
    b_d = gs[:, None] * (d_p + E32 * (p - oh).abs()) + E32 * d.abs() + FLT_MIN * gs[:, None]
    b_loss = torch.where(ign, torch.zeros_like(lse), d_lse + E32 * (loss.abs() + z_lab.abs()))
    zf = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))
    b_dot = (b_d * zf).sum(1) + (B + 2 * E32) * dz.abs().sum(1) + E32 * rowdot.abs()
    return (dict(lse=lse, loss=loss, pred=pred, dlogits=d, rowdot=rowdot, p=p, ignored=ign),
            dict(loss=b_loss, dlogits=b_d, rowdot=b_dot))


def reduce_dot(a, b=None, alpha=1.0, mul=1.0, out0=0.0, drop_wave=None):
    """out = out0 + alpha mul sum a b.  drop_wave: plant an error - the partial of that one of the kernel's 16 waves (elements
    with (i % 1024) // 64 == wave) is left out.  Returns (ref, bound) as 0-d tensors."""
    t = a.double() * (1.0 if b is None else b.double())
    n = t.numel()
    sel = torch.ones(n, dtype=torch.bool, device=t.device)
    if drop_wave is not None:
        sel = (torch.arange(n, device=t.device) % 1024) // 64 != drop_wave
    k = f32(alpha) * mul
    ref = out0 + k * t[sel].sum()
    # a b (E), alpha * mul (E), the scaling (E), the accumulate (E |ref|)
    bound = (red(n) + 3 * E32) * abs(k) * t.abs().sum() + E32 * (abs(out0) + ref.abs())
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW (both forms), fp32 GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def adamw(p, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, steps=(1,), correct_bias=True,
          grad_scale=1.0, mode=0, f32_hyper=True, skip=None):
    """len(steps) updates with the same gradient, step numbers as listed.  mode 0: transformers.AdamW (update, then decoupled
    decay), mode 1: torch.optim.AdamW (decay first, eps added after the bias-corrected sqrt).  f32_hyper: the hyper-parameters
    and the bias corrections are the fp32 values the C entry point receives / forms (float arguments; bc = (float)(1 - b^t)),
    so the reference is fed what the kernel is fed; False keeps them in double (the comparison with torch's own optimiser).
    A trajectory: `g` a list / tuple of gradients and / or `lr` a list / tuple of learning rates, one per step; `skip` a list /
    tuple with one entry per step, None or a boolean mask of the elements that are SKIPPED at that step - their p, m, v and the
    three bounds are carried unchanged (an optimiser that leaves a parameter without a gradient alone).
    Returns (dict p / m / v, dict of bounds), the bounds carried through the steps."""
    r = f32 if f32_hyper else float
    b1, b2, eps, wd, gsc = r(beta1), r(beta2), r(eps), r(weight_decay), r(grad_scale)
    n_steps = len(steps)
    gs = list(g) if isinstance(g, (list, tuple)) else [g] * n_steps
    lrs = [r(x) for x in lr] if isinstance(lr, (list, tuple)) else [r(lr)] * n_steps
    skips = [None] * n_steps if skip is None else list(skip)
    assert len(gs) == n_steps and len(lrs) == n_steps and len(skips) == n_steps, "one gradient / lr / skip mask per step"
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    dp, dm, dv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    for step, g_t, lr, sk in zip(steps, gs, lrs, skips):
        gr = g_t.double() * gsc
        held = None if sk is None else tuple(t.clone() for t in (p, m, v, dp, dm, dv))
        bc1 = r(1.0 - b1 ** step) if correct_bias else 1.0
        bc2 = r(1.0 - b2 ** step) if correct_bias else 1.0
        # g * grad_scale (E), the two products and the sum (3E)
        dm = b1 * dm + 4 * E32 * (b1 * m.abs() + (1 - b1) * gr.abs()) + FLT_MIN
        m = b1 * m + (1 - b1) * gr
        # gr^2 (3E), * (1 - b2) (E), b2 v (E), the sum (E)
        dv = b2 * dv + 6 * E32 * (b2 * v + (1 - b2) * gr * gr) + FLT_MIN
        v = b2 * v + (1 - b2) * gr * gr
        sq = v.sqrt()
        d_sq = torch.minimum(dv / (2 * sq).clamp_min(1e-300), dv.sqrt()) + E32 * sq
        if mode == 0:
            ss = lr * math.sqrt(bc2) / bc1
            den = sq + eps
            upd = ss * m / den
            # sqrtf(bc2), * lr, / bc1, * m, + eps, the division: 6E
            d_upd = upd.abs() * (6 * E32 + d_sq / den) + ss * dm / den
            p = p - upd
            dp = dp + d_upd + E32 * p.abs()
            if wd > 0:
                dec = lr * wd * p
                p = p - dec
                dp = dp + 3 * E32 * dec.abs() + E32 * p.abs()
        else:
            p = p * (1.0 - lr * wd)
            dp = dp + 3 * E32 * p.abs()
            s2 = math.sqrt(bc2)
            den = sq / s2 + eps
            d_den = d_sq / s2 + 3 * E32 * sq / s2
            upd = (lr / bc1) * m / den
            d_upd = upd.abs() * (5 * E32 + d_den / den) + (lr / bc1) * dm / den
            p = p - upd
            dp = dp + d_upd + E32 * p.abs()
        dp = dp + FLT_MIN
        if held is not None:
            p, m, v, dp, dm, dv = (torch.where(sk, old, new) for old, new in zip(held, (p, m, v, dp, dm, dv)))
    return dict(p=p, m=m, v=v), dict(p=dp, m=dm, v=dv)


def gemm_f32(A, B, C0=None, alpha=1.0, beta=0.0, drop=None):
    """C = alpha A B^T + beta C0 (A [M, K], B [N, K]); beta == 0: C0 is not an operand.  drop = (m0, m1, n0, n1, k0, k1): plant an
    error - that K range is left out of that output block.
    Bound: C_RED E sqrt(K) |alpha| (|A| |B|^T) + E (|beta C0| + |ref|)."""
    A, B = A.double(), B.double()
    K = A.shape[1]
    alpha, beta = f32(alpha), f32(beta)
    prod = A @ B.t()
    if drop is not None:
        m0, m1, n0, n1, k0, k1 = drop
        prod = prod.clone()
        prod[m0:m1, n0:n1] -= A[m0:m1, k0:k1] @ B[n0:n1, k0:k1].t()
    prior = beta * C0.double() if beta != 0.0 else torch.zeros_like(prod)
    ref = alpha * prod + prior
    bound = C_RED * E32 * math.sqrt(K) * abs(alpha) * (A.abs() @ B.abs().t()) + E32 * (prior.abs() + ref.abs())
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------
# the planted-error cases: the operands, the reference, the reference with one structural error and the bound.  The GPU tests
# run the kernel on exactly these operands; the CPU tests show that the bound separates "correct to fp32" (the reference
# rounded to fp32) from the planted error without any kernel.
# ---------------------------------------------------------------------------------------------------------------------------
def case_ln_short_mean(D=1024, rows=7, row=3):
    g = gen(100 + D)
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    ref, bnd = ln_fwd(x, gamma, beta)
    wrong, _ = ln_fwd(x, gamma, beta, short_mean_row=row)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref["y"], wrong=wrong["y"], bound=bnd["y"] + 1e-300)


def case_embed_missing_chunk(D=260, V=6, hot=2, run=129):
    g = gen(200 + D)
    ids = torch.cat([torch.full((run,), hot), torch.randint(0, V, (40,), generator=g)])
    ids = ids[torch.randperm(ids.numel(), generator=g)].to(torch.int32)
    rows = ids.numel()
    dx = torch.randn(rows, D, generator=g)
    demb0 = torch.randn(V, D, generator=g)
    ref, bound = embed_grad(ids, dx, demb0)
    wrong, _ = embed_grad(ids, dx, demb0, drop_first_chunk_of=hot)
    return dict(ids=ids, dx=dx, demb0=demb0, ref=ref, wrong=wrong, bound=bound + 1e-300)


def case_colsum_missing_lane(dt, R=4097, C=100, row=2000):
    """16-bit input: the half lane of C % 8 == 4 (columns 96..99, a 4-column load); fp32 input: a full lane's 8 columns"""
    g = gen(300 + R + C)
    x = torch.randn(R, C, generator=g).to(dt)
    out0 = torch.randn(C, generator=g)
    c0, c1 = (C // 8 * 8, C) if dt != torch.float32 else (8, 16)
    ref, bound = colsum(x, out0)
    wrong, _ = colsum(x, out0, drop=(row, c0, c1))
    return dict(x=x, out0=out0, ref=ref, wrong=wrong, bound=bound + 1e-300)


def case_reduce_dot_missing_wave(n=100003, wave=7):
    g = gen(400 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref, bound = reduce_dot(a, b, alpha=0.5, mul=0.37, out0=1.25)
    wrong, _ = reduce_dot(a, b, alpha=0.5, mul=0.37, out0=1.25, drop_wave=wave)
    return dict(a=a, b=b, ref=ref.reshape(1), wrong=wrong.reshape(1), bound=bound.reshape(1) + 1e-300)


def case_gemm_missing_kstep(M=65, N=33, K=64, tile=32, kstep=32):
    """the last K step of the last (ragged) tile"""
    g = gen(500 + M + N + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    C0 = torch.randn(M, N, generator=g)
    m0, n0, k0 = (M - 1) // tile * tile, (N - 1) // tile * tile, (K - 1) // kstep * kstep
    ref, bound = gemm_f32(A, B, C0, alpha=0.5, beta=2.0)
    wrong, _ = gemm_f32(A, B, C0, alpha=0.5, beta=2.0, drop=(m0, M, n0, N, k0, K))
    return dict(A=A, B=B, C0=C0, ref=ref, wrong=wrong, bound=bound + 1e-300)


PLANTED = {
    "layernorm: one row's mean over D-4 columns": case_ln_short_mean,
    "layernorm D=100: one row's mean over D-4 columns": lambda: case_ln_short_mean(D=100),
    "embedding gradient: one 64-row chunk missing": case_embed_missing_chunk,
    "colsum bf16: one half lane missing": lambda: case_colsum_missing_lane(torch.bfloat16),
    "colsum f16: one half lane missing": lambda: case_colsum_missing_lane(torch.float16),
    "colsum f32: one lane missing": lambda: case_colsum_missing_lane(torch.float32),
    "reduce_dot: one wave partial missing": case_reduce_dot_missing_wave,
    "gemm_f32: one K step missing from one tile": case_gemm_missing_kstep,
}
