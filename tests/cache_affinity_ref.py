"""TEST-ONLY helper of test_cache_affinity_cpu.py, test_cache_affinity_gpu.py and test_fewshot_gpu.py: problems, a float64
reference of the class affinities, the derived tolerance, a torch restatement of ops.cache_affinity for host-logic tests, and
the seeded classification fixture.

Reference.  A_ref[q, c] = sum over the rows n with labels[n] == c, n != exclude[q], of exp(beta * (<q, g_n> - 1)) in float64 on
the SAME 16-bit operands, with a plain per-class loop over the ORIGINAL row order: it shares no layout code with the product.

Tolerance, per element, derived and not fitted:
    tol[q, c] = A_ref[q, c] * ( beta * D * 2^-22 * max|q| * max|g|                      # (1)
                                + (8 * beta * (1 + max|s|) + 8 + N_c) * 2^-24 )         # (2)
(1) the score error: products of two 16-bit operands are exact in fp32, so only the D - 1 additions round; D 2^-24 |q| |g|
    sequentially, a factor 4 for the MFMA's internal order (kernel_tol of test_retrieval_gpu.py; |.| = largest row 2-norm),
    times beta because d/ds exp(beta (s - 1)) = beta exp(..).
(2) the exponent beta * (s - 1) is formed with two roundings and scaled by log2(e) inside the kernel's __expf with one more,
    each at most |beta| (1 + |s|) 2^-24 in the exponent, i.e. relative in the result; v_exp_f32 itself is documented at 1 ulp.
    The factor 8 covers these five roundings with room.  A class sum is N_c non-negative terms: at most N_c - 1 additions of
    2^-24 relative each, in any order.  (N_c = the class's live count, excluded row or not.)
An element whose reference is 0 (empty class, or only row excluded) has tol 0: the kernel must give exactly 0.0.

Largest err / tol measured on the MI355X (every case prints its own `[cache] ... err/tol`): 2.14e-2 (bf16, un-normalised rows of
small norm, D = 64); 2.02e-2 for fp16 on the same case; every normalised case stays below 7e-3.
"""
import math

import torch

DTYPES = [torch.bfloat16, torch.float16]


def make_problem(seed, Q, sizes, D, dtype, normalise=True, scale=1.0):
    """Class sizes `sizes` (class c has sizes[c] rows) scattered over the ORIGINAL row order.  Returns (q16 [Q, D], g16 [N, D],
    labels int64 [N]) on the host; rows normalised in fp32 and then rounded to `dtype` (or `scale` * randn, un-normalised)."""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.cat([torch.full((n,), c, dtype=torch.long) for c, n in enumerate(sizes)])
    labels = labels[torch.randperm(labels.numel(), generator=gen)]
    q, g = torch.randn(Q, D, generator=gen), torch.randn(labels.numel(), D, generator=gen)
    if normalise:
        g = g + 0.5 * q[torch.randint(0, Q, (g.shape[0],), generator=gen)]       # some stored rows near some query: A not flat
        q, g = q / q.norm(dim=1, keepdim=True), g / g.norm(dim=1, keepdim=True)
    else:
        q, g = q * scale, g * scale
    return q.to(dtype), g.to(dtype), labels


def reference(q16, g16, labels, C, beta, exclude=None):
    """float64 A_ref [Q, C] and the scores s [Q, N]; exclude: ORIGINAL rows [Q] (or -1), or None"""
    q, g = q16.double().cpu(), g16.double().cpu()
    s = q @ g.t()
    e = torch.exp(beta * (s - 1.0))
    if exclude is not None:
        ex = torch.as_tensor(exclude).long()
        for i in range(q.shape[0]):
            if ex[i] >= 0:
                e[i, ex[i]] = 0.0
    A = torch.zeros(q.shape[0], C, dtype=torch.float64)
    for c in range(C):
        rows = (labels == c).nonzero()[:, 0]
        for n in rows.tolist():
            A[:, c] += e[:, n]
    return A, s


def tolerance(A_ref, beta, q16, g16, labels, s):
    D = q16.shape[1]
    qn = q16.double().norm(dim=1).max().item()
    gn = g16.double().norm(dim=1).max().item() if g16.shape[0] else 0.0
    smax = s.abs().max().item() if s.numel() else 0.0
    counts = torch.bincount(labels, minlength=A_ref.shape[1]).double()
    b = abs(beta)
    rel = b * D * 2.0 ** -22 * qn * gn + (8.0 * b * (1.0 + smax) + 8.0 + counts) * 2.0 ** -24
    return A_ref * rel[None, :]


def ratio(out, A_ref, tol):
    """largest err / tol over the elements (0 / 0 counts as 0, err > 0 at tol 0 as inf)"""
    err = (out.double().cpu() - A_ref).abs()
    r = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def check(out, A_ref, tol, what):
    assert out.shape == A_ref.shape and out.dtype == torch.float32, what
    assert not torch.isnan(out).any(), f"{what}: NaN in the output"
    r = ratio(out, A_ref, tol)
    print(f"[cache] {what} err/tol {r:.3e}")
    assert r <= 1.0, f"{what}: err / tol = {r:.3e}"
    return r


def lay_out(g16, labels, C):
    """the product's layout of a problem: (laid [Np, D] with NaN padding, gather, class_off, class_len)"""
    from cclip_hip import ops
    gather, off, ln = ops.cache_layout(labels, C)
    laid = torch.full((gather.numel(), g16.shape[1]), float("nan"), dtype=g16.dtype)
    laid[gather >= 0] = g16[gather[gather >= 0]]
    return laid, gather, off, ln


def to_laid(exclude, gather):
    """ORIGINAL rows [Q] (or -1) -> int32 laid-out rows"""
    pos = torch.full((int(gather.max()) + 2,), -1, dtype=torch.long)
    pos[gather[gather >= 0]] = torch.arange(gather.numel())[gather >= 0]
    ex = torch.as_tensor(exclude).long()
    return torch.where(ex >= 0, pos[ex.clamp(min=0)], ex).to(torch.int32)


def torch_cache_affinity(q, g, class_off, class_len, beta, *, exclude=None, out=None):
    """ops.cache_affinity's contract restated with torch ops in fp32 on whatever device the operands live on (matmul, exp,
    masked per-class sums): what the host logic of clip.fewshot is run on where there is no GPU."""
    assert q.dtype == g.dtype and q.dtype in DTYPES and class_off.dtype == torch.int32 and class_len.dtype == torch.int32
    Q, C = q.shape[0], class_len.numel()
    assert class_off.numel() == C + 1 and int(class_off[-1]) == g.shape[0]
    s = q.float() @ g.float().t()
    rows = torch.arange(g.shape[0])
    res = torch.zeros(Q, C, dtype=torch.float32) if out is None else out
    for c in range(C):
        o, n = int(class_off[c]), int(class_len[c])
        live = ((rows >= o) & (rows < o + n))[None, :].expand(Q, -1)
        if exclude is not None:
            live = live & (rows[None, :] != exclude.long().cpu()[:, None])
        e = torch.exp(beta * (s - 1.0))
        res[:, c] = torch.where(live, e, torch.zeros_like(e)).sum(dim=1)
    return res


# ---- the classification fixture of test_cache_affinity_cpu.py and test_fewshot_gpu.py ---------------------------------
FIX_C, FIX_E, FIX_SHOTS, FIX_Q = 9, 512, 12, 90
FIX_ALPHA, FIX_BETA = 20.0, 5.5      # the cache term has to outweigh logit_scale = 100 times noise of the random text features


def fewshot_fixture():
    """C = 9 class centroids in E = 512 plus noise: 12 stored rows per class (class-major order shuffled), 90 queries, and
    random text features that carry no information about the classes.  fp32, on the host, seeded."""
    gen = torch.Generator().manual_seed(20221023)
    cent = torch.randn(FIX_C, FIX_E, generator=gen)
    lab = torch.arange(FIX_C).repeat_interleave(FIX_SHOTS)[torch.randperm(FIX_C * FIX_SHOTS, generator=gen)]
    feats = cent[lab] + 0.5 * torch.randn(lab.numel(), FIX_E, generator=gen)
    qlab = torch.arange(FIX_Q) % FIX_C
    queries = cent[qlab] + 0.5 * torch.randn(FIX_Q, FIX_E, generator=gen)
    text = torch.randn(FIX_C, FIX_E, generator=gen)
    return dict(features=feats, labels=lab, queries=queries, query_labels=qlab, text=text)


def round_rows(x, dtype):
    """fp32 L2 normalisation then rounding to `dtype`, on the host (what retrieval.normalize_rows leaves on the device, up to
    the last bit of the fp32 norm)"""
    x = x.float()
    return (x / x.norm(dim=1, keepdim=True)).to(dtype)


def reference_logits(q16, g16, labels, C, alpha, beta, text=None, logit_scale=100.0, exclude=None):
    """float64 logits of the cache model on the 16-bit rows, and the per-element tolerance of the cache term times alpha.
    The zero-shot term is taken in float64 on the same 16-bit query rows and the fp32 text features, normalised in float64."""
    A, s = reference(q16, g16, labels, C, beta, exclude)
    tol = alpha * tolerance(A, beta, q16, g16, labels, s)
    logits = alpha * A
    if text is not None:
        qd, td = q16.double(), text.double()
        qd, td = qd / qd.norm(dim=1, keepdim=True), td / td.norm(dim=1, keepdim=True)
        logits = logits + logit_scale * (qd @ td.t())
        tol = tol + logit_scale * (q16.shape[1] + 8) * 2.0 ** -24     # the E-term fp32 dot product of unit vectors, their normalisations
    return logits, tol


def decided(logits, tol):
    """rows whose top-2 margin in the reference exceeds the two classes' tol: (mask [Q], argmax [Q])"""
    top = logits.topk(2, dim=1)
    margin = top.values[:, 0] - top.values[:, 1]
    slack = tol.gather(1, top.indices).sum(dim=1)
    return margin > slack, top.indices[:, 0]
