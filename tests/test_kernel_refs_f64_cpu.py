"""CPU: the hand-written float64 references of tests/kernel_refs_f64.py against torch's own float64 operators (layer_norm,
cross_entropy, norm, index_add_, torch.optim.AdamW, the restated transformers.AdamW of oracle/optim_oracle.py, matmul) to
1e-12 relative, so that the GPU tests never compare a kernel with a reference that is itself wrong; and the planted-error
checks of tests/test_kernels_f32_gpu.py with the kernel replaced by "the reference rounded to fp32": every bound accepts that
and rejects the planted error, so it separates the two without a kernel."""
import math

import pytest
import torch

import kernel_refs_f64 as KR

RT = 1e-12


def same(name, got, ref, scale=None):
    """|got - ref| <= 1e-12 * (|ref| + scale), scale = the magnitude the value was formed from (default: none)"""
    got, ref = got.double(), ref.double()
    tol = RT * (ref.abs() + (0.0 if scale is None else scale))
    bad = ~((got - ref).abs() <= tol)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements differ, worst {(got - ref).abs().max().item():.3g}"


def G(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("rows,D,shift", [(7, 4, 0.5), (7, 100, 0.5), (5, 1024, 1e3), (9, 260, 0.0)])
def test_layernorm_reference_matches_torch_float64(rows, D, shift):
    g = G(rows + D)
    x = (torch.randn(rows + 4, D, generator=g, dtype=torch.float64) + shift)
    x[1] = 0.75                                                         # a constant row
    x[2] = 0.0
    gamma = 1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    idx = torch.randperm(rows + 4, generator=g)[:rows].to(torch.int32)
    ref, bnd = KR.ln_fwd(x, gamma, beta, row_index=idx)
    xs = x[idx.long()].clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xs, (D,), gr, br, 1e-5)
    # a value formed from x - mean carries 1e-16 |x| rstd of cancellation noise in either implementation
    noise = (xs.detach().abs() * ref["rstd"][:, None]).amax(1, keepdim=True) * gamma.abs()
    same("y", ref["y"], y.detach(), noise)
    same("mean", ref["mean"], xs.detach().mean(1))
    same("rstd", ref["rstd"], torch.rsqrt(xs.detach().var(1, unbiased=False) + 1e-5), ref["rstd"] * noise[:, 0])
    assert all(bool((b >= 0).all()) for b in bnd.values())
    dy = torch.randn(rows, D, generator=g, dtype=torch.float64)
    res = torch.randn(rows, D, generator=g, dtype=torch.float64)
    g0, b0 = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    y.backward(dy)
    out, bb = KR.ln_bwd(dy, x, gamma, ref["mean"], ref["rstd"], row_index=idx, dx_res=res, dgamma0=g0, dbeta0=b0)
    mag = bb["dx"] / KR.E32                                            # the magnitudes dx is formed from
    same("dx", out["dx"], xs.grad + res, mag * (1 + noise))
    same("dgamma", out["dgamma"], gr.grad + g0, bb["dgamma"] / KR.E32 * (1 + noise.max()))
    same("dbeta", out["dbeta"], br.grad + b0, bb["dbeta"] / KR.E32)
    plain, _ = KR.ln_bwd(dy, x, gamma, ref["mean"], ref["rstd"], row_index=idx)
    same("dx without a residual", plain["dx"], xs.grad, mag * (1 + noise))
    same("dgamma, not accumulated", plain["dgamma"], gr.grad, bb["dgamma"] / KR.E32 * (1 + noise.max()))


def test_vit_x0_and_gathers_match_plain_indexing():
    g = G(3)
    B, T, D, V, L = 3, 5, 8, 7, 4
    patch, cls, pos = torch.randn(B * T, D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g)
    want = patch.view(B, T, D) + pos
    want[:, 0] = want[:, 0] + cls
    assert torch.equal(KR.vit_x0(patch, cls, pos, T), want.view(B * T, D))
    assert torch.equal(KR.vit_x0(patch[:4], cls, pos[:1], 1), patch[:4] + pos[0] + cls)          # T = 1: every row is a class row
    emb, posl = torch.randn(V, D, generator=g), torch.randn(L, D, generator=g)
    ids = torch.tensor([0, 6, -1, 7, 12, 3, 3, 1], dtype=torch.int32)
    cl = torch.tensor([0, 6, 0, 6, 6, 3, 3, 1])
    assert torch.equal(KR.text_embed(ids, emb, posl, L), emb[cl] + posl.repeat(2, 1))
    assert torch.equal(KR.text_embed(ids, emb, None, L), emb[cl])
    P, Lt = 2, 4
    prefix = torch.randn(2, P * D, generator=g)
    wpe = torch.randn(P + Lt, D, generator=g)
    want = torch.cat([prefix.view(2, P, D), emb[cl].view(2, Lt, D)], 1) + wpe
    assert torch.equal(KR.caption_embed(prefix, ids, emb, wpe, 2, P, Lt), want.view(-1, D))
    assert torch.equal(KR.caption_embed(prefix[:, :0], ids, emb, wpe[:Lt], 2, 0, Lt), (emb[cl].view(2, Lt, D) + wpe[:Lt]).view(-1, D))
    assert torch.equal(KR.caption_embed(prefix, None, emb, wpe[:P], 2, P, 0), (prefix.view(2, P, D) + wpe[:P]).view(-1, D))
    e = torch.randn(6, D, generator=g)
    assert torch.equal(KR.add_positional(e, wpe[:3], 3), e + wpe[:3].repeat(2, 1))


def test_embedding_gradient_and_colsum_references_match_index_add_and_sum():
    g = G(4)
    V, D, rows = 6, 12, 300
    ids = torch.randint(-2, V + 3, (rows,), generator=g).to(torch.int32)
    dx = torch.randn(rows, D, generator=g, dtype=torch.float64)
    base = torch.randn(V, D, generator=g, dtype=torch.float64)
    keep = torch.rand(rows, generator=g) > 0.3
    ref, bound = KR.embed_grad(ids, dx, base, keep=keep)
    want = base.clone().index_add_(0, ids.long().clamp(0, V - 1)[keep], dx[keep])
    same("embed_grad", ref, want, bound / KR.E32)
    # the GPT-2 row mapping
    Bq, S, P, Lt = 4, 9, 3, 5
    ids2 = torch.randint(0, V, (Bq * Lt,), generator=g).to(torch.int32)
    dxs = torch.randn(Bq * S, D, generator=g, dtype=torch.float64)
    ref2, b2 = KR.embed_grad(ids2, dxs, base, L=Lt, seq_stride=S, seq_off=P)
    want2 = base.clone().index_add_(0, ids2.long(), dxs.view(Bq, S, D)[:, P:P + Lt].reshape(-1, D))
    same("embed_grad rows", ref2, want2, b2 / KR.E32)
    none, _ = KR.embed_grad(ids, dx, base, keep=torch.zeros(rows, dtype=torch.bool))
    assert torch.equal(none, base)
    x = torch.randn(65, 20, generator=g, dtype=torch.float64)
    o0 = torch.randn(20, generator=g, dtype=torch.float64)
    ref, bound = KR.colsum(x, o0)
    same("colsum", ref, o0 + x.sum(0), bound / KR.E32)
    same("colsum plain", KR.colsum(x)[0], x.sum(0), bound / KR.E32)


@pytest.mark.parametrize("D", [1, 63, 65, 1000])
def test_l2norm_reference_matches_torch_float64(D):
    g = G(D)
    x = torch.randn(6, D, generator=g, dtype=torch.float64).requires_grad_(True)
    y = x / x.norm(dim=1, keepdim=True)
    ref, _ = KR.l2norm_fwd(x.detach())
    same("y", ref["y"], y.detach())
    same("inv", ref["inv"], 1 / x.detach().norm(dim=1))
    dy = torch.randn(6, D, generator=g, dtype=torch.float64)
    (y * 0.37).backward(dy)
    dx, bound = KR.l2norm_bwd(dy, ref["y"], ref["inv"], 0.37)
    same("dx", dx, x.grad, bound / KR.E32)
    zero, _ = KR.l2norm_fwd(torch.zeros(1, max(D, 2)))
    assert bool(zero["y"].isnan().all()) and bool(torch.isinf(zero["inv"]).all())      # what x / x.norm() gives


@pytest.mark.parametrize("R,C", [(9, 1), (9, 2), (9, 65), (9, 1000)])
def test_xent_reference_matches_torch_float64(R, C):
    g = G(R * C)
    z = (torch.randn(R, C, generator=g, dtype=torch.float64) * 3)
    labels = torch.randint(0, C, (R,), generator=g).to(torch.int32)
    labels[1], labels[2], labels[3] = -100, -1, C                     # the three ways a row is ignored
    if C > 1:
        z[4, C - 1] = z[4, 0] = z[4].max() + 1                         # a tie of the maximum: first index
        z[5] = 0.25
    zr = z.clone().requires_grad_(True)
    tl = labels.long().clone()
    tl[(tl < 0) | (tl >= C)] = -100
    loss = torch.nn.functional.cross_entropy(zr, tl, reduction="none", ignore_index=-100)
    loss.sum().backward()
    ref, bnd = KR.xent(z, labels, ignore_index=-100, grad_scale=0.5)
    same("loss", ref["loss"], loss.detach(), ref["lse"].abs())
    same("dlogits", ref["dlogits"], 0.5 * zr.grad, 1.0)
    same("rowdot", ref["rowdot"], (0.5 * zr.grad * z).sum(1), (0.5 * zr.grad * z).abs().sum(1))
    same("lse", ref["lse"], torch.logsumexp(z, 1))
    assert torch.equal(ref["pred"], z.argmax(1)) or C > 1               # torch.argmax promises no order on ties: checked below
    if C > 1:
        assert ref["pred"][4].item() == 0 and ref["pred"][5].item() == 0
        keep = torch.ones(R, dtype=torch.bool); keep[4] = keep[5] = False
        assert torch.equal(ref["pred"][keep], z.argmax(1)[keep])
    for r in (1, 2, 3):
        assert ref["loss"][r] == 0 and bool((ref["dlogits"][r] == 0).all()) and ref["rowdot"][r] == 0
    assert all(bool((b >= 0).all()) for b in bnd.values())
    other, _ = KR.xent(z, labels, ignore_index=int(labels[0]), grad_scale=0.5)     # label == ignore_index
    assert other["loss"][0] == 0 and bool((other["dlogits"][0] == 0).all())


def test_xent_reference_with_minus_infinity_logits():
    z = torch.tensor([[0.5, float("-inf"), 1.5, -2.0], [float("-inf"), 0.0, 0.0, 1.0]], dtype=torch.float64)
    ref, _ = KR.xent(z, torch.tensor([2, 3], dtype=torch.int32))
    want = torch.nn.functional.cross_entropy(z, torch.tensor([2, 3]), reduction="none")
    same("loss", ref["loss"], want)
    assert ref["p"][0, 1] == 0 and ref["p"][1, 0] == 0 and bool(torch.isfinite(ref["rowdot"]).all())


@pytest.mark.parametrize("n", [1, 63, 1025])
def test_reduce_dot_reference(n):
    g = G(n)
    a, b = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    ref, bound = KR.reduce_dot(a, b, alpha=0.5, mul=0.25, out0=1.5)
    same("dot", ref, 1.5 + 0.125 * torch.dot(a, b), bound / KR.E32)
    same("sum", KR.reduce_dot(a)[0], a.sum(), bound / KR.E32)
    parts = sum(KR.reduce_dot(a, b)[0] - KR.reduce_dot(a, b, drop_wave=w)[0] for w in range(16))
    same("the 16 wave partials add up to the sum", parts, torch.dot(a, b), (a * b).abs().sum())


# hyper-parameters that fp32 holds exactly: torch's optimisers take them as doubles
HYP = dict(lr=2.0 ** -10, beta1=0.875, beta2=1 - 2.0 ** -10, eps=2.0 ** -20)


def _adam_state(g, n=64):
    p = torch.randn(n, generator=g, dtype=torch.float64)
    gr = torch.randn(n, generator=g, dtype=torch.float64)
    gr[:4] = 0.0
    gr[4:8] = 1e-20
    return p, gr


@pytest.mark.parametrize("wd", [0.0, 2.0 ** -7])
def test_adamw_reference_mode1_matches_torch_optim_adamw(wd):
    p, gr = _adam_state(G(7))
    tp = torch.nn.Parameter(p.clone())
    tp.grad = gr.clone()
    opt = torch.optim.AdamW([tp], lr=HYP["lr"], betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"], weight_decay=wd)
    for _ in range(3):
        opt.step()
    z = torch.zeros_like(p)
    ref, _ = KR.adamw(p, gr, z, z, weight_decay=wd, steps=(1, 2, 3), mode=1, f32_hyper=False, **HYP)
    same("p", ref["p"], tp.detach())
    st = opt.state[tp]
    same("m", ref["m"], st["exp_avg"])
    same("v", ref["v"], st["exp_avg_sq"])


@pytest.mark.parametrize("wd,correct_bias", [(0.0, True), (2.0 ** -7, True), (2.0 ** -7, False)])
def test_adamw_reference_mode0_matches_the_restated_transformers_adamw(wd, correct_bias):
    from oracle.optim_oracle import HFAdamW
    p, gr = _adam_state(G(8))
    params = {"w": p.clone()}
    opt = HFAdamW(params, lr=HYP["lr"], betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"], weight_decay=wd, correct_bias=correct_bias)
    for _ in range(3):
        opt.step({"w": gr})
    z = torch.zeros_like(p)
    ref, bnd = KR.adamw(p, gr, z, z, weight_decay=wd, steps=(1, 2, 3), mode=0, correct_bias=correct_bias, f32_hyper=False, **HYP)
    same("p", ref["p"], params["w"])
    same("m", ref["m"], opt.state["w"]["exp_avg"])
    same("v", ref["v"], opt.state["w"]["exp_avg_sq"])
    if wd == 0.0:
        assert torch.equal(ref["p"][:4], p[:4]), "g = 0, m = v = 0, no decay: the parameter does not move"
    # grad_scale multiplies the gradient; fp32 hyper-parameters move the result by rounding only
    half, _ = KR.adamw(p, gr * 4, z, z, weight_decay=wd, steps=(1, 2, 3), mode=0, correct_bias=correct_bias, grad_scale=0.25, f32_hyper=False, **HYP)
    same("grad_scale", half["p"], ref["p"])
    r32, _ = KR.adamw(p, gr, z, z, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=wd, steps=(1, 2, 3), correct_bias=correct_bias)
    r64, _ = KR.adamw(p, gr, z, z, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=wd, steps=(1, 2, 3), correct_bias=correct_bias, f32_hyper=False)
    assert bool(((r32["p"] - r64["p"]).abs() <= 1e-4 * (r64["p"] - p).abs() + 1e-12).all())
    assert bool((bnd["p"] > 0).all())


@pytest.mark.parametrize("wd,correct_bias", [(0.0, True), (2.0 ** -7, True), (2.0 ** -7, False)])
def test_adamw_reference_trajectory_and_skip_mask_match_the_restated_transformers_adamw(wd, correct_bias):
    """The trajectory form: 4 steps, a gradient and a learning rate per step (the first lr is 0, as under a warm-up schedule), and
    a skip mask per step, against the oracle handed grad=None for the skipped parameters.  Three parameters in one flat vector:
    `a` always has a gradient, `b` has none at steps 3 and 4, `c` has none at step 2 and has one again afterwards.  The oracle
    keeps a step count per parameter (transformers.AdamW), the reference takes the step numbers it is given: with the global
    numbers 1..4 they agree wherever no counted step was skipped before (a, b; c too without bias correction); c under bias
    correction agrees when the reference is given c's own count."""
    from oracle.optim_oracle import HFAdamW
    g = G(9)
    n, names = 64, ("a", "b", "c")
    p0 = {k: torch.randn(n, generator=g, dtype=torch.float64) for k in names}
    grads = [{k: torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (i - 2) for k in names} for i in range(4)]
    for gs in grads:
        gs["a"][:4] = 0.0
    lrs = [0.0, HYP["lr"] / 2, HYP["lr"], HYP["lr"] * 0.75]
    absent = {"a": (), "b": (3, 4), "c": (2,)}
    hyp = {k: v for k, v in HYP.items() if k != "lr"}
    params = {k: v.clone() for k, v in p0.items()}
    opt = HFAdamW(params, lr=0.0, betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"], weight_decay=wd, correct_bias=correct_bias)
    after_first = None
    for i, lr in enumerate(lrs):
        opt.lr = lr
        opt.step({k: (None if i + 1 in absent[k] else grads[i][k]) for k in names})
        if i == 0:
            after_first = {k: v.clone() for k, v in params.items()}
    flat = lambda d: torch.cat([d[k] for k in names])                  # noqa: E731
    skip = [torch.cat([torch.full((n,), i + 1 in absent[k]) for k in names]) for i in range(4)]
    z = torch.zeros(3 * n, dtype=torch.float64)
    kw = dict(weight_decay=wd, mode=0, correct_bias=correct_bias, f32_hyper=False, **hyp)
    ref, bnd = KR.adamw(flat(p0), [flat(gs) for gs in grads], z, z, lr=lrs, steps=(1, 2, 3, 4), skip=skip, **kw)
    first, _ = KR.adamw(flat(p0), [flat(grads[0])], z, z, lr=lrs[:1], steps=(1,), skip=skip[:1], **kw)
    assert torch.equal(first["p"], flat(p0)), "lr = 0: the parameter does not move"
    assert torch.equal(first["p"], flat(after_first)) and bool((first["m"][4:] != 0).all()) and bool((first["v"][4:] != 0).all())
    for j, k in enumerate(names):
        sl = slice(j * n, (j + 1) * n)
        if k == "c" and correct_bias:
            own, _ = KR.adamw(p0[k], [gs[k] for gs in grads], z[sl], z[sl], lr=lrs, steps=(1, 2, 2, 3), skip=[s[sl] for s in skip], **kw)
            got = own
            assert not torch.equal(own["p"], ref["p"][sl]), "the global and the per-parameter step count must differ here"
        else:
            got = {nm: ref[nm][sl] for nm in ("p", "m", "v")}
        same(k + " p", got["p"], params[k])
        same(k + " m", got["m"], opt.state[k]["exp_avg"])
        same(k + " v", got["v"], opt.state[k]["exp_avg_sq"])
    # a skipped element carries everything unchanged, the bounds included
    two, b2 = KR.adamw(flat(p0), [flat(gs) for gs in grads[:2]], z, z, lr=lrs[:2], steps=(1, 2), skip=skip[:2], **kw)
    b_sl = slice(n, 2 * n)
    for nm in ("p", "m", "v"):
        assert torch.equal(ref[nm][b_sl], two[nm][b_sl]) and torch.equal(bnd[nm][b_sl], b2[nm][b_sl]), nm
    # the sequence form with one entry repeated is the present form
    rep, brep = KR.adamw(flat(p0), [flat(grads[1])] * 3, z, z, lr=[HYP["lr"]] * 3, steps=(1, 2, 3), skip=[None] * 3, **kw)
    old, bold = KR.adamw(flat(p0), flat(grads[1]), z, z, lr=HYP["lr"], steps=(1, 2, 3), **kw)
    assert all(torch.equal(rep[nm], old[nm]) and torch.equal(brep[nm], bold[nm]) for nm in ("p", "m", "v"))


@pytest.mark.parametrize("M,N,K", [(31, 33, 32), (33, 32, 31), (65, 33, 64)])
def test_gemm_reference_matches_matmul(M, N, K):
    g = G(M + N + K)
    A, B = torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64)
    C0 = torch.randn(M, N, generator=g, dtype=torch.float64)
    ref, bound = KR.gemm_f32(A, B, C0, alpha=0.5, beta=2.0)
    same("gemm", ref, 0.5 * (A @ B.t()) + 2.0 * C0, bound / KR.E32)
    nan = torch.full_like(C0, float("nan"))
    same("beta = 0 does not read C", KR.gemm_f32(A, B, nan, alpha=0.5)[0], 0.5 * (A @ B.t()), bound / KR.E32)
    same("alpha = 0", KR.gemm_f32(A, B, C0, alpha=0.0, beta=2.0)[0], 2.0 * C0)


@pytest.mark.parametrize("name", sorted(KR.PLANTED))
def test_every_bound_separates_fp32_rounding_from_its_planted_error(name):
    c = KR.PLANTED[name]()
    got = c["ref"].float()                                             # "a kernel that is correct to fp32"
    assert bool(((got.double() - c["ref"]).abs() <= c["bound"]).all()), "the bound rejects the reference rounded to fp32"
    assert KR.rejects(got, c["wrong"], c["bound"]), "the bound cannot see the planted error"
    assert not KR.rejects(got, c["ref"], c["bound"])
