"""ops.adamw_step_groups and ops.sumsq at the C boundary (csrc/optim.hip), both shadow dtypes and both AdamW forms.

Sizes: 4, 64, 128 + 4, 64 * 257 and one at which a thread takes a second trip round its grid-stride loop, computed from the
launcher's own grid (ops.adamw_grid / ops.sumsq_workspace).  Group tables: one group, groups alternating per chunk, 256 groups, a
table that starts at a non-zero (odd) offset of a longer one.
  K1 bit for bit: one group, no scalar, no EMA == ops.adamw_step; max_norm = 1e30 == the run without a scalar; skip_nonfinite with
     one planted inf leaves p, m, v, ema and shadow alone and raises the counter by one, without it the same step proceeds.
  K2 per element: two steps with a clip coefficient (the first clipped, the second not) and an EMA, p / m / v / ema within the
     carried float64 bound of tests/optim_groups_ref.py; the coefficient of the reference is formed in double from the gradients,
     the bound widened by the derived relative error of the sum of squares; the shadow equals the rounded master.
  K3 sumsq: against float64 within (chain + butterfly + partials) * 2^-24, from a non-zero start too; equal bits from two launches;
     NaN and inf propagate and are counted; the workspace size is honoured and a smaller one raises.
The float64 references of the largest size run on the device (plain torch there)."""
import pytest
import torch

import kernel_refs_f64 as KR
import optim_groups_ref as OR

pytestmark = pytest.mark.gpu

DTS = [torch.bfloat16, torch.float16]
HYP = dict(beta1=0.9, beta2=0.999, eps=1e-6)


def _dtn(dt):
    return str(dt).replace("torch.", "")


def _second_trip():
    """the smallest interesting n past the launcher's grid cap: 2 float4 groups per thread and trip, plus a ragged tail"""
    from cclip_hip import ops
    cap = ops.adamw_grid(1 << 40)
    assert cap == ops.adamw_grid(4 * 256 * cap) and cap > ops.adamw_grid(4 * 256 * (cap - 1))
    return 4 * 2 * 256 * cap + 128 + 4


SMALL = [4, 64, 128 + 4, 64 * 257]


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _table(kind, n, dev):
    """(the uint8 chunk table to pass, the number of groups)"""
    chunks = (n + 63) // 64
    c = torch.arange(chunks)
    if kind == "one":
        return torch.zeros(chunks, dtype=torch.uint8, device=dev), 1
    if kind == "alt":
        return (c % 3).to(torch.uint8).to(dev), 3
    if kind == "256":
        assert chunks >= 256
        return ((c * 7 + 5) % 256).to(torch.uint8).to(dev), 256
    assert kind == "offset"
    long = torch.cat([torch.full((3,), 9, dtype=torch.int64), (c * 5 + 1) % 4, torch.full((5,), 9, dtype=torch.int64)]).to(torch.uint8).to(dev)
    return long[3:3 + chunks], 4              # a view: its pointer is 3 bytes into the allocation; group 9 must never be read


def _data(n, seed, dev):
    g = KR.gen(seed)
    mag = 10.0 ** (-4.0 + 5.0 * torch.rand((n + 63) // 64, generator=g)).repeat_interleave(64)[:n]
    p = torch.randn(n, generator=g)
    g1 = torch.randn(n, generator=g) * mag
    g2 = torch.randn(n, generator=g) * mag * 0.05
    g1[:2] = 0.0
    return p.to(dev), [g1.to(dev), g2.to(dev)]


def _hyper(G):
    lrs = [[1e-3 * (1 + k % 5) for k in range(G)], [2e-3 / (1 + k % 3) for k in range(G)]]
    wds = [0.0 if k % 2 else 0.05 + 0.001 * k for k in range(G)]
    return lrs, wds


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("mode", [0, 1])
def test_one_group_without_scalar_or_ema_is_adamw_step_bit_for_bit(mode, dt):
    """K1"""
    from cclip_hip import ops
    for n in SMALL + [_second_trip()]:
        p, grads = _data(n, 11, "cuda")
        tab, _ = _table("one", n, "cuda")
        a = [p.clone(), torch.zeros_like(p), torch.zeros_like(p), torch.zeros(n, device="cuda", dtype=dt)]
        b = [t.clone() for t in a]
        for step, g in enumerate(grads, 1):
            kw = dict(step=step, correct_bias=step == 1 or mode == 1, grad_scale=0.25, mode=mode, **HYP)
            ops.adamw_step(a[0], g, a[1], a[2], lr=1e-3 * step, weight_decay=0.05, bf16_shadow=a[3], **kw)
            ops.adamw_step_groups(b[0], g, b[1], b[2], tab, lrs=[1e-3 * step], weight_decays=[0.05], bf16_shadow=b[3], **kw)
            for nm, x, y in zip(("p", "m", "v", "shadow"), a, b):
                assert _same(x, y), f"n {n} step {step}: {nm} differs from adamw_step"
        assert not torch.equal(a[0], p)


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("mode", [0, 1])
def test_huge_max_norm_is_the_unclipped_run_and_nonfinite_steps_are_skipped(mode, dt):
    """K1"""
    from cclip_hip import ops
    n = 64 * 257
    p, grads = _data(n, 12, "cuda")
    tab, G = _table("alt", n, "cuda")
    lrs, wds = _hyper(G)
    kw = dict(lrs=lrs[0], weight_decays=wds, step=3, grad_scale=-0.5, mode=mode, ema_decay=0.75, **HYP)

    def fresh():
        return [p.clone(), grads[1].clone() * 3, grads[0].abs() * 2, torch.zeros(n, device="cuda", dtype=dt), p.clone() * 0.5]

    def run(s, g, **more):
        ops.adamw_step_groups(s[0], g, s[1], s[2], tab, bf16_shadow=s[3], ema=s[4], **kw, **more)

    plain, big = fresh(), fresh()
    ss = ops.sumsq(grads[0])
    run(plain, grads[0])
    run(big, grads[0], sumsq_dev=ss, max_norm=1e30)
    assert all(_same(x, y) for x, y in zip(plain, big)), "max_norm = 1e30 must not change a bit"
    clipped = fresh()
    run(clipped, grads[0], sumsq_dev=ss, max_norm=1e-3)
    assert not _same(clipped[1], plain[1]), "a small max_norm must clip"
    # one planted inf
    bad = grads[0].clone()
    bad[n // 2 + 1] = float("inf")
    count = torch.full((1,), 41, device="cuda", dtype=torch.int32)
    ss = ops.sumsq(bad, nonfinite_count=count)
    assert int(count) == 42 and not bool(torch.isfinite(ss).any())
    skipped, before = fresh(), fresh()
    run(skipped, bad, sumsq_dev=ss, max_norm=1.0, skip_nonfinite=True)
    for nm, x, y in zip(("p", "m", "v", "shadow", "ema"), skipped, before):
        assert _same(x, y), f"a skipped step wrote {nm}"
    run(skipped, bad, sumsq_dev=ss, max_norm=1.0, skip_nonfinite=False)
    assert not _same(skipped[1], before[1]) and not _same(skipped[4], before[4]), "without skip_nonfinite the same step proceeds"
    ops.sumsq(grads[0], out=ss, nonfinite_count=count)
    assert int(count) == 42, "a finite sum is not counted"
    run(before, grads[0], sumsq_dev=ss, max_norm=1e30, skip_nonfinite=True)
    assert all(_same(x, y) for x, y in zip(plain, before)), "skip_nonfinite with a finite sum is the plain step"


CASES = [(4, "one"), (64, "one"), (128 + 4, "alt"), (64 * 257, "alt"), (64 * 257, "256"), (64 * 257, "offset"), (None, "256")]


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,kind", CASES, ids=[f"{n or 'second-trip'}-{k}" for n, k in CASES])
def test_grouped_step_per_element_f64(n, kind, mode, dt):
    """K2.  Step 1 is clipped (max_norm = half its norm), step 2 is not (its gradients are 20 times smaller)."""
    from cclip_hip import ops
    n = n or _second_trip()
    dev = "cuda" if n > 10 ** 6 else "cpu"                   # where the float64 reference runs
    p0, grads = _data(n, 13, "cuda")
    tab, G = _table(kind, n, "cuda")
    lrs, wds = _hyper(G)
    gs = 0.5
    max_norm = float(0.5 * gs * grads[0].double().norm())
    assert gs * float(grads[1].double().norm()) < 0.9 * max_norm
    decays = [0.5, 0.9]
    s = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros(n, device="cuda", dtype=dt), p0.clone()]
    ws = torch.empty(ops.sumsq_workspace(n) // 4, device="cuda")
    ss = torch.zeros(1, device="cuda")
    for t in range(2):
        ops.sumsq(grads[t], out=ss, workspace=ws)
        ops.adamw_step_groups(s[0], grads[t], s[1], s[2], tab, lrs=lrs[t], weight_decays=wds, step=t + 1, grad_scale=gs, mode=mode,
                              bf16_shadow=s[3], sumsq_dev=ss, max_norm=max_norm, ema=s[4], ema_decay=decays[t], **HYP)
    group_of = tab.long().to(dev).repeat_interleave(64)[:n]
    ref, bnd = OR.trajectory(p0.to(dev), [g.to(dev) for g in grads], group_of, lrs, wds, steps=(1, 2), grad_scale=gs, max_norm=max_norm,
                             ema_decays=decays, sumsq_rel=OR.sumsq_rel(n, ops.sumsq_workspace(1 << 40) // 4), mode=mode, **HYP)
    worst = {}
    for nm, got in (("p", s[0]), ("m", s[1]), ("v", s[2]), ("ema", s[4])):
        got = got.to(dev).double()
        assert bool(torch.isfinite(got).all()), nm
        ratio = (got - ref[nm]).abs() / (bnd[nm] + 1e-300)
        worst[nm] = float(ratio.max())
        assert worst[nm] <= 1.0, f"{nm}: {int((ratio > 1).sum())}/{n} elements outside the bound, worst err/bound {worst[nm]:.3g} at {int(ratio.argmax())}"
    print(f"n {n} {kind} mode {mode} {_dtn(dt)}: worst err/bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert _same(s[3], s[0].to(dt)), "the shadow is not the rounded master"
    if n == 64 * 257 and kind == "alt":                      # the comparison can see something
        for fault, where in (("table_shift", "p"), ("decay_no_decay", "p"), ("ema_p_old", "ema"), ("coef_after_moments", "m")):
            wrong, _ = OR.trajectory(p0.cpu(), [g.cpu() for g in grads], group_of, lrs, wds, steps=(1, 2), grad_scale=gs, max_norm=max_norm,
                                     ema_decays=decays, fault=fault, mode=mode, **HYP)
            got = dict(p=s[0], m=s[1], ema=s[4])[where].cpu()
            assert KR.rejects(got, wrong[where], bnd[where]), f"the bound cannot see the planted fault {fault}"


def _sumsq_terms(n):
    from cclip_hip import ops
    blocks = ops.sumsq_workspace(n) // 4
    n4 = n // 4
    return 4 * ((n4 + blocks * 256 - 1) // (blocks * 256)), blocks


def test_sumsq_f64_bits_nonfinite_and_workspace():
    """K3"""
    from cclip_hip import ops
    cap = ops.sumsq_workspace(1 << 40) // 4
    assert ops.sumsq_workspace(4) == 4 and ops.sumsq_workspace(1024 * cap) == 4 * cap == ops.sumsq_workspace(1024 * cap + 4)
    assert ops.sumsq_workspace(0) == 0 and ops.sumsq_workspace(6) == 0
    sizes = SMALL + [1024 * cap + 128 + 4]                   # the last: some threads take a second trip
    assert _sumsq_terms(sizes[-1]) == (8, cap) and _sumsq_terms(64 * 257) == (4, 17)
    for n in sizes:
        x = _data(n, 14, "cuda")[1][0] * 30
        chain, blocks = _sumsq_terms(n)
        ws = torch.full((blocks + 7,), -7.0, device="cuda")
        out = ops.sumsq(x, workspace=ws)
        ref, b = OR.sumsq(x.cpu(), chain=chain, butterfly=9, partials=blocks)
        err = abs(float(out.double()) - float(ref))
        print(f"sumsq n {n}: err/bound {err / float(b):.3g}")
        assert err <= float(b), (n, err, float(b))
        assert bool((ws[blocks:] == -7.0).all()) and bool((ws[:blocks] >= 0).all()), "the workspace beyond sumsq_workspace(n) was written"
        again = ops.sumsq(x, workspace=ws)
        assert _same(out, again), "two launches differ"
        # a non-zero start
        acc = torch.full((1,), 3.25, device="cuda")
        ops.sumsq(x, out=acc, accumulate=True)
        ref2, b2 = OR.sumsq(x.cpu(), out0=3.25, chain=chain, butterfly=9, partials=blocks + 1)
        assert abs(float(acc.double()) - float(ref2)) <= float(b2), n
        with pytest.raises(ValueError, match="workspace"):
            ops.sumsq(x, workspace=torch.empty(blocks - 1, device="cuda")) if blocks > 1 else ops.sumsq(x, workspace=torch.empty(0, device="cuda"))
        for bad in (float("nan"), float("inf"), float("-inf")):
            y = x.clone()
            y[n - 1] = bad
            count = torch.zeros(1, device="cuda", dtype=torch.int32)
            o = ops.sumsq(y, nonfinite_count=count)
            assert not bool(torch.isfinite(o).any()) and int(count) == 1, (n, bad)
            ops.sumsq(x, out=o, accumulate=True, nonfinite_count=count)
            assert not bool(torch.isfinite(o).any()) and int(count) == 2, "a non-finite start stays non-finite"


def test_argument_errors_name_the_argument():
    from cclip_hip import ops
    n = 128
    p, (g, _) = _data(n, 15, "cuda")
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    tab = torch.zeros(2, dtype=torch.uint8, device="cuda")
    ok = dict(lrs=[1e-3], weight_decays=[0.0])
    ops.adamw_step_groups(p, g, m, v, tab, **ok)
    for kw, msg in ((dict(lrs=[], weight_decays=[]), "groups"), (dict(lrs=[1.0] * 257, weight_decays=[0.0] * 257), "groups"),
                    (dict(ok, max_norm=1.0), "sumsq_dev"), (dict(ok, sumsq_dev=torch.ones(1, device="cuda")), "max_norm"),
                    (dict(ok, sumsq_dev=torch.ones(1, device="cuda"), max_norm=float("inf")), "max_norm"),
                    (dict(ok, ema=p.clone(), ema_decay=1.5), "ema_decay"), (dict(ok, step=0), "step")):
        with pytest.raises(ValueError, match=msg):
            ops.adamw_step_groups(p, g, m, v, tab, **kw)
    with pytest.raises(ValueError, match="chunk_group"):
        ops.adamw_step_groups(p, g, m, v, tab[:1], **ok)
    with pytest.raises(TypeError, match="chunk_group"):
        ops.adamw_step_groups(p, g, m, v, tab.int(), **ok)
    with pytest.raises(TypeError, match="grad"):
        ops.adamw_step_groups(p, g.cpu(), m, v, tab, **ok)
    with pytest.raises(ValueError, match="16-byte"):
        ops.adamw_step_groups(torch.zeros(n + 4, device="cuda")[1:n + 1], g, m, v, tab, **ok)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.sumsq(p[:6])
    with pytest.raises(TypeError, match="x"):
        ops.sumsq(p.double())
    with pytest.raises(ValueError, match="accumulate"):
        ops.sumsq(p, accumulate=True)
