"""clip.optim.AdamW with parameter groups, norm clipping, skipped steps and EMA weights over a whole ParamArena (test-tiny geometry,
both operand dtypes), and interpolate_weights.  Synthetic gradients as in tests/test_optim_arena_gpu.py: one magnitude per
parameter spread over 1e-6 .. 1e2, delivered in the arena slot, as a foreign tensor, or not at all.

  B1 trajectory: four steps under warm-up with layer_decay_groups (which carries the no-decay split) + clip + EMA under its own
     warm-up, p / m / v / ema within the carried float64 bound of tests/optim_groups_ref.py; padding exactly zero; shadows and
     transposed shadows consistent; exactly one adamw_step_groups launch per step and no adamw_step launch.
  B2 None gradients: such parameters keep p, m, v, ema and shadow and stay out of the norm (their slots hold NaN); values planted in
     the slots' padding cannot reach the norm either.
  B3 pending= ranges give the one-pass bits.   B4 the state-dict round trip gives the bits of the uninterrupted run, EMA included.
  B5 ema_weights() / ema_state_dict().   B6 interpolate_weights.   B7 without a new keyword: adamw_step, one launch, the same bits."""
import pytest
import torch

import kernel_refs_f64 as KR
import optim_groups_ref as OR

pytestmark = pytest.mark.gpu

DTS = [torch.bfloat16, torch.float16]
HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6)
N_STEPS = 4
FOREIGN = ("logit_scale", "visual.proj", "transformer.resblocks.1.attn.in_proj_bias")
NAN = float("nan")
MAX_NORM = 50.0
NEW = dict(max_grad_norm=MAX_NORM, ema_decay=0.99, ema_warmup=True)


def _dtn(dt):
    return str(dt).replace("torch.", "")


def _build(dt, seed=3):
    import clip
    from clip.weights import MODELS, init_state_dict
    return clip.build_model(init_state_dict(MODELS["test-tiny"], seed), dt).cuda()


def _opt(model, **kw):
    from clip import optim as coptim
    groups = coptim.layer_decay_groups(model, 0.5, weight_decay=0.05)
    return coptim.AdamW(model, **HYP, param_groups=groups, **dict(NEW, **kw))


class Layout:
    """the arena's geometry on the host and the synthetic gradients of every step"""

    def __init__(self, arena):
        self.names = list(arena.names)
        self.off = dict(arena.offsets)
        self.numel = {n: arena.params[n].numel() for n in self.names}
        self.total = arena.total
        self.pad = torch.ones(self.total, dtype=torch.bool)
        for n in self.names:
            self.pad[self.off[n]:self.off[n] + self.numel[n]] = False
        g = KR.gen(78)
        order = torch.randperm(len(self.names), generator=g)
        mag = torch.zeros(self.total)
        for i, n in enumerate(self.names):
            mag[self.off[n]:self.off[n] + self.numel[n]] = 10.0 ** (-6.0 + 8.0 * order[i].item() / (len(self.names) - 1))
        self.grads = [torch.randn(self.total, generator=g) * mag * (1.0 if t != 1 else 1e-3) for t in range(N_STEPS)]   # step 2 is not clipped

    def slot(self, n):
        return slice(self.off[n], self.off[n] + (self.numel[n] + 63) // 64 * 64)

    def skip_mask(self, none_names):
        m = torch.zeros(self.total, dtype=torch.bool)
        for n in none_names:
            m[self.slot(n)] = True
        return m


LAYOUT = {}


def _layout(arena):
    if "l" not in LAYOUT:
        LAYOUT["l"] = Layout(arena)
    assert LAYOUT["l"].total == arena.total and LAYOUT["l"].off == dict(arena.offsets)
    return LAYOUT["l"]


def _install(model, lay, t, none=()):
    ar = model.arena
    ar.gflat.copy_(lay.grads[t])
    for n, p in ar.params.items():
        if n in none:
            ar.g[n].fill_(NAN)
            p.grad = None
        elif n in FOREIGN:
            p.grad = ar.g[n].clone()
            ar.g[n].fill_(NAN)
        else:
            p.grad = ar.g[n]


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(model, opt):
    return dict(flat=model.arena.flat, m=opt._m, v=opt._v, ema=opt._ema, bflat=model.arena.bflat)


def _count(monkeypatch):
    from clip import optim as coptim
    calls = dict(groups=[], plain=[])
    for key, name in (("groups", "adamw_step_groups"), ("plain", "adamw_step")):
        real = getattr(coptim.ops, name)
        monkeypatch.setattr(coptim.ops, name, lambda param, *a, _r=real, _k=key, **k: (calls[_k].append(param.numel()), _r(param, *a, **k))[1])
    return calls


def _group_of(opt, lay):
    go = torch.zeros(lay.total, dtype=torch.int64)
    for gi, g in enumerate(opt.param_groups):
        for n in g["names"]:
            go[lay.slot(n)] = gi
    return go


def _ema_decays(n):
    return [min(NEW["ema_decay"], (1.0 + t) / (10.0 + t)) for t in range(1, n + 1)]


def _check_copies(model, opt, lay, what):
    ar = model.arena
    pad = lay.pad.cuda()
    for nm, buf in (("flat", ar.flat), ("gflat", ar.gflat), ("_m", opt._m), ("_v", opt._v), ("_ema", opt._ema), ("bflat", ar.bflat)):
        assert bool((buf[pad] == 0).all()), f"{what}: padding of {nm} is not zero"
    assert _same(ar.bflat, ar.flat.to(ar.shadow_dtype)), f"{what}: a shadow is not the rounded master"
    gen = ar.shadow_gen
    ar.refresh_shadows()
    assert ar.shadow_gen == gen, f"{what}: the step did not mark the shadows fresh"
    ar.refresh_transposed()
    assert ar.t
    for n, tv in ar.t.items():
        assert _same(tv.contiguous(), ar.b[n].t().contiguous()), f"{what}: transposed shadow of {n}"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("torch_semantics", [False, True], ids=["hf", "torch"])
def test_grouped_trajectory_over_the_arena_f64(torch_semantics, dt, monkeypatch):
    """B1.  get_linear_schedule_with_warmup(opt, 2, 6): factors 0, 1/2, 1, 3/4 on every group's own base learning rate."""
    from clip import optim as coptim
    from cclip_hip import ops
    from oracle.optim_oracle import linear_schedule
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    p0 = ar.flat.detach().cpu().double()
    opt = _opt(model, torch_semantics=torch_semantics)
    assert len(opt.param_groups) >= 8 and not opt.param_groups[0]["names"], "layer_decay_groups lists every parameter"
    decayed = {n for g in opt.param_groups if g["weight_decay"] > 0 for n in g["names"]}
    assert decayed == set(coptim.no_decay_groups(model, 0.05)[0]["params"])
    base = [g["lr"] for g in opt.param_groups]
    assert len(set(base)) == 4, "one learning rate per layer id"
    sched = coptim.get_linear_schedule_with_warmup(opt, 2, 6)
    lrs = [[b * linear_schedule(s, 2, 6) for b in base] for s in range(N_STEPS)]
    calls = _count(monkeypatch)
    gs = 0.5
    for t in range(N_STEPS):
        opt.zero_grad()
        _install(model, lay, t)
        assert [g["lr"] for g in opt.param_groups] == lrs[t]
        opt.step(grad_scale=gs)
        sched.step()
        assert calls["groups"] == [ar.total] * (t + 1) and not calls["plain"], "ONE adamw_step_groups launch per step, no adamw_step"
    norms = [gs * float(g.double().norm()) for g in lay.grads]
    assert norms[0] > MAX_NORM > norms[1], "clipped and unclipped steps"
    got_norm = float(opt.last_grad_norm)
    assert abs(got_norm - norms[-1]) <= norms[-1] * (OR.sumsq_rel(lay.total) / 2 + 4 * KR.E32), "last_grad_norm"
    assert opt.skipped_steps.dtype == torch.int32 and opt.skipped_steps.is_cuda and int(opt.skipped_steps) == 0
    ref, bnd = OR.trajectory(p0, lay.grads, _group_of(opt, lay), lrs, [g["weight_decay"] for g in opt.param_groups], steps=(1, 2, 3, 4),
                             grad_scale=gs, max_norm=MAX_NORM, ema_decays=_ema_decays(N_STEPS), sumsq_rel=OR.sumsq_rel(lay.total),
                             beta1=0.9, beta2=0.999, eps=1e-6, mode=int(torch_semantics))
    what = f"{'torch' if torch_semantics else 'hf'} {_dtn(dt)}"
    worst = {}
    for nm, got in (("p", ar.flat), ("m", opt._m), ("v", opt._v), ("ema", opt._ema)):
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all())
        ratio = (got - ref[nm]).abs() / (bnd[nm] + 1e-300)
        worst[nm] = float(ratio.max())
        assert worst[nm] <= 1.0, f"{what} {nm}: {int((ratio > 1).sum())} elements outside the bound, worst {worst[nm]:.3g} at flat index {int(ratio.argmax())}"
    print(f"{what}: worst err/bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    _check_copies(model, opt, lay, what)
    for fault, where in (("decay_no_decay", "p"), ("ema_p_old", "ema"), ("coef_after_moments", "m")):
        wrong, _ = OR.trajectory(p0, lay.grads, _group_of(opt, lay), lrs, [g["weight_decay"] for g in opt.param_groups], steps=(1, 2, 3, 4),
                                 grad_scale=gs, max_norm=MAX_NORM, ema_decays=_ema_decays(N_STEPS), fault=fault, mode=int(torch_semantics))
        got = dict(p=ar.flat, m=opt._m, ema=opt._ema)[where].detach().cpu()
        assert KR.rejects(got, wrong[where], bnd[where]), f"the bound cannot see {fault}"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_none_gradients_and_padding_stay_out(dt):
    """B2"""
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    none = {lay.names[0], "transformer.resblocks.0.ln_1.weight", "token_embedding.weight", "logit_scale"}
    ar.refresh_shadows()
    opt = _opt(model)
    _install(model, lay, 0)
    opt.step()
    before = {k: v.clone() for k, v in _state(model, opt).items()}
    _install(model, lay, 2, none=none)
    ar.gflat[lay.pad.cuda()] = 1e30                      # padding: of live and of skipped slots alike
    opt.step()
    after = _state(model, opt)
    for n in none:
        for k in before:
            assert _same(after[k][lay.slot(n)], before[k][lay.slot(n)]), f"{k} of {n} changed although its .grad is None"
    live = ~lay.skip_mask(none) & ~lay.pad
    want = float(lay.grads[2][live].double().norm())
    got = float(opt.last_grad_norm)
    assert abs(got - want) <= want * (OR.sumsq_rel(lay.total, ranges=8) / 2 + 4 * KR.E32), f"norm {got} against {want}: None slots or padding reached it"
    assert bool((ar.flat[lay.pad.cuda()] == 0).all()) and bool((opt._ema[lay.pad.cuda()] == 0).all())
    moved = [n for n in lay.names if n not in none and not _same(after["flat"][lay.slot(n)], before["flat"][lay.slot(n)])]
    assert len(moved) == len(lay.names) - len(none)
    assert _same(ar.bflat, ar.flat.to(dt))


class _Work:
    def __init__(self):
        self.waits = 0

    def wait(self):
        self.waits += 1


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_pending_ranges_give_the_one_pass_bits(dt):
    """B3.  With a norm to take every work object is waited on (once) before anything is launched."""
    from clip import parallel
    one, rng = _build(dt), _build(dt)
    lay = _layout(one.arena)
    buckets = parallel.grad_buckets(rng.arena, 300_000)
    assert len(buckets) >= 3
    works = [_Work() for _ in buckets]
    pending = [(s, e, w) for (s, e), w in zip(buckets, works)]
    o1, o2 = _opt(one), _opt(rng)
    o3m = _build(dt)
    o3 = _opt(o3m, max_grad_norm=None)                   # no norm: range by range
    o4m = _build(dt)
    o4 = _opt(o4m, max_grad_norm=None)
    for t in range(2):
        none = ("token_embedding.weight", "ln_final.bias") if t == 1 else ()
        for m in (one, rng, o3m, o4m):
            _install(m, lay, t, none=none)
        o1.step(grad_scale=0.25)
        o4.step(grad_scale=0.25)
        for m, o in ((rng, o2), (o3m, o3)):
            m.arena.adopt_foreign_grads()
            o.step(grad_scale=0.25, pending=pending)
        assert [w.waits for w in works] == [2 * (t + 1)] * len(works)
        for (a, b) in ((_state(one, o1), _state(rng, o2)), (_state(o4m, o4), _state(o3m, o3))):
            for k in a:
                assert _same(a[k], b[k]), f"step {t + 1}: {k} differs between one pass and pending ranges"
    assert not _same(one.arena.flat, o4m.arena.flat), "the clip changed nothing"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_state_dict_round_trip_is_bit_identical(dt):
    """B4"""
    import clip
    from clip.optim import get_linear_schedule_with_warmup

    def steps(model, opt, sched, ts):
        lay = _layout(model.arena)
        for t in ts:
            opt.zero_grad()
            _install(model, lay, t)
            opt.step()
            sched.step()

    whole = _build(dt)
    ow = _opt(whole)
    steps(whole, ow, get_linear_schedule_with_warmup(ow, 2, 6), range(4))
    first = _build(dt)
    of = _opt(first)
    sf = get_linear_schedule_with_warmup(of, 2, 6)
    steps(first, of, sf, range(2))
    msd = {k: v.detach().cpu().clone() for k, v in first.state_dict().items()}
    osd = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in of.state_dict().items()}
    assert osd["step"] == 2 and osd["ema"].numel() == first.arena.total and len(osd["param_groups"]) == len(of.param_groups)
    second = clip.build_model(msd, dt).cuda()
    os_ = _opt(second)
    os_.load_state_dict(osd)
    for g, b in zip(os_.param_groups, sf.base_lrs):      # the loaded groups hold step 2's scheduled rates: a schedule starts from the base rates
        g["lr"] = b
    ss = get_linear_schedule_with_warmup(os_, 2, 6)
    ss.step()
    ss.step()
    assert [g["lr"] for g in os_.param_groups] == [g["lr"] for g in of.param_groups]
    steps(second, os_, ss, range(2, 4))
    a, b = _state(whole, ow), _state(second, os_)
    for k in a:
        assert _same(a[k], b[k]), f"{k} after a resume differs from the uninterrupted run"
    assert os_.step_count == 4 and int(os_.skipped_steps) == 0


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_skipped_step_counts_and_changes_nothing(dt):
    model = _build(dt)
    lay = _layout(model.arena)
    opt = _opt(model, skip_nonfinite=True)
    _install(model, lay, 0)
    opt.step()
    before = {k: v.clone() for k, v in _state(model, opt).items()}
    _install(model, lay, 1)
    model.arena.g["ln_final.weight"][3] = float("inf")
    opt.step()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 2
    for k, v in _state(model, opt).items():
        assert _same(v, before[k]), f"a skipped step wrote {k}"
    assert _same(model.arena.bflat, model.arena.flat.to(dt))
    _install(model, lay, 1)
    opt.step()
    assert int(opt.skipped_steps) == 1 and not _same(model.arena.flat, before["flat"])


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_ema_weights_context_and_state_dict(dt):
    """B5"""
    import clip
    from clip.weights import MODELS, synthetic_images
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    opt = _opt(model)
    for t in range(2):
        _install(model, lay, t)
        opt.step()
    model.eval()
    img = synthetic_images(3, MODELS["test-tiny"], 4).cuda()
    with torch.no_grad():
        own = model.encode_image(img).clone()
    ar.refresh_transposed()
    old = [t.clone() for t in (ar.flat, ar.bflat, ar.tflat)]
    esd = opt.ema_state_dict()
    assert set(esd) == set(model.state_dict()) and not torch.equal(esd["visual.proj"], model.state_dict()["visual.proj"])
    fresh = clip.build_model({k: v.cpu() for k, v in esd.items()}, dt).cuda().eval()
    with torch.no_grad():
        want = fresh.encode_image(img)

    def restored():
        ar.refresh_transposed()
        return all(_same(a, b) for a, b in zip(old, (ar.flat, ar.bflat, ar.tflat)))

    with opt.ema_weights():
        with torch.no_grad():
            got = model.encode_image(img)
        assert _same(ar.flat, opt._ema) and _same(ar.bflat, ar.flat.to(dt))
        for n, tv in ar.t.items():
            assert _same(tv.contiguous(), ar.b[n].t().contiguous())
    assert _same(got, want), "inside ema_weights() the model is not the model of ema_state_dict()"
    assert not _same(got, own)
    assert restored(), "ema_weights() did not restore the arena"
    with pytest.raises(RuntimeError, match="boom"):
        with opt.ema_weights():
            raise RuntimeError("boom")
    assert restored(), "ema_weights() did not restore the arena after an exception"
    with torch.no_grad():
        assert _same(model.encode_image(img), own)


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_interpolate_weights(dt):
    """B6"""
    from clip.optim import interpolate_weights
    model, other = _build(dt), _build(dt, seed=4)
    ar = model.arena
    osd = {k: v.detach().cpu() for k, v in other.state_dict().items()}
    ar.refresh_transposed()
    start = ar.flat.clone()
    interpolate_weights(model, osd, 0.0)
    assert _same(ar.flat, start), "alpha = 0 is the identity"
    interpolate_weights(model, osd, 0.5)
    assert _same(ar.flat, torch.lerp(start, other.arena.flat, 0.5)) and not _same(ar.flat, start)
    assert _same(ar.bflat, ar.flat.to(dt)), "the shadows are not fresh"
    gen = ar.shadow_gen
    ar.refresh_shadows()
    ar.refresh_transposed()
    assert ar.shadow_gen == gen
    for n, tv in ar.t.items():
        assert _same(tv.contiguous(), ar.b[n].t().contiguous())
    interpolate_weights(model, osd, 1.0)
    assert _same(ar.flat, other.arena.flat), "alpha = 1 gives other"
    bad = dict(osd, text_projection=osd["text_projection"][:, :-1])
    with pytest.raises(ValueError, match="text_projection"):
        interpolate_weights(model, bad, 0.5)
    with pytest.raises(ValueError, match="logit_scale"):
        interpolate_weights(model, {k: v for k, v in osd.items() if k != "logit_scale"}, 0.5)
    assert _same(ar.flat, other.arena.flat), "a refused call changed the masters"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_without_new_keywords_the_step_is_adamw_step(dt, monkeypatch):
    """B7"""
    from clip import optim as coptim
    from cclip_hip import ops
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    opt = coptim.AdamW(model, **HYP, weight_decay=0.01)
    assert not opt.grouped and opt.last_grad_norm is None and opt.skipped_steps is None
    real_step = ops.adamw_step
    calls = _count(monkeypatch)
    p, m, v, sh = ar.flat.clone(), torch.zeros_like(ar.flat), torch.zeros_like(ar.flat), ar.bflat.clone()
    for t in range(2):
        _install(model, lay, t)
        opt.step(grad_scale=0.5)
        real_step(p, lay.grads[t].cuda(), m, v, lr=HYP["lr"], eps=HYP["eps"], weight_decay=0.01, step=t + 1, grad_scale=0.5, bf16_shadow=sh)
        assert calls["plain"] == [ar.total] * (t + 1) and not calls["groups"]
    for a, b in ((p, ar.flat), (m, opt._m), (v, opt._v), (sh, ar.bflat)):
        assert _same(a, b)
    assert opt._ema is None and set(opt.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "param_groups"}
