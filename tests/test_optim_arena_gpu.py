"""clip.optim.AdamW over a whole ParamArena (test-tiny geometry, both operand dtypes), per element against the float64 trajectory
reference of tests/kernel_refs_f64.py (`adamw` with a gradient, a learning rate and a skip mask per step; pinned on the CPU against
the restated transformers.AdamW by tests/test_kernel_refs_f64_cpu.py).  No forward pass: the gradients are synthetic, one magnitude
per parameter spread over 1e-6 .. 1e2 (eps-dominated and v-dominated updates both occur), and reach the optimiser the three ways
the code base delivers them - in the arena slot (publish_grads), as a foreign tensor (autograd, logit_scale), or not at all (None).

  A1 trajectory:  4 steps under the linear warm-up schedule (the first at lr = 0), three configurations; p / m / v per element within
                  the carried fp64 bound, padding exactly zero, shadows == rounded masters bit for bit, no second cast, transposed
                  shadows == shadows^T; exactly one adamw_step launch per step; a foreign gradient that was not adopted is rejected.
  A2 None:        a parameter without a gradient is left alone (p, m, v, shadow bits), with weight decay, in both modes.
  A3 pending=:    range by range == one pass, bit for bit; every work object waited on once per step; bad ranges raise.
  A4 resume:      state_dict round trip == the uninterrupted run, bit for bit; a wrong-sized optimiser state raises.
The tolerance is the reference's own bound throughout; every other comparison is bit for bit."""
import pytest
import torch

import kernel_refs_f64 as KR

pytestmark = pytest.mark.gpu

DTS = [torch.bfloat16, torch.float16]
HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6)
CONFIGS = [dict(weight_decay=0.0, correct_bias=True),                                   # the reference's
           dict(weight_decay=0.01, correct_bias=False, grad_scale=0.25),
           dict(weight_decay=0.01, torch_semantics=True)]
SEED = 3
N_STEPS = 4
FOREIGN = ("logit_scale", "visual.proj", "transformer.resblocks.1.attn.in_proj_bias", "visual.transformer.resblocks.0.mlp.c_fc.weight")
NAN = float("nan")


def _dtn(dt):
    return str(dt).replace("torch.", "")


def _build(dt, seed=SEED):
    import clip
    from clip.weights import MODELS, init_state_dict
    return clip.build_model(init_state_dict(MODELS["test-tiny"], seed), dt).cuda()


def _opt(model, cfg):
    from clip import optim as coptim
    kw = {k: v for k, v in cfg.items() if k != "grad_scale"}
    return coptim.AdamW(model, **HYP, **kw)


def _ref_kw(cfg):
    return dict(beta1=HYP["betas"][0], beta2=HYP["betas"][1], eps=HYP["eps"], weight_decay=cfg["weight_decay"],
                correct_bias=cfg.get("correct_bias", True), grad_scale=cfg.get("grad_scale", 1.0), mode=1 if cfg.get("torch_semantics") else 0)


class Layout:
    """the arena's geometry on the host: offsets, sizes, the padding mask, and the synthetic gradients of every step"""

    def __init__(self, arena):
        self.names = list(arena.names)
        self.off = dict(arena.offsets)
        self.numel = {n: arena.params[n].numel() for n in self.names}
        self.total = arena.total
        self.pad = torch.ones(self.total, dtype=torch.bool)
        for n in self.names:
            self.pad[self.off[n]:self.off[n] + self.numel[n]] = False
        g = KR.gen(77)
        order = torch.randperm(len(self.names), generator=g)
        mag = torch.zeros(self.total)
        for i, n in enumerate(self.names):
            mag[self.off[n]:self.off[n] + self.numel[n]] = 10.0 ** (-6.0 + 8.0 * order[i].item() / (len(self.names) - 1))
        self.grads = []
        for _ in range(N_STEPS):
            gr = torch.randn(self.total, generator=g) * mag
            for n in self.names:
                gr[self.off[n]:self.off[n] + min(4, self.numel[n] - 1)] = 0.0       # g = 0 from the start: m = v = 0 (not the whole of a scalar)
            self.grads.append(gr)

    def sl(self, n):
        return slice(self.off[n], self.off[n] + self.numel[n])

    def slot(self, n):
        return slice(self.off[n], self.off[n] + (self.numel[n] + 63) // 64 * 64)

    def skip_mask(self, none_names):
        if not none_names:
            return None
        m = torch.zeros(self.total, dtype=torch.bool)
        for n in none_names:
            m[self.slot(n)] = True
        return m


LAYOUT = {}


def _layout(arena):
    if "l" not in LAYOUT:
        LAYOUT["l"] = Layout(arena)
    lay = LAYOUT["l"]
    assert lay.total == arena.total and lay.off == dict(arena.offsets)
    return lay


def _install(model, lay, t, none=()):
    """step t's gradients: the arena slot (as publish_grads leaves it), a foreign tensor (as autograd leaves it) with NaN in the slot
    it has to be adopted into, or None with NaN left in the slot (a skipped slot may not be read)"""
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


def _within(what, got, ref, bound, lay):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite elements"
    err = (got - ref).abs()
    bad = ~(err <= bound + 1e-300)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        name = next((n for n in lay.names if lay.off[n] <= i < lay.off[n] + lay.numel[n]), "padding")
        pytest.fail(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound; first flat index {i} ({name}): got {got[i].item():.9g} "
                    f"ref {ref[i].item():.9g} bound {bound[i].item():.3g}; worst err/bound {(err / (bound + 1e-300)).max().item():.3g}")
    return (err / (bound + 1e-300)).max().item()


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_copies(model, opt, lay, what):
    """everything A1 asks of the buffers besides the fp64 comparison"""
    ar = model.arena
    pad = lay.pad.cuda()
    for nm, buf in (("flat", ar.flat), ("gflat", ar.gflat), ("_m", opt._m), ("_v", opt._v), ("bflat", ar.bflat)):
        assert bool((buf[pad] == 0).all()), f"{what}: padding of {nm} is not zero"
    assert _same_bits(ar.bflat, ar.flat.to(ar.shadow_dtype)), f"{what}: a shadow is not the rounded master"
    gen = ar.shadow_gen
    ar.refresh_shadows()
    assert ar.shadow_gen == gen, f"{what}: the step did not mark the shadows fresh (a second cast ran)"
    ar.refresh_transposed()
    assert ar.t, "no transposed shadows are registered"
    for n, tv in ar.t.items():
        assert _same_bits(tv.contiguous(), ar.b[n].t().contiguous()), f"{what}: transposed shadow of {n}"


def _count_launches(monkeypatch):
    from clip import optim as coptim
    calls = []
    real = coptim.ops.adamw_step

    def counting(param, *a, **k):
        calls.append(param.numel())
        return real(param, *a, **k)

    monkeypatch.setattr(coptim.ops, "adamw_step", counting)
    return calls


REFS = {}


def _trajectory_ref(ci, lay, p0, lrs, n_steps, skips=None, key=None):
    """the fp64 reference of configuration ci after n_steps, computed once and shared by both dtypes"""
    k = (ci, n_steps, key)
    if k not in REFS:
        z = torch.zeros(lay.total, dtype=torch.float64)
        REFS[k] = KR.adamw(p0, lay.grads[:n_steps], z, z, lr=list(lrs[:n_steps]), steps=tuple(range(1, n_steps + 1)),
                           skip=None if skips is None else skips[:n_steps], **_ref_kw(CONFIGS[ci]))
    return REFS[k]


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_adamw_trajectory_over_the_arena_f64(ci, dt, monkeypatch):
    """A1.  Four steps under get_linear_schedule_with_warmup(opt, 2, 6): learning rates 0, lr/2, lr, 3lr/4."""
    from clip.optim import get_linear_schedule_with_warmup
    from oracle.optim_oracle import linear_schedule
    cfg = CONFIGS[ci]
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    p0 = ar.flat.detach().cpu().double()
    p0_dev = ar.flat.clone()
    assert bool((p0[lay.pad] == 0).all())
    opt = _opt(model, cfg)
    sched = get_linear_schedule_with_warmup(opt, 2, 6)
    lrs = [HYP["lr"] * linear_schedule(s, 2, 6) for s in range(N_STEPS)]
    assert lrs[0] == 0.0 and lrs[1] > 0.0
    calls = _count_launches(monkeypatch)
    for t in range(N_STEPS):
        opt.zero_grad()
        _install(model, lay, t)
        assert opt.param_groups[0]["lr"] == lrs[t], "the schedule's learning rate"
        opt.step(grad_scale=cfg.get("grad_scale", 1.0))
        sched.step()
        assert calls == [ar.total] * (t + 1), "with every gradient present the step is ONE launch over the flat arena"
        assert all(p.grad is not None and p.grad.data_ptr() == ar.g[n].data_ptr() for n, p in ar.params.items()), "foreign gradients are adopted"
        if t in (0, N_STEPS - 1):
            what = f"cfg{ci} {_dtn(dt)} after step {t + 1}"
            ref, bnd = _trajectory_ref(ci, lay, p0, lrs, t + 1)
            worst = {nm: _within(f"{what} {nm}", got, ref[nm], bnd[nm], lay) for nm, got in (("p", ar.flat), ("m", opt._m), ("v", opt._v))}
            print(f"{what}: worst err/bound p {worst['p']:.3g} m {worst['m']:.3g} v {worst['v']:.3g}")
            _check_copies(model, opt, lay, what)
        if t == 0:
            assert _same_bits(ar.flat, p0_dev), "lr = 0: a parameter moved"
            live = ~lay.pad.cuda() & (ar.gflat != 0)
            assert bool((opt._m[live] != 0).all()) and bool((opt._v[live] != 0).all()), "lr = 0: the moments must still move"
    # the comparison can see something: the reference without one parameter's foreign gradient is rejected for that parameter
    ref, bnd = _trajectory_ref(ci, lay, p0, lrs, N_STEPS)
    for n in FOREIGN:
        s = lay.sl(n)
        z = torch.zeros(lay.numel[n], dtype=torch.float64)
        wrong, _ = KR.adamw(p0[s], [torch.zeros(lay.numel[n])] * N_STEPS, z, z, lr=lrs, steps=(1, 2, 3, 4), **_ref_kw(cfg))
        for nm, got in (("p", ar.flat), ("m", opt._m), ("v", opt._v)):
            assert KR.rejects(got[s].cpu(), wrong[nm], bnd[nm][s]), f"the bound cannot see a foreign gradient of {n} that was not adopted ({nm})"
            assert not KR.rejects(got[s].cpu(), ref[nm][s], bnd[nm][s])


# A2: which parameters have no gradient at which step (1-based).  NEVER: at no step (a frozen parameter); ONCE: gradients at
# steps 1-2, None at 3, a gradient again at 4; TAIL: gradients at steps 1-2, None at 3 and 4.
def _none_plan(lay):
    never = {lay.names[0], "transformer.resblocks.0.ln_1.weight", "visual.transformer.resblocks.1.mlp.c_proj.weight"}
    once = {"logit_scale", "visual.transformer.resblocks.1.attn.out_proj.weight", "transformer.resblocks.1.attn.in_proj_bias"}
    tail = {lay.names[-1], "token_embedding.weight", "ln_final.weight", "ln_final.bias"}
    assert not (never & once) and not (never & tail) and not (once & tail) and all(n in lay.off for n in never | once | tail)
    plan = [set(never), set(never), never | once | tail, never | tail]
    return never, once, tail, plan


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("ci", [1, 2])
def test_adamw_leaves_a_parameter_without_gradient_alone(ci, dt, monkeypatch):
    """A2.  weight_decay = 0.01 in both modes, constant lr: a parameter whose .grad is None at a step keeps its p, m, v and shadow
    bits at that step (its gradient slot holds NaN: it is not even read); every other element follows the reference with the skip
    mask; a parameter that gets a gradient again at step 4 follows the reference at the GLOBAL step number 4."""
    cfg = CONFIGS[ci]
    assert cfg["weight_decay"] > 0
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    never, once, tail, plan = _none_plan(lay)
    ar.refresh_shadows()                                     # as the forward pass of a real step does
    p0 = ar.flat.detach().cpu().double()
    opt = _opt(model, cfg)
    lrs = [HYP["lr"]] * N_STEPS
    skips = [lay.skip_mask(s) for s in plan]
    calls = _count_launches(monkeypatch)
    snap = lambda: [t.clone() for t in (ar.flat, opt._m, opt._v, ar.bflat)]          # noqa: E731
    for t in range(N_STEPS):
        opt.zero_grad()
        _install(model, lay, t, none=plan[t])
        before = snap() if t else [ar.flat.clone(), torch.zeros_like(ar.flat), torch.zeros_like(ar.flat), ar.bflat.clone()]
        del calls[:]
        opt.step(grad_scale=cfg.get("grad_scale", 1.0))
        after = snap()
        for n in plan[t]:
            s = lay.slot(n)
            for nm, b, a in zip(("p", "m", "v", "shadow"), before, after):
                assert _same_bits(a[s], b[s]), f"cfg{ci} {_dtn(dt)} step {t + 1}: {nm} of {n} changed although its .grad is None"
        live = ar.slot_ranges([n for n in lay.names if n not in plan[t]])
        assert calls == [e - s for s, e in live], "one launch per contiguous run of slots that have gradients"
        moved = [n for n in lay.names if n not in plan[t] and not _same_bits(after[0][lay.sl(n)], before[0][lay.sl(n)])]
        assert len(moved) == len(lay.names) - len(plan[t]), "every parameter with a gradient moves (decay alone moves it)"
    what = f"cfg{ci} {_dtn(dt)} with None gradients, after step {N_STEPS}"
    ref, bnd = _trajectory_ref(ci, lay, p0, lrs, N_STEPS, skips, key="none")
    for nm, got in (("p", ar.flat), ("m", opt._m), ("v", opt._v)):
        _within(f"{what} {nm}", got, ref[nm], bnd[nm], lay)
    _check_copies(model, opt, lay, what)
    for n in never:
        s = lay.slot(n)
        assert torch.equal(ar.flat[s].cpu().double(), p0[s]) and not bool(opt._m[s].any()) and not bool(opt._v[s].any()), n
    # the global step count: the reference that numbers ONCE's steps 1, 2, 3 (one count per parameter) is told apart
    if cfg.get("correct_bias", True):
        for n in once:
            s = lay.sl(n)
            z = torch.zeros(lay.numel[n], dtype=torch.float64)
            own, _ = KR.adamw(p0[s], [g[s] for g in lay.grads], z, z, lr=lrs, steps=(1, 2, 2, 3), skip=[None, None, torch.ones(lay.numel[n], dtype=torch.bool), None],
                              **_ref_kw(cfg))
            assert KR.rejects(ar.flat[s].cpu(), own["p"], bnd["p"][s]), f"{n}: a per-parameter step count would pass as well"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_adamw_partial_step_casts_stale_shadows_first(dt):
    """A step that skips parameters marks the shadows fresh afterwards, so it has to bring the skipped parameters' shadows up to date
    itself when they are stale: here they were never cast (no forward pass has run)."""
    model = _build(dt)
    ar = model.arena
    lay = _layout(ar)
    never, _, _, plan = _none_plan(lay)
    opt = _opt(model, CONFIGS[1])
    _install(model, lay, 0, none=plan[0])
    opt.step()
    assert _same_bits(ar.bflat, ar.flat.to(ar.shadow_dtype))
    assert all(bool(ar.b[n].any()) for n in never)


class _Work:
    def __init__(self):
        self.waits = 0

    def wait(self):
        self.waits += 1


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
def test_adamw_pending_ranges_equal_one_pass(dt):
    """A3.  The ranges of parallel.grad_buckets (at least 3), stand-in work objects: three steps range by range are bit-identical to
    three one-pass steps on a second model, every step (the second one with parameters that have no gradient); every work object is
    waited on once per step; ranges with a gap, or short of arena.total, raise and change nothing."""
    from clip import parallel
    cfg = CONFIGS[1]
    one, rng = _build(dt), _build(dt)
    lay = _layout(one.arena)
    _, _, tail, _ = _none_plan(lay)
    buckets = parallel.grad_buckets(rng.arena, 300_000)
    assert len(buckets) >= 3
    works = [_Work() for _ in buckets]
    pending = [(s, e, w) for (s, e), w in zip(buckets, works)]
    o1, o2 = _opt(one, cfg), _opt(rng, cfg)
    for t in range(3):
        none = tail if t == 1 else ()
        for model in (one, rng):
            _install(model, lay, t, none=none)
        o1.step(grad_scale=0.25)
        rng.arena.adopt_foreign_grads()              # what the reducer does before it reduces
        o2.step(grad_scale=0.25, pending=pending)
        assert [w.waits for w in works] == [t + 1] * len(works), "every work object is waited on once per step"
        for nm, a, b in (("flat", one.arena.flat, rng.arena.flat), ("_m", o1._m, o2._m), ("_v", o1._v, o2._v), ("bflat", one.arena.bflat, rng.arena.bflat)):
            assert _same_bits(a, b), f"step {t + 1}: {nm} differs between one pass and range by range"
        assert rng.arena.shadow_gen == one.arena.shadow_gen
    assert not _same_bits(one.arena.flat, _build(dt).arena.flat)
    ar = rng.arena
    state = [t.clone() for t in (ar.flat, o2._m, o2._v, ar.bflat)]
    count = o2.step_count
    gap = [pending[0]] + pending[2:]
    short = pending[:-1]
    late = pending[1:]                                # does not start at 0
    for bad in (gap, short, late):
        with pytest.raises((ValueError, AssertionError)):
            o2.step(pending=bad)
        assert o2.step_count == count
        assert all(_same_bits(a, b) for a, b in zip(state, (ar.flat, o2._m, o2._v, ar.bflat))), "a refused step changed the state"
    assert [w.waits for w in works] == [3] * len(works), "a refused step waited on a work object"


@pytest.mark.parametrize("dt", DTS, ids=_dtn)
@pytest.mark.parametrize("ci", [0, 2])
def test_adamw_resume_from_state_dicts_is_bit_identical(ci, dt):
    """A4.  Two steps, model.state_dict() and opt.state_dict() cloned to the host, a fresh model and optimiser loaded from them, steps 3-4:
    bit-identical to the uninterrupted four steps.  An optimiser state whose moment buffers do not have arena.total elements raises
    (at load_state_dict or at the next step) and the step does not run."""
    import clip
    from clip.optim import get_linear_schedule_with_warmup
    cfg = CONFIGS[ci]

    def steps(model, opt, sched, ts):
        lay = _layout(model.arena)
        for t in ts:
            opt.zero_grad()
            _install(model, lay, t)
            opt.step(grad_scale=cfg.get("grad_scale", 1.0))
            sched.step()

    whole = _build(dt)
    ow = _opt(whole, cfg)
    sw = get_linear_schedule_with_warmup(ow, 2, 6)
    steps(whole, ow, sw, range(4))

    first = _build(dt)
    of = _opt(first, cfg)
    sf = get_linear_schedule_with_warmup(of, 2, 6)
    steps(first, of, sf, range(2))
    msd = {k: v.detach().cpu().clone() for k, v in first.state_dict().items()}
    osd = of.state_dict()
    osd = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in osd.items()}
    assert osd["step"] == 2 and osd["exp_avg"].numel() == first.arena.total

    second = clip.build_model(msd, dt).cuda()
    os_ = _opt(second, cfg)
    os_.load_state_dict(osd)
    ss = get_linear_schedule_with_warmup(os_, 2, 6)
    ss.step()
    ss.step()
    assert os_.param_groups[0]["lr"] == of.param_groups[0]["lr"]
    steps(second, os_, ss, range(2, 4))
    for nm, a, b in (("flat", whole.arena.flat, second.arena.flat), ("_m", ow._m, os_._m), ("_v", ow._v, os_._v),
                     ("bflat", whole.arena.bflat, second.arena.bflat)):
        assert _same_bits(a, b), f"{nm} after a resume differs from the uninterrupted run"
    assert os_.step_count == 4

    # a state saved for another geometry
    ar = second.arena
    before = [t.clone() for t in (ar.flat, os_._m, os_._v, ar.bflat)]
    bad = dict(osd, exp_avg=torch.ones(ar.total + 64), exp_avg_sq=torch.ones(ar.total + 64))
    fresh = _opt(second, cfg)
    with pytest.raises((ValueError, RuntimeError)) as exc:
        fresh.load_state_dict(bad)
        _install(second, _layout(ar), 2)
        fresh.step()
    assert "arena" in str(exc.value) or "geometry" in str(exc.value), "the error should say what does not fit"
    assert _same_bits(ar.flat, before[0]) and _same_bits(ar.bflat, before[3]), "the refused step ran"
    assert fresh._m is None or fresh._m.numel() != ar.total or bool(fresh._m.any()), "the moments were quietly reset"
