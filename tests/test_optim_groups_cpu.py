"""CPU: the float64 reference of the grouped AdamW step (tests/optim_groups_ref.py) and the host side of clip.optim's parameter
groups.

  R1  the reference in double (f32_hyper=False, mode 1) against torch.optim.AdamW with real param groups + clip_grad_norm_ + a
      plain EMA loop;
  R2  every planted fault of the reference exceeds the carried bound, the reference itself does not;
  G1  the group builders on the (name, shape) lists of the test-tiny CLIP and caption models;
  G2  the group validation errors;  G3  the schedule over several groups;  G4  a state dict in the earlier format loads."""
import pytest
import torch

import kernel_refs_f64 as KR
import optim_groups_ref as OR


def _case(seed=5, n=64 * 6, n_groups=3, T=4):
    g = KR.gen(seed)
    p0 = torch.randn(n, generator=g).double()
    grads = [torch.randn(n, generator=g).double() * 10.0 ** (-2 + t) for t in range(T)]       # norms below and above max_norm
    group_of = (torch.arange(n) // 64) % n_groups
    lrs = [[1e-3 * (t + 1) * 0.5 ** k for k in range(n_groups)] for t in range(T)]
    wds = [0.1, 0.0, 0.02][:n_groups]
    return p0, grads, group_of, lrs, wds


def test_reference_in_double_equals_torch_adamw_with_groups_clip_and_ema():
    """R1"""
    p0, grads, group_of, lrs, wds = _case()
    T, max_norm, d = len(grads), 1.0, 0.9
    params = [torch.nn.Parameter(p0[group_of == k].clone()) for k in range(len(wds))]
    opt = torch.optim.AdamW([dict(params=[q], lr=lrs[0][k], weight_decay=wds[k]) for k, q in enumerate(params)], betas=(0.9, 0.999), eps=1e-6)
    ema = [q.detach().clone() for q in params]
    clipped = 0
    for t in range(T):
        for k, q in enumerate(params):
            q.grad = grads[t][group_of == k].clone()
            opt.param_groups[k]["lr"] = lrs[t][k]
        clipped += float(torch.nn.utils.clip_grad_norm_(params, max_norm)) > max_norm
        opt.step()
        for e, q in zip(ema, params):
            e.mul_(d).add_(q.detach(), alpha=1 - d)
    assert 0 < clipped < T, "the case must have clipped and unclipped steps"
    ref, _ = OR.trajectory(p0, grads, group_of, lrs, wds, steps=tuple(range(1, T + 1)), max_norm=max_norm, ema_decays=[d] * T,
                           mode=1, f32_hyper=False)
    for k, q in enumerate(params):
        sel = group_of == k
        assert torch.allclose(ref["p"][sel], q.detach(), rtol=1e-12, atol=1e-14), k
        assert torch.allclose(ref["m"][sel], opt.state[q]["exp_avg"], rtol=1e-12, atol=1e-16), k
        assert torch.allclose(ref["v"][sel], opt.state[q]["exp_avg_sq"], rtol=1e-12, atol=1e-18), k
        assert torch.allclose(ref["ema"][sel], ema[k], rtol=1e-12, atol=1e-14), k


@pytest.mark.parametrize("mode", [0, 1])
def test_every_planted_fault_exceeds_the_bound(mode):
    """R2.  The bound is the one the GPU tests use, widened for a sum of squares over the whole range."""
    p0, grads, group_of, lrs, wds = _case()
    T = len(grads)
    kw = dict(steps=tuple(range(1, T + 1)), max_norm=1.0, ema_decays=[0.9] * T, mode=mode, sumsq_rel=OR.sumsq_rel(p0.numel()))
    ref, bnd = OR.trajectory(p0, grads, group_of, lrs, wds, **kw)
    assert all(bool((bnd[k] > 0).all()) and bool((bnd[k] < 1e-4 * (ref[k].abs() + 1e-3)).all()) for k in ref), "a bound of no use"
    seen = {"table_shift": "p", "decay_no_decay": "p", "ema_p_old": "ema", "coef_after_moments": "m"}
    assert set(seen) == set(OR.FAULTS)
    for fault, where in seen.items():
        wrong, _ = OR.trajectory(p0, grads, group_of, lrs, wds, fault=fault, **kw)
        assert KR.rejects(ref[where], wrong[where], bnd[where]), f"the bound cannot see the planted fault {fault} in {where}"
    for k in ref:
        assert not KR.rejects(ref[k], ref[k], bnd[k])


def test_sumsq_reference_and_bound():
    x = torch.randn(1000, generator=KR.gen(1))
    ref, b = OR.sumsq(x, out0=2.0, chain=4, butterfly=9, partials=2)
    assert abs(float(ref) - (2.0 + float((x.double() ** 2).sum()))) < 1e-9 and float(b) == 15 * KR.E32 * float(ref)
    # one trip of one block; the cap; a second trip past the cap
    assert OR.sumsq_rel(4) == (4 + 9 + 1) * KR.E32
    assert OR.sumsq_rel(1024 * 1024) == (4 + 9 + 1024) * KR.E32
    assert OR.sumsq_rel(1024 * 1024 + 4) == (8 + 9 + 1024) * KR.E32


# ---- G1: the group builders ----
def _clip_named():
    from clip.weights import MODELS, init_state_dict
    return [(k, tuple(v.shape)) for k, v in init_state_dict(MODELS["test-tiny"], 3).items()]


def _caption_named():
    from clip_caption.weights import GPT2_MODELS, init_caption_state_dict, init_transformer_mapper_state_dict
    geo = GPT2_MODELS["test-tiny"]
    mlp = [(k, tuple(v.shape)) for k, v in init_caption_state_dict(geo, 3).items()]
    tr = [(k, tuple(v.shape)) for k, v in init_transformer_mapper_state_dict(geo, 4, 2).items()]      # the mapper alone
    assert all(k.startswith("clip_project.") for k, _ in tr)
    return mlp, tr + [(k, s) for k, s in mlp if not k.startswith("clip_project.")]


@pytest.mark.parametrize("which", ["clip", "caption-mlp", "caption-transformer"])
def test_group_builders_partition_the_parameters(which):
    from clip import optim as coptim
    named = _clip_named() if which == "clip" else _caption_named()[0 if which == "caption-mlp" else 1]
    names = [n for n, _ in named]
    for groups in (coptim.no_decay_groups(named, 0.1), coptim.layer_decay_groups(named, 0.75, 0.1), coptim.layer_decay_groups(named, 0.75)):
        listed = [n for g in groups for n in g["params"]]
        assert sorted(listed) == sorted(names), "every parameter in exactly one group"
        assert all(g["params"] for g in groups) and len(groups) <= 255
    decay, rest = coptim.no_decay_groups(named, 0.1)
    assert decay["weight_decay"] == 0.1 and rest["weight_decay"] == 0.0
    shape = dict(named)
    for n in rest["params"]:
        assert len(shape[n]) < 2 or any(m in n for m in coptim.NO_DECAY_MARKS), n
    for n in decay["params"]:
        assert len(shape[n]) >= 2 and "bias" not in n and "ln_" not in n, n
    if which == "clip":
        for n in ("logit_scale", "positional_embedding", "visual.positional_embedding", "visual.class_embedding", "visual.ln_pre.weight",
                  "ln_final.bias", "transformer.resblocks.1.ln_2.weight", "visual.transformer.resblocks.0.attn.in_proj_bias"):
            assert n in rest["params"], n
        for n in ("visual.conv1.weight", "visual.proj", "text_projection", "token_embedding.weight",
                  "transformer.resblocks.0.attn.in_proj_weight", "visual.transformer.resblocks.1.mlp.c_proj.weight"):
            assert n in decay["params"], n
    else:
        for n in ("model.transformer.ln_f.weight", "model.transformer.h.0.ln_1.bias", "model.transformer.h.1.attn.c_attn.bias"):
            assert n in rest["params"], n
        for n in ("model.transformer.wte.weight", "model.lm_head.weight", "model.transformer.h.0.mlp.c_fc.weight"):
            assert n in decay["params"], n


@pytest.mark.parametrize("which", ["clip", "caption-mlp", "caption-transformer"])
def test_layer_ids_are_monotone_per_tower_and_scale_the_lr(which):
    from clip import optim as coptim
    named = _clip_named() if which == "clip" else _caption_named()[0 if which == "caption-mlp" else 1]
    ids = coptim.layer_ids(named)
    towers = {}
    for n, _ in named:                                   # model order
        tower, lid, L = ids[n]
        if tower is None:
            assert n.startswith("clip_project.") and lid == L + 1 == 0
            continue
        towers.setdefault(tower, []).append(lid)
        assert L == 2 and 0 <= lid <= L + 1
    assert set(towers) == ({"visual.transformer.", "transformer."} if which == "clip" else {"model.transformer."})
    for tower, seq in towers.items():
        assert seq == sorted(seq) and set(seq) == {0, 1, 2, 3}, (tower, seq)
    if which == "clip":
        want = {"visual.conv1.weight": 0, "visual.class_embedding": 0, "visual.positional_embedding": 0, "visual.ln_pre.bias": 0,
                "token_embedding.weight": 0, "positional_embedding": 0, "visual.transformer.resblocks.0.ln_1.weight": 1,
                "transformer.resblocks.1.mlp.c_fc.bias": 2, "visual.ln_post.weight": 3, "visual.proj": 3, "ln_final.weight": 3,
                "text_projection": 3, "logit_scale": 3}
    else:
        want = {"model.transformer.wte.weight": 0, "model.transformer.wpe.weight": 0, "model.transformer.h.1.ln_2.bias": 2,
                "model.transformer.ln_f.bias": 3, "model.lm_head.weight": 3}
    for n, lid in want.items():
        assert ids[n][1] == lid, n
    scale = {n: g["lr_scale"] for g in coptim.layer_decay_groups(named, 0.5, 0.1) for n in g["params"]}
    for n, (tower, lid, L) in ids.items():
        assert scale[n] == 0.5 ** (L + 1 - lid), n
    wd = {n: g["weight_decay"] for g in coptim.layer_decay_groups(named, 0.5, 0.1) for n in g["params"]}
    shape = dict(named)
    assert all(wd[n] == (0.0 if coptim.is_no_decay(n, shape[n]) else 0.1) for n in wd)


# ---- G2-G4: the host side of the optimiser (no arena is touched before the first step) ----
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(4, 4)
        self.ln_1 = torch.nn.LayerNorm(4)
        self.scale = torch.nn.Parameter(torch.ones(()))


def test_param_group_validation_and_order():
    from clip.optim import AdamW
    toy = _Toy()
    opt = AdamW(toy, lr=1e-3, weight_decay=0.1, param_groups=[dict(params=["a.bias", toy.ln_1.weight], weight_decay=0.0, lr_scale=0.5),
                                                             dict(params=["scale"], lr=1e-2)])
    assert [g["names"] for g in opt.param_groups] == [["a.weight", "ln_1.bias"], ["a.bias", "ln_1.weight"], ["scale"]], "default first"
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 0.5e-3, 1e-2] and [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0, 0.1]
    assert opt.param_groups[1]["params"][1] is toy.ln_1.weight
    assert len(AdamW(toy, max_grad_norm=1.0).param_groups) == 1 and AdamW(toy, max_grad_norm=1.0).grouped and not AdamW(toy).grouped
    with pytest.raises(ValueError, match="does not have"):
        AdamW(toy, param_groups=[dict(params=["nope"])])
    with pytest.raises(ValueError, match="does not have"):
        AdamW(toy, param_groups=[dict(params=[torch.nn.Parameter(torch.ones(2))])])
    with pytest.raises(ValueError, match="a.bias is in"):
        AdamW(toy, param_groups=[dict(params=["a.bias"]), dict(params=[toy.a.bias])])
    with pytest.raises(ValueError, match="256"):
        AdamW(toy, param_groups=[dict(params=[])] * 256)
    AdamW(toy, param_groups=[dict(params=[])] * 255)
    with pytest.raises(ValueError, match="may hold"):
        AdamW(toy, param_groups=[dict(params=["scale"], betas=(0.5, 0.5))])
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=float("inf")), dict(ema_decay=1.5), dict(ema_warmup=True)):
        with pytest.raises(ValueError):
            AdamW(toy, **bad)


def test_schedule_scales_every_groups_own_base_lr():
    from clip.optim import AdamW, get_linear_schedule_with_warmup
    from oracle.optim_oracle import linear_schedule
    toy = _Toy()
    opt = AdamW(toy, lr=1e-3, param_groups=[dict(params=["a.bias"], lr_scale=0.5), dict(params=["scale"], lr=1e-2)])
    sched = get_linear_schedule_with_warmup(opt, 2, 6)
    base = [1e-3, 0.5e-3, 1e-2]
    for s in range(7):
        f = linear_schedule(s, 2, 6)
        assert [g["lr"] for g in opt.param_groups] == [b * f for b in base] == sched.get_last_lr(), s
        sched.step()
    one = AdamW(toy, lr=1e-3)
    s1 = get_linear_schedule_with_warmup(one, 2, 6)
    s1.step()
    assert one.param_groups[0]["lr"] == 1e-3 * linear_schedule(1, 2, 6) == s1.get_last_lr()[0] and s1.base_lr == 1e-3


def test_state_dict_of_the_earlier_format_loads():
    from clip.optim import AdamW
    toy = _Toy()
    old = dict(step=7, exp_avg=torch.arange(8.0), exp_avg_sq=torch.arange(8.0) * 2,
               param_groups=[dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True)])
    for opt in (AdamW(toy), AdamW(toy, param_groups=[dict(params=["scale"], lr=1e-2)], ema_decay=0.99, skip_nonfinite=True)):
        opt.load_state_dict(old)
        assert opt.step_count == 7 and torch.equal(opt._m, old["exp_avg"]) and torch.equal(opt._v, old["exp_avg_sq"])
        assert opt.param_groups[0]["lr"] == 5e-4 and opt._ema is None
    assert opt.param_groups[1]["lr"] == 1e-2 and opt._skipped == 0
    # the plain optimiser's own state dict keeps the earlier layout
    assert set(AdamW(toy).state_dict()) == {"step", "exp_avg", "exp_avg_sq", "param_groups"}
    # a grouped state goes into its like only
    sd = opt.state_dict()
    assert sd["param_groups"][1]["names"] == ["scale"] and sd["hyper"]["ema_decay"] == 0.99 and "params" not in sd["param_groups"][0]
    sd["exp_avg"], sd["exp_avg_sq"] = old["exp_avg"], old["exp_avg_sq"]
    with pytest.raises(ValueError, match="without any"):
        AdamW(toy).load_state_dict(sd)
    with pytest.raises(ValueError, match="do not hold"):
        AdamW(toy, param_groups=[dict(params=["a.bias"])]).load_state_dict(sd)
    AdamW(toy, param_groups=[dict(params=["scale"])]).load_state_dict(sd)
