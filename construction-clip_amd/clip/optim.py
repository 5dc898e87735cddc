"""Fused optimiser for models whose parameters live in a cclip_hip ParamArena.

`AdamW` reproduces `transformers.AdamW(lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
correct_bias=True)` - what the reference optimises with (/root/reference/CLIP/train.py:143,
/root/reference/CLIP_prefix_caption/train.py:336; the class no longer exists in transformers >= 5) -
as ONE launch over the flat arena that also rewrites the bf16 weight shadows.
`get_linear_schedule_with_warmup` restates the schedule of CLIP/train.py:145-147.
Any torch.optim optimiser also works on the model's parameters (they are ordinary nn.Parameters);
this one is simply ~400 launches cheaper per step.

What a fine-tuning run needs on top of that - parameter groups (`no_decay_groups`, `layer_decay_groups`), gradient-norm
clipping, skipping a step whose gradients overflowed, an EMA of the weights (`ema_state_dict`, `ema_weights`) - rides in the
same single launch (`ops.adamw_step_groups`) and is switched on by keywords; without them `step()` is the path above, bit for
bit.  `interpolate_weights` is WiSE-FT.
"""
from __future__ import annotations

import contextlib
import re

import torch

from cclip_hip import ops

_GROUP_KEYS = {"params", "lr", "weight_decay", "lr_scale"}
_FLT_MAX = 3.4028234e38


# ---- group builders: rules on (name, shape) lists, so that they can be checked without a device ---------------------------------
NO_DECAY_MARKS = ("bias", "ln_", ".ln", "logit_scale", "positional_embedding", "class_embedding")
_BLOCK = re.compile(r"^(.*?)(?:resblocks|\bh)\.(\d+)\.")       # CLIP's towers (`...transformer.resblocks.i.`), GPT-2 (`...transformer.h.i.`)
_FIRST = ("conv1", "class_embedding", "positional_embedding", "ln_pre", "token_embedding", "wte.", "wpe.")


def _named_shapes(model):
    """[(name, shape)] of a module's parameters; a list of such pairs passes through"""
    if isinstance(model, (list, tuple)):
        return [(n, tuple(s)) for n, s in model]
    return [(n, tuple(p.shape)) for n, p in model.named_parameters()]


def is_no_decay(name: str, shape) -> bool:
    """open_clip's exclusion rule: gains, biases, scalars (ndim < 2), and by name the LayerNorms, `logit_scale` and the learned
    positional / class embeddings"""
    return len(shape) < 2 or any(m in name for m in NO_DECAY_MARKS)


def no_decay_groups(model, weight_decay: float):
    """param_groups for AdamW: [the decayed parameters at `weight_decay`, the rest at 0]; every parameter is in exactly one"""
    named = _named_shapes(model)
    return [dict(params=[n for n, s in named if not is_no_decay(n, s)], weight_decay=float(weight_decay)),
            dict(params=[n for n, s in named if is_no_decay(n, s)], weight_decay=0.0)]


def layer_ids(model):
    """{name: (tower, layer_id, L)} for layer-wise learning-rate decay.  A tower is a stack of numbered blocks (the prefix before
    `resblocks.i.` / `h.i.`), L its block count: the embeddings, the patch conv and the pre-norm are layer 0, block i is layer
    i + 1, whatever follows the blocks (final norms, projections, lm_head, `logit_scale`) is layer L + 1.  A parameter outside
    every tower (the caption model's mapper `clip_project.*`, trained from scratch) has tower None and layer_id == L + 1 == 0."""
    named = _named_shapes(model)
    depth = {}
    for n, _ in named:
        m = _BLOCK.match(n)
        if m:
            depth[m.group(1)] = max(depth.get(m.group(1), 0), int(m.group(2)) + 1)
    out = {}
    for n, _ in named:
        m = _BLOCK.match(n)
        if m:
            out[n] = (m.group(1), int(m.group(2)) + 1, depth[m.group(1)])
            continue
        # the tower a parameter outside the blocks belongs to: the longest tower prefix whose parent module holds it
        # (`visual.transformer.` -> `visual.`, `model.transformer.` -> `model.`; CLIP's text tower `transformer.` -> the root)
        tower = None
        if not n.startswith("clip_project."):
            for t in sorted(depth, key=len, reverse=True):
                parent = t[:-len("transformer.")] if t.endswith("transformer.") else t
                if n.startswith(parent) and (parent or not n.startswith("visual.")):
                    tower = t
                    break
        if tower is None:
            out[n] = (None, 0, -1)
        else:
            L = depth[tower]
            out[n] = (tower, 0 if any(f in n for f in _FIRST) else L + 1, L)
    return out


def layer_decay_groups(model, decay: float, weight_decay: float = 0.0):
    """param_groups with lr_scale = decay ** (L + 1 - layer_id) per tower (`layer_ids`), combined with the no-decay split: one
    group per (lr_scale, weight decay) pair that occurs, deepest layers first."""
    named = _named_shapes(model)
    ids = layer_ids(named)
    groups = {}
    for n, s in named:
        _, lid, L = ids[n]
        key = (L + 1 - lid, 0.0 if is_no_decay(n, s) else float(weight_decay))
        groups.setdefault(key, []).append(n)
    return [dict(params=names, lr_scale=float(decay) ** k, weight_decay=wd) for (k, wd), names in sorted(groups.items())]


class AdamW:
    """A parameter whose `.grad` is None at a step is left alone at that step - its value, both moments and its 16-bit shadow
    keep their bits, whatever the weight decay - as `transformers.AdamW` (and torch's optimisers) skip it: a frozen GPT-2 under
    prefix-only training does not decay.  One difference stays: the bias correction uses ONE step count for the whole arena
    (the number of `step()` calls), not one per parameter as `transformers.AdamW` keeps; a parameter that sat out some steps is
    corrected as if it had not.
    With every gradient present the step is one launch over the flat arena; otherwise one launch per contiguous run of slots
    that have gradients (`ParamArena.slot_ranges`).

    Any of the keywords below switches `step()` to the grouped kernel (`ops.adamw_step_groups`, still one launch per run):
      param_groups   [dict(params=[names or Parameters], lr=, weight_decay=, lr_scale=)]: a group's learning rate is
                     (its `lr`, else the optimiser's) * `lr_scale`; a parameter is in exactly one group, the unlisted ones in a
                     default group that `optimizer.param_groups` lists FIRST (so `param_groups[0]["lr"]` keeps its meaning).
                     betas, eps and correct_bias are the optimiser's, for every group.
      max_grad_norm  torch.nn.utils.clip_grad_norm_ over the parameters that have a gradient, on the true gradients
                     (grad_scale * the arena's): the sum of squares is taken on the device over the live slot ranges
                     (`ops.sumsq`; the slots' padding is zeroed first, so it cannot contribute), the kernel forms the coefficient
                     from that device scalar.  `last_grad_norm` is a device tensor, nothing is read on the host in `step()`.
      skip_nonfinite a step whose gradient norm is inf or NaN writes nothing (the fp16 operand mode under its static loss scale);
                     `skipped_steps` (device int32) counts them.  The HOST step count advances on a skipped step too: the bias
                     correction of the next step is that of its own number, as if the skipped step had been taken with g = 0
                     and no decay.
      ema_decay      e = d e + (1 - d) p_new, written in the same pass; the buffer starts at the first step as a copy of the
                     masters.  ema_warmup: d = min(ema_decay, (1 + t) / (10 + t)) at step t.  A slot skipped at a step keeps
                     its EMA bits, as it keeps its moments.
    With `pending=` and a norm to take, every work object is waited on BEFORE the norm (the norm needs all reduced gradients), so
    the update no longer overlaps the reductions; without a norm the ranges are updated one by one as before."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 correct_bias: bool = True, torch_semantics: bool = False, *, param_groups=None, max_grad_norm=None,
                 skip_nonfinite: bool = False, ema_decay=None, ema_warmup: bool = False):
        self.model = model
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        self.mode = 1 if torch_semantics else 0
        self.step_count = 0
        self._m = self._v = None
        if max_grad_norm is not None and not 0.0 < float(max_grad_norm) <= _FLT_MAX:
            raise ValueError(f"AdamW: max_grad_norm must be finite and > 0, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"AdamW: ema_decay must lie in [0, 1], got {ema_decay}")
        if ema_warmup and ema_decay is None:
            raise ValueError("AdamW: ema_warmup without ema_decay")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.grouped = param_groups is not None or max_grad_norm is not None or self.skip_nonfinite or ema_decay is not None
        self._ema = self._table = self._sumsq = self._ws = self._pad_idx = None
        self._skipped = 0                     # until the device counter exists
        self.skipped_steps = None
        self._norm_scale = None
        if self.grouped:
            self.param_groups = self._make_groups(param_groups or [])
        else:
            self.param_groups = [dict(self.defaults, params=list(model.parameters()))]

    # ---- groups ----
    def _make_groups(self, user):
        named = list(self.model.named_parameters())
        by_id = {id(p): n for n, p in named}
        by_name = dict(named)
        if len(user) + 1 > 256:
            raise ValueError(f"AdamW: at most 256 parameter groups (the default group included), got {len(user) + 1}")
        owner, groups = {}, []
        for gi, g in enumerate(user):
            extra = set(g) - _GROUP_KEYS
            if "params" not in g or extra:
                raise ValueError(f"AdamW: param_groups[{gi}] needs `params` and may hold lr, weight_decay, lr_scale; got {sorted(g)}")
            names = []
            for q in g["params"]:
                n = q if isinstance(q, str) else by_id.get(id(q))
                if n is None or n not in by_name:
                    raise ValueError(f"AdamW: param_groups[{gi}] names a parameter the model does not have: {q if isinstance(q, str) else tuple(q.shape)}")
                if n in owner:
                    raise ValueError(f"AdamW: parameter {n} is in param_groups[{owner[n]}] and in param_groups[{gi}]")
                owner[n] = gi
                names.append(n)
            scale = float(g.get("lr_scale", 1.0))
            groups.append(dict(self.defaults, lr=float(g.get("lr", self.defaults["lr"])) * scale, lr_scale=scale,
                               weight_decay=float(g.get("weight_decay", self.defaults["weight_decay"])),
                               names=names, params=[by_name[n] for n in names]))
        rest = [n for n, _ in named if n not in owner]
        return [dict(self.defaults, lr_scale=1.0, names=rest, params=[by_name[n] for n in rest])] + groups

    def _state(self):
        """The arena, with the moment buffers on its device.  Moments of another size (a state saved for another geometry) are an
        error: re-zeroing them would restart the moments under a step count that says otherwise."""
        arena = self.model.arena
        if self._m is None:
            self._m = torch.zeros_like(arena.flat)
            self._v = torch.zeros_like(arena.flat)
        for name, t in (("exp_avg", self._m), ("exp_avg_sq", self._v)) + ((("ema", self._ema),) if self._ema is not None else ()):
            if t.numel() != arena.total or t.dtype != torch.float32:
                raise ValueError(f"AdamW: the optimiser state does not fit this model: {name} holds {t.numel()} {t.dtype} elements, "
                                 f"the parameter arena {arena.total} float32 (a state_dict saved for another geometry?)")
        if self._m.device != arena.flat.device or self._v.device != arena.flat.device:
            self._m, self._v = self._m.to(arena.flat.device), self._v.to(arena.flat.device)
        if self.grouped and self._table is None:
            self._build_tables(arena)
        if self._ema is not None and self._ema.device != arena.flat.device:
            self._ema = self._ema.to(arena.flat.device)
        return arena

    def _build_tables(self, arena):
        """one group byte per 64-element chunk of the arena (slots are 64-aligned: a chunk never straddles two parameters), the
        indices of the slots' padding, the norm's device scalar and scratch, the skipped-step counter"""
        dev = arena.flat.device
        table = torch.zeros(arena.total // 64, dtype=torch.uint8)
        pad = []
        for gi, g in enumerate(self.param_groups):
            for n in g["names"]:
                off, k = arena.offsets[n], arena.params[n].numel()
                end = off + (k + 63) // 64 * 64
                table[off // 64:end // 64] = gi
                pad.append(torch.arange(off + k, end))
        self._table = table.to(dev)
        self._pad_idx = torch.cat(pad).to(dev) if pad else torch.zeros(0, dtype=torch.int64, device=dev)
        self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        self._ws = torch.empty(max(1, ops.sumsq_workspace(arena.total) // 4), device=dev, dtype=torch.float32)
        self.skipped_steps = torch.full((1,), int(self._skipped), device=dev, dtype=torch.int32)

    @property
    def last_grad_norm(self):
        """the total norm of the last step's true gradients, before clipping (what clip_grad_norm_ returns): a device tensor [1],
        formed when asked for; None before the first step that took a norm"""
        return None if self._norm_scale is None else self._sumsq.sqrt() * self._norm_scale

    def step(self, grad_scale: float = 1.0, pending=None) -> None:
        """pending: [(start, end, work)] from parallel.allreduce_gradients_async - the arena is then updated range by range,
        each as soon as its all-reduce has finished (the ranges must cover the arena; same result as one pass)."""
        arena = self._state()
        if pending:
            if not (pending[0][0] == 0 and pending[-1][1] == arena.total and all(a[1] == b[0] for a, b in zip(pending, pending[1:]))):
                raise ValueError("AdamW.step: the pending ranges must cover the arena [0, %d) in order, without gaps: %s"
                                 % (arena.total, [(s, e) for s, e, _ in pending]))
        else:
            arena.adopt_foreign_grads()      # (with pending reductions the reducer adopted them before it reduced)
        g = self.param_groups[0]
        self.step_count += 1
        # Parameters without a gradient are skipped: only the slot ranges of the others are updated.
        # (With pending reductions every rank takes the same branch: p.grad is None depends on the model, not on the data.)
        names = [n for n, p in arena.params.items() if p.grad is not None]
        live = [(0, arena.total)] if len(names) == len(arena.params) else arena.slot_ranges(names)
        if len(names) != len(arena.params) or self.skip_nonfinite:
            arena.refresh_shadows()           # the skipped slots keep their shadows, and the step marks ALL shadows fresh: no-op unless stale
        if self.grouped:
            update = self._grouped_update(arena, grad_scale, live, pending)
            if self.max_grad_norm is not None or self.skip_nonfinite:
                pending = None                # every work object was waited on before the norm
        else:
            kw = dict(lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                      step=self.step_count, correct_bias=g["correct_bias"], grad_scale=grad_scale, mode=self.mode)

            def update(s, e):
                ops.adamw_step(arena.flat[s:e], arena.gflat[s:e], self._m[s:e], self._v[s:e], bf16_shadow=arena.bflat[s:e], **kw)

        if pending:
            for s, e, w in pending:
                w.wait()
                for ls, le in live:
                    if max(s, ls) < min(e, le):
                        update(max(s, ls), min(e, le))
        else:
            for s, e in live:
                update(s, e)
        arena.mark_shadows_fresh()            # the kernel rewrote masters and shadows together

    def _grouped_update(self, arena, grad_scale, live, pending):
        """the norm of this step (when one is asked for) and the per-range launch of the grouped kernel"""
        g = self.param_groups[0]
        sumsq_dev = max_norm = None
        if self.max_grad_norm is not None or self.skip_nonfinite:
            for _, _, w in pending or ():
                w.wait()
            if self._pad_idx.numel():
                arena.gflat.index_fill_(0, self._pad_idx, 0.0)
            if not live:
                self._sumsq.zero_()
            for i, (s, e) in enumerate(live):
                ops.sumsq(arena.gflat[s:e], out=self._sumsq, accumulate=i > 0, workspace=self._ws,
                          nonfinite_count=self.skipped_steps if self.skip_nonfinite and i == len(live) - 1 else None)
            sumsq_dev = self._sumsq
            max_norm = _FLT_MAX if self.max_grad_norm is None else self.max_grad_norm
            self._norm_scale = abs(float(grad_scale))
        d = 0.0
        if self.ema_decay is not None:
            if self._ema is None:
                self._ema = arena.flat.detach().clone()
            d = min(self.ema_decay, (1.0 + self.step_count) / (10.0 + self.step_count)) if self.ema_warmup else self.ema_decay
        kw = dict(lrs=[q["lr"] for q in self.param_groups], weight_decays=[q["weight_decay"] for q in self.param_groups],
                  beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], step=self.step_count, correct_bias=g["correct_bias"],
                  grad_scale=grad_scale, mode=self.mode, sumsq_dev=sumsq_dev, max_norm=max_norm,
                  skip_nonfinite=self.skip_nonfinite, ema_decay=d)

        def update(s, e):
            if s % 64:
                raise ValueError(f"AdamW.step: a range must start at a slot boundary (a multiple of 64 elements), got {s}")
            ops.adamw_step_groups(arena.flat[s:e], arena.gflat[s:e], self._m[s:e], self._v[s:e], self._table[s // 64:(e + 63) // 64],
                                  bf16_shadow=arena.bflat[s:e], ema=None if self._ema is None else self._ema[s:e], **kw)

        return update

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.model.parameters():
            p.grad = None

    # ---- averaged weights ----
    def ema_state_dict(self):
        """the averaged weights in the model's state_dict layout (whatever is not an arena parameter is copied from the model)"""
        if self._ema is None:
            raise RuntimeError("AdamW.ema_state_dict: no EMA yet (ema_decay is unset, or no step has run)")
        arena = self.model.arena
        out = {}
        for k, v in self.model.state_dict().items():
            if k in arena.offsets:
                off = arena.offsets[k]
                out[k] = self._ema[off:off + v.numel()].view(v.shape).clone()
            else:
                out[k] = v.detach().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the arena holds the averaged weights - masters, shadows and transposed shadows consistent - for evaluation;
        on exit, also when the body raises, the masters get their bits back and the shadows are cast from them again."""
        if self._ema is None:
            raise RuntimeError("AdamW.ema_weights: no EMA yet (ema_decay is unset, or no step has run)")
        arena = self._state()
        saved = arena.flat.detach().clone()
        with torch.no_grad():
            arena.flat.copy_(self._ema)
        _recast(arena)
        try:
            yield self.model
        finally:
            with torch.no_grad():
                arena.flat.copy_(saved)
            _recast(arena)

    # ---- state ----
    def state_dict(self):
        groups = [{k: (list(v) if k == "names" else v) for k, v in g.items() if k != "params"} for g in self.param_groups]
        sd = dict(step=self.step_count, exp_avg=self._m, exp_avg_sq=self._v, param_groups=groups)
        if self.grouped:
            sd.update(ema=self._ema, skipped_steps=self._skipped if self.skipped_steps is None else self.skipped_steps.clone(),
                      hyper=dict(max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite, ema_decay=self.ema_decay,
                                 ema_warmup=self.ema_warmup))
        return sd

    def load_state_dict(self, sd):
        """The moments are copied (onto the arena's device at the next step); a state whose moment buffers do not hold one
        element per arena element is refused there - see _state().  Groups are matched by parameter NAME: a state whose groups
        hold other parameters than this optimiser's is refused.  A state saved without groups (by an optimiser without the new
        keywords, or by an earlier version) loads into any optimiser: its one group's values go to the default group."""
        m, v = sd["exp_avg"], sd["exp_avg_sq"]
        if (m is None) != (v is None) or (m is not None and m.numel() != v.numel()):
            raise ValueError("AdamW.load_state_dict: exp_avg and exp_avg_sq do not match each other")
        saved = sd["param_groups"]
        plain = len(saved) == 1 and "names" not in saved[0]
        if not plain:
            if not self.grouped:
                raise ValueError("AdamW.load_state_dict: the state has parameter groups, this optimiser was built without any")
            if len(saved) != len(self.param_groups) or any(set(a["names"]) != set(b["names"]) for a, b in zip(saved, self.param_groups)):
                raise ValueError("AdamW.load_state_dict: the state's parameter groups do not hold the parameters of this optimiser's "
                                 f"({[len(a['names']) for a in saved]} against {[len(b['names']) for b in self.param_groups]} names)")
        self._m = None if m is None else m.detach().clone().reshape(-1)
        self._v = None if v is None else v.detach().clone().reshape(-1)
        self.step_count = sd["step"]
        for mine, theirs in zip(self.param_groups, saved):
            mine.update({k: v for k, v in theirs.items() if k != "names"})
        if self.grouped:
            ema = sd.get("ema")
            self._ema = None if ema is None else ema.detach().clone().reshape(-1)
            self._skipped = int(sd.get("skipped_steps", 0))
            if self.skipped_steps is not None:
                self.skipped_steps.fill_(self._skipped)
            for k, val in sd.get("hyper", {}).items():
                setattr(self, k, val)


def _recast(arena) -> None:
    """after a raw write into arena.flat: shadows and transposed shadows again from the masters"""
    arena.refresh_shadows(force=True)
    arena.refresh_transposed()


def interpolate_weights(model, other_state_dict, alpha: float) -> None:
    """WiSE-FT: masters <- (1 - alpha) * model + alpha * other over the arena (torch.lerp: alpha = 0 keeps the model's bits,
    alpha = 1 gives other's), then shadows and transposed shadows are cast again.  `other_state_dict` must hold every parameter
    of the model with its shape; what else it holds is ignored."""
    arena = model.arena
    other = torch.zeros_like(arena.flat)
    for n, p in arena.params.items():
        t = other_state_dict.get(n)
        if t is None or tuple(t.shape) != tuple(p.shape):
            raise ValueError(f"interpolate_weights: {n}: the other state dict has {'no such entry' if t is None else tuple(t.shape)}, "
                             f"the model {tuple(p.shape)} (another geometry?)")
        off = arena.offsets[n]
        other[off:off + p.numel()].copy_(t.detach().reshape(-1).to(device=other.device, dtype=torch.float32))
    with torch.no_grad():
        torch.lerp(arena.flat, other, float(alpha), out=arena.flat)
    _recast(arena)


class LinearWarmupSchedule:
    """get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps): lr * min(step/warmup,
    (total-step)/(total-warmup)) (CLIP/train.py:145-147).  The factor is applied to every parameter group's own base learning
    rate (the one it has when the schedule is made)."""

    def __init__(self, optimizer: AdamW, num_warmup_steps: int, num_training_steps: int):
        self.optimizer, self.warmup, self.total = optimizer, num_warmup_steps, num_training_steps
        self.base_lrs = [g["lr"] for g in optimizer.param_groups]
        self.base_lr = self.base_lrs[0]
        self.last_step = 0
        self._apply()

    def _factor(self, step: int) -> float:
        if step < self.warmup:
            return float(step) / float(max(1, self.warmup))
        return max(0.0, float(self.total - step) / float(max(1, self.total - self.warmup)))

    def _apply(self):
        f = self._factor(self.last_step)
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = base * f

    def step(self):
        self.last_step += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int):
    return LinearWarmupSchedule(optimizer, num_warmup_steps, num_training_steps)
