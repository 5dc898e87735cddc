"""Fused optimiser for models whose parameters live in a cclip_hip ParamArena.

`AdamW` reproduces `transformers.AdamW(lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
correct_bias=True)` - what the reference optimises with (/root/reference/CLIP/train.py:143,
/root/reference/CLIP_prefix_caption/train.py:336; the class no longer exists in transformers >= 5) -
as ONE launch over the flat arena that also rewrites the bf16 weight shadows.
`get_linear_schedule_with_warmup` restates the schedule of CLIP/train.py:145-147.
Any torch.optim optimiser also works on the model's parameters (they are ordinary nn.Parameters);
this one is simply ~400 launches cheaper per step.
"""
from __future__ import annotations

import torch

from cclip_hip import ops


class AdamW:
    """A parameter whose `.grad` is None at a step is left alone at that step - its value, both moments and its 16-bit shadow
    keep their bits, whatever the weight decay - as `transformers.AdamW` (and torch's optimisers) skip it: a frozen GPT-2 under
    prefix-only training does not decay.  One difference stays: the bias correction uses ONE step count for the whole arena
    (the number of `step()` calls), not one per parameter as `transformers.AdamW` keeps; a parameter that sat out some steps is
    corrected as if it had not.
    With every gradient present the step is one launch over the flat arena; otherwise one launch per contiguous run of slots
    that have gradients (`ParamArena.slot_ranges`)."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 correct_bias: bool = True, torch_semantics: bool = False):
        self.model = model
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        self.param_groups = [dict(self.defaults, params=list(model.parameters()))]
        self.mode = 1 if torch_semantics else 0
        self.step_count = 0
        self._m = self._v = None

    def _state(self):
        """The arena, with the moment buffers on its device.  Moments of another size (a state saved for another geometry) are an
        error: re-zeroing them would restart the moments under a step count that says otherwise."""
        arena = self.model.arena
        if self._m is None:
            self._m = torch.zeros_like(arena.flat)
            self._v = torch.zeros_like(arena.flat)
        for name, t in (("exp_avg", self._m), ("exp_avg_sq", self._v)):
            if t.numel() != arena.total or t.dtype != torch.float32:
                raise ValueError(f"AdamW: the optimiser state does not fit this model: {name} holds {t.numel()} {t.dtype} elements, "
                                 f"the parameter arena {arena.total} float32 (a state_dict saved for another geometry?)")
        if self._m.device != arena.flat.device or self._v.device != arena.flat.device:
            self._m, self._v = self._m.to(arena.flat.device), self._v.to(arena.flat.device)
        return arena

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
        if len(names) != len(arena.params):
            arena.refresh_shadows()           # the skipped slots keep their shadows, and the step marks ALL shadows fresh: no-op unless stale
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

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.model.parameters():
            p.grad = None

    def state_dict(self):
        return dict(step=self.step_count, exp_avg=self._m, exp_avg_sq=self._v, param_groups=[
            {k: v for k, v in self.param_groups[0].items() if k != "params"}])

    def load_state_dict(self, sd):
        """The moments are copied (onto the arena's device at the next step); a state whose moment buffers do not hold one
        element per arena element is refused there - see _state()."""
        m, v = sd["exp_avg"], sd["exp_avg_sq"]
        if (m is None) != (v is None) or (m is not None and m.numel() != v.numel()):
            raise ValueError("AdamW.load_state_dict: exp_avg and exp_avg_sq do not match each other")
        self._m = None if m is None else m.detach().clone().reshape(-1)
        self._v = None if v is None else v.detach().clone().reshape(-1)
        self.step_count = sd["step"]
        self.param_groups[0].update(sd["param_groups"][0])


class LinearWarmupSchedule:
    """get_linear_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps): lr * min(step/warmup,
    (total-step)/(total-warmup)) (CLIP/train.py:145-147)."""

    def __init__(self, optimizer: AdamW, num_warmup_steps: int, num_training_steps: int):
        self.optimizer, self.warmup, self.total = optimizer, num_warmup_steps, num_training_steps
        self.base_lr = optimizer.param_groups[0]["lr"]
        self.last_step = 0
        self._apply()

    def _factor(self, step: int) -> float:
        if step < self.warmup:
            return float(step) / float(max(1, self.warmup))
        return max(0.0, float(self.total - step) / float(max(1, self.total - self.warmup)))

    def _apply(self):
        self.optimizer.param_groups[0]["lr"] = self.base_lr * self._factor(self.last_step)

    def step(self):
        self.last_step += 1
        self._apply()

    def get_last_lr(self):
        return [self.optimizer.param_groups[0]["lr"]]


def get_linear_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int):
    return LinearWarmupSchedule(optimizer, num_warmup_steps, num_training_steps)
