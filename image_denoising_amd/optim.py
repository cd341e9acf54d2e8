"""Adam over the flat parameter buffer + the reference's MultiStepLR schedule.

train.py:332-340: optim.Adam(network.parameters(), lr=opt.lr) and
MultiStepLR(milestones=[int(20r)-1, int(40r)-1, int(60r)-1, int(80r)-1], gamma=opt.gamma),
r = n_epoch/100, stepped once per epoch (train.py:375).

`GradGuard` adds train_opt.py:128-157's guards to the step (skip a bad batch, skip a bad gradient,
clip), decided on the device.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib


@dataclass
class GradGuard:
    """train_opt.py:118-119's `grad_clip`, `max_loss_skip`, `max_grad_norm`.  The step is skipped
    when the loss is non-finite or > max_loss_skip (:136), else when the gradient's L2 norm is
    non-finite or > 10 * max_grad_norm (:149); otherwise the gradient is clipped to norm grad_clip
    (clip_grad_norm_, :155) and applied.  None turns each guard off on its own."""

    grad_clip: float | None = 1.0
    max_loss_skip: float | None = 5.0
    max_grad_norm: float | None = 20.0

    @property
    def max_norm_skip(self) -> float | None:
        """the norm above which the step is skipped (train_opt.py:149)"""
        return None if self.max_grad_norm is None else 10.0 * self.max_grad_norm


class FlatAdam:
    """torch.optim.Adam (amsgrad=False, weight_decay=0) as ONE fused HIP kernel over a flat
    fp32 buffer; state tensors are flat too.  `grad_scale` folds the 1/world_size of a
    data-parallel all-reduce(sum) into the same pass.

    With a `guard` the step is dn_adam_step_guarded: norm, decision and update are three launches
    and no host read.  The step count then lives in the device guard state (a skipped step must
    not advance the bias correction, and the host does not know which steps were skipped);
    `step_count` holds its value at the last guard_stats() / state_dict() / load_state_dict()."""

    def __init__(self, params: torch.Tensor, lr: float = 3e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, guard: GradGuard | None = None):
        if params.dtype != torch.float32 or not params.is_contiguous():
            raise ValueError("FlatAdam needs a contiguous fp32 buffer")
        self.params = params
        self.lr = lr
        self.betas = betas
        self.eps = eps
        self.exp_avg = torch.zeros_like(params)
        self.exp_avg_sq = torch.zeros_like(params)
        self.step_count = 0
        self.guard = guard
        self._guard_state = None  # device bytes (dn_guard_state_size), made at the first launch

    def step(self, grad: torch.Tensor, grad_scale: float = 1.0,
             loss: torch.Tensor | None = None) -> None:
        """`loss` (guarded steps only): the step's total loss, a 0-dim or 1-element fp32 tensor
        on the parameters' device; None leaves the loss test out"""
        if grad.shape != self.params.shape:
            raise ValueError("grad and params differ in shape")
        if self.guard is None:
            if loss is not None:
                raise ValueError("a loss is only taken by a FlatAdam built with a guard")
            self.step_count += 1
            adam_launch(self, grad.contiguous(), float(grad_scale))
            return
        if loss is not None and (loss.dtype != torch.float32 or loss.numel() != 1
                                 or loss.device != self.params.device):
            raise ValueError("loss must be one fp32 element on the parameters' device")
        guarded_adam_launch(self, grad.contiguous(), float(grad_scale), loss)

    def guard_state(self) -> torch.Tensor:
        """the caller-owned device state of the guarded step, created on first use"""
        if self.guard is None:
            raise ValueError("this FlatAdam has no guard")
        if self._guard_state is None:
            self._guard_state = _lib.scratch(_lib.lib().dn_guard_state_size(), self.params.device)
            _lib.call("dn_guard_state_init", self._guard_state.data_ptr(), int(self.step_count),
                      _lib.stream_of(self.params))
        return self._guard_state

    def guard_stats(self) -> dict:
        """the guard state's dn_guard_stats as a dict: step, applied, skipped_loss, skipped_norm,
        last_norm, last_coef, apply, gscale, step_size, bc2s, last_loss.  Synchronises the host."""
        st = _lib.DnGuardStats()
        _lib.call("dn_guard_state_read", self.guard_state().data_ptr(), st,
                  _lib.stream_of(self.params))
        out = {name: getattr(st, name) for name, _ in st._fields_}
        self.step_count = int(out["step"])
        return out

    def state_dict(self):
        if self.guard is not None:
            self.guard_stats()  # the device step count
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "lr": self.lr, "betas": self.betas, "eps": self.eps}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.lr, self.betas, self.eps = sd["lr"], tuple(sd["betas"]), sd["eps"]
        if self.guard is not None:  # the counters restart, the step count carries over
            _lib.call("dn_guard_state_init", self.guard_state().data_ptr(), self.step_count,
                      _lib.stream_of(self.params))


def adam_launch(opt: FlatAdam, grad: torch.Tensor, grad_scale: float) -> None:
    """one dn_adam_step over the flat buffers (step count already incremented)"""
    b1, b2 = opt.betas
    _lib.call("dn_adam_step", _lib.ptr(opt.params), _lib.ptr(grad), _lib.ptr(opt.exp_avg),
              _lib.ptr(opt.exp_avg_sq), opt.params.numel(), float(opt.lr), float(b1), float(b2),
              float(opt.eps), opt.step_count, float(grad_scale), _lib.stream_of(opt.params))


def guarded_adam_launch(opt: FlatAdam, grad: torch.Tensor, grad_scale: float,
                        loss: torch.Tensor | None) -> None:
    """one dn_adam_step_guarded over the flat buffers: the norm of grad_scale * grad, the decision
    (which also advances the device step count) and the Adam pass that obeys it"""
    b1, b2 = opt.betas
    g = opt.guard
    off = lambda v: 0.0 if v is None else float(v)  # noqa: E731  (<= 0: that guard is off)
    _lib.call("dn_adam_step_guarded", _lib.ptr(opt.params), _lib.ptr(grad), _lib.ptr(opt.exp_avg),
              _lib.ptr(opt.exp_avg_sq), opt.params.numel(), float(opt.lr), float(b1), float(b2),
              float(opt.eps), float(grad_scale), _lib.ptr(loss), off(g.max_loss_skip),
              off(g.max_norm_skip), off(g.grad_clip), opt.guard_state().data_ptr(),
              _lib.stream_of(opt.params))


def reference_milestones(n_epoch: int):
    ratio = n_epoch / 100
    return [int(20 * ratio) - 1, int(40 * ratio) - 1, int(60 * ratio) - 1, int(80 * ratio) - 1]


def lr_at_epoch(epoch: int, base_lr: float, n_epoch: int, gamma: float = 0.5) -> float:
    """lr in effect during 1-based `epoch` (MultiStepLR.last_epoch == epoch-1).

    MultiStepLR multiplies by gamma**count(m) when last_epoch reaches milestone m (the
    construction step sets last_epoch = 0, so a milestone 0 fires at once; repeated milestones
    count with multiplicity).  last_epoch never equals a negative milestone, which
    reference_milestones() yields for n_epoch < 5 (int(20r) = 0): those never fire."""
    last = epoch - 1
    k = sum(1 for m in reference_milestones(n_epoch) if 0 <= m <= last)
    return base_lr * gamma ** k
