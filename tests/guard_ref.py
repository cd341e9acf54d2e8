"""CPU restatement of the guarded step of train_opt.py:128-157 in torch: the loss test (:136), the
gradient-norm test (:149), torch.nn.utils.clip_grad_norm_ (:155) and torch.optim.Adam (:157), fed
g * float32(scale) formed in fp32 as dn_adam_step forms it.  The norm the decision uses is taken in
fp64 from those same float32 values (the reference sums per-parameter fp32 norms; one flat buffer
has one norm).  Shared by test_guard_cpu.py and test_gpu_guarded_step.py."""
import math

import numpy as np
import torch


def scaled(g: torch.Tensor, scale: float) -> torch.Tensor:
    """g * float32(scale) in fp32 (g itself at scale 1: k_adam's gg)"""
    g = g.detach().to(torch.float32).cpu()
    return g.clone() if scale == 1.0 else g * torch.tensor(scale, dtype=torch.float32)


def norm64(g: torch.Tensor, scale: float = 1.0) -> float:
    """fp64 L2 norm of the float32 values g * float32(scale)"""
    x = scaled(g, scale).numpy().astype(np.float64).reshape(-1)
    return float(np.sqrt(np.dot(x, x)))


def clip_coef(norm: float, clip) -> float:
    """clip_grad_norm_'s coefficient in fp64: min(1, max_norm / (total_norm + 1e-6))"""
    return 1.0 if clip is None else min(1.0, clip / (norm + 1e-6))


class GuardRef:
    """One flat parameter under torch.optim.Adam behind the reference's guards.  `guard`: anything
    with grad_clip, max_loss_skip, max_grad_norm (None: that guard is off); the norm threshold is
    10 * max_grad_norm (train_opt.py:149)."""

    def __init__(self, params: torch.Tensor, guard, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        self.p = torch.nn.Parameter(params.detach().to(torch.float32).cpu().clone())
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=betas, eps=eps)
        self.guard = guard
        self.stats = dict(applied=0, skipped_loss=0, skipped_norm=0, last_norm=0.0, last_coef=1.0)

    def set_lr(self, lr: float) -> None:
        self.opt.param_groups[0]["lr"] = lr

    def step(self, g: torch.Tensor, scale: float = 1.0, loss=None) -> str:
        """-> 'applied' | 'skipped_loss' | 'skipped_norm'"""
        gd = self.guard
        if loss is not None and gd.max_loss_skip is not None:
            loss = float(loss)
            if not math.isfinite(loss) or loss > gd.max_loss_skip:      # train_opt.py:136
                self.stats["skipped_loss"] += 1
                return "skipped_loss"
        gs = scaled(g, scale)
        total_norm = norm64(g, scale)
        self.stats["last_norm"] = total_norm
        any_norm_guard = gd.max_grad_norm is not None or gd.grad_clip is not None
        if (any_norm_guard and not np.isfinite(total_norm)) or \
                (gd.max_grad_norm is not None and total_norm > gd.max_grad_norm * 10):  # :149
            self.stats["skipped_norm"] += 1
            return "skipped_norm"
        self.p.grad = gs.reshape(self.p.shape).clone()
        if gd.grad_clip is not None:                                    # :154-155
            torch.nn.utils.clip_grad_norm_([self.p], max_norm=gd.grad_clip)
        self.stats["last_coef"] = clip_coef(total_norm, gd.grad_clip)
        self.opt.step()                                                 # :157
        self.stats["applied"] += 1
        return "applied"

    @property
    def params(self) -> torch.Tensor:
        return self.p.detach()

    @property
    def exp_avg(self) -> torch.Tensor:
        return self.opt.state[self.p]["exp_avg"]

    @property
    def exp_avg_sq(self) -> torch.Tensor:
        return self.opt.state[self.p]["exp_avg_sq"]
