"""The step of the reference's finetune_memory.py: a frozen base denoiser, a nearest-patch lookup
in the memory bank, and the trainable hyper-gated adapter, trained with L1 + lambda_grad *
gradient_loss [+ lambda_iqsl * iqsl].

    base_out  = base(noisy)            [no grad]   dn_unet_forward (fp32 or bf16 base)
    idx       = nearest noisy bank patch           dn_memory_select
    mem_clean = its clean partner                  dn_memory_gather
    pred      = adapter(noisy, base_out, mem)      dn_memadapter_forward
    loss4, dpred                                   dn_finetune_iqsl_loss  (loss3: dn_finetune_loss)
    dA        = adapter backward(dpred)            dn_memadapter_backward
    [data parallel: one RCCL all-reduce(sum) of the flat gradient; every rank holds the whole bank]
    Adam(A, dA / world)                            dn_adam_step

With DenoiserWithMemoryAdapter(freeze_base=False, use_no_grad_for_base=False) the base trains too
(the joint step): its forward is saved, the selection and the gather are unchanged, and
    dA, dbase = adapter backward(dpred)            dn_memadapter_backward_input   (one call)
    dB        = base backward(dbase)               dn_<family>_backward_prec
    [data parallel: both flat gradients all-reduced]
    Adam(A, dA / world), Adam(B, dB / world)       dn_adam_step

No host synchronisation inside the step.
"""
from __future__ import annotations

import torch

from .finetune import _AdapterStepBase
from .memory import DenoiserWithMemoryAdapter


class MemoryFinetuneTrainer(_AdapterStepBase):
    """Returns loss4 = [loss_l1, loss_grad, loss_iqsl, loss] when lambda_iqsl > 0 (`iqsl` =
    dict(t1, t2[, tau, margin, ce_factor])), else loss3 = [loss_l1, loss_grad, loss].  guard:
    optim.GradGuard around the update, tested against the total (the last entry).

    A model built with freeze_base=False takes the joint step (`joint`): the base's forward is
    saved in `set_precision`'s 'fp32' / 'fp32_x6' arithmetic (the bf16 inference plan is
    forward-only and not used), one dn_memadapter_backward_input call yields the adapter's
    parameter gradient and dL/dbase_out, the base's HIP backward follows, and a second FlatAdam
    (same lr, same step count) updates the base's flat buffer (`base_grad`, `base_opt`).
    distributed=True all-reduces both gradients.  The base must be a HipNet (TypeError) and
    guard= is refused there (ValueError), as in FinetuneTrainer."""

    def __init__(self, model: DenoiserWithMemoryAdapter, lr: float = 1e-4, lambda_grad: float = 0.1,
                 distributed: bool | None = None, lambda_iqsl: float = 0.0,
                 iqsl: dict | None = None, guard=None):
        if not isinstance(model, DenoiserWithMemoryAdapter):
            raise TypeError("MemoryFinetuneTrainer drives a DenoiserWithMemoryAdapter")
        super().__init__(model, lr, lambda_grad, distributed, lambda_iqsl, iqsl, guard)

    def train_step(self, clean: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
        clean, noisy = clean.contiguous(), noisy.contiguous()
        if clean.shape != noisy.shape:
            raise ValueError("clean and noisy must share one shape")
        ad, bank = self.model.adapter, self.model.bank
        if self.joint:
            b = self._joint_base_forward(noisy)
            mem = bank.gather_clean(bank.select(noisy))
            feat = ad._run_forward(noisy, b["base"], mem, b["pred"])
            loss, dpred = self._loss(b["pred"], clean)
            ad._run_backward_input(noisy, b["base"], feat, dpred, self.grad, b["dbase"])
            self._joint_update(b, noisy)
            return loss
        b = self._buffers(noisy.shape, noisy.device)
        self._base_forward(noisy, b["base"])
        mem = bank.gather_clean(bank.select(noisy))
        feat = ad._run_forward(noisy, b["base"], mem, b["pred"])
        loss, dpred = self._loss(b["pred"], clean)
        ad._run_backward(noisy, b["base"], feat, dpred, self.grad)
        self._update(loss=loss[-1] if self.guard is not None else None)
        return loss
