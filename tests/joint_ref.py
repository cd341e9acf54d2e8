"""The joint finetune (DenoiserWithAdapter(freeze_base=False, use_no_grad_for_base=False),
adapter.py:64-66, under finetune.py:269-289's step) as torch-CPU autograd, composed from the
repository's own restatements: oracle/unet_ref.py (UNet), tests/resnet_ref.py (RESNET) and
oracle/adapter_ref.py (OutputAdapter, the finetune loss).  Test infrastructure only; the dtype of
the flat parameter buffers decides the arithmetic (fp64 for the GPU tests' reference truth).

tests/test_joint_ref_cpu.py pins it to a fixture the reference produced
(tests/golden/make_golden_joint.py)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resnet_ref  # noqa: E402
from oracle import adapter_ref, unet_ref  # noqa: E402

BASES = {"UNet": unet_ref, "RESNET": resnet_ref}


def layer_ranges(arch: str, C: int):
    """[(layer name, begin, end)] of each base layer's weight + bias in the base's flat buffer"""
    out, off = [], 0
    for name, ws, bl, _ in BASES[arch].layer_table(C, C):
        n = int(np.prod(ws)) + bl
        out.append((name, off, off + n))
        off += n
    return out


def forward(base_flat, ad_flat, noisy, arch: str = "UNet"):
    """(pred, base_out): adapter.py:59-67 with use_no_grad_for_base=False"""
    C = noisy.shape[1]
    base_out = BASES[arch].forward(base_flat, noisy, C, C)
    return adapter_ref.adapter_forward(ad_flat, noisy, base_out), base_out


def loss_and_grads(base_flat, ad_flat, clean, noisy, arch: str = "UNet", lambda_grad: float = 0.1,
                   dtype=torch.float64):
    """One loss.backward() through the adapter into the base.  Returns dict(loss3 = [loss_l1,
    loss_grad, loss], gbase, gad, pred, base_out, dbase), tensors of `dtype`."""
    pb = base_flat.detach().to(dtype).clone().requires_grad_(True)
    pa = ad_flat.detach().to(dtype).clone().requires_grad_(True)
    pred, base_out = forward(pb, pa, noisy.to(dtype), arch)
    base_out.retain_grad()
    l1, lg, loss = adapter_ref.finetune_loss(pred, clean.to(dtype), lambda_grad)
    loss.backward()
    return dict(loss3=[float(v.detach()) for v in (l1, lg, loss)], gbase=pb.grad.detach(),
                gad=pa.grad.detach(), pred=pred.detach(), base_out=base_out.detach(),
                dbase=base_out.grad.detach())


def steps(base_flat, ad_flat, batches, arch: str = "UNet", lr: float = 1e-4,
          lambda_grad: float = 0.1, dtype=torch.float64):
    """finetune.py:260-289 over `batches` = [(clean, noisy)]: ONE torch.optim.Adam over the base's
    and the adapter's parameters.  Returns dict(losses = [loss3 per step], gbase / gad of the
    first step, base / adapter = the parameters after the last step)."""
    pb = base_flat.detach().to(dtype).clone().requires_grad_(True)
    pa = ad_flat.detach().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([pb, pa], lr=lr)
    out = dict(losses=[])
    for clean, noisy in batches:
        opt.zero_grad()
        pred, _ = forward(pb, pa, noisy.to(dtype), arch)
        l1, lg, loss = adapter_ref.finetune_loss(pred, clean.to(dtype), lambda_grad)
        loss.backward()
        out["losses"].append([float(v.detach()) for v in (l1, lg, loss)])
        if "gbase" not in out:
            out["gbase"], out["gad"] = pb.grad.detach().clone(), pa.grad.detach().clone()
        opt.step()
    out["base"], out["adapter"] = pb.detach().clone(), pa.detach().clone()
    return out


def adapter_input_grads(ad_flat, noisy, base_out, dout, dtype=torch.float64):
    """(dnoisy, dbase, hidden-off share) of the adapter alone for the cotangent dout"""
    import torch.nn.functional as F

    p = ad_flat.detach().to(dtype)
    n = noisy.detach().to(dtype).clone().requires_grad_(True)
    b = base_out.detach().to(dtype).clone().requires_grad_(True)
    adapter_ref.adapter_forward(p, n, b).backward(dout.to(dtype))
    w1, b1, _, _ = adapter_ref.unflatten(p, noisy.shape[1])
    pre = F.conv2d(torch.cat([n, b], 1).detach(), w1, b1, padding=1)
    return n.grad.detach(), b.grad.detach(), float((pre <= 0).double().mean())
