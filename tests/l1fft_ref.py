"""fp64 restatement of the L1FFT loss and its gradient, in torch on the CPU.

    D = pred - target (real),  n = N C H W,  F = fft2(D) per plane, unnormalised
    loss_pix  = sum|D| / n
    loss_freq = sum_k |F_k| / n over the full H x W spectrum
              = sum over the half spectrum (W/2+1 columns) with columns 1 .. W/2-1 counted twice
    U_k = F_k / |F_k| (0 where |F_k| = 0)
    dloss/dpred = alpha sgn(D) / n + beta (H W / n) Re ifft2(U)        (sgn(0) = 0)

U is Hermitian, so the inverse is the c2r transform of the same half spectrum.  reduction='sum'
drops every 1/n.  Written from the formulas, not from the reference program.
"""
from __future__ import annotations

import numpy as np
import torch

# the shapes of tests/test_gpu_l1fft.py with the torch.rand seed of each: chosen on the CPU so
# that min|F_k| > 1e-3 median|F_k| (asserted by the test), which keeps F / |F| well conditioned
SEEDS = {(2, 1, 8, 8): 0, (1, 3, 16, 64): 0, (2, 1, 64, 16): 0, (3, 1, 32, 32): 0,
         (1, 1, 8, 1024): 0, (2, 1, 256, 256): 0}
GOLDEN_SHAPES = [(2, 1, 8, 8), (1, 3, 16, 64)]
GOLDEN_ALPHA, GOLDEN_BETA = 1.0, 0.7  # the weights of the fixture's combined loss


def inputs(shape, seed=None):
    """(pred, target) fp32 CPU tensors: torch.rand of a fixed seed"""
    g = torch.Generator(device="cpu").manual_seed(SEEDS[tuple(shape)] if seed is None else seed)
    pred = torch.rand(shape, generator=g, dtype=torch.float32)
    target = torch.rand(shape, generator=g, dtype=torch.float32)
    return pred, target


def half_weights(W: int) -> torch.Tensor:
    w = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64)
    w[0] = 1.0
    w[W // 2] = 1.0
    return w


def half_spectrum(pred, target) -> torch.Tensor:
    """F over the W/2+1 stored columns, complex128"""
    D = pred.double() - target.double()
    return torch.fft.fft(torch.fft.rfft(D, dim=-1), dim=-2)


def restatement(pred, target, alpha=1.0, beta=1.0, reduction="mean"):
    """-> (loss3 = [pixel, freq, total] float64 tensor, dpred float64 tensor)"""
    D = pred.double() - target.double()
    N, C, H, W = D.shape
    n = D.numel() if reduction == "mean" else 1
    F = half_spectrum(pred, target)
    mag = F.abs()
    pix = D.abs().sum() / n
    frq = (mag * half_weights(W)).sum() / n
    U = torch.where(mag > 0, F / torch.where(mag > 0, mag, torch.ones_like(mag)),
                    torch.zeros_like(F))
    # c2r of the half spectrum: unnormalised inverse along H, then the Hermitian inverse along W
    g = torch.fft.irfft(torch.fft.ifft(U, dim=-2, norm="forward"), n=W, dim=-1, norm="forward")
    dpred = alpha * torch.sign(D) / n + beta * g / n
    return torch.stack([pix, frq, alpha * pix + beta * frq]), dpred


def full_spectrum_parts(pred, target, reduction="mean"):
    """[pixel, freq] by the direct sum over the full H x W spectrum"""
    D = pred.double() - target.double()
    n = D.numel() if reduction == "mean" else 1
    return torch.stack([D.abs().sum() / n, torch.fft.fft2(D).abs().sum() / n])


def torch_fp32(pred, target, alpha=1.0, beta=1.0):
    """the reference's formulation in fp32 on the CPU (fft2 of each tensor, complex abs, mean,
    autograd): the error class the kernel's gradient is measured against"""
    p = pred.clone().float().requires_grad_(True)
    t = target.float()
    pix = (p - t).abs().mean()
    frq = (torch.fft.fft2(p) - torch.fft.fft2(t)).abs().mean()
    (alpha * pix + beta * frq).backward()
    return torch.stack([pix.detach(), frq.detach(), (alpha * pix + beta * frq).detach()]), p.grad


def conditioning(pred, target):
    """(min|F_k|, median|F_k|) of the fp64 half spectrum"""
    mag = half_spectrum(pred, target).abs()
    return float(mag.min()), float(mag.median())
