"""Structure_loss (util.py:41-70 of the reference), computed by one HIP reduction kernel.

L = alpha*L1(pred, target) + beta*(L1(pred2[:,:,1:],pred2[:,:,:-1]) + L1(pred2[...,1:],pred2[...,:-1]))/2
    + gamma*L1(pred2, target)      with pred = net(noisy), pred2 = net(clean) (train.py:361-363)

and L1FFT (util.py:5-38), by the row / column / row FFT kernels of csrc/fft_loss.hip:

L = alpha*L1(pred, target) + beta*mean|fft2(pred) - fft2(target)|      (train.py:318-321)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .n2n import _partials_for


def structure_loss_into(pred, pred2, target, alpha, beta, gamma, dpred, dpred2, loss5):
    """dn_structure_loss into given contiguous buffers: loss5 = [pixel, tv1, tv2, cst, total],
    dpred = dL/dpred, dpred2 = dL/dpred2 (all on pred's device and stream)"""
    for t in (pred, pred2, target, dpred, dpred2, loss5):
        if not t.is_contiguous():
            raise ValueError("structure_loss_into needs contiguous tensors")
    if (pred.shape != pred2.shape or pred.shape != target.shape or pred.dim() != 4
            or dpred.shape != pred.shape or dpred2.shape != pred.shape or loss5.numel() != 5):
        raise ValueError("pred, pred2, target, dpred and dpred2 must share one [N,C,H,W] shape")
    N, C, H, W = pred.shape
    _lib.call("dn_structure_loss", _lib.ptr(pred), _lib.ptr(pred2), _lib.ptr(target), N, C, H, W,
              float(alpha), float(beta), float(gamma), _lib.ptr(dpred), _lib.ptr(dpred2),
              _lib.ptr(loss5), _partials_for(pred.device).data_ptr(), _lib.stream_of(pred))


def structure_loss(pred, pred2, target, alpha=1.0, beta=0.5, gamma=0.5):
    """returns (loss5 = [pixel, tv1, tv2, cst, total] device tensor, dpred, dpred2)"""
    pred, pred2, target = pred.contiguous(), pred2.contiguous(), target.contiguous()
    if pred.shape != pred2.shape or pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("pred, pred2 and target must share one [N,C,H,W] shape")
    dpred = torch.empty_like(pred)
    dpred2 = torch.empty_like(pred2)
    loss5 = torch.empty(5, dtype=torch.float32, device=pred.device)
    structure_loss_into(pred, pred2, target, alpha, beta, gamma, dpred, dpred2, loss5)
    return loss5, dpred, dpred2


class _StructureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, pred2, target, alpha, beta, gamma):
        loss5, dp, dp2 = structure_loss(pred, pred2, target, alpha, beta, gamma)
        ctx.save_for_backward(dp, dp2)
        return loss5[4]

    @staticmethod
    def backward(ctx, g):
        dp, dp2 = ctx.saved_tensors
        return dp * g, dp2 * g, None, None, None, None


class Structure_loss(nn.Module):  # noqa: N801  (reference name, util.py:41)
    def __init__(self, alpha: float = 1.0, beta: float = .5, gamma: float = .5,
                 reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference default) is supported")
        self.alpha, self.beta, self.gamma, self.reduction = alpha, beta, gamma, reduction

    def forward(self, pred, pred2, target):
        return _StructureFn.apply(pred, pred2, target, self.alpha, self.beta, self.gamma)


# ---- L1FFT (util.py:5-38 of the reference) -------------------------------------------------
_l1fft_ws = {}


L1FFT_RULE = "H and W of the form m * 2^k with m odd, 1 <= m <= 31, k >= 3, at most 1024"


def l1fft_supported(H: int, W: int) -> bool:
    """the transform lengths dn_l1fft_loss has, H and W independently: L = m * 2^k with m odd,
    1 <= m <= 31, k >= 3 and L <= 1024 (every multiple of 32 and every power of two from 8 up
    to 1024)"""
    def ok(v: int) -> bool:
        if v < 8 or v > 1024 or v % 8:
            return False
        return v // (v & -v) <= 31  # the odd part

    return ok(int(H)) and ok(int(W))


def _l1fft_ws_for(N, C, H, W, device) -> torch.Tensor:
    """the loss's workspace (half spectrum + block partials), one per device, grown on demand"""
    need = _lib.lib().dn_l1fft_ws_size(N, C, H, W)
    t = _l1fft_ws.get(device)
    if t is None or t.numel() < need:
        t = _lib.scratch(need, device)
        _l1fft_ws[device] = t
    return t


def l1fft_loss_into(pred, target, alpha, beta, dpred, loss3, reduction="mean"):
    """dn_l1fft_loss into given contiguous buffers: loss3 = [pixel, freq, total],
    dpred = dL/dpred (all on pred's device and stream).  H and W must each be m * 2^k with m odd,
    1 <= m <= 31, k >= 3, and at most 1024 (l1fft_supported): anything else raises ValueError
    (there is no other path)."""
    if reduction not in ("mean", "sum"):
        raise NotImplementedError("L1FFT supports reduction='mean' and 'sum'")
    for t in (pred, target, dpred, loss3):
        if not t.is_contiguous():
            raise ValueError("l1fft_loss_into needs contiguous tensors")
    if (pred.dim() != 4 or pred.shape != target.shape or dpred.shape != pred.shape
            or loss3.numel() != 3):
        raise ValueError("pred, target and dpred must share one [N,C,H,W] shape, loss3 holds 3")
    N, C, H, W = pred.shape
    if N < 1 or C < 1 or not l1fft_supported(H, W):
        raise ValueError(f"L1FFT needs {L1FFT_RULE}, got {H} x {W}")
    ws = _l1fft_ws_for(N, C, H, W, pred.device)
    _lib.call("dn_l1fft_loss", _lib.ptr(pred), _lib.ptr(target), N, C, H, W, float(alpha),
              float(beta), int(reduction == "sum"), _lib.ptr(dpred), _lib.ptr(loss3),
              ws.data_ptr(), ws.numel(), _lib.stream_of(pred))


def l1fft_loss(pred, target, alpha=1.0, beta=1.0, reduction="mean"):
    """returns (loss3 = [pixel, freq, total] device tensor, dpred)"""
    pred, target = pred.contiguous(), target.contiguous()
    dpred = torch.empty_like(pred)
    loss3 = torch.empty(3, dtype=torch.float32, device=pred.device)
    l1fft_loss_into(pred, target, alpha, beta, dpred, loss3, reduction)
    return loss3, dpred


class _L1FFTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, alpha, beta, reduction):
        loss3, dp = l1fft_loss(pred, target, alpha, beta, reduction)
        ctx.save_for_backward(dp)
        return loss3[2]

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None, None, None, None


class L1FFT(nn.Module):  # reference name, util.py:5
    """alpha * L1(pred, target) + beta * |fft2(pred) - fft2(target)| reduced like the L1 term.
    The gradient flows to pred only (the target is data), as for the other losses here.
    H and W: m * 2^k with m odd, 1 <= m <= 31, k >= 3, at most 1024 (every multiple of 32 up to
    1024, so 96, 352 or 704 as well as the powers of two); ValueError otherwise."""

    def __init__(self, alpha: float = 1.0, beta: float = 1.0, reduction: str = "mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise NotImplementedError("L1FFT supports reduction='mean' and 'sum', not 'none'")
        self.alpha, self.beta, self.reduction = alpha, beta, reduction

    def forward(self, pred, target):
        return _L1FFTFn.apply(pred, target, self.alpha, self.beta, self.reduction)
