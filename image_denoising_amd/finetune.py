"""Adapter finetune path of finetune.py (reference): a frozen base denoiser + a trainable
OutputAdapter, trained with L1 + lambda_grad * gradient_loss on random patches.

    base_out = base(noisy)           [no grad]   dn_unet_forward        (adapter.py:59-61)
    pred     = adapter(noisy, base_out)          dn_adapter_forward     (adapter.py:22-26)
    loss3, dpred = L1 + lambda*grad-L1           dn_finetune_loss       (finetune.py:153-162, :283-285)
      [+ lambda_iqsl * iqsl -> loss4]            dn_finetune_iqsl_loss  (finetune_iqsl.py:291-383)
    dA       = adapter backward(dpred)           dn_adapter_backward
    [data parallel: one RCCL all-reduce(sum) of the 449-float gradient]
    Adam(A, dA / world)                          dn_adam_step           (finetune.py:246-249, :288)

With DenoiserWithAdapter(freeze_base=False, use_no_grad_for_base=False) the base trains too
(FinetuneTrainer's joint step): its forward is saved, and after dA
    dbase    = adapter input gradient(dpred)     dn_adapter_backward_input
    dB       = base backward(dbase)              dn_<family>_backward_prec
    Adam(B, dB / world)                          dn_adam_step

No host synchronisation inside the step.  `DenoisePatchDataset` restates the reference's host
loader (finetune.py:100-150); the training command feeds the step from the device-resident
sampler instead (data.DevicePatchSampler, one dn_patch_sample launch per batch):

    python -m image_denoising_amd.finetune --data_dir D --pretrained_ckpt base.pth [--arch UNet]
        [--seed 0] [--precision fp32|fp32_x6] [--base_bf16]        (finetune.py:221-345's loop)
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import dist as dp
from .adapter import DenoiserWithAdapter
from .arch_unet import UNet
from .checkpoint import strip_module_prefix
from .flat_module import HipNet
from .n2n import _partials_for
from .optim import FlatAdam
from .trainer import _FlatStepBase


def gradient(x: torch.Tensor):
    """finetune.py:153-156 (views only)"""
    dx = x[:, :, :, 1:] - x[:, :, :, :-1]
    dy = x[:, :, 1:, :] - x[:, :, :-1, :]
    return dx, dy


def finetune_loss(pred: torch.Tensor, target: torch.Tensor, lambda_grad: float = 0.1):
    """loss_l1 + lambda_grad * gradient_loss (finetune.py:283-285) and its gradient in one HIP
    pass.  Returns (loss3 = [loss_l1, loss_grad, loss] device tensor, dloss/dpred)."""
    pred, target = pred.contiguous(), target.contiguous()
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("pred and target must share one [N,C,H,W] shape")
    N, C, H, W = pred.shape
    dpred = torch.empty_like(pred)
    loss3 = torch.empty(3, dtype=torch.float32, device=pred.device)
    _lib.call("dn_finetune_loss", _lib.ptr(pred), _lib.ptr(target), N, C, H, W,
              float(lambda_grad), _lib.ptr(dpred), _lib.ptr(loss3),
              _partials_for(pred.device).data_ptr(), _lib.stream_of(pred))
    return loss3, dpred


class _FinetuneLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lam, which):
        loss3, dpred = finetune_loss(pred, target, lam)
        ctx.save_for_backward(dpred)
        return loss3[which]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None


class FinetuneLoss(nn.Module):
    """l1_criterion(pred, clean) + lambda_grad * gradient_loss(pred, clean) as one module."""

    def __init__(self, lambda_grad: float = 0.1):
        super().__init__()
        self.lambda_grad = lambda_grad

    def forward(self, pred, target):
        return _FinetuneLossFn.apply(pred, target, self.lambda_grad, 2)


_iqsl_partials = {}


def _iqsl_partials_for(device) -> torch.Tensor:
    key = (device.type, device.index)
    if key not in _iqsl_partials:
        _iqsl_partials[key] = _lib.scratch(_lib.lib().dn_iqsl_partials_size(), device)
    return _iqsl_partials[key]


def _iqsl_inputs(pred, target):
    """finetune_iqsl.py:309-316: [B,H,W] gets a channel axis; one shape, C == 1"""
    if pred.dim() == 3:
        pred = pred.unsqueeze(1)
    if target.dim() == 3:
        target = target.unsqueeze(1)
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError("pred and target must have the same [B,1,H,W] or [B,H,W] shape")
    if pred.shape[1] != 1:
        raise ValueError("IQSL currently assumes single-channel grayscale input.")
    return pred.contiguous(), target.contiguous()


def finetune_iqsl_loss(pred: torch.Tensor, target: torch.Tensor, lambda_grad: float = 0.1,
                       lambda_iqsl: float = 0.1, t1: float = 0.2, t2: float = 0.8,
                       tau: float = 0.1, margin: float = 0.0, ce_factor: float = 0.5):
    """loss_l1 + lambda_grad * gradient_loss + lambda_iqsl * iqsl_loss (finetune_iqsl.py:476-491)
    and its gradient, no host read.  Returns (loss4 = [loss_l1, loss_grad, loss_iqsl, loss] device
    tensor, dloss/dpred)."""
    pred, target = _iqsl_inputs(pred, target)
    if not float(t1) < float(t2):
        raise ValueError(f"IQSL needs t1 < t2, got {t1}, {t2}")
    N, C, H, W = pred.shape
    dpred = torch.empty_like(pred)
    loss4 = torch.empty(4, dtype=torch.float32, device=pred.device)
    _lib.call("dn_finetune_iqsl_loss", _lib.ptr(pred), _lib.ptr(target), N, C, H, W,
              float(lambda_grad), float(lambda_iqsl), float(t1), float(t2), float(tau),
              float(margin), float(ce_factor), _lib.ptr(dpred), _lib.ptr(loss4),
              _iqsl_partials_for(pred.device).data_ptr(), _lib.stream_of(pred))
    return loss4, dpred


class _IqslLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, t1, t2, tau, margin, ce_factor):
        p, t = _iqsl_inputs(pred.detach(), target.detach())
        N, C, H, W = p.shape
        dpred = torch.empty_like(p)
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        _lib.call("dn_iqsl_loss", _lib.ptr(p), _lib.ptr(t), N, C, H, W, float(t1), float(t2),
                  float(tau), float(margin), float(ce_factor), _lib.ptr(dpred), _lib.ptr(loss),
                  _iqsl_partials_for(p.device).data_ptr(), _lib.stream_of(p))
        ctx.save_for_backward(dpred)
        ctx.shape = pred.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred * g).view(ctx.shape), None, None, None, None, None, None


def iqsl_loss(pred: torch.Tensor, target: torch.Tensor, t1: float, t2: float, tau: float = 0.1,
              margin: float = 0.0, ce_factor: float = 0.5) -> torch.Tensor:
    """finetune_iqsl.py:291-383 (eps = 1e-6): the scalar Intensity-Quantized Structural Loss of
    [B,1,H,W] or [B,H,W] tensors, differentiable w.r.t. pred (dn_iqsl_loss)."""
    if not float(t1) < float(t2):
        raise ValueError(f"IQSL needs t1 < t2, got {t1}, {t2}")
    return _IqslLossFn.apply(pred, target, t1, t2, tau, margin, ce_factor)


def estimate_intensity_thresholds(data_dir: str, q1: float = 0.2, q2: float = 0.8,
                                  max_images: int = 50):
    """finetune_iqsl.py:262-288: the q1 / q2 quantiles of every pixel / 255 of the first
    max_images files of data_dir/clean (host code, as there)."""
    from PIL import Image

    clean_paths = sorted(glob.glob(os.path.join(data_dir, "clean", "*")))[:max_images]
    if len(clean_paths) == 0:
        raise RuntimeError(f"No clean images found in {os.path.join(data_dir, 'clean')}")
    all_pixels = np.concatenate(
        [(np.array(Image.open(p), dtype=np.float32) / 255.0).reshape(-1) for p in clean_paths], axis=0)
    q1, q2 = float(q1), float(q2)
    assert 0.0 < q1 < q2 < 1.0, "iqsl_q1, iqsl_q2 must satisfy 0 < q1 < q2 < 1."
    return float(np.quantile(all_pixels, q1)), float(np.quantile(all_pixels, q2))


class DenoisePatchDataset(torch.utils.data.Dataset):
    """finetune.py:100-150: data_dir/{clean,noise}/* paired by sorted name (first 5 images),
    len = images x patches_per_image, one random ps x ps crop per item (np.random), /255."""

    def __init__(self, data_dir: str, patch_size: int, patches_per_image: int):
        super().__init__()
        self.data_dir = data_dir
        self.clean = sorted(glob.glob(os.path.join(data_dir, "clean", "*")))[:5]
        self.noise = sorted(glob.glob(os.path.join(data_dir, "noise", "*")))[:5]
        assert len(self.clean) == len(self.noise) and len(self.clean) > 0, \
            "clean and noise must have the same number of images and be non-empty."
        self.patch_size = patch_size
        self.patches_per_image = patches_per_image

    def __len__(self) -> int:
        return len(self.clean) * self.patches_per_image

    def _load_pair(self, i: int):
        from PIL import Image
        return (np.array(Image.open(self.clean[i]), dtype=np.float32),
                np.array(Image.open(self.noise[i]), dtype=np.float32))

    @staticmethod
    def _to_tensor(a: np.ndarray) -> torch.Tensor:
        # transforms.ToTensor on a float32 array: HW -> 1HW, HWC -> CHW, no rescaling
        if a.ndim == 2:
            a = a[:, :, None]
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))

    def __getitem__(self, index: int):
        clean, noise = self._load_pair(index // self.patches_per_image)
        h, w = clean.shape[:2]
        ps = self.patch_size
        assert h >= ps and w >= ps, f"Image size ({h},{w}) smaller than patch_size {ps}."
        top = np.random.randint(0, h - ps + 1)
        left = np.random.randint(0, w - ps + 1)
        c = clean[top:top + ps, left:left + ps]
        n = noise[top:top + ps, left:left + ps]
        return self._to_tensor(c) / 255.0, self._to_tensor(n) / 255.0


def build_base_model(arch: str, n_channel: int = 1, n_feature: int = 48) -> nn.Module:
    """finetune.py:180-196: the base network by name."""
    if arch == "UNet":
        return UNet(in_nc=n_channel, out_nc=n_channel, n_feature=n_feature)
    if arch == "RESNET":
        from .resnet import RESNET
        return RESNET(in_nc=n_channel, out_nc=n_channel, n_feature=n_feature)
    if arch == "UNetImproved":
        from .improved_unet import ImprovedUNet
        return ImprovedUNet(in_nc=n_channel, out_nc=n_channel, n_feature=n_feature)
    raise ValueError(f"Unknown or unsupported arch: {arch}")


def load_base_weights(model: nn.Module, ckpt_path: str):
    """finetune.py:199-212: strip a DataParallel `module.` prefix, load non-strict."""
    state = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    state = strip_module_prefix(state)
    return model.load_state_dict(state, strict=False)


class _AdapterStepBase(_FlatStepBase):
    """What the adapter finetune steps share: the loss settings, the replicas' broadcast, Adam over
    the adapter's flat buffer, the step's buffers and the workspace-reusing frozen-base call; and,
    for a model built with freeze_base=False (`joint`), the second flat buffer with its FlatAdam,
    the joint step's buffers and the update of both."""

    def __init__(self, model, lr: float, lambda_grad: float, distributed: bool | None,
                 lambda_iqsl: float, iqsl: dict | None, guard=None):
        # freeze_base=False: the joint step, base and adapter trained together (adapter.py:64-66)
        self.joint = not model.freeze_base
        if self.joint:
            if not isinstance(model.base, HipNet):
                raise TypeError("the joint step needs a base of this package (UNet, RESNET, "
                                "ImprovedUNet): it runs the base's HIP backward")
            if guard is not None:
                raise ValueError("guard= with a trained base is not built: the guard's gradient "
                                 "norm would have to span both flat buffers (the base's and the "
                                 "adapter's); train with freeze_base=True or without a guard")
        self.model = model
        self.lambda_grad = lambda_grad
        self.lambda_iqsl = float(lambda_iqsl)
        self.iqsl = None
        if self.lambda_iqsl > 0.0:
            if iqsl is None or "t1" not in iqsl or "t2" not in iqsl:
                raise ValueError("lambda_iqsl > 0 needs iqsl = dict(t1=..., t2=...[, tau, margin, "
                                 "ce_factor])")
            unknown = set(iqsl) - {"t1", "t2", "tau", "margin", "ce_factor"}
            if unknown:
                raise ValueError(f"unknown IQSL settings: {sorted(unknown)}")
            self.iqsl = dict(iqsl)
        # identical replicas, as nn.DataParallel's per-forward broadcast: the adapter, and the
        # frozen base when it is one of ours (loaded per rank from one checkpoint)
        base = model.base
        self._init_step(model.adapter.flat_params, lr, distributed,
                        frozen=base.flat_params.data if isinstance(base, HipNet) else None,
                        guard=guard)
        if self.joint:
            # the second flat buffer: Adam is elementwise, so two FlatAdams with one lr and one
            # step count are the reference's single Adam over every trainable parameter
            # (finetune.py:260-263); _init_step already broadcast the base to the replicas
            self.base_opt = FlatAdam(model.base.flat_params, lr=lr)
            self.base_grad = torch.zeros_like(model.base.flat_params)

    def _buffers(self, shape, device):
        key = (tuple(shape), device)
        if key not in self._bufs:
            f = dict(dtype=torch.float32, device=device)
            self._bufs = {key: dict(base=torch.empty(shape, **f), pred=torch.empty(shape, **f))}
        return self._bufs[key]

    def _base_forward(self, noisy, out):
        base = self.model.base
        if isinstance(base, HipNet):  # workspace reused across steps; UNet: bf16 if set
            N, _, H, W = noisy.shape
            base._run_forward_inference(noisy, out, base._workspace(N, H, W, with_backward=False))
        else:
            with torch.no_grad():
                out.copy_(base(noisy))

    def _loss(self, pred, clean):
        """(loss4, dpred) with IQSL, else (loss3, dpred)"""
        if self.iqsl is not None:
            return finetune_iqsl_loss(pred, clean, self.lambda_grad, self.lambda_iqsl, **self.iqsl)
        return finetune_loss(pred, clean, self.lambda_grad)

    def _joint_buffers(self, noisy):
        key = (tuple(noisy.shape), noisy.device, "joint")
        if key not in self._bufs:
            N, _, H, W = noisy.shape
            f = dict(dtype=torch.float32, device=noisy.device)
            self._bufs = {key: dict(
                base=torch.empty(noisy.shape, **f), pred=torch.empty(noisy.shape, **f),
                dbase=torch.empty(noisy.shape, **f),
                ws=self.model.base._workspace(N, H, W, with_backward=True, fresh=True))}
        return self._bufs[key]

    def _joint_base_forward(self, noisy):
        """the base's saved forward into the joint buffers"""
        base = self.model.base
        base._check_input(noisy)
        N, _, H, W = noisy.shape
        base._check_size(H, W)
        b = self._joint_buffers(noisy)
        base._run_forward(noisy, b["base"], b["ws"])
        return b

    def _joint_update(self, b, noisy):
        """base backward(dbase) -> [all-reduce both gradients] -> Adam on both buffers"""
        N, _, H, W = noisy.shape
        self.model.base._run_backward(b["dbase"], self.base_grad, b["ws"], N, H, W)
        scale = 1.0
        if self.distributed:
            scale = dp.allreduce_grads(self.grad)
            dp.allreduce_grads(self.base_grad)
        self.opt.step(self.grad, grad_scale=scale)
        self.base_opt.step(self.base_grad, grad_scale=scale)


class FinetuneTrainer(_AdapterStepBase):
    """The finetune.py:269-289 step, fused; returns loss3 = [loss_l1, loss_grad, loss].

    lambda_iqsl > 0 makes it the finetune_iqsl.py:469-494 step: `iqsl` = dict(t1, t2[, tau,
    margin, ce_factor]) (the thresholds from `estimate_intensity_thresholds`), and the step returns
    loss4 = [loss_l1, loss_grad, loss_iqsl, loss].  Each rank's loss is the mean over its own
    batch, as an nn.DataParallel replica computes it.  guard: optim.GradGuard around the update,
    tested against the total (the last entry).

    A model built with freeze_base=False takes the joint step: the base's forward is saved
    (set_precision's 'fp32' / 'fp32_x6' arithmetic; the bf16 inference plan is forward-only and
    not used), dn_adapter_backward_input turns dpred into dL/dbase_out, the base's HIP backward
    follows, and a second FlatAdam (same lr, same step count) updates the base's flat buffer
    (`base_grad`, `base_opt`).  Every base parameter is trained.  distributed=True all-reduces
    both gradients.  guard= is refused there (ValueError): its norm would have to span both
    buffers."""

    def __init__(self, model: DenoiserWithAdapter, lr: float = 1e-4, lambda_grad: float = 0.1,
                 distributed: bool | None = None, lambda_iqsl: float = 0.0,
                 iqsl: dict | None = None, guard=None):
        if not isinstance(model, DenoiserWithAdapter):
            raise TypeError("FinetuneTrainer drives a DenoiserWithAdapter")
        super().__init__(model, lr, lambda_grad, distributed, lambda_iqsl, iqsl, guard)

    def _joint_step(self, clean, noisy):
        """base forward [saved] -> adapter -> loss -> adapter's parameter and input gradients ->
        base backward(dbase) -> [all-reduce both gradients] -> Adam on both buffers"""
        ad = self.model.adapter
        b = self._joint_base_forward(noisy)
        ad._run_forward(noisy, b["base"], b["pred"])
        loss3, dpred = self._loss(b["pred"], clean)
        ad._run_backward(noisy, b["base"], dpred, self.grad)
        ad._run_backward_input(noisy, b["base"], dpred, b["dbase"])
        self._joint_update(b, noisy)
        return loss3

    def train_step(self, clean: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
        clean, noisy = clean.contiguous(), noisy.contiguous()
        if clean.shape != noisy.shape:
            raise ValueError("clean and noisy must share one shape")
        if self.joint:
            return self._joint_step(clean, noisy)
        ad = self.model.adapter
        b = self._buffers(noisy.shape, noisy.device)
        self._base_forward(noisy, b["base"])
        ad._run_forward(noisy, b["base"], b["pred"])
        loss3, dpred = self._loss(b["pred"], clean)
        ad._run_backward(noisy, b["base"], dpred, self.grad)
        self._update(loss=loss3[-1] if self.guard is not None else None)
        return loss3


def parse_args(argv=None):
    """finetune.py:23-81, same names and defaults (parse_known_args there too), plus --seed,
    --precision and --base_bf16.  --num_workers and --gpu_devices are accepted and ignored: the
    loader is the device sampler, and the process uses the current device."""
    import argparse

    ap = argparse.ArgumentParser(prog="python -m image_denoising_amd.finetune")
    ap.add_argument("--data_dir", type=str, required=True,
                    help="B-domain root. Must contain clean/ and noise/ subfolders.")
    ap.add_argument("--pretrained_ckpt", type=str, required=True,
                    help="Checkpoint of the base model trained on A-domain.")
    ap.add_argument("--arch", type=str, default="UNetImproved",
                    choices=["UNet", "RESNET", "UNetImproved"])
    ap.add_argument("--save_model_path", type=str, default="./results_ft")
    ap.add_argument("--log_name", type=str, default="UNetImproved_adapter_ft")
    ap.add_argument("--gpu_devices", default="0", type=str)
    ap.add_argument("--parallel", action="store_true")
    ap.add_argument("--n_feature", type=int, default=48)
    ap.add_argument("--n_channel", type=int, default=1)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--n_epoch", type=int, default=20)
    ap.add_argument("--batchsize", type=int, default=4)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--adapter_hidden", type=int, default=16)
    ap.add_argument("--lambda_grad", type=float, default=0.1)
    ap.add_argument("--save_every", type=int, default=1)
    ap.add_argument("--patch_size", type=int, default=128)
    ap.add_argument("--patches_per_image", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0,
                    help="Seeds the adapter's initialisation, the epoch shuffles and the crops.")
    ap.add_argument("--precision", type=str, default="fp32", choices=["fp32", "fp32_x6"],
                    help="set_precision of the base.")
    ap.add_argument("--base_bf16", action="store_true",
                    help="set_inference_precision('bf16') of the frozen base (UNet).")
    args, _ = ap.parse_known_args(argv)
    if args.parallel:
        ap.error("--parallel (nn.DataParallel) is not built: start one process per GPU with "
                 "torchrun and drive FinetuneTrainer(model, distributed=True) from "
                 "DevicePatchSampler.batches(epoch, batch, world, rank)")
    if args.base_bf16 and args.arch != "UNet":
        ap.error("--base_bf16: only UNet has the bf16 inference plan")
    return args


def main(argv=None):
    """The loop of finetune.py:221-345 on the device path: DevicePatchSampler.batches feeds
    FinetuneTrainer; the adapter is initialised under torch.manual_seed(--seed), the same seed
    drives the sampler.  The host reads a loss only where a line is printed, and the epoch's
    stacked losses once at its end (the mean L1).  Returns dict(losses = every step's [loss_l1,
    loss_grad, loss], mean_l1 per epoch, checkpoints = the files written, psnr = {epoch: [dB per
    validation image]})."""
    import datetime
    import time

    from PIL import Image

    from .checkpoint import save_finetune_checkpoint
    from .data import DevicePatchSampler
    from .evaluation import _device, psnr_device, validation_denoise
    from .evaluation_adapter import denoise

    opt = parse_args(argv)
    dev = _device()
    systime = datetime.datetime.now().strftime("%Y-%m-%d-%H-%M")
    sampler = DevicePatchSampler.from_dir(opt.data_dir, opt.patch_size, opt.patches_per_image,
                                          seed=opt.seed, device=dev)
    print(f"B-domain: {len(sampler.sizes)} images, {opt.patches_per_image} patches/image/epoch → "
          f"{len(sampler)} samples/epoch.")
    valid = validation_denoise(opt.data_dir)

    base = build_base_model(opt.arch, opt.n_channel, opt.n_feature)
    missing, unexpected = load_base_weights(base, opt.pretrained_ckpt)
    if missing:
        print(f"[Warning] Missing keys when loading base model: {missing}")
    if unexpected:
        print(f"[Warning] Unexpected keys when loading base model: {unexpected}")
    print(f"Loaded base weights from {opt.pretrained_ckpt}")
    base.set_precision(opt.precision)
    if opt.base_bf16:
        base.set_inference_precision("bf16")
    torch.manual_seed(opt.seed)
    model = DenoiserWithAdapter(base, in_channels=opt.n_channel, hidden_channels=opt.adapter_hidden,
                                freeze_base=True, use_no_grad_for_base=True).to(dev)
    trainer = FinetuneTrainer(model, lr=opt.lr, lambda_grad=opt.lambda_grad, distributed=False)

    print(f"==> Start finetuning with adapter + patches. Num epochs={opt.n_epoch}, "
          f"batchsize={opt.batchsize}, lr={opt.lr}, lambda_grad={opt.lambda_grad}, "
          f"patch_size={opt.patch_size}, patches_per_image={opt.patches_per_image}")
    out_dir = os.path.join(opt.save_model_path, opt.log_name)
    steps = sampler.steps_per_epoch(opt.batchsize)
    res = dict(losses=[], mean_l1=[], checkpoints=[], psnr={})
    for epoch in range(1, opt.n_epoch + 1):
        model.train()
        epoch_st = time.time()
        losses = []
        for i, (clean, noisy) in enumerate(sampler.batches(epoch, opt.batchsize), start=1):
            loss3 = trainer.train_step(clean, noisy)
            losses.append(loss3)
            if i % 10 == 0 or i == steps:
                l1, lg, lt = loss3.tolist()
                print(f"Epoch [{epoch}/{opt.n_epoch}] Iter [{i}/{steps}] "
                      f"L1={l1:.6f} Grad={lg:.6f} Total={lt:.6f}")
        ep = torch.stack(losses).cpu()  # the epoch's one read of every step's loss
        res["losses"].extend(ep.tolist())
        mean_loss = float(np.mean(ep[:, 0].double().numpy()))
        res["mean_l1"].append(mean_loss)
        print(f"End of epoch {epoch}, mean L1 loss={mean_loss:.6f}, "
              f"time={time.time() - epoch_st:.2f}s")

        if epoch % opt.save_every == 0 or epoch == opt.n_epoch:
            path = save_finetune_checkpoint(
                model, os.path.join(out_dir, f"epoch_adapter_{epoch:03d}.pth"))
            print(f"Checkpoint saved to {path}")
            res["checkpoints"].append(path)
            model.eval()
            save_dir = os.path.join(out_dir, f"val_{systime}_ep{epoch:03d}")
            os.makedirs(save_dir, exist_ok=True)
            res["psnr"][epoch] = []
            for i, (clean_u8, noisy_u8) in enumerate(zip(valid[0], valid[1])):
                clean_name = os.path.basename(valid[2][i]).split(".")[0]
                noisy_name = os.path.basename(valid[3][i]).split(".")[0]
                p8 = denoise(model, noisy_u8)
                c8 = torch.from_numpy(clean_u8).to(dev)
                c8 = c8.unsqueeze(0) if c8.dim() == 2 else c8.permute(2, 0, 1).contiguous()
                # finetune.py:165-173: mse == 0 -> 99.0
                psnr = 99.0 if torch.equal(p8, c8) else float(psnr_device(p8, c8).cpu())
                res["psnr"][epoch].append(psnr)
                print(f"Val ep{epoch} [{i + 1}/{len(valid[0])}] {noisy_name}: psnr={psnr:.2f} dB")
                if i == 0:
                    pred = p8.cpu().numpy()
                    vis = pred[0] if pred.shape[0] == 1 else np.transpose(pred, (1, 2, 0))
                    Image.fromarray(clean_u8).convert("L").save(
                        os.path.join(save_dir, f"{clean_name}_clean.png"))
                    Image.fromarray(noisy_u8).convert("L").save(
                        os.path.join(save_dir, f"{noisy_name}_noisy.png"))
                    Image.fromarray(vis).convert("L").save(
                        os.path.join(save_dir, f"{noisy_name}_denoised_ep{epoch:03d}.png"))
    print("Finetuning complete.")
    return res


if __name__ == "__main__":
    main()
