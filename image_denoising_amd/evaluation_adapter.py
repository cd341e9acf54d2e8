"""evaluation_adapter.py / evaluation_adapter_iqsl.py on the HIP path: inference of a
DenoiserWithAdapter (frozen base + OutputAdapter, adapter.py:29-67) over <data_dir>/noise/*, saving
<name>_denoised.png and, when <data_dir>/clean/ exists, printing each image's PSNR
(evaluation_adapter.py:63-166) and, with --compute_iq_iou, its 3-class intensity-quantised IoU
and the nanmean averages (evaluation_adapter_iqsl.py:245-273).

    python -m image_denoising_amd.evaluation_adapter --data_dir D --ckpt X.pth [--arch UNet]
    python -m image_denoising_amd.evaluation_adapter --data_dir D --base_ckpt B.pth \
        --adapter_ckpt epoch_adapter_only_020.pth [--compute_iq_iou]

--ckpt is one file with `base.*` and `adapter.*` keys (finetune.py's checkpoint); --base_ckpt +
--adapter_ckpt pair the base's own checkpoint with the adapter-only file finetune_iqsl.py writes.

The base runs on the HIP executors (UNet or ImprovedUNet), the adapter on dn_adapter_forward;
quantisation (clip(x*255 + 0.5) -> uint8), PSNR and the IoU counts on device (dn_quantize_u8,
dn_psnr_u8, dn_iq_iou_u8).
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np
import torch

from . import _lib
from .evaluation import _device, compute_iq_iou, psnr_device


def parse_args(argv=None):
    """evaluation_adapter.py:17-43, evaluation_adapter_iqsl.py:17-62 (parse_known_args: unknown
    options are ignored there too)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", type=str, required=True)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--base_ckpt", type=str, default=None)
    ap.add_argument("--adapter_ckpt", type=str, default=None)
    ap.add_argument("--arch", type=str, default="UNetImproved", choices=["UNet", "RESNET", "UNetImproved"])
    ap.add_argument("--save_dir", type=str, default="./results_infer_adapter")
    ap.add_argument("--gpu_devices", default="0", type=str)
    ap.add_argument("--parallel", action="store_true")  # one GPU per process here: ignored
    ap.add_argument("--n_feature", type=int, default=48)
    ap.add_argument("--n_channel", type=int, default=1)
    ap.add_argument("--adapter_hidden", type=int, default=16)
    ap.add_argument("--compute_iq_iou", action="store_true")
    ap.add_argument("--iq_low_q", type=float, default=0.25)
    ap.add_argument("--iq_high_q", type=float, default=0.75)
    args, _ = ap.parse_known_args(argv)
    paired = args.base_ckpt is not None or args.adapter_ckpt is not None
    if paired and (args.ckpt is not None or args.base_ckpt is None or args.adapter_ckpt is None):
        ap.error("give either --ckpt, or --base_ckpt together with --adapter_ckpt")
    if not paired and args.ckpt is None:
        ap.error("one of --ckpt or --base_ckpt/--adapter_ckpt is required")
    return args


def build_model(arch: str, n_channel: int, n_feature: int, hidden: int):
    """evaluation_adapter.py:46-55 + :114-121"""
    from .adapter import DenoiserWithAdapter
    from .finetune import build_base_model

    base = build_base_model(arch, n_channel, n_feature)
    return DenoiserWithAdapter(base, in_channels=n_channel, hidden_channels=hidden,
                               freeze_base=True, use_no_grad_for_base=True)


def load_adapter_weights(model, ckpt_path: str):
    """evaluation_adapter.py:58-68: strip a DataParallel 'module.' prefix, load non-strict"""
    from .checkpoint import read_state_dict

    missing, unexpected = model.load_state_dict(read_state_dict(ckpt_path), strict=False)
    if missing:
        print(f"[Warning] Missing keys when loading adapter model: {missing}")
    if unexpected:
        print(f"[Warning] Unexpected keys when loading adapter model: {unexpected}")
    print(f"Loaded adapter+base weights from {ckpt_path}")


def load_base_and_adapter(model, base_ckpt: str, adapter_ckpt: str):
    """evaluation_adapter_iqsl.py:76-108: the base's checkpoint into model.base (non-strict,
    'module.' prefix stripped), then the adapter-only state into model.adapter (non-strict)"""
    from .checkpoint import load_adapter_checkpoint, load_checkpoint

    missing, unexpected = load_checkpoint(model.base, base_ckpt, strict=False)
    if missing:
        print(f"[Warning] Missing keys when loading base model: {missing}")
    if unexpected:
        print(f"[Warning] Unexpected keys when loading base model: {unexpected}")
    print(f"Loaded base weights from {base_ckpt}")
    missing, unexpected = load_adapter_checkpoint(model, adapter_ckpt)
    if missing:
        print(f"[Warning] Missing keys when loading adapter: {missing}")
    if unexpected:
        print(f"[Warning] Unexpected keys when loading adapter: {unexpected}")
    print(f"Loaded adapter-only weights from {adapter_ckpt}")


@torch.no_grad()
def denoise(model, noisy_u8: np.ndarray):
    """evaluation_adapter.py:133-145: [H,W(,C)] uint8 -> pred255 uint8 on device [C,H,W]"""
    dev = _device()
    x8 = torch.from_numpy(np.ascontiguousarray(noisy_u8)).to(dev)
    x8 = x8.unsqueeze(0) if x8.dim() == 2 else x8.permute(2, 0, 1).contiguous()
    C, H, W = x8.shape
    x = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
    _lib.call("dn_u8_to_unit", _lib.ptr(x8), x8.numel(), _lib.ptr(x), _lib.stream_of(x))
    pred = model(x).contiguous()
    p8 = torch.empty((C, H, W), dtype=torch.uint8, device=dev)
    _lib.call("dn_quantize_u8", _lib.ptr(pred), pred.numel(), 1, _lib.ptr(p8), _lib.stream_of(pred))
    return p8


def main(argv=None):
    from PIL import Image

    opt = parse_args(argv)
    noise_paths = sorted(glob.glob(os.path.join(opt.data_dir, "noise", "*")))
    if not noise_paths:
        raise RuntimeError(f"No files found in {os.path.join(opt.data_dir, 'noise')}")
    clean_dir = os.path.join(opt.data_dir, "clean")
    clean_paths = sorted(glob.glob(os.path.join(clean_dir, "*"))) if os.path.isdir(clean_dir) else []
    has_clean = len(clean_paths) > 0
    if has_clean and len(clean_paths) != len(noise_paths):
        print("[Warning] clean/ and noise/ have different counts; PSNR may be misaligned.")
    os.makedirs(opt.save_dir, exist_ok=True)
    print(f"Found {len(noise_paths)} noisy images for inference.")
    model = build_model(opt.arch, opt.n_channel, opt.n_feature, opt.adapter_hidden).to(_device())
    model.eval()
    if opt.ckpt is not None:
        load_adapter_weights(model, opt.ckpt)
    else:
        load_base_and_adapter(model, opt.base_ckpt, opt.adapter_ckpt)
    psnrs, ious = [], []
    for idx, n_path in enumerate(noise_paths):
        name = os.path.basename(n_path)
        base_name = os.path.splitext(name)[0]
        noisy = np.array(Image.open(n_path), dtype=np.float32).astype(np.uint8)
        p8 = denoise(model, noisy)
        out = p8.cpu().numpy()
        img = Image.fromarray(out[0]).convert("L") if out.shape[0] == 1 else \
            Image.fromarray(np.transpose(out, (1, 2, 0))).convert("RGB")
        save_path = os.path.join(opt.save_dir, f"{base_name}_denoised.png")
        img.save(save_path)
        if has_clean and idx < len(clean_paths):
            clean = np.array(Image.open(clean_paths[idx]), dtype=np.float32).astype(np.uint8)
            c8 = torch.from_numpy(clean).to(p8.device)
            c8 = c8.unsqueeze(0) if c8.dim() == 2 else c8.permute(2, 0, 1).contiguous()
            # evaluation_adapter.py:75-83: mse == 0 -> 99.0
            ps = 99.0 if torch.equal(p8, c8) else float(psnr_device(p8, c8).cpu())
            psnrs.append(ps)
            msg = f"[{idx + 1:03d}/{len(noise_paths):03d}] {name} → PSNR={ps:.2f} dB, saved to {save_path}"
            if opt.compute_iq_iou:
                pred_hw = out[0] if out.shape[0] == 1 else np.transpose(out, (1, 2, 0))
                iou = compute_iq_iou(pred_hw, clean, opt.iq_low_q, opt.iq_high_q)
                ious.append(iou)
                msg += f", IoU(d/m/b)=({iou[0]:.3f},{iou[1]:.3f},{iou[2]:.3f})"
            print(msg)
        else:
            print(f"[{idx + 1:03d}/{len(noise_paths):03d}] {name} → saved to {save_path}")
    res = dict(psnr=psnrs)
    if opt.compute_iq_iou and ious:
        res["iq_iou"] = ious
        with np.errstate(all="ignore"):
            res["avg_iq_iou"] = [float(v) for v in np.nanmean(np.array(ious, np.float64), axis=0)]
        d, m, b = res["avg_iq_iou"]
        print(f"Average IQ-3class IoU - dark: {d:.4f}, mid: {m:.4f}, bright: {b:.4f}")
    print("Inference with adapter model finished.")
    return res


if __name__ == "__main__":
    main()
