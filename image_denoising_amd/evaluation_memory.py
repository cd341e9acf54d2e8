"""`python -m image_denoising_amd.evaluation_memory`: the reference's
evaluation_704_iqsl_memory.py (same flags, same per-image lines) on the HIP path: a base checkpoint,
a memory bank built from the first `--num_memory_images` clean/noise pairs, an adapter-only
checkpoint, patchwise whole-image inference with the Hann blend, PSNR on pred255 and the optional
3-class IQ-IoU.
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np
import torch

from .evaluation import _device, calculate_psnr, compute_iq_iou


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--base_ckpt", type=str, required=True)
    p.add_argument("--adapter_ckpt", type=str, required=True)
    p.add_argument("--arch", type=str, default="UNetImproved", choices=["UNet", "RESNET", "UNetImproved"])
    p.add_argument("--save_dir", type=str, default="./results_infer_adapter_memory")
    p.add_argument("--gpu_devices", default="0", type=str)
    p.add_argument("--parallel", action="store_true")
    p.add_argument("--n_feature", type=int, default=48)
    p.add_argument("--n_channel", type=int, default=1)
    p.add_argument("--adapter_hidden", type=int, default=16)
    p.add_argument("--patch_size", type=int, default=128)
    p.add_argument("--overlap", type=int, default=64)
    p.add_argument("--num_memory_images", type=int, default=5)
    p.add_argument("--memory_stride", type=int, default=64)
    p.add_argument("--compute_iq_iou", action="store_true")
    p.add_argument("--iq_low_q", type=float, default=0.25)
    p.add_argument("--iq_high_q", type=float, default=0.75)
    args, _ = p.parse_known_args(argv)
    return args


def main(argv=None, out=print):
    from PIL import Image

    from .checkpoint import load_adapter_checkpoint
    from .finetune import build_base_model, load_base_weights
    from .memory import DenoiserWithMemoryAdapter, build_memory_bank, denoise_full_image_patchwise

    opt = parse_args(argv)
    if opt.parallel:
        out("[Warning] --parallel: one process drives one GPU here; running on a single device.")
    dev = _device()
    noise_dir, clean_dir = os.path.join(opt.data_dir, "noise"), os.path.join(opt.data_dir, "clean")
    os.makedirs(opt.save_dir, exist_ok=True)
    noise_paths = sorted(glob.glob(os.path.join(noise_dir, "*")))
    if not noise_paths:
        raise RuntimeError(f"No files found in {noise_dir}")
    clean_paths = sorted(glob.glob(os.path.join(clean_dir, "*"))) if os.path.isdir(clean_dir) else []
    if not clean_paths:
        raise RuntimeError("Memory bank needs clean/ and noise/ pairs; clean/ not found.")
    if len(clean_paths) != len(noise_paths):
        out("[Warning] clean/ and noise/ have different counts; PSNR may be misaligned.")
    out(f"Found {len(noise_paths)} noisy images for inference.")
    base = build_base_model(opt.arch, opt.n_channel, opt.n_feature)
    load_base_weights(base, opt.base_ckpt)
    num_mem = min(opt.num_memory_images, len(clean_paths))
    bank = build_memory_bank(clean_paths[:num_mem], noise_paths[:num_mem], opt.patch_size,
                             opt.memory_stride, dev)
    model = DenoiserWithMemoryAdapter(base, opt.n_channel, opt.adapter_hidden, bank).to(dev)
    model.eval()
    missing, unexpected = load_adapter_checkpoint(model, opt.adapter_ckpt)
    if missing:
        out(f"[Warning] Missing keys when loading adapter: {missing}")
    if unexpected:
        out(f"[Warning] Unexpected keys when loading adapter: {unexpected}")
    out(f"Loaded adapter-only weights from {opt.adapter_ckpt}")
    psnrs, ious = [], []
    for idx, n_path in enumerate(noise_paths):
        name = os.path.basename(n_path)
        base_name = os.path.splitext(name)[0]
        noisy = np.array(Image.open(n_path), dtype=np.float32)
        _, pred255 = denoise_full_image_patchwise(model, noisy, opt.patch_size, opt.overlap,
                                                  device=dev, return_pred255=True)
        save_path = os.path.join(opt.save_dir, f"{base_name}_denoised_mem.png")
        Image.fromarray(pred255.squeeze(-1)).convert("L").save(save_path)
        if idx < len(clean_paths):
            clean = np.array(Image.open(clean_paths[idx]), dtype=np.float32).astype(np.uint8)
            ps = calculate_psnr(pred255.squeeze(-1), clean)
            psnrs.append(ps)
            msg = f"[{idx + 1:03d}/{len(noise_paths):03d}] {name} → PSNR={ps:.2f} dB, saved to {save_path}"
            if opt.compute_iq_iou:
                iou = compute_iq_iou(pred255.squeeze(-1), clean, opt.iq_low_q, opt.iq_high_q)
                ious.append(iou)
                msg += f", IoU(d/m/b)=({iou[0]:.3f},{iou[1]:.3f},{iou[2]:.3f})"
            out(msg)
        else:
            out(f"[{idx + 1:03d}/{len(noise_paths):03d}] {name} → saved to {save_path}")
    res = dict(psnr=psnrs)
    if opt.compute_iq_iou and ious:
        res["iq_iou"] = ious
        with np.errstate(all="ignore"):
            d, m, b = (float(v) for v in np.nanmean(np.array(ious, np.float64), axis=0))
        out(f"Average IQ-3class IoU - dark: {d:.4f}, mid: {m:.4f}, bright: {b:.4f}")
    out("Inference with memory adapter model finished.")
    return res


if __name__ == "__main__":
    main()
