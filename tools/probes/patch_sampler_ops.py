"""Probe of the device patch sampler (csrc/patch_sample.hip, data.DevicePatchSampler, DESIGN.md
§19) against the loader the reference has (finetune.DenoisePatchDataset under a DataLoader).  Its
output is profiles/patch_sampler_ops.txt.

    python tools/probes/patch_sampler_ops.py [out.txt]

The set is five synthetic 704^2 pairs written as PNG to a temporary folder.
(i)   dn_patch_sample at 16 x 1 x 512^2, 4 x 1 x 128^2 and 64 x 1 x 256^2: HIP events around each
      call, median of 200 after 20 warm-ups, and 200 calls back to back inside one event pair
      (what a training loop sees).  Beside it the kernel's floor: 4 * N * C * ps^2 * 4 bytes (one
      read and one write per element, two pools) at the 8 TB/s HBM peak.
(ii)  batches per second at 16 x 1 x 512^2 with no consumer: DevicePatchSampler.batches against
      DenoisePatchDataset in a DataLoader(shuffle, num_workers=4, pin_memory=True) followed by
      the two .to(device) copies, as finetune.py:233-240, :278-279 has them.
(iii) one finetune epoch (frozen bf16 UNet(48) base + adapter, 20 steps of 16 x 1 x 512^2) fed by
      each loader, beside 20 x the step time on resident tensors.
"""
from __future__ import annotations

import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from image_denoising_amd import _lib  # noqa: E402
from image_denoising_amd.adapter import DenoiserWithAdapter  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.data import DevicePatchSampler  # noqa: E402
from image_denoising_amd.finetune import DenoisePatchDataset, FinetuneTrainer  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)
LINES = []


def say(s: str) -> None:
    print(s, flush=True)
    LINES.append(s)


def write_pairs(root: str) -> None:
    from PIL import Image

    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, 704), np.linspace(0, 1, 704), indexing="ij")
    for d in ("clean", "noise"):
        os.makedirs(os.path.join(root, d))
    for i in range(5):
        c = np.clip(128 + 90 * np.sin(7 * xx + 5 * yy + i), 0, 255).astype(np.uint8)
        n = np.clip(c.astype(int) + rng.integers(-25, 26, c.shape), 0, 255).astype(np.uint8)
        Image.fromarray(c).save(os.path.join(root, "clean", f"img{i}.png"))
        Image.fromarray(n).save(os.path.join(root, "noise", f"img{i}.png"))


def kernel_times(root: str) -> None:
    say("# (i) dn_patch_sample, five 704^2 pairs resident (2 x 9.9 MB): us per call")
    say("#     single = median of 200 calls, one HIP event pair each; chained = 200 calls in one pair")
    say("#     launch = the chained figure of a one-workgroup call (1 x 1 x 4^2) in the same run")
    launch = None
    for N, ps in ((1, 4), (16, 512), (4, 128), (64, 256)):
        s = DevicePatchSampler.from_dir(root, ps, 16, seed=1, device=DEV)
        idx = torch.randint(0, 5, (N,), dtype=torch.int32).to(DEV)
        clean = torch.empty((N, 1, ps, ps), device=DEV)
        noisy = torch.empty_like(clean)
        run = lambda k=0: s._launch(idx, N, 1, k * N, None, clean, noisy, None)  # noqa: E731
        for k in range(20):
            run(k)
        torch.cuda.synchronize()
        single = []
        for k in range(200):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(k)
            b.record()
            b.synchronize()
            single.append(a.elapsed_time(b) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(200):
            run(k)
        b.record()
        b.synchronize()
        chained = a.elapsed_time(b) * 1e3 / 200
        nbytes = 4 * N * ps * ps * 4
        floor = nbytes / HBM_PEAK * 1e6
        us = statistics.median(single)
        if launch is None:
            launch = chained
            say(f"  1 x 1 x 4^2: single {us:7.2f} us, chained {chained:7.2f} us  (the launch)")
            continue
        # within 2x of a floor: that floor limits it; else neither does
        if floor >= launch and chained <= 2 * floor:
            bound = "limited by the bytes"
        elif chained <= 2 * launch:
            bound = "limited by the launch"
        else:
            bound = (f"{chained / max(floor, launch):.1f} x the larger floor: neither the bytes "
                     "nor the launch (the per-quad index arithmetic, DESIGN.md §19)")
        say(f"{N:3d} x 1 x {ps}^2: single {us:7.2f} us, chained {chained:7.2f} us; "
            f"{nbytes / 1e6:6.2f} MB -> floor {floor:6.2f} us at 8 TB/s; chained = "
            f"{nbytes / chained / 1e6:5.2f} TB/s; {bound}")


def host_loader(root: str, ps: int, ppi: int, batch: int):
    ds = DenoisePatchDataset(root, patch_size=ps, patches_per_image=ppi)
    return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True, num_workers=4,
                                       pin_memory=True, drop_last=False)


def host_batches(loader):
    for clean, noisy in loader:
        yield clean.to(DEV), noisy.to(DEV)


def wall(fn) -> float:
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def loader_rates(root: str, ps: int, ppi: int, batch: int):
    s = DevicePatchSampler.from_dir(root, ps, ppi, seed=1, device=DEV)
    steps = s.steps_per_epoch(batch)
    say(f"# (ii) batches per second, {batch} x 1 x {ps}^2, {steps} batches per epoch, no consumer")

    def drain(it):
        for _ in it:
            pass

    drain(s.batches(0, batch))
    t_dev = statistics.median(wall(lambda e=e: drain(s.batches(e, batch))) for e in range(1, 6))
    loader = host_loader(root, ps, ppi, batch)
    drain(host_batches(loader))
    t_host = statistics.median(wall(lambda: drain(host_batches(loader))) for _ in range(3))
    say(f"  DevicePatchSampler.batches                      : {steps / t_dev:10.0f} batches/s "
        f"({t_dev / steps * 1e3:.4f} ms per batch, median of 5 epochs)")
    say(f"  DenoisePatchDataset + DataLoader(4 workers) + .to: {steps / t_host:10.1f} batches/s "
        f"({t_host / steps * 1e3:.1f} ms per batch, median of 3 epochs)")
    return s, loader, steps


def epoch_times(s, loader, steps: int, ps: int, batch: int) -> None:
    say(f"# (iii) finetune epoch, frozen bf16 UNet(48) base + adapter, {steps} steps of "
        f"{batch} x 1 x {ps}^2")
    torch.manual_seed(0)
    base = UNet(1, 1, 48).set_inference_precision("bf16")
    tr = FinetuneTrainer(DenoiserWithAdapter(base, 1, 16).to(DEV), lr=1e-4, lambda_grad=0.1,
                         distributed=False)
    g = torch.Generator().manual_seed(1)
    clean = torch.rand(batch, 1, ps, ps, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(batch, 1, ps, ps, generator=g).to(DEV)).contiguous()

    def resident():
        for _ in range(steps):
            tr.train_step(clean, noisy)

    def fed(it):
        for c, n in it:
            tr.train_step(c, n)

    resident()
    t_res = statistics.median(wall(resident) for _ in range(5))
    fed(s.batches(0, batch))
    t_dev = statistics.median(wall(lambda e=e: fed(s.batches(e, batch))) for e in range(1, 6))
    t_host = statistics.median(wall(lambda: fed(host_batches(loader))) for _ in range(3))
    say(f"  step on resident tensors        : {t_res / steps * 1e3:8.3f} ms  "
        f"(x {steps} = {t_res * 1e3:.1f} ms)")
    say(f"  epoch, device sampler           : {t_dev * 1e3:8.1f} ms = {t_dev / t_res:.3f} x the "
        f"steps alone ({(t_dev - t_res) / steps * 1e3:+.3f} ms per step)")
    say(f"  epoch, host loader (4 workers)  : {t_host * 1e3:8.1f} ms = {t_host / t_res:.2f} x the "
        f"steps alone")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "patch_sampler_ops.txt")
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    with tempfile.TemporaryDirectory() as root:
        write_pairs(root)
        kernel_times(root)
        s, loader, steps = loader_rates(root, 512, 64, 16)
        epoch_times(s, loader, steps, 512, 16)
    say("# one box, one run: figures move by a few per cent from box to box (README)")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
