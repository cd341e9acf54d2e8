"""Probe of the L1FFT loss (csrc/fft_loss.hip) and the supervised step.  Its output is
profiles/l1fft_ops.txt (--mixed: profiles/l1fft_mixed_ops.txt).

    python tools/probes/l1fft_ops.py [out.txt]
    python tools/probes/l1fft_ops.py --mixed [out.txt]     -> profiles/l1fft_mixed_ops.txt

--mixed runs part (i) and (ii) alone at the mixed-radix sizes 4 x 1 x 704^2 (whole images, the
batch of the reference's default log name) and 16 x 1 x 352^2 (the evaluation tiles).

(i)   dn_l1fft_loss at 64 x 1 x 256^2 and 16 x 1 x 512^2 against the same loss and gradient
      through torch.fft autograd on the same GPU, and dn_structure_loss at the same sizes as
      the elementwise floor: medians of 5 rounds of 20 calls after a warm-up, HIP events;
(ii)  bytes the launch sequence moves by construction against the algorithmic minimum (pred,
      target and dpred once each, the half-spectrum workspace written and read twice);
(iii) a SupervisedTrainer step against a StructureTrainer step at 64 x 1 x 256^2, UNet(48).
"""
from __future__ import annotations

import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from image_denoising_amd import _lib, util  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.trainer import StructureTrainer, SupervisedTrainer  # noqa: E402

DEV = torch.device("cuda:0")
LINES = []


def say(s: str) -> None:
    print(s, flush=True)
    LINES.append(s)


def timed(fn, calls: int = 20, rounds: int = 5, warm: int = 5):
    """ms per call: one figure per round (HIP events around `calls` back-to-back calls)"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def fmt(v):
    return " ".join(f"{x:.4f}" for x in v) + f"  (median {statistics.median(v):.4f})"


def torch_l1fft(pred, target):
    p = pred.detach().requires_grad_(True)
    loss = (p - target).abs().mean() + (torch.fft.fft2(p) - torch.fft.fft2(target)).abs().mean()
    loss.backward()
    return loss, p.grad


def main():
    args = [a for a in sys.argv[1:] if a != "--mixed"]
    mixed = "--mixed" in sys.argv[1:]
    g = torch.Generator().manual_seed(0)
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    say("# (i) loss + gradient, ms per call, 5 rounds of 20 calls (HIP events)")
    for N, HW in ((4, 704), (16, 352)) if mixed else ((64, 256), (16, 512)):
        pred = torch.rand(N, 1, HW, HW, generator=g).to(DEV)
        tgt = torch.rand(N, 1, HW, HW, generator=g).to(DEV)
        dp, dp2 = torch.empty_like(pred), torch.empty_like(pred)
        l3, l5 = torch.empty(3, device=DEV), torch.empty(5, device=DEV)
        _, gt = torch_l1fft(pred, tgt)
        util.l1fft_loss_into(pred, tgt, 1.0, 1.0, dp, l3)
        say(f"{N} x 1 x {HW}^2: max |dpred - torch| = {float((dp - gt).abs().max()):.3e} "
            f"(max |dpred| {float(gt.abs().max()):.3e})")
        t_hip = timed(lambda: util.l1fft_loss_into(pred, tgt, 1.0, 1.0, dp, l3))
        t_l1 = timed(lambda: util.l1fft_loss_into(pred, tgt, 1.0, 0.0, dp, l3))
        t_ref = timed(lambda: torch_l1fft(pred, tgt))
        t_st = timed(lambda: util.structure_loss_into(pred, pred, tgt, 1.0, .5, .5, dp, dp2, l5))
        elems = pred.numel()
        spec = N * HW * (HW // 2 + 1) * 8
        moved = 4 * elems * (2 + 2 + 1) + 4 * spec  # pred, target read by both row passes
        least = 4 * elems * 3 + 4 * spec
        m = statistics.median(t_hip)
        say(f"  dn_l1fft_loss            : {fmt(t_hip)} ms")
        say(f"  dn_l1fft_loss, beta = 0  : {fmt(t_l1)} ms")
        say(f"  torch.fft autograd       : {fmt(t_ref)} ms   ratio torch / HIP = "
            f"{statistics.median(t_ref) / m:.2f}x")
        say(f"  dn_structure_loss (floor): {fmt(t_st)} ms")
        say(f"  (ii) bytes by construction {moved / 1e6:.1f} MB ({moved / m / 1e6:.0f} GB/s at the "
            f"median), algorithmic minimum {least / 1e6:.1f} MB: {moved / least:.2f}x")
        del pred, tgt, dp, dp2, gt
        torch.cuda.empty_cache()

    if mixed:
        return write(args, "l1fft_mixed_ops.txt")
    say("# (iii) training step at 64 x 1 x 256^2, UNet(48), ms per step")
    clean = torch.rand(64, 1, 256, 256, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(64, 1, 256, 256, generator=g).to(DEV)).clamp(0, 1)
    for name, make in (("SupervisedTrainer l1fft", lambda n: SupervisedTrainer(n, "l1fft", distributed=False)),
                       ("SupervisedTrainer l1   ", lambda n: SupervisedTrainer(n, "l1", distributed=False)),
                       ("StructureTrainer       ", lambda n: StructureTrainer(n, distributed=False))):
        torch.manual_seed(0)
        tr = make(UNet(1, 1, 48).to(DEV))
        say(f"  {name}: {fmt(timed(lambda: tr.train_step(clean, noisy), calls=5, rounds=5, warm=3))} ms")
        del tr
        torch.cuda.empty_cache()
    write(args, "l1fft_ops.txt")


def write(args, default):
    out = args[0] if args else os.path.join(ROOT, "profiles", default)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
