"""Probe of the memory-bank adapter's input gradient (csrc/memory.hip) and of the
joint MemoryFinetuneTrainer step built on it.  Its output is profiles/memadapter_dinput_ops.txt.

    python tools/probes/memadapter_dinput_ops.py [out.txt]

(i)   at 4 x 1 x 128^2 and 16 x 1 x 512^2: dn_memadapter_backward_input with dparams against
      dn_memadapter_backward (the difference is the cost of the input gradient), the same call
      with dparams null, the hyper adjoint alone (dn_memadapter_feature_adjoint), and torch's
      forward + autograd.grad w.r.t. base_out through the same adapter written with nn.Conv2d,
      torch.fft.rfft and nn.Linear.  HIP events around each call, median of 50 after 10 warm-ups,
      the variants taking turns call by call.
(ii)  the MemoryFinetuneTrainer step at 4 x 1 x 128^2 with a UNet(48) base: joint 'fp32_x6' and
      'fp32' beside the frozen step, median of 20 after 5 warm-ups, alternating.
"""
from __future__ import annotations

import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from image_denoising_amd import _lib  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer  # noqa: E402
from image_denoising_amd.memory import (DenoiserWithMemoryAdapter,  # noqa: E402
                                        HyperGatedResidualAdapter_FFT, MemoryBank)

DEV = torch.device("cuda:0")
LINES = []


def say(s: str) -> None:
    print(s, flush=True)
    LINES.append(s)


def one_call_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns: dict, calls: int, warm: int) -> dict:
    """median ms per call of each fn, the fns taking turns call by call"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            times[k].append(one_call_ms(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def randomise(ad):
    """non-zero parameters: at the reference initialisation two of the three routes are dead"""
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ad.flat_params.copy_(((torch.rand(ad.flat_params.numel(), generator=g) - 0.5) * 0.2)
                             .to(ad.flat_params.device))


class TorchAdapter(nn.Module):
    """the same adapter in stock torch modules (C = 1, hidden 16, three bands)"""

    def __init__(self, ad):
        super().__init__()
        self.c1, self.c2 = nn.Conv2d(2, 16, 3, padding=1), nn.Conv2d(16, 16, 3, padding=1)
        self.c3 = nn.Conv2d(16, 1, 3, padding=1)
        self.l1, self.l2 = nn.Linear(15, 16), nn.Linear(16, 2)
        with torch.no_grad():
            for p, q in zip(self.parameters(), ad.parameters()):
                p.copy_(q)
                p.requires_grad_(False)

    @staticmethod
    def bands(x):
        B, C, H, W = x.shape
        sp = torch.fft.rfft(x.reshape(B, C * H, W), dim=-1)
        pw = (sp.real ** 2 + sp.imag ** 2).mean(1)
        F = pw.shape[-1]
        bs = F // 3
        f = torch.log1p(torch.stack([pw[:, :bs].mean(-1), pw[:, bs:2 * bs].mean(-1),
                                     pw[:, 2 * bs:].mean(-1)], 1))
        return f / (f.mean(1, keepdim=True) + 1e-6)

    def forward(self, noisy, base, mem):
        st = []
        for t in (noisy, base, mem):
            v = t.flatten(1)
            st += [v.mean(1), v.std(1)]
        feat = torch.cat([torch.stack(st, 1)] + [self.bands(t) for t in (noisy, base, mem)], 1)
        hy = self.l2(torch.relu(self.l1(feat)))
        gamma = torch.sigmoid(hy[:, :1])[:, :, None, None]
        beta = (0.1 * torch.tanh(hy[:, 1:]))[:, :, None, None]
        r = self.c3(torch.relu(self.c2(torch.relu(self.c1(torch.cat([noisy, base], 1))))))
        return (base + gamma * r + beta).clamp(0, 1)


def kernel_case(N, S):
    g = torch.Generator().manual_seed(N)
    ad = HyperGatedResidualAdapter_FFT(1, 16, 3, True).to(DEV)
    randomise(ad)
    noisy, base, mem = (torch.rand(N, 1, S, S, generator=g).to(DEV) for _ in range(3))
    dout = torch.randn(N, 1, S, S, generator=g).to(DEV)
    feat = ad._run_forward(noisy, base, mem, torch.empty_like(base))
    dflat, dbase = torch.empty_like(ad.flat_params), torch.empty_like(base)
    dfeat = torch.randn(N, 5, generator=g).to(DEV)
    tad = TorchAdapter(ad).to(DEV)

    def torch_grad():
        b = base.detach().requires_grad_(True)
        return torch.autograd.grad(tad(noisy, b, mem), [b], dout)

    got = torch_grad()[0]
    ad._run_backward_input(noisy, base, feat, dout, None, dbase)
    err = float((got - dbase).abs().max() / got.abs().max())
    return err, {"dn_memadapter_backward (dparams)":
                 lambda: ad._run_backward(noisy, base, feat, dout, dflat),
                 "dn_memadapter_backward_input (dparams, dbase)":
                 lambda: ad._run_backward_input(noisy, base, feat, dout, dflat, dbase),
                 "dn_memadapter_backward_input (dbase)":
                 lambda: ad._run_backward_input(noisy, base, feat, dout, None, dbase),
                 "dn_memadapter_feature_adjoint (hyper alone)":
                 lambda: ad._feature_adjoint(base, dfeat),
                 "torch fwd + autograd.grad (dbase)": torch_grad}


def trainer(prec, freeze, S):
    g = torch.Generator().manual_seed(2)
    noise = torch.rand(2, 1, S + 32, S + 32, generator=g)
    bank = MemoryBank(noise.to(DEV), (noise * 0.8 + 0.1).to(DEV), S, 4)
    torch.manual_seed(0)
    base = UNet(1, 1, 48).set_precision(prec)
    m = DenoiserWithMemoryAdapter(base, 1, 16, bank, freeze_base=freeze,
                                  use_no_grad_for_base=freeze).to(DEV)
    randomise(m.adapter)
    return MemoryFinetuneTrainer(m, lr=1e-4, lambda_grad=0.1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                             "memadapter_dinput_ops.txt")
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    say("# (i) ms per call, median of 50 single calls (HIP events, alternating)")
    say("#     (the torch row also runs the adapter's forward, which autograd needs; the")
    say("#      feature-adjoint row includes its scratch allocation)")
    for N, S in ((4, 128), (16, 512)):
        err, fns = kernel_case(N, S)
        med = alternating(fns, calls=50, warm=10)
        say(f"{N} x 1 x {S}^2:   (HIP dbase vs torch fp32 autograd: {err:.1e} of the maximum)")
        for k, ms in med.items():
            say(f"  {k:48s}: {ms:.4f} ms")
        both = med["dn_memadapter_backward_input (dparams, dbase)"]
        say(f"  input gradient's cost over dn_memadapter_backward : "
            f"{both - med['dn_memadapter_backward (dparams)']:.4f} ms")
        say(f"  torch / HIP (dbase)                               : "
            f"{med['torch fwd + autograd.grad (dbase)'] / med['dn_memadapter_backward_input (dbase)']:.2f}x")
    say("# (ii) MemoryFinetuneTrainer step, UNet(48) base, 4 x 1 x 128^2: median of 20 (alternating)")
    N, S = 4, 128
    g = torch.Generator().manual_seed(1)
    clean = torch.rand(N, 1, S, S, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(N, 1, S, S, generator=g).to(DEV)).contiguous()
    trs = {"joint fp32_x6": trainer("fp32_x6", False, S), "joint fp32": trainer("fp32", False, S),
           "frozen": trainer("fp32", True, S)}
    med = alternating({k: (lambda t=t: t.train_step(clean, noisy)) for k, t in trs.items()},
                      calls=20, warm=5)
    for k, ms in med.items():
        say(f"  {k:14s}: {ms:.3f} ms")
    say("# one box, one run: figures move by a few per cent from box to box (README)")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
