"""Probe of the adapter's input gradient (csrc/adapter.hip k_adapter_dinput) and of
the joint finetune step built on it.  Its output is profiles/adapter_dinput_ops.txt.

    python tools/probes/adapter_dinput_ops.py [out.txt]

(i)   dn_adapter_backward_input at 16 x 1 x 512^2 and 16 x 3 x 512^2, with and without dnoisy:
      HIP events around each call, median of 50 after 10 warm-ups, the variants taking turns call
      by call; the achieved share of the HBM peak (8 TB/s) from the 16 C / 20 C bytes per pixel
      the kernel has to move.  Beside it torch.autograd.grad through the same adapter built from
      nn.Conv2d (base_out alone / base_out and noisy), on the same box in the same turn order.
(ii)  the joint FinetuneTrainer step at 16 x 1 x 512^2 with a UNet(48) base in 'fp32' and
      'fp32_x6', and the frozen step (its default forward arithmetic) beside it, median of 20
      after 5 warm-ups, alternating.
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
from image_denoising_amd.adapter import DenoiserWithAdapter, OutputAdapter  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.finetune import FinetuneTrainer  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)
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


def kernel_case(N, C, S):
    g = torch.Generator().manual_seed(C)
    torch.manual_seed(0)
    ad = OutputAdapter(C, 16).to(DEV)
    noisy, base, dout = (torch.randn(N, C, S, S, generator=g).to(DEV) for _ in range(3))
    dbase, dnoisy = torch.empty_like(base), torch.empty_like(base)
    net = nn.Sequential(nn.Conv2d(2 * C, 16, 3, padding=1), nn.ReLU(inplace=True),
                        nn.Conv2d(16, C, 3, padding=1)).to(DEV)
    with torch.no_grad():
        for p, q in zip(net.parameters(), ad.parameters()):
            p.copy_(q)
            p.requires_grad_(False)

    def torch_grad(with_noisy):
        b = base.detach().requires_grad_(True)
        n = noisy.detach().requires_grad_(with_noisy)
        out = b + net(torch.cat([n, b], 1))
        return torch.autograd.grad(out, [b, n] if with_noisy else [b], dout)

    return {"dn_adapter_backward_input (dbase)":
            lambda: ad._run_backward_input(noisy, base, dout, dbase, None),
            "dn_adapter_backward_input (dbase, dnoisy)":
            lambda: ad._run_backward_input(noisy, base, dout, dbase, dnoisy),
            "torch fwd + autograd.grad (dbase)": lambda: torch_grad(False),
            "torch fwd + autograd.grad (dbase, dnoisy)": lambda: torch_grad(True)}


def trainer(prec, freeze):
    torch.manual_seed(0)
    base = UNet(1, 1, 48).set_precision(prec)
    torch.manual_seed(1)
    m = DenoiserWithAdapter(base, 1, 16, freeze_base=freeze, use_no_grad_for_base=freeze).to(DEV)
    return FinetuneTrainer(m, lr=1e-4, lambda_grad=0.1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adapter_dinput_ops.txt")
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    say("# (i) ms per call, median of 50 single calls (HIP events, alternating); HBM share of 8 TB/s")
    say("#     (the torch rows also run the adapter's forward, which autograd needs)")
    N, S = 16, 512
    for C in (1, 3):
        med = alternating(kernel_case(N, C, S), calls=50, warm=10)
        say(f"{N} x {C} x {S}^2:")
        for k, ms in med.items():
            extra = ""
            if k.startswith("dn_"):
                bpp = (20 if "dnoisy" in k else 16) * C
                bw = bpp * N * S * S / (ms * 1e-3)
                extra = f"   {bw / 1e12:.2f} TB/s = {100 * bw / HBM_PEAK:.0f}% of the HBM peak"
            say(f"  {k:44s}: {ms:.4f} ms{extra}")
        for tail in ("(dbase)", "(dbase, dnoisy)"):
            say(f"  torch / HIP {tail:17s}: "
                f"{med['torch fwd + autograd.grad ' + tail] / med['dn_adapter_backward_input ' + tail]:.1f}x")
    say("# (ii) FinetuneTrainer step, UNet(48) base, 16 x 1 x 512^2: median of 20 (alternating)")
    g = torch.Generator().manual_seed(1)
    clean = torch.rand(N, 1, S, S, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(N, 1, S, S, generator=g).to(DEV)).contiguous()
    trs = {"joint fp32": trainer("fp32", False), "joint fp32_x6": trainer("fp32_x6", False),
           "frozen": trainer("fp32", True)}
    med = alternating({k: (lambda t=t: t.train_step(clean, noisy)) for k, t in trs.items()},
                      calls=20, warm=5)
    for k, ms in med.items():
        say(f"  {k:14s}: {ms:.3f} ms")
    say("# one box, one run: figures move by a few per cent from box to box (README)")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
