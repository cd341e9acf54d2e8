"""Probe of the guarded optimizer step (csrc/guard.hip).  Its output is
profiles/guarded_adam_ops.txt.

    python tools/probes/guarded_adam_ops.py [out.txt]

(i)   dn_adam_step_guarded (norm + decision + Adam, three launches) against dn_adam_step (one
      launch) and dn_grad_norm alone at n = 1,256,689 (the UNet's flat buffer) and n = 449 (the
      adapter's): HIP events around each call, median of 50 after 10 warm-ups, the two optimizers
      alternating call by call on the same box.  A second figure times 50 back-to-back calls
      between one pair of events (what a step sees: launches queued behind each other).
(ii)  one SupervisedTrainer('l1') step of UNet(48) at 64 x 1 x 256^2 with and without
      GradGuard(), alternating, median of 20 after 5 warm-ups.
"""
from __future__ import annotations

import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from image_denoising_amd import _lib  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.optim import FlatAdam, GradGuard  # noqa: E402
from image_denoising_amd.trainer import SupervisedTrainer  # noqa: E402

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


def back_to_back(fn, calls: int = 50) -> float:
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def optimizers(n: int):
    g = torch.Generator().manual_seed(0)
    p0 = (torch.randn(n, generator=g) * 0.05).to(DEV)
    grad = torch.randn(n, generator=g)
    grad = (grad / grad.norm() * 0.5).to(DEV)  # below the clip: every guarded step applies
    loss = torch.full((1,), 0.3, device=DEV)
    plain = FlatAdam(p0.clone())
    guarded = FlatAdam(p0.clone(), guard=GradGuard())
    state = guarded.guard_state()
    stream = _lib.stream_of(p0)

    def norm_only():
        _lib.call("dn_grad_norm", _lib.ptr(grad), n, 1.0, state.data_ptr(), None, stream)

    return {"dn_adam_step": lambda: plain.step(grad),
            "dn_adam_step_guarded": lambda: guarded.step(grad, loss=loss),
            "dn_grad_norm": norm_only}, guarded


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "guarded_adam_ops.txt")
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    say("# (i) ms per call: median of 50 single calls (HIP events, alternating) | 50 calls back to back")
    for n in (1256689, 449):
        fns, guarded = optimizers(n)
        med = alternating(fns, calls=50, warm=10)
        b2b = {k: back_to_back(fn) for k, fn in fns.items()}
        s = guarded.guard_stats()
        say(f"n = {n}: (guarded: applied {s['applied']}, skipped {s['skipped_loss'] + s['skipped_norm']})")
        for k in fns:
            say(f"  {k:22s}: {med[k]:.4f} | {b2b[k]:.4f} ms")
        say(f"  guarded / unguarded   : {med['dn_adam_step_guarded'] / med['dn_adam_step']:.2f}x | "
            f"{b2b['dn_adam_step_guarded'] / b2b['dn_adam_step']:.2f}x; added "
            f"{1e3 * (b2b['dn_adam_step_guarded'] - b2b['dn_adam_step']):.1f} us back to back")
    say("# (ii) SupervisedTrainer('l1') step, UNet(48), 64 x 1 x 256^2: median of 20 (alternating)")
    g = torch.Generator().manual_seed(1)
    clean = torch.rand(64, 1, 256, 256, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(64, 1, 256, 256, generator=g).to(DEV)).contiguous()
    trainers = {}
    for name, guard in (("unguarded", None), ("guarded", GradGuard())):
        torch.manual_seed(0)
        trainers[name] = SupervisedTrainer(UNet(1, 1, 48).to(DEV), "l1", guard=guard)
    med = alternating({k: (lambda t=t: t.train_step(clean, noisy)) for k, t in trainers.items()},
                      calls=20, warm=5)
    s = trainers["guarded"].guard_stats()
    say(f"  unguarded: {med['unguarded']:.3f} ms   guarded: {med['guarded']:.3f} ms   "
        f"difference {1e3 * (med['guarded'] - med['unguarded']):.0f} us "
        f"(guarded: applied {s['applied']}, skipped {s['skipped_loss'] + s['skipped_norm']})")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
