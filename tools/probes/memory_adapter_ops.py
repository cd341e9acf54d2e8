"""Probe of the memory-bank adapter path at the reference's shipped setting (C = 1, P = 128, a bank
of 5 x 352^2 images at stride 4: N = 16,245 windows).  Its output is profiles/memory_adapter_ops.txt.

    python tools/probes/memory_adapter_ops.py [out.txt]

(i)   dn_memory_select against the reference's method on the same GPU (materialised bank,
      a^2 + b^2 - 2 (q @ bank.T), argmin, torch ops), at B = 4 (training) and B = 25 (one 352^2
      image at overlap 64): medians of 5 rounds of 20 calls after a warm-up, HIP events;
(ii)  the whole MemoryFinetuneTrainer step at 4 x 1 x 128^2 with a UNet(48) base, and its per-op
      breakdown (dn_profile_ops records plus event-timed select / gather);
(iii) (not here) fetched bytes come from a counters-only run of their own:
      rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -o run -- python <a script that only
      calls MemoryBank.select at B = 4 and B = 25 on the same bank>.
"""
from __future__ import annotations

import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from image_denoising_amd import _lib  # noqa: E402
from image_denoising_amd.arch_unet import UNet  # noqa: E402
from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer  # noqa: E402
from image_denoising_amd.memory import DenoiserWithMemoryAdapter, MemoryBank  # noqa: E402

DEV = torch.device("cuda:0")
P, S, HW, NIMG = 128, 4, 352, 5
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


def main():
    g = torch.Generator().manual_seed(0)
    clean = torch.rand(NIMG, 1, HW, HW, generator=g)
    noise = (clean + 0.1 * torch.randn(NIMG, 1, HW, HW, generator=g)).clamp(0, 1)
    bank = MemoryBank(noise.to(DEV), clean.to(DEV), P, S)
    N = len(bank)
    say(f"# {torch.cuda.get_device_name(0)}; {_lib.lib().dn_version().decode()}")
    say(f"# bank: {NIMG} x {HW}^2, P = {P}, stride {S}: N = {N} windows, D = {P * P}; "
        f"images {noise.numel() * 4 / 1e6:.2f} MB, materialised bank {N * P * P * 4 / 1e9:.3f} GB")
    say("# (i) selection, ms per call, 5 rounds of 20 calls (HIP events)")
    mat = bank.noise_patches()  # [N,1,P,P], what the reference keeps as a buffer
    mem_flat = mat.reshape(N, -1)
    for B in (4, 25):
        q = torch.rand(B, 1, P, P, generator=g).to(DEV)

        def ref():
            qf = q.reshape(B, -1)
            a2 = qf.pow(2).sum(dim=1, keepdim=True)
            b2 = mem_flat.pow(2).sum(dim=1, keepdim=True).t()
            return (a2 + b2 - 2.0 * (qf @ mem_flat.t())).argmin(dim=1)

        agree = int((ref() == bank.select(q)).sum())
        t_hip = timed(lambda: bank.select(q))
        t_ref = timed(ref)
        gf = 2.0 * B * N * P * P / 1e9  # GFLOP; per ms = TFLOP/s
        say(f"B={B:2d} dn_memory_select           : {fmt(t_hip)} ms   {gf / statistics.median(t_hip):.0f} TFLOP/s")
        say(f"B={B:2d} torch materialised a2+b2-2ab: {fmt(t_ref)} ms   indices agree {agree}/{B}")
        say(f"B={B:2d} ratio torch / HIP = {statistics.median(t_ref) / statistics.median(t_hip):.2f}x")
    del mat, mem_flat
    torch.cuda.empty_cache()

    say("# (ii) MemoryFinetuneTrainer step, 4 x 1 x 128^2, UNet(48) base (fp32_x6), lambda_iqsl = 0.1")
    torch.manual_seed(0)
    model = DenoiserWithMemoryAdapter(UNet(1, 1, 48), 1, 16, bank).to(DEV)
    with torch.no_grad():  # a non-zero adapter, so that no gradient path is trivially empty
        model.adapter.flat_params.copy_(0.05 * torch.randn(model.adapter.flat_params.shape, generator=g))
    tr = MemoryFinetuneTrainer(model, lr=1e-4, lambda_grad=0.1, lambda_iqsl=0.1, iqsl=dict(t1=0.3, t2=0.7))
    cl = torch.rand(4, 1, P, P, generator=g).to(DEV)
    no = (cl + 0.1 * torch.randn(4, 1, P, P, generator=g).to(DEV)).clamp(0, 1)
    say(f"step: {fmt(timed(lambda: tr.train_step(cl, no)))} ms/step")
    ad = model.adapter
    base_out, pred = torch.empty_like(no), torch.empty_like(no)
    tr._base_forward(no, base_out)
    idx = bank.select(no)
    mem = bank.gather_clean(idx)
    feat = ad._run_forward(no, base_out, mem, pred)
    dflat = torch.empty_like(ad.flat_params)
    dpred = torch.rand_like(pred) - 0.5
    say(f"  base forward          : {fmt(timed(lambda: tr._base_forward(no, base_out)))} ms")
    say(f"  dn_memory_select      : {fmt(timed(lambda: bank.select(no)))} ms")
    say(f"  dn_memory_gather      : {fmt(timed(lambda: bank.gather_clean(idx)))} ms")
    say(f"  dn_memadapter_forward : {fmt(timed(lambda: ad._run_forward(no, base_out, mem, pred)))} ms")
    say(f"  dn_memadapter_backward: {fmt(timed(lambda: ad._run_backward(no, base_out, feat, dpred, dflat)))} ms")
    say(f"  FlatAdam              : {fmt(timed(lambda: tr.opt.step(dflat)))} ms")
    _lib.profile_ops(True)
    for _ in range(3):
        tr.train_step(cl, no)
    recs = _lib.profile_ops_take()
    _lib.profile_ops(False)
    agg = {}
    for r in recs:
        agg.setdefault(r["op"], []).append(r["ms"])
    say("  dn_profile_ops records of 3 single-stream steps (op: launches, ms per step):")
    for op, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        say(f"    {op:16s} {len(v) // 3:3d}  {sum(v) / 3:.4f}")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
