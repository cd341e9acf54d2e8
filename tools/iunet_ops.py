"""Per-op view of ImprovedUNet passes from the launch profiler (dn_profile_ops).

    python tools/iunet_ops.py [bs] [--prec fp32|fp32_x6]
        one forward + backward at bs x 1 x 128 x 128 (after a warm-up pass): ms, TF/s and count
        per op and shape, sorted by time
    python tools/iunet_ops.py --dump
        for both precisions and three small shapes: every launch record of a forward and a
        backward in order (op, kernel, K, NOUT, H, W, N; no times) and the SHA-256 of y and of
        the flat gradient -- two builds that print the same text issue the same launches and
        compute the same bits
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from image_denoising_amd import _lib  # noqa: E402
from image_denoising_amd.improved_unet import ImprovedUNet  # noqa: E402

DUMP_SHAPES = [(1, 1, 32, 48), (2, 3, 32, 128), (8, 1, 128, 128)]


def profiled_step(net, x, dy):
    """forward + backward under the launch profiler -> (y, flat gradient, launch records)"""
    N, _, H, W = x.shape
    ws = net._workspace(N, H, W, True, fresh=True)
    y = torch.empty(N, net.out_nc, H, W, device=x.device)
    g = torch.empty_like(net.flat_params)
    _lib.profile_ops(True)
    try:
        net._run_forward(x, y, ws)
        net._run_backward(dy, g, ws, N, H, W)
        recs = _lib.profile_ops_take()
    finally:
        _lib.profile_ops(False)
    return y, g, recs


def table(recs):
    agg = {}
    for r in recs:
        key = f"{r['op']:<7s} {r['NOUT']}x{r['K']} @{r['H']}x{r['W']}"
        a = agg.setdefault(key, [0.0, 0.0, 0])
        a[0] += r["ms"]
        a[1] += r["flops"]
        a[2] += 1
    print(f"{sum(r['ms'] for r in recs):.3f} ms in {len(recs)} launches")
    for key, (ms, flops, n) in sorted(agg.items(), key=lambda kv: -kv[1][0]):
        print(f"  {ms:8.3f} ms  {flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0:7.1f} TF/s  x{n:<3d} {key}")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def dump():
    for prec in ("fp32", "fp32_x6"):
        for (N, C, H, W) in DUMP_SHAPES:
            torch.manual_seed(0)
            net = ImprovedUNet(C, C, 48).cuda().set_precision(prec)
            gen = torch.Generator().manual_seed(1)
            x = torch.rand(N, C, H, W, generator=gen).cuda()
            dy = torch.randn(N, C, H, W, generator=gen).cuda()
            y, g, recs = profiled_step(net, x, dy)
            print(f"== {prec} {N}x{C}x{H}x{W}: {len(recs)} launches")
            for r in recs:
                print(f"{r['op']} {r['kernel']} K={r['K']} NOUT={r['NOUT']} H={r['H']} W={r['W']} N={r['N']}")
            print(f"sha256 y    {sha(y)}")
            print(f"sha256 grad {sha(g)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("bs", nargs="?", type=int, default=64)
    ap.add_argument("--prec", default="fp32", choices=["fp32", "fp32_x6"])
    ap.add_argument("--dump", action="store_true")
    a = ap.parse_args()
    if a.dump:
        return dump()
    net = ImprovedUNet(1, 1, 48).cuda().set_precision(a.prec)
    x = torch.rand(a.bs, 1, 128, 128, device="cuda")
    dy = torch.rand_like(x)
    profiled_step(net, x, dy)  # warm-up
    table(profiled_step(net, x, dy)[2])


if __name__ == "__main__":
    main()
