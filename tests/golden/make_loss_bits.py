"""Records tests/golden/loss_bits.json: the bits of every loss and metric whose kernels sum in the
fixed order of DESIGN.md §11a (fp64 block partials, one 256-thread block that gathers and trees
them), from a library built BEFORE those kernels moved onto csrc/block_reduce.h.

The committed file was recorded on an MI355X from commit 54a0d96 ("One flat-parameter module base
for the networks, adapters and trainers"), the parent of that refactor:

    python -m image_denoising_amd._build          (at 54a0d96)
    python tests/golden/make_loss_bits.py tests/golden/loss_bits.json 54a0d96

The existing tests bound these kernels against fp64 references, which a reordered sum passes;
equal bits pin the order itself.  tests/test_gpu_loss_bits.py recomputes every case with run()
below and compares.  Scalars are stored as the hex of their fp32 / fp64 bits, tensors of more than
eight elements as SHA-256 of their bytes.  Inputs come from CPU torch.Generators with fixed seeds
and are then copied to the device.  IQSL's exp / log and SSIM's exp come from the compiler's
device math library, so the file also names the toolchain it was recorded with.

Cases (each the smallest shape at which its reduction can still go wrong):
  fixed-grid losses (1024 blocks x 256 threads, grid-stride) at three element counts: `one`
    1x1x2x2 (n2n: h = w = 1) has one to four active threads, `ragged` 2x3x5x7 = 210 elements
    fills three waves and part of a fourth, `big` 1x1x517x509 = 263153 > 1024 * 256 takes a
    ragged second trip.  IQSL takes one channel, so its `ragged` is 6x1x5x7.
  dn_l1fft_loss: beta = 0 (the fixed-grid pixel kernel) at 8x8 and 512x544; beta != 0 at 8x8,
    1x2x24x40, and 257x1x64x64: a 64-point transform packs 32 row pairs / 32 columns per block,
    so a 64x64 plane is 1 row block and 2 column blocks, and 257 planes are the fewest with more
    than 256 of each (the finalize's gather takes a second trip in both segments).
  dn_psnr_u8 / dn_l1_mean: n = 1, 255, and 256 * parts + 257 + 3 (parts = the 1024 slots of
    dn_eval_partials_size(): the grid cap and a ragged trip).
  dn_ssim_u8: 1x11x11 (one valid pixel), 3x40x52 channel-first and channel-last.
  dn_l1_mean_batched: (P, n) = (3, 1), (3, 1027).
  dn_groupnorm_backward: dgamma, dbeta at N = 1 and N = 65 (k_gn_dparams' second lane trip) at
    H = W = 1, C = 4, G = 1, and at N = 65, 2x2, C = 8, G = 2.
  dn_memadapter_forward / _backward: features, out, dparams at 1x1x1x2 (hidden 8, no FFT bins)
    and at 2x1x20x36 (hidden 8, 3 bins: six 16x16 conv tiles per image).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

DEV = "cuda"
SHAPES = {"one": (1, 1, 2, 2), "ragged": (2, 3, 5, 7), "big": (1, 1, 517, 509)}
LAMBDA_GRAD, LAMBDA_IQSL = 0.1, 0.1
T1, T2, TAU, CE = 0.2, 0.8, 0.1, 0.5
MARGINS = {"m0": 0.0, "m05": 0.05}


def _lib():
    from image_denoising_amd import _lib as m
    return m


def rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def randu8(seed, *shape, high=256):
    return torch.randint(0, high, shape, generator=torch.Generator().manual_seed(seed),
                         dtype=torch.uint8)


def _f32(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=DEV)


def _bytes(n):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=DEV)


def _call(name, *args):
    L = _lib()
    L.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _loss_parts():
    return _bytes(_lib().lib().dn_loss_partials_size())


def _iqsl_parts():
    return _bytes(_lib().lib().dn_iqsl_partials_size())


def _eval_parts():
    return _bytes(_lib().lib().dn_eval_partials_size())


# ---- the ops: CPU inputs in, dict of CPU tensors out -------------------------------------------
def n2n(shape):
    N, C, h, w = (1, 1, 1, 1) if shape == "one" else SHAPES[shape]
    out, sub2 = rand(1, N, C, h, w).to(DEV), rand(2, N, C, h, w).to(DEV)
    den, rd = rand(3, N, C, 2 * h, 2 * w).to(DEV), randu8(4, N, h, w, high=8).to(DEV)
    dout, loss3 = _f32(N, C, h, w), _f32(3)
    _call("dn_n2n_loss", out, sub2, den, rd, N, C, h, w, 2.0, dout, loss3, _loss_parts())
    return {"loss3": loss3.cpu(), "dout": dout.cpu()}


def structure(shape):
    N, C, H, W = SHAPES[shape]
    p, p2, t = (rand(s, N, C, H, W).to(DEV) for s in (5, 6, 7))
    dp, dp2, loss5 = _f32(N, C, H, W), _f32(N, C, H, W), _f32(5)
    _call("dn_structure_loss", p, p2, t, N, C, H, W, 1.0, 0.5, 0.5, dp, dp2, loss5, _loss_parts())
    return {"loss5": loss5.cpu(), "dpred": dp.cpu(), "dpred2": dp2.cpu()}


def _pair(shape, one_channel=False):
    N, C, H, W = SHAPES[shape]
    if one_channel:
        N, C = N * C, 1
    return rand(8, N, C, H, W).to(DEV), rand(9, N, C, H, W).to(DEV)


def finetune(shape, one_channel=False):
    p, t = _pair(shape, one_channel)
    N, C, H, W = p.shape
    dp, loss3 = _f32(N, C, H, W), _f32(3)
    _call("dn_finetune_loss", p, t, N, C, H, W, LAMBDA_GRAD, dp, loss3, _loss_parts())
    return {"loss3": loss3.cpu(), "dpred": dp.cpu()}


def finetune_iqsl(shape, margin, lam_iq):
    p, t = _pair(shape, True)
    N, C, H, W = p.shape
    dp, loss4 = _f32(N, C, H, W), _f32(4)
    _call("dn_finetune_iqsl_loss", p, t, N, C, H, W, LAMBDA_GRAD, lam_iq, T1, T2, TAU,
          MARGINS[margin], CE, dp, loss4, _iqsl_parts())
    return {"loss4": loss4.cpu(), "dpred": dp.cpu()}


def iqsl(shape, margin):
    p, t = _pair(shape, True)
    N, C, H, W = p.shape
    dp, loss1 = _f32(N, C, H, W), _f32(1)
    _call("dn_iqsl_loss", p, t, N, C, H, W, T1, T2, TAU, MARGINS[margin], CE, dp, loss1,
          _iqsl_parts())
    return {"loss1": loss1.cpu(), "dpred": dp.cpu()}


def l1fft(N, C, H, W, beta, reduction):
    p, t = rand(10, N, C, H, W).to(DEV), rand(11, N, C, H, W).to(DEV)
    dp, loss3 = _f32(N, C, H, W), _f32(3)
    ws = _bytes(_lib().lib().dn_l1fft_ws_size(N, C, H, W))
    _call("dn_l1fft_loss", p, t, N, C, H, W, 1.0, beta, int(reduction == "sum"), dp, loss3, ws,
          ws.numel())
    return {"loss3": loss3.cpu(), "dpred": dp.cpu()}


def eval_n(which):
    parts = _lib().lib().dn_eval_partials_size() // 8
    return {"1": 1, "255": 255, "cap": 256 * parts + 257 + 3}[which]


def psnr(which):
    n = eval_n(which)
    a, b = randu8(12, n).to(DEV), randu8(13, n).to(DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    _call("dn_psnr_u8", a, b, n, _eval_parts(), out)
    return {"psnr": out.cpu()}


def l1_mean(which):
    n = eval_n(which)
    a, b = rand(14, n).to(DEV), rand(15, n).to(DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    _call("dn_l1_mean", a, b, n, _eval_parts(), out)
    return {"l1": out.cpu()}


def ssim(C, H, W, hwc):
    shape = (H, W, C) if hwc else (C, H, W)
    a = randu8(16, *shape)
    b = (a.int() + randu8(17, *shape, high=32).int() - 16).clamp(0, 255).to(torch.uint8)
    a, b = a.to(DEV), b.to(DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    _call("dn_ssim_u8", a, b, C, H, W, int(hwc), _eval_parts(), out)
    return {"ssim": out.cpu()}


def l1_batched(P, n):
    a, b = rand(18, P, n).to(DEV), rand(19, P, n).to(DEV)
    out = torch.empty(P, dtype=torch.float64, device=DEV)
    _call("dn_l1_mean_batched", a, b, P, n, out)
    return {"l1": out.cpu()}


def groupnorm(N, H, W, C, G):
    """dense NHWC views (pixel stride C, offset 0), no residual, no activation"""
    z, dy = (rand(20, N, H, W, C) * 2 - 1).to(DEV), (rand(21, N, H, W, C) - 0.5).to(DEV)
    gamma, beta = (rand(22, C) + 0.5).to(DEV), (rand(23, C) - 0.5).to(DEV)
    y, dz, stats = _f32(N, H, W, C), _f32(N, H, W, C), _f32(2 * N * G)
    dgamma, dbeta = _f32(C), _f32(C)
    sc = _bytes(_lib().lib().dn_groupnorm_scratch_size(N, H, W, C))
    _call("dn_groupnorm_forward", z, C, 0, None, C, 0, y, C, 0, N, H, W, C, G, gamma, beta, 0,
          stats, sc, sc.numel())
    _call("dn_groupnorm_backward", dy, C, 0, z, C, 0, dz, C, 0, N, H, W, C, G, gamma, stats,
          dgamma, dbeta, sc, sc.numel())
    return {"dgamma": dgamma.cpu(), "dbeta": dbeta.cpu(), "dz": dz.cpu()}


def memadapter(N, C, H, W, hid, nb):
    import ctypes

    L = _lib()
    n = ctypes.c_size_t()
    L.check(L.lib().dn_memadapter_param_count(C, hid, nb, ctypes.byref(n)), "param_count")
    prm = ((rand(24, n.value) - 0.5) * 0.6).to(DEV)
    noisy, base, mem = (rand(s, N, C, H, W).to(DEV) for s in (25, 26, 27))
    dout = (rand(28, N, C, H, W) - 0.5).to(DEV)
    out, feat, dprm = _f32(N, C, H, W), _f32(N, 6 + 3 * nb), _f32(n.value)
    ws = _bytes(max(L.lib().dn_memadapter_ws_size(N, C, H, W, hid, nb, 0),
                    L.lib().dn_memadapter_ws_size(N, C, H, W, hid, nb, 1)))
    _call("dn_memadapter_forward", prm, noisy, base, mem, out, feat, N, C, H, W, hid, nb, 1, ws,
          ws.numel())
    _call("dn_memadapter_backward", prm, noisy, base, feat, dout, dprm, N, C, H, W, hid, nb, 1, ws,
          ws.numel())
    return {"features": feat.cpu(), "out": out.cpu(), "dparams": dprm.cpu()}


# ---- the cases --------------------------------------------------------------------------------
CASES = {}
for _s in SHAPES:
    CASES[f"n2n:{_s}"] = (n2n, (_s,))
    CASES[f"structure:{_s}"] = (structure, (_s,))
    CASES[f"finetune:{_s}"] = (finetune, (_s,))
    for _m in MARGINS:
        CASES[f"iqsl:{_s}:{_m}"] = (iqsl, (_s, _m))
        for _l in (0.0, LAMBDA_IQSL):
            CASES[f"finetune_iqsl:{_s}:{_m}:lam{_l}"] = (finetune_iqsl, (_s, _m, _l))
for _r in ("mean", "sum"):
    for _n, _c, _h, _w, _b in ((1, 1, 8, 8, 0.0), (1, 1, 512, 544, 0.0), (1, 1, 8, 8, 0.5),
                               (1, 2, 24, 40, 0.5), (257, 1, 64, 64, 0.5)):
        CASES[f"l1fft:{_n}x{_c}x{_h}x{_w}:beta{_b}:{_r}"] = (l1fft, (_n, _c, _h, _w, _b, _r))
for _k in ("1", "255", "cap"):
    CASES[f"psnr:{_k}"] = (psnr, (_k,))
    CASES[f"l1_mean:{_k}"] = (l1_mean, (_k,))
CASES["ssim:1x11x11"] = (ssim, (1, 11, 11, False))
CASES["ssim:3x40x52:chw"] = (ssim, (3, 40, 52, False))
CASES["ssim:3x40x52:hwc"] = (ssim, (3, 40, 52, True))
CASES["l1_batched:3x1"] = (l1_batched, (3, 1))
CASES["l1_batched:3x1027"] = (l1_batched, (3, 1027))
CASES["groupnorm:N1:1x1:C4:G1"] = (groupnorm, (1, 1, 1, 4, 1))
CASES["groupnorm:N65:1x1:C4:G1"] = (groupnorm, (65, 1, 1, 4, 1))
CASES["groupnorm:N65:2x2:C8:G2"] = (groupnorm, (65, 2, 2, 8, 2))
CASES["memadapter:1x1x1x2:hid8:nb0"] = (memadapter, (1, 1, 1, 2, 8, 0))
CASES["memadapter:2x1x20x36:hid8:nb3"] = (memadapter, (2, 1, 20, 36, 8, 3))
KEYS = list(CASES)


def bits(t):
    """hex of every element's bits (at most eight elements), else SHA-256 of the bytes"""
    a = t.detach().cpu().contiguous().numpy()
    if a.size > 8:
        return "sha256:" + hashlib.sha256(a.tobytes()).hexdigest()
    u = a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return [format(int(v), f"0{2 * a.dtype.itemsize}x") for v in u]


def run(key):
    fn, args = CASES[key]
    return fn(*args)


def digests(key):
    return {k: bits(v) for k, v in run(key).items()}


def toolchain():
    return {"dn_version": _lib().lib().dn_version().decode(), "rocm": str(torch.version.hip),
            "device": torch.cuda.get_device_name(0)}


def main(out, commit):
    info = toolchain()
    print("library:", _lib().LIB_PATH, info)
    cases = {}
    for key in KEYS:
        a, b = digests(key), digests(key)
        if a != b:
            raise SystemExit(f"NOT bit-reproducible: {key} {[k for k in a if a[k] != b[k]]}")
        cases[key] = a
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, **info, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(cases), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2])
