"""Every layer of the forward-only bf16 plan (dn_unet_forward_bf16) against fp64, buffer by buffer.

One forward runs on a caller-owned workspace filled with 0xFF bytes (whatever the pass never wrote
reads back as NaN); dn_unet_debug_buffers then locates every activation buffer, and each layer's
output is compared with bf16_layers_ref's restatement of that layer evaluated on the DEVICE'S OWN
input to it.  No rounding flip of an earlier layer propagates, so what is left is the fp32
accumulation order (1e-5 of max|ref|, the bound test_conv_bf16_vs_fp64_of_rounded_operands holds
for this kernel family) plus half a bf16 ulp where the output is stored as bf16 -- for every
element, with no fraction exempt.  The head, which rounds na inside, is held to four times the
measured disagreement of two accumulation orders (bf16_layers_ref.head_bound).
"""
import ctypes
import time

import pytest
import torch

import bf16_layers_ref as R
from test_gpu_ws_independence import _net

pytestmark = pytest.mark.gpu

DEV = "cuda"
NF = 48
# dn_unet_debug_buffers order of the forward-only plan's buffers
FWD_BUFS = ["c1", "a0", "a1", "c2", "c3", "c4", "c5", "a2", "a3", "a4", "a5", "p5", "a6",
            "d2a", "d3a", "d4a", "d5a", "d2b", "d3b", "d4b", "d5b", "d1a", "d1b", "na", "nb"]
WIN = 40   # side of a reference window
FULL = 64  # buffers up to FULL x FULL per image are checked in full


def _layers(C):
    """(layer, reference, input (buffer, c0, c1, bf16), output (buffer, c0, c1, bf16)) in the
    order of run_forward (unet.cpp), inputs and outputs as it wires them: a0, d{l}a and d1b are
    stored as bf16, the pooled encoder outputs land in the skip slices of the concat buffers
    c_l = [up_l | skip] (c5 = [up5 (nf) | pool4 (nf)]), c1 = [up1 (2nf) | x (C) | zero pad]."""
    f32, b16 = False, True
    t = [("enc_conv0", R.enc0, ("x", 0, C, f32), ("a0", 0, NF, b16)),
         ("enc_conv1", R.conv3_pool, ("a0", 0, NF, b16), ("c2", 2 * NF, 3 * NF, f32)),
         ("enc_conv2", R.conv3_pool, ("c2", 2 * NF, 3 * NF, f32), ("c3", 2 * NF, 3 * NF, f32)),
         ("enc_conv3", R.conv3_pool, ("c3", 2 * NF, 3 * NF, f32), ("c4", 2 * NF, 3 * NF, f32)),
         ("enc_conv4", R.conv3_pool, ("c4", 2 * NF, 3 * NF, f32), ("c5", NF, 2 * NF, f32)),
         ("enc_conv5", R.conv3_pool, ("c5", NF, 2 * NF, f32), ("p5", 0, NF, f32)),
         ("enc_conv6", R.conv3, ("p5", 0, NF, f32), ("a6", 0, NF, f32)),
         ("up5.deconv", R.deconv, ("a6", 0, NF, f32), ("c5", 0, NF, f32))]
    for l in (5, 4, 3, 2):
        ck = 2 * NF if l == 5 else 3 * NF
        t += [(f"dec_conv{l}a", R.conv3, (f"c{l}", 0, ck, f32), (f"d{l}a", 0, 2 * NF, b16)),
              (f"dec_conv{l}b", R.conv3, (f"d{l}a", 0, 2 * NF, b16), (f"d{l}b", 0, 2 * NF, f32)),
              (f"up{l - 1}.deconv", R.deconv, (f"d{l}b", 0, 2 * NF, f32), (f"c{l - 1}", 0, 2 * NF, f32))]
    t += [("dec_conv1a", R.conv3, ("c1", 0, 2 * NF + C, f32), ("d1a", 0, 96, b16)),
          ("dec_conv1b", R.conv3, ("d1a", 0, 96, b16), ("d1b", 0, 96, b16)),
          ("head", R.head, ("d1b", 0, 96, b16), ("y", 0, None, f32))]
    return t


def _windows(N, oh, ow, windowed):
    """None: the whole buffer (cases checked in full; in the windowed ones, buffers up to FULL x
    FULL).  Else (n, y0, y1, x0, x1): WIN x WIN windows at the four corners of the first and the
    last image, and one inside image 1 that straddles a 16-row and a 16-column tile seam (at 256
    and 512 rows also a multiple of 32: the seam of an 8-rows-per-wave tile)"""
    if not windowed or (oh <= FULL and ow <= FULL):
        return None
    wins = [(n, y0, y0 + WIN, x0, x0 + WIN) for n in sorted({0, N - 1})
            for y0 in (0, oh - WIN) for x0 in (0, ow - WIN)]
    y0, x0 = oh // 2 - WIN // 2 - 4, ow // 2 - WIN // 2 + 4
    assert any(y0 < s < y0 + WIN for s in range(16, oh, 16)) and any(x0 < s < x0 + WIN for s in range(16, ow, 16))
    return wins + [(min(1, N - 1), y0, y0 + WIN, x0, x0 + WIN)]


def _run(C, OC, N, H, W):
    """one forward on a 0xFF workspace -> (parameters, {buffer: (offset, stride, level)}, x, y, ws)"""
    from image_denoising_amd import _lib

    net = _net(C, OC, "bf16")
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    ws = net._workspace(N, H, W, with_backward=False, fresh=True).fill_(0xFF)
    y = torch.full((N, OC, H, W), float("nan"), device=DEV)
    net._run_forward_inference(x, y, ws)
    torch.cuda.synchronize()
    desc = (ctypes.c_int64 * 300)()
    n = ctypes.c_int()
    _lib.call("dn_unet_debug_buffers", ctypes.byref(net._cfg), N, H, W, 0, desc, 100, ctypes.byref(n))
    assert n.value == len(FWD_BUFS)
    bufs = {name: (desc[3 * i], desc[3 * i + 1], desc[3 * i + 2]) for i, name in enumerate(FWD_BUFS)}
    return R.params(net.flat_params, C, OC), bufs, x, y, ws


def _check_case(C, OC, N, H, W, only=None, windowed=False):
    P, bufs, x, y, ws = _run(C, OC, N, H, W)

    def view(spec):  # NCHW view on the device; nothing is copied here
        name, c0, c1, bf16 = spec
        if name == "x":
            return x
        if name == "y":
            return y
        return R.nchw(R.read_buffer(ws, bufs[name], N, H, W, bf16, c0, c1))

    assert bool(torch.isfinite(y).all()), "y: not finite"
    # enc_conv0 copies the image into its slice of the up1 concat buffer and zeroes the pad
    c1k, c1kp = 2 * NF + C, (2 * NF + C + 3) // 4 * 4
    assert torch.equal(view(("c1", 2 * NF, c1k, False)), x), "c1[2nf:2nf+C] is not x bit for bit"
    assert bool((view(("c1", c1k, c1kp, False)) == 0).all()), "c1's pad channels are not zero"

    failures, floor = [], None
    for name, layer, src, dst in _layers(C):
        if only is not None and name not in only:
            continue
        prm = (*P["nin_a"], *P["nin_b"], *P["nin_c"]) if layer is R.head else P[name]
        xin, out = view(src), view(dst)
        wins = _windows(N, *out.shape[-2:], windowed)
        if wins is None:
            dev, xr = out.cpu(), xin.cpu().double()
        else:  # only the windows (and their halos) leave the device
            dev = torch.cat([out[n:n + 1, :, y0:y1, x0:x1].cpu() for n, y0, y1, x0, x1 in wins])
        if layer is R.head:
            if wins is not None:  # per-pixel: the windows side by side
                xr = torch.cat([xin[n:n + 1, :, y0:y1, x0:x1].cpu().double() for n, y0, y1, x0, x1 in wins])
            ref, rel, floor = R.head_bound(xr, prm)
            c = R.check(dev, ref, False, rel=rel)
        else:
            fn = R.bind(layer, *prm)
            ref = fn(xr) if wins is None else torch.cat(
                [R.windowed(fn, xin[n:n + 1], y0, y1, x0, x1) for n, y0, y1, x0, x1 in wins])
            c = R.check(dev, ref, dst[3])
        print(f"bf16-layers C={C} OC={OC} {N}x{H}x{W} {name:<11} worst/bound {c.worst:.3f} at {c.index}"
              + (f" (head floor {floor:.2e})" if layer is R.head else "")
              + ("" if wins is None else f" [{len(wins)} windows]"))
        if not c.ok:
            failures.append(f"{name}: |dev - ref| = {c.err:.3e} > {c.bound:.3e} ({c.worst:.2f} x the bound) "
                            f"at {c.index} of {tuple(ref.shape)}")
    assert not failures, "\n".join(failures)


# (id, C, out_nc, N, H, W, layers checked (None: all), windowed); each the smallest shape that
# reaches its route, as derived from fwd_routes (unet.cpp), launch_fwd_bf16 (conv_bf16.hip),
# launch_deconv_x6 and launch_nin_head_x6.  Common to all: enc_conv0 on k_enc0_fwd<C> with the bf16
# store; the pooled convs are never `small` (pool_out set) and their views are float4-aligned, so
# they take the pipelined k_fwd_bf16p<3, 4 or 8> with the pool in the epilogue and only the pooled
# output stored; upsample5 (48 -> 48: no bf16x6 deconv image, F_UP_BF16) runs its four parities as
# 1x1 convs in one grid, k_fwd_bf16<3, 1, false> with OUT_UP2; upsample4..1 on k_deconv_x6<true>;
# the head on k_nin_head_x6<false, false, true, true>.
# "floor": the head's measured floor of legitimate disagreement (bf16_layers_ref.head_bound) for
# the case's input, relative to max|y|; the device is held to 4 x floor.
CASES = [
    # 2 x 4 = 8 tiles at level 0: every unpooled 3x3 on the one-row-per-wave k_fwd_bf16<., 1, true>
    # (dec_conv1a: K = c1kp = 100 with a 4-channel last chunk); every level ragged, down to 1 x 2 at
    # level 5; the fused pool on 2 x 4 .. 16 x 32 outputs, at level 4 OH = 2 < the tile's 16 rows.
    # floor 1.47e-05
    ("all-1x32x64", 1, 1, 1, 32, 64, None, False),
    # C = 3: c1k = 99, c1kp = 100 (one zero pad channel); six column tiles at level 0, 1.5 at level
    # 2; two images (the image stride).  floor 3.35e-04
    ("all-c3-2x64x96", 3, 3, 2, 64, 96, None, False),
    # the other two k_enc0_fwd<C> instantiations; C = 4: c1kp = c1k = 100, no pad channel.
    # floors 3.09e-05 (C = 2), 3.31e-04 (C = 4)
    ("all-c2-1x32x32", 2, 2, 1, 32, 32, None, False),
    ("all-c4-1x32x32", 4, 4, 1, 32, 32, None, False),
    # out_nc = X6_HEAD_OCMAX: the far end of the fused bf16 head.  floor 8.53e-05
    ("head-oc16-1x32x32", 1, 16, 1, 32, 32, ("dec_conv1b", "head"), False),
    # 4 x 16 x 16 = 1024 tiles at level 0, not `small`: dec_conv1a on k_fwd_bf16p<6, 4, false> (K =
    # 100, 4-channel last chunk, bf16 output), dec_conv1b on k_fwd_bf16p<6, 4, true>; level 1 (256
    # tiles) stays on k_fwd_bf16<6, 1, true>; enc_conv1 on k_fwd_bf16p<3, 4, true> (512 < 4096 tiles
    # of 32 rows).  Levels 0 and 1 on windows, level 2 (64 x 64) and below in full.  floor 1.37e-04
    ("all-4x256x256", 1, 1, 4, 256, 256, None, True),
    # 8 x 16 x 32 = 4096 tiles of 32 rows: enc_conv1 on k_fwd_bf16p<3, 8, true> (eight rows per wave,
    # bf16 input, fused pool, pool_only), the kernel of the full-size configs[4] step.  Windows only:
    # enc_conv1's pooled corner windows (conv rows 0..79) and its interior one (conv rows 208..287)
    # straddle multiples of 32, the seam between two waves' 8 rows x 4 waves.  (No head: no floor.)
    ("enc1-rows8-8x512x512", 1, 1, 8, 512, 512, ("enc_conv0", "enc_conv1", "dec_conv1a", "dec_conv1b"), True),
]


@pytest.mark.parametrize("C,OC,N,H,W,only,windowed", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bf16_plan_layer_by_layer(C, OC, N, H, W, only, windowed):
    t0 = time.perf_counter()
    _check_case(C, OC, N, H, W, only, windowed)
    print(f"bf16-layers C={C} OC={OC} {N}x{H}x{W}: {time.perf_counter() - t0:.2f} s")
