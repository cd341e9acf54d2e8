"""k_upconv3_x6 (csrc/upconv_x6.hip): dec_conv1a(cat(up1(d2b), x)) as one launch in forward-only
plans -- the ConvTranspose2d(96, 96, 2, 2) composed into the 3x3 conv's 96 up1 channels (2x2 taps
per output parity over the low-resolution input), the image channels a 3x3 conv of x.

Per op through dn_upconv3_forward_x6 against fp64 on the CPU (conv_transpose2d -> cat with x ->
conv2d(padding=1) -> LeakyReLU, from the same fp32 weights; the slope is the network's 0.2, the
one every dec_conv1a kernel here applies), at tests/test_gpu_x6.py's bound for the forward kernels,
in NaN-filled guarded buffers (x6_edge_util): guard bands and gap channels untouched bit for bit.
Weights at unit gain, so both layers and the bias table are O(1) of the output.

Whole network: dn_unet_forward on a forward-only workspace (fused) against a with-backward
workspace (always the two launches), within the bound the pair-pass test applies against the
full forward; the launch records say which kernel ran.  The fused launch is taken from the grid
size at which k_c3w6 takes dec_conv1a (512 tiles of 8 x 16), which excludes 2 x 32^2 and
1 x 64 x 48: the smallest sizes it accepts with the same channel counts are used instead
(4 x 1 x 128^2 and 8 x 3 x 64 x 128).  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_x6 import X6_TOL
from x6_edge_util import assert_regions, guarded, ran_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def L():
    from image_denoising_amd import _lib

    return _lib


def S():
    return torch.cuda.current_stream().cuda_stream


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(N, h, w, C, zero_bd=False, zero_img=False):
    """unit-gain inputs and the fp64 reference (NHWC), once per case"""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + C)
    xlo = torch.randn(N, 96, h, w, generator=g)
    img = torch.rand(N, C, 2 * h, 2 * w, generator=g)
    wd = torch.randn(96, 96, 2, 2, generator=g) / 96 ** 0.5
    bd = torch.zeros(96) if zero_bd else torch.randn(96, generator=g) * 0.5
    w3 = torch.randn(96, 96 + C, 3, 3, generator=g) / (9 * 96) ** 0.5
    w3[:, 96:] *= (9 * 96 / (9 * C)) ** 0.5  # the image channels' part O(1) too
    if zero_img:
        w3[:, 96:] = 0
    b3 = torch.randn(96, generator=g) * 0.5
    up = F.conv_transpose2d(xlo.double(), wd.double(), bd.double(), stride=2)
    ref = F.leaky_relu(F.conv2d(torch.cat([up, img.double()], 1), w3.double(), b3.double(), padding=1), 0.2)
    return nhwc(xlo), img, w3, b3, wd, bd, nhwc(ref).numpy()


def _run(case, x_stride=96, y_stride=96, lead=4):
    _lib = L()
    xlo, img, w3, b3, wd, bd, ref = case
    N, h, w, _ = xlo.shape
    C = img.shape[1]
    gx = guarded((N, h, w, 96), x_stride, lead, NAN, DEV)
    gx.data.copy_(xlo)
    gy = guarded((N, 2 * h, 2 * w, 96), y_stride, lead, NAN, DEV)
    dev = [t.contiguous().to(DEV) for t in (img, w3, b3, wd, bd)]
    pk = _lib.scratch(_lib.lib().dn_upconv3_x6_pack_size(), DEV)
    with ran_kernel(_lib, "k_upconv3_x6") as ran:
        _lib.call("dn_upconv3_forward_x6", gx.ptr, x_stride, N, h, w, dev[0].data_ptr(), C,
                  dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), gy.ptr,
                  y_stride, pk.data_ptr(), pk.numel(), S())
    rec = ran.record
    assert (rec["op"], rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == \
        ("fwd3", 96 + C, 96, N, 2 * h, 2 * w), rec
    torch.cuda.synchronize()
    gy.check(what="y")
    gx.check(what="xlo")
    y = gy.data.cpu()
    assert bool(torch.isfinite(y).all()), "non-finite or unwritten outputs"
    err = assert_regions(y.numpy(), ref, X6_TOL, f"{tuple(xlo.shape)} C={C}", TH=16, TW=16)
    print(f"upconv {tuple(xlo.shape)} C={C}: max region error {err:.3g} of max|ref|")
    return err


@pytest.mark.parametrize("C", [1, 3])
def test_whole_tiles(C):
    _run(_case(2, 8, 16, C))


@pytest.mark.parametrize("C", [1, 3])
def test_ragged_tile_all_bias_classes(C):
    _run(_case(1, 5, 7, C))


def test_one_past_a_tile_batch_boundary():
    _run(_case(3, 9, 17, 1))


def test_every_pixel_on_a_border():
    _run(_case(1, 1, 2, 1))


def test_strided_views():
    _run(_case(2, 8, 16, 1), x_stride=160, y_stride=128)


def test_zero_deconv_bias():
    _run(_case(1, 5, 7, 1, zero_bd=True))


def test_zero_image_weights():
    _run(_case(1, 5, 7, 3, zero_img=True))


# ---- whole network -------------------------------------------------------------------------------
def _unit_gain(net, seed=0):
    """weights x10 (undoing the reference's x0.1 init) and random biases (tests/test_gpu_parity.py)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(p.device))


@pytest.mark.parametrize("N,C,H,W", [(4, 1, 128, 128), (8, 3, 64, 128)])
def test_unet_forward_fused_vs_two_launches(N, C, H, W):
    from image_denoising_amd import UNet

    _lib = L()
    torch.manual_seed(0)
    net = UNet(in_nc=C, out_nc=C, n_feature=48).to(DEV).set_precision("fp32_x6")
    _unit_gain(net)
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(7)).to(DEV)
    ys, recs = [], []
    for bwd in (False, True):
        ws = net._workspace(N, H, W, with_backward=bwd, fresh=True)
        y = torch.full((N, C, H, W), NAN, device=DEV)
        _lib.profile_ops(True)
        try:
            net._run_forward(x, y, ws)
            recs.append(_lib.profile_ops_take())
        finally:
            _lib.profile_ops(False)
        ys.append(y.cpu())
    top = lambda rs, op: [r for r in rs if r["op"] == op and (r["H"], r["W"]) in ((H, W), (H // 2, W // 2))]
    d1a = lambda rs: [r for r in top(rs, "fwd3") if r["K"] == 96 + C and r["H"] == H]
    fused, plain = recs
    assert [r["kernel"] for r in d1a(fused)] == ["k_upconv3_x6"], d1a(fused)
    assert d1a(fused)[0]["flops"] == d1a(plain)[0]["flops"]
    assert not [r for r in top(fused, "deconv") if r["H"] == H // 2], "up1 still launched"
    assert [r["kernel"][:6] for r in d1a(plain)] == ["k_c3w6"], d1a(plain)
    assert len([r for r in top(plain, "deconv") if r["H"] == H // 2]) == 1
    assert bool(torch.isfinite(ys[0]).all())
    err = (ys[0] - ys[1]).abs().max().item() / ys[1].abs().max().item()
    print(f"fused vs two launches {N}x{C}x{H}x{W}: {err:.3g} of max|y|")
    assert err <= 2e-5, err
