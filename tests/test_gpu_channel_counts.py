"""The UNet's training pass at the channel counts the other suites never build: in_nc 2 and 4,
out_nc 2, 4 and 5..16, in_nc != out_nc.  Those counts pick kernels, not loop bounds: the <2> and
<4> instantiations of enc_conv0 / its weight gradient / dL/dx, dec_conv1a's K = 98 and 100 with
its thin weight-gradient slice scattered behind 96 channels, nin_c's weight gradient on the thin
kernel (out_nc <= 4) or the 1x1 route (above), the bf16x6 head backward up to 4 outputs and the
fp32 one above, and the NCHW -> NHWC transpose of dy for every out_nc > 1.

As tests/test_gpu_parity.py::test_unet_unit_gain_fwd_bwd_vs_fp64, at its bounds: unit-gain
weights, y, dL/dx and all 50 parameter gradients against the fp64 oracle under the device's own
LeakyReLU slopes and pool routing, both 3x3 arithmetics; and the launch records name the
branches taken.  Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_parity as parity
from test_gpu_parity import DEV, FP32_TOL, PRECS, rel_err

pytestmark = pytest.mark.gpu

POOLED = ["a1", "a2", "a3", "a4", "a5"]  # the activations a 2x2 max-pool follows


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _decisions(acts):
    """what the masked oracle takes from the device's activations: the sign of every one, and the
    argmax of every pool window"""
    d = {k: v > 0 for k, v in acts.items()}
    for k in POOLED:
        d["pool_" + k] = F.max_pool2d(acts[k], 2, return_indices=True)[1]
    return d


def _fp64_reference(flat, x, r, C, OC, acts):
    from oracle.unet_ref import forward

    p64 = flat.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    y64 = forward(p64, x64, C, OC, masks=acts)
    (y64 * r.double()).sum().backward()
    return y64.detach().numpy(), x64.grad.numpy(), p64.grad.numpy()


def _check_records(recs, prec, C, OC, N, H, W):
    # the thin 3x3 weight gradients with this in_nc: enc_conv0 (48 outputs) and dec_conv1a's
    # input-channel slice (96 outputs, scattered behind the 96 up1 channels)
    thin = {(q["K"], q["NOUT"]) for q in recs if q["op"] == "wgrad3_thin"}
    assert thin == {(C, 48), (C, 96)}, thin
    enc0 = [q for q in recs if q["op"] == "enc0"]
    assert [(q["K"], q["NOUT"]) for q in enc0] == [(C, 48)], enc0
    head = [q for q in recs if q["op"] == "head_bwd"]
    assert [(q["K"], q["NOUT"]) for q in head] == [(OC, 96)], head
    ninc = [q for q in recs if q["op"] == "wgrad1" and q["NOUT"] == OC and q["K"] == 96]
    if prec == "fp32_x6":
        # up to X6_HEAD_BWD_OCMAX = 4 outputs the bf16x6 head backward (dy in registers); above,
        # the fp32 k_head_bwd on the fp32 images (it sets no kernel label)
        if OC <= 4:
            assert head[0]["kernel"] == "k_head_bwd_x6<4>", head
        else:
            assert head[0]["kernel"] != "k_head_bwd_x6<4>", head
        # nin_c's weight gradient: folded into nin_b's launch at one output, its own launch above
        assert len(ninc) == (0 if OC == 1 else 1), ninc
        # nin_b's weight gradient recomputes g_nb from dy only behind the bf16x6 head backward
        nab = [q["kernel"] for q in recs if q["op"] == "wgrad1" and q["NOUT"] == 96 and q["K"] == 96]
        want = ["k_wgrad1p<false,gnb>" if OC <= 4 else "k_wgrad1p<false>", "k_wgrad1p<false>"]
        assert nab == want, nab
    else:
        assert head[0]["kernel"] != "k_head_bwd_x6<4>", head
        assert len(ninc) == 1, ninc
    # dec_conv1a's forward: K = 96 + in_nc; on the Winograd kernel from one round of 8 x 16 tiles
    d1a = [q for q in recs if q["op"] == "fwd3" and q["K"] == 96 + C and q["NOUT"] == 96]
    assert len(d1a) == 1, d1a
    if prec == "fp32_x6":
        winograd = N * (H // 8) * (W // 16) >= 512
        assert d1a[0]["kernel"].startswith("k_c3w6<") == winograd, d1a
        if winograd:  # the one-channel six-slot tail at in_nc = 1, the packed tail chunk above
            assert d1a[0]["kernel"] == ("k_c3w6<3,96>" if C == 1 else "k_c3w6<1,96>"), d1a


# 2 x C x 32 x 96: the direct kernels, two images, W = one and a half 64-pixel segments of
# k_wgrad_c3_thin<., 96>.  4 x C x 128 x 128: the smallest grid at which the Winograd kernel
# takes dec_conv1a (512 tiles of 8 x 16).
SMALL = [(2, 2), (4, 4), (1, 2), (3, 4), (4, 1), (2, 3), (1, 5), (3, 8), (4, 16)]
LARGE = [(2, 2), (4, 4), (1, 16)]
CASES = [(C, OC, 2, 32, 96) for C, OC in SMALL] + [(C, OC, 4, 128, 128) for C, OC in LARGE]


@pytest.mark.parametrize("C,OC,N,H,W", CASES)
def test_unet_unit_gain_fwd_bwd_vs_fp64_channel_counts(C, OC, N, H, W):
    """Per (in_nc, out_nc): both arithmetics' y within 1e-4, dL/dx and each of the 50 parameter
    gradients within 2e-5 of its tensor's max, against ONE fp64 reference when the two runs took
    the same slopes and pool routes (else one each); the launch records name the branches."""
    from image_denoising_amd import _lib
    from oracle.unet_ref import layer_table

    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1))
    r = torch.randn(N, OC, H, W, generator=torch.Generator().manual_seed(2))
    refs = []
    for prec in PRECS:
        net = parity._net(C, prec, out_nc=OC)
        parity._unit_gain(net)
        _lib.profile_ops(True)
        try:
            y, gg, acts = parity._device_activations(net, x, r)
            recs = _lib.profile_ops_take()
        finally:
            _lib.profile_ops(False)
        dx = parity._device_activations.dx
        assert y.shape == (N, OC, H, W) and dx.shape == (N, C, H, W)
        _check_records(recs, prec, C, OC, N, H, W)
        dec = _decisions(acts)
        ref = next((v for d, v in refs if all(torch.equal(d[k], dec[k]) for k in dec)), None)
        if ref is None:
            ref = _fp64_reference(net.flat_params.detach().cpu(), x, r, C, OC, acts)
            refs.append((dec, ref))
        y64, dx64, g64 = ref
        e_y, e_dx = rel_err(y.numpy(), y64), rel_err(dx.numpy(), dx64)
        gg = gg.numpy()
        errs, off = [], 0
        for name_, ws, bl, _ in layer_table(C, OC):
            n = int(np.prod(ws)) + bl
            errs.append((rel_err(gg[off:off + n], g64[off:off + n]), name_))
            off += n
        assert off == gg.size
        print(f"\n({C},{OC}) {N}x{H}x{W} {prec}: y {e_y:.2e} dx {e_dx:.2e} worst grads "
              f"{sorted(errs, reverse=True)[:3]} refs {len(refs)}")
        assert e_y < FP32_TOL, (prec, e_y)
        assert e_dx < 2e-5, (prec, e_dx)
        bad = [(n_, e) for e, n_ in errs if not e < 2e-5]
        assert not bad, (prec, bad)


def test_wrong_input_channel_count_is_rejected_before_any_launch():
    """a forward whose input has another channel count than in_nc: ValueError from the module's
    own check for each network, and the launch records stay empty"""
    from image_denoising_amd import RESNET, ImprovedUNet, UNet, _lib

    _lib.profile_ops(True)
    try:
        for net, bad in ((UNet(2, 5, 48), 5), (UNet(4, 4, 48), 3), (RESNET(2, 2, 48), 1),
                         (ImprovedUNet(2, 4, 48), 4), (ImprovedUNet(3, 2, 48), 2)):
            net = net.to(DEV)
            with pytest.raises(ValueError, match=f"N,{net.in_nc},H,W"):
                net(torch.rand(1, bad, 32, 32, device=DEV))
            with torch.no_grad(), pytest.raises(ValueError, match=f"N,{net.in_nc},H,W"):
                net(torch.rand(1, bad, 32, 32, device=DEV))
        assert _lib.profile_ops_take() == []
    finally:
        _lib.profile_ops(False)
