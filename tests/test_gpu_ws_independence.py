"""A UNet pass reads no weight image and no activation that it did not itself write.

The executor decides per pass which kernel and which weight image every layer takes
(unet.cpp fwd_routes / bwd_routes), packs exactly those images and launches on them.  The
workspace is caller-owned, uninitialised memory, so a launch that read an image or a buffer the
pass never wrote would give silently wrong numbers.  Every case here runs once in a workspace
filled with zero bytes and once in one filled with 0xFF bytes (an fp32 word of 0xFF bytes is a
NaN, a bf16 pair two NaNs): every result must be finite and bit-equal between the two runs.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0  # prefill of an output the pass writes only in part


def _net(C, OC, prec):
    from image_denoising_amd import UNet

    torch.manual_seed(0)
    net = UNet(in_nc=C, out_nc=OC, n_feature=48).to(DEV)
    if prec == "bf16":
        net.set_inference_precision("bf16")
    else:
        net.set_precision(prec)
    # unit gain (the reference init x10, random biases): every level contributes O(1) to y
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(DEV))
    return net


def _ws(net, N, H, W, with_backward, fill):
    return net._workspace(N, H, W, with_backward=with_backward, fresh=True).fill_(fill)


def _pair_mask(rd, N, H, W):
    """bool [N,1,H,W]: the two pair pixels of every 2x2 cell"""
    from oracle import n2n_ref

    m1, m2 = n2n_ref.masks_from_rd(rd.numpy().astype(np.int64))
    cells = (m1 | m2).reshape(N, H // 2, W // 2, 2, 2)
    return torch.from_numpy(cells.transpose(0, 1, 3, 2, 4).reshape(N, 1, H, W).copy())


def _train(net, x, fill):
    """forward on a with-backward workspace, then the backward: y, dparams, dx"""
    N, _, H, W = x.shape
    ws = _ws(net, N, H, W, True, fill)
    y = torch.zeros(N, net.out_nc, H, W, device=DEV)
    net._run_forward(x, y, ws)
    dy = torch.rand(y.shape, generator=torch.Generator().manual_seed(5)).to(DEV) - 0.5
    dflat, dx = torch.zeros_like(net.flat_params), torch.zeros_like(x)
    net._run_backward(dy, dflat, ws, N, H, W, dx=dx)
    return {"y": y, "dparams": dflat, "dx": dx}


def _infer(net, x, fill):
    N, _, H, W = x.shape
    y = torch.zeros(N, net.out_nc, H, W, device=DEV)
    net._run_forward_inference(x, y, _ws(net, N, H, W, False, fill))
    return {"y": y}


def _prepacked(net, x, fill):
    """the workspace is poisoned before dn_unet_pack_weights, not between the two calls"""
    N, _, H, W = x.shape
    ws = _ws(net, N, H, W, False, fill)
    net._pack_weights(ws, N, H, W)
    y = torch.zeros(N, net.out_nc, H, W, device=DEV)
    net._run_forward_prepacked(x, y, ws)
    return {"y": y}


def _n2n(net, x, fill):
    """the pair pass writes y at the pair pixels and nowhere else"""
    N, C, H, W = x.shape
    rd = torch.randint(0, 8, (N * (H // 2) * (W // 2),), generator=torch.Generator().manual_seed(7),
                       dtype=torch.uint8)
    y = torch.full((N, net.out_nc, H, W), SENTINEL, device=DEV)
    net._run_forward_n2n(x, y, _ws(net, N, H, W, False, fill), rd.to(DEV))
    sel = _pair_mask(rd, N, H, W).to(DEV).expand(N, net.out_nc, H, W)
    assert bool((y[~sel] == SENTINEL).all()), "y written outside the pair pixels"
    return {"y at the pair pixels": y[sel]}


# (id, runner, precision, N, C, out_nc, H, W); the shapes are the smallest that reach each route:
# 1 x 32 x 64 runs the direct kernels, 4 x 128 x 128 is the smallest grid where the Winograd kernel
# takes dec_conv1a (one-channel tail, the fused up1 launch without a backward) and the pair pass
# runs on cell lists.  out_nc <= 16 is all the parameter layout admits, so every bf16 forward takes
# the fused bf16 head (out_nc <= X6_HEAD_OCMAX = 16); 1 and 16 are its two ends.
CASES = [
    ("train-fp32", _train, "fp32", 1, 1, 1, 32, 64),
    ("train-fp32_x6", _train, "fp32_x6", 1, 1, 1, 32, 64),
    ("fwd-fp32_x6-direct", _infer, "fp32_x6", 1, 1, 1, 32, 64),
    ("fwd-fp32_x6-fused-up1", _infer, "fp32_x6", 4, 1, 1, 128, 128),
    ("fwd-bf16-oc1", _infer, "bf16", 1, 1, 1, 32, 64),
    ("fwd-bf16-oc16", _infer, "bf16", 1, 1, 16, 32, 64),
    ("n2n-direct", _n2n, "fp32_x6", 1, 1, 1, 32, 64),
    ("n2n-cell-lists", _n2n, "fp32_x6", 4, 1, 1, 128, 128),
    ("prepacked-fp32_x6", _prepacked, "fp32_x6", 1, 1, 1, 32, 64),
    ("prepacked-bf16", _prepacked, "bf16", 1, 1, 1, 32, 64),
]


@pytest.mark.parametrize("run,prec,N,C,OC,H,W", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_pass_independent_of_workspace_contents(run, prec, N, C, OC, H, W):
    net = _net(C, OC, prec)
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    zero, ones = run(net, x, 0x00), run(net, x, 0xFF)
    for name in zero:
        assert bool(torch.isfinite(ones[name]).all()), f"{name}: not finite in a 0xFF workspace"
        assert bool(torch.isfinite(zero[name]).all()), f"{name}: not finite in a zeroed workspace"
        assert torch.equal(zero[name], ones[name]), f"{name} depends on the workspace's contents"
