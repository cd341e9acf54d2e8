"""RESNET on the HIP path against the reference fixtures (tests/golden/resnet_c*.npz), the fp64
restatement (tests/resnet_ref.py), through autograd, the N2N trainer, the adapter and evaluate();
and the UNet's head bits unchanged by the residual-head variants.  Needs an MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resnet_ref
from resnet_ref import FIX, GOLD, fixture_params, rel, tensor_ranges

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP32_TOL = 1e-4
GRAD_TOL = 1e-3  # per tensor, relative to that tensor's max|g| (tests/test_gpu_iunet.py)
PRECS = ["fp32", "fp32_x6"]
# dn_resnet_debug_buffers order (with_backward: na, nb follow the forward-only plan's buffers)
FWD_BUFS = ["c1", "a0", "c2", "c3", "c4", "c5", "a5", "d2a", "d3a", "d4a", "d5a", "d1a", "d1b",
            "na", "nb"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _net(C, prec, flat=None, seed=0):
    from image_denoising_amd import RESNET

    torch.manual_seed(seed)
    net = RESNET(C, C, 48)
    if flat is not None:
        with torch.no_grad():
            net.flat_params.copy_(flat)
    return net.to(DEV).set_precision(prec)


def _unit_gain(C, prec, seed=3):
    """the seed's init x8 with random biases: every layer contributes O(1)"""
    from image_denoising_amd.resnet import layer_shapes, reference_init

    torch.manual_seed(seed)
    flat = reference_init(C, C, 48) * 8.0
    g = torch.Generator().manual_seed(seed)
    off = 0
    for _, ws, bl, _ in layer_shapes(C, C, 48):
        off += int(np.prod(ws))
        flat[off:off + bl] = 0.1 * torch.randn(bl, generator=g)
        off += bl
    return _net(C, prec, flat)


def _activations(net, ws, N, H, W):
    """the saved activations under resnet_ref.ACT_NAMES (NCHW, CPU) of a with-backward workspace"""
    from image_denoising_amd import _lib

    desc = (ctypes.c_int64 * 300)()
    n = ctypes.c_int()
    _lib.call("dn_resnet_debug_buffers", ctypes.byref(net._cfg), N, H, W, 1, desc, 100,
              ctypes.byref(n))
    torch.cuda.synchronize()
    wsf = ws.view(torch.float32)
    buf = {}
    for i, name in enumerate(FWD_BUFS):
        off, st = desc[3 * i], desc[3 * i + 1]
        buf[name] = wsf[off:off + N * H * W * st].view(N, H, W, st).permute(0, 3, 1, 2).cpu().clone()
    a = {k: buf[k] for k in ("a0", "a5", "d2a", "d3a", "d4a", "d5a", "d1a", "d1b", "na", "nb")}
    a["a6"], a["a4"] = buf["c5"][:, :48], buf["c5"][:, 48:]
    for k, j in ((4, 3), (3, 2), (2, 1)):
        a[f"d{k + 1}b"], a[f"a{j}"] = buf[f"c{k}"][:, :96], buf[f"c{k}"][:, 96:]
    a["d2b"] = buf["c1"][:, :96]
    return a


def _run(net, x, dy=None, fill=None):
    """forward (+ backward for a given dy) on a fresh with-backward workspace"""
    N, C, H, W = x.shape
    ws = net._workspace(N, H, W, True, fresh=True)
    if fill is not None:
        ws.fill_(fill)
    xd = x.to(DEV).contiguous()
    y = torch.empty(N, C, H, W, device=DEV)
    net._run_forward(xd, y, ws)
    if dy is None:
        return y.cpu(), ws
    dflat = torch.full_like(net.flat_params, float("nan"))
    dx = torch.full((N, C, H, W), float("nan"), device=DEV)
    net._run_backward(dy.to(DEV).contiguous(), dflat, ws, N, H, W, dx=dx)
    torch.cuda.synchronize()
    return y.cpu(), dflat.cpu(), dx.cpu(), ws


def _first_mismatch(net, ws, flat, x, C):
    """name and error of the first intermediate that leaves the restatement (failure report)"""
    N, _, H, W = x.shape
    acts = _activations(net, ws, N, H, W)
    rec = {}
    resnet_ref.forward(flat.double().requires_grad_(True), x.double(), C, C, record=rec)
    for name in resnet_ref.ACT_NAMES:
        e = rel(acts[name].numpy(), rec[name].detach().numpy())
        if e > FP32_TOL:
            return f"first mismatching intermediate: {name} (rel {e:.3g})"
    return "every intermediate within tolerance"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [1, 3, 2, 4])
def test_forward_backward_vs_reference_fixture(C, prec):
    g = np.load(os.path.join(GOLD, FIX[C]))
    flat = fixture_params(g, C)
    net = _net(C, prec, flat)
    x = torch.from_numpy(g["x"])
    yref = torch.from_numpy(g["y"])
    dy = 2.0 * yref / yref.numel()  # d mean(y^2) / dy at the reference output
    y, dflat, dx, ws = _run(net, x, dy)
    why = lambda: _first_mismatch(net, ws, flat, x, C)
    e_y, e_r = rel(y.numpy(), g["y"]), rel((y - x).numpy(), g["y"] - g["x"])
    loss = float((y.double() ** 2).mean())
    print(f"C={C} {prec}: y {e_y:.3g} y-x {e_r:.3g} loss {abs(loss - float(g['loss'])):.3g}")
    assert e_y < FP32_TOL, why()
    assert e_r < FP32_TOL, why()
    assert abs(loss - float(g["loss"])) < FP32_TOL * float(g["loss"])
    b, e = resnet_ref.ranges(C, C)["up5.deconv"]
    assert torch.equal(dflat[b:e], torch.zeros(e - b))  # exactly zero
    assert torch.isfinite(dflat).all() and torch.isfinite(dx).all()
    if prec != "fp32":
        return
    e_dx = rel(dx.numpy(), g["dx"])
    print(f"  dx {e_dx:.3g}")
    assert e_dx < GRAD_TOL, why()
    # the sample, each element against its tensor's max|g|; the per-tensor norms
    starts = np.array([o for _, o, _ in tensor_ranges(C)])
    tid = np.searchsorted(starts, g["grad_idx"], side="right") - 1
    gmax = np.maximum(g["grad_max"][tid], 1e-30)
    es = np.abs(dflat.numpy()[g["grad_idx"]].astype(np.float64) - g["grad_sample"]) / gmax
    assert es.max() < GRAD_TOL, (int(tid[es.argmax()]), float(es.max()), why())
    for t, (_, o, n) in enumerate(tensor_ranges(C)):
        nrm = float(dflat[o:o + n].double().norm())
        assert abs(nrm - g["grad_norms"][t]) <= GRAD_TOL * max(g["grad_norms"][t], 1e-30) + 1e-12, t


def _check_grads(got, want, C):
    """every tensor (weight and bias apart) within GRAD_TOL of the wanted gradient, relative to
    that tensor's max|g|; up5.deconv exactly zero"""
    for name, o, n in tensor_ranges(C):
        if name.startswith("up5.deconv"):
            assert not got[o:o + n].any(), name
            continue
        e = rel(got[o:o + n], want[o:o + n])
        assert e < GRAD_TOL, (name, e)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,C,H,W", [(1, 1, 32, 48), (2, 3, 13, 22), (1, 1, 1, 5), (3, 1, 9, 17),
                                     (2, 2, 13, 22), (1, 2, 32, 48), (2, 4, 13, 22), (1, 4, 32, 48)])
def test_grads_vs_fp64_with_device_masks(N, C, H, W, prec):
    """every parameter gradient and dx against an fp64 backward that takes its LeakyReLU slopes
    from the device's own activations (only the rounding of the linear ops remains)"""
    net = _unit_gain(C, prec)
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1))
    r = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(2))
    y, dflat, dx, ws = _run(net, x, r)
    acts = _activations(net, ws, N, H, W)
    p64 = net.flat_params.detach().cpu().double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    y64 = resnet_ref.forward(p64, x64, C, C, masks=acts)
    assert rel(y.numpy(), y64.detach().numpy()) < FP32_TOL
    (y64 * r.double()).sum().backward()
    assert rel(dx.numpy(), x64.grad.numpy()) < GRAD_TOL
    _check_grads(dflat.numpy(), p64.grad.numpy(), C)


def test_large_grid_routes_vs_fp64():
    """32 x 1 x 3 x 250 has 512 tiles of 8 x 16, one full round: the executor's bf16x6 routes are
    the ones of real sizes -- the Winograd kernel with its tail-packed images (48 -> 48, the
    K = 100 dec_conv1a), the 96 -> 144 data gradient in blocks of 48 behind a stride-144 mask.
    The launch records name the kernels taken; results against the fp64 restatement."""
    _large_grid_routes_vs_fp64(1)


def test_large_grid_routes_vs_fp64_two_channels():
    """the same grid at in_nc = out_nc = 2: dec_conv1a's K = 98 (two live channels and two zero
    ones in the packed tail chunk) on the Winograd kernel, the <2> thin weight gradients and
    dL/dx, the head backward with two outputs"""
    _large_grid_routes_vs_fp64(2)


def _large_grid_routes_vs_fp64(C):
    from image_denoising_amd import _lib

    N, H, W = 32, 3, 250
    net = _unit_gain(C, "fp32_x6")
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1))
    r = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(2))
    _lib.profile_ops(True)
    try:
        y, dflat, dx, ws = _run(net, x, r)
        recs = _lib.profile_ops_take()
    finally:
        _lib.profile_ops(False)
    kernels = {(q["op"], q["K"], q["NOUT"]): q["kernel"] for q in recs}
    assert kernels[("fwd3", 48, 48)] == "k_c3w6<2,48>", kernels
    assert kernels[("fwd3", 96 + C, 96)] == "k_c3w6<1,96>", kernels
    assert {(q["K"], q["NOUT"]) for q in recs if q["op"] == "wgrad3_thin"} == {(C, 48), (C, 96)}
    assert kernels[("fwd3", 144, 96)] == "k_c3w6<2,96>", kernels
    assert kernels[("dgrad3", 96, 144)] == "k_c3w6<0,48>", kernels
    acts = _activations(net, ws, N, H, W)
    p64 = net.flat_params.detach().cpu().double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    y64 = resnet_ref.forward(p64, x64, C, C, masks=acts)
    assert rel(y.numpy(), y64.detach().numpy()) < FP32_TOL
    (y64 * r.double()).sum().backward()
    assert rel(dx.numpy(), x64.grad.numpy()) < GRAD_TOL
    _check_grads(dflat.numpy(), p64.grad.numpy(), C)


def test_fp32_head_on_a_wide_grid():
    """64 x 1 x 3 x 250 has 1024 tiles of 16 x 16, where the fp32 residual head takes its
    two-row form (k_nin_head<2, RES>): the forward against the fp64 restatement"""
    N, C, H, W = 64, 1, 3, 250
    net = _unit_gain(C, "fp32")
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y = net(x.to(DEV)).cpu()
        y64 = resnet_ref.forward(net.flat_params.cpu().double(), x.double(), C, C)
    assert rel(y.numpy(), y64.numpy()) < FP32_TOL
    assert rel((y - x).numpy(), (y64 - x.double()).numpy()) < FP32_TOL


@pytest.mark.parametrize("prec", PRECS)
def test_autograd_module_matches_c_abi(prec):
    net = _unit_gain(1, prec)
    x = torch.rand(2, 1, 13, 22, generator=torch.Generator().manual_seed(4))
    r = torch.randn(2, 1, 13, 22, generator=torch.Generator().manual_seed(5))
    y0, dflat, dx, _ = _run(net, x, r)
    xg = x.to(DEV).requires_grad_(True)
    y = net(xg)
    (y * r.to(DEV)).sum().backward()
    assert torch.equal(y.detach().cpu(), y0)
    assert torch.equal(xg.grad.cpu(), dx)
    got = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()
    assert torch.equal(got, dflat)
    with torch.no_grad():
        assert torch.equal(net(x.to(DEV)).cpu(), y0)  # forward-only plan: the same bits


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,C,H,W", [(2, 3, 13, 22), (1, 1, 32, 48)])
def test_workspace_independence(N, C, H, W, prec):
    """a workspace of zero bytes and one of 0xFF bytes (NaNs) give identical, finite results"""
    net = _unit_gain(C, prec)
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(6))
    r = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(7))
    a = _run(net, x, r, fill=0)[:3]
    b = _run(net, x, r, fill=0xFF)[:3]
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    N2 = net._workspace(N, H, W, False, fresh=True).fill_(0xFF)
    y = torch.empty(N, C, H, W, device=DEV)
    net._run_forward(x.to(DEV), y, N2)
    assert torch.equal(y.cpu(), a[0])


def test_unet_head_bits_unchanged():
    """the UNet forward (fp32_x6, through k_nin_head_x6) is bit-identical to the output recorded
    before the head gained its residual variants (tests/golden/make_unet_head_bits.py, run with
    the parent commit's library)"""
    from image_denoising_amd import UNet

    g = np.load(os.path.join(GOLD, "unet_head_bits.npz"))
    torch.manual_seed(0)
    net = UNet(1, 1, 48)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
    net = net.to(DEV).set_precision("fp32_x6")
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        y = net(x).cpu().numpy()
    np.testing.assert_array_equal(y.view(np.uint32), g["y"].view(np.uint32))
    ws = net._workspace(1, 32, 32, True, fresh=True)
    yb = torch.empty(1, 1, 32, 32, device=DEV)
    net._run_forward(x, yb, ws)
    np.testing.assert_array_equal(yb.cpu().numpy().view(np.uint32), g["y_bwd_plan"].view(np.uint32))


@pytest.mark.parametrize("prec", PRECS)
def test_n2n_train_step(prec):
    from image_denoising_amd import N2NTrainer
    from oracle import n2n_ref

    net = _unit_gain(1, prec)
    flat0 = net.flat_params.detach().cpu().clone()
    N, H, W = 2, 32, 32
    gen = torch.Generator().manual_seed(8)
    noisy = torch.rand(N, 1, H, W, generator=gen)
    rd = torch.randint(0, 8, (N, H // 2, W // 2), generator=gen, dtype=torch.uint8)
    tr = N2NTrainer(net, distributed=False)
    lam = tr.lambda_for(3)
    loss3 = tr.train_step(noisy.to(DEV), epoch=3, rd_idx=rd.to(DEV), noisy=noisy.to(DEV)).cpu()
    m1, m2 = n2n_ref.masks_from_rd(rd.numpy().astype(np.int64))
    sub1 = torch.from_numpy(n2n_ref.generate_subimages(noisy.numpy(), m1))
    sub2 = n2n_ref.generate_subimages(noisy.numpy(), m2)
    p = flat0.clone().requires_grad_(True)
    with torch.no_grad():
        den = resnet_ref.forward(flat0, noisy, 1, 1)
    out = resnet_ref.forward(p, sub1, 1, 1)
    l1, l2, l, dout = n2n_ref.n2n_loss(out.detach().numpy(), sub2, den.numpy(), rd.numpy().astype(np.int64), lam)
    out.backward(torch.from_numpy(dout))
    for got, want in zip(loss3.numpy(), (l1, l2, l)):
        assert abs(got - want) <= FP32_TOL * abs(want) + 1e-9
    _check_grads(tr.grad.cpu().numpy(), p.grad.numpy(), 1)
    b, e = resnet_ref.ranges(1, 1)["up5.deconv"]
    assert torch.equal(net.flat_params[b:e].cpu(), flat0[b:e])  # unchanged by the step
    assert not torch.equal(net.flat_params.cpu(), flat0)


def test_adapter_over_resnet():
    from image_denoising_amd import DenoiserWithAdapter
    from oracle import adapter_ref

    base = _unit_gain(1, "fp32")
    model = DenoiserWithAdapter(base, in_channels=1, hidden_channels=16).to(DEV)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        model.adapter.flat_params.copy_(0.05 * torch.randn(model.adapter.flat_params.shape, generator=g))
    x = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(9))
    y = model(x.to(DEV)).detach().cpu()
    with torch.no_grad():
        want = adapter_ref.adapter_forward(model.adapter.flat_params.cpu(), x,
                                           resnet_ref.forward(base.flat_params.cpu(), x, 1, 1))
    assert rel(y.numpy(), want.numpy()) < FP32_TOL


@pytest.mark.parametrize("tiled", [False, True])
def test_evaluate_vs_oracle(tiled):
    from image_denoising_amd import evaluation
    from oracle import eval_ref

    net = _unit_gain(1, "fp32")
    net.eval()
    H, W = 40, 56
    rng = np.random.default_rng(21)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    c = np.clip(128 + 90 * np.sin(3 * xx + 2 * yy), 0, 255).astype(np.uint8)
    n = np.clip(c.astype(int) + rng.integers(-25, 26, c.shape), 0, 255).astype(np.uint8)
    if tiled:  # denoise_tiled with a RESNET against the restated tiling (evaluation_704.py:70-115)
        out, p8, l1 = evaluation.denoise_tiled(net, n, patch=28, overlap=8)
        tiles = eval_ref.tile_extract(n, 28, 8)
        with torch.no_grad():
            pred = resnet_ref.forward(net.flat_params.cpu(), torch.from_numpy(tiles), 1, 1).numpy()
        den, q = eval_ref.tile_blend(pred, H, W, 28, 8)
        assert rel(out.cpu().numpy()[0], den) < FP32_TOL
        # uint8 quantisation: a value on a rounding boundary may fall either way
        d8 = np.abs(p8.cpu().numpy()[0].astype(int) - q.astype(int))
        assert d8.max() <= 1 and (d8 != 0).mean() < 1e-3
        assert float(l1) == pytest.approx(float(np.abs(pred - tiles).mean()), rel=1e-4)
        return
    res = evaluation.evaluate(net, [c], [n])
    x = torch.from_numpy(n.astype(np.float32) / 255.0)[None, None]
    with torch.no_grad():
        y = resnet_ref.forward(net.flat_params.cpu(), x, 1, 1)
    q = eval_ref.quantize_full(y.numpy()[0, 0])
    # the eval CLI test's tolerances (single-pixel flips of the uint8 quantisation)
    assert res["avg_psnr"] == pytest.approx(eval_ref.psnr(q, c), abs=2e-3)
    assert res["avg_ssim"] == pytest.approx(eval_ref.calculate_ssim(q, c), abs=1e-4)
    assert res["avg_l1"] == pytest.approx(float((y - x).abs().mean()), rel=1e-4)


def test_rejections():
    from image_denoising_amd import RESNET, _lib

    with pytest.raises(ValueError):
        RESNET(1, 3, 48)
    with pytest.raises(ValueError):
        RESNET(1, 1, 32)
    with pytest.raises(NotImplementedError):
        RESNET(1, 1, 48, blindspot=True)
    net = _net(1, "fp32")
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    x = torch.rand(1, 1, 8, 8, device=DEV)
    y = torch.empty_like(x)
    ws = net._workspace(1, 8, 8, False)
    st = _lib.lib().dn_resnet_forward_prec(ctypes.byref(net._cfg), _lib.ptr(net.flat_params),
                                           _lib.ptr(x), _lib.ptr(y), 1, 8, 8, ws.data_ptr(),
                                           ws.numel(), 1, None)
    assert st == -1 and "precision" in _lib.last_error()  # DN_ERR_ARG for DN_PREC_BF16
    with pytest.raises(ValueError):
        net(torch.rand(1, 3, 8, 8, device=DEV))
