"""ImprovedUNet (arch_unet.py:421-531) on the HIP kernels vs the reference fixtures and the CPU
oracle (oracle/iunet_ref.py), through the C-ABI.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import iunet_ref, n2n_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-4  # north_star: 1e-4 relative fp32 on the denoised image and the loss
# Parameter gradients per tensor, relative to that tensor's max |g|: GroupNorm and LeakyReLU
# make the backward a long chain of cancelling fp32 sums (torch CPU vs MFMA tile order);
# 1e-3 still catches any indexing or layout error (those are O(1)).
GRAD_TOL = 1e-3
# both arithmetics of the 3x3 convs (DN_PREC_FP32 / DN_PREC_FP32_X6) meet the same tolerances
PRECS = ["fp32", "fp32_x6"]


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _net(C, prec="fp32", out_nc=None):
    from image_denoising_amd.improved_unet import ImprovedUNet

    torch.manual_seed(0)
    return ImprovedUNet(in_nc=C, out_nc=C if out_nc is None else out_nc,
                        n_feature=48).set_precision(prec)


def _trace_mismatches(net, x, ws, flat_cpu, C):
    """first intermediate activation that differs from the oracle (diagnostic for failures)"""
    from image_denoising_amd import _lib

    N, _, H, W = x.shape
    desc = (ctypes.c_int64 * (3 * 64))()
    n = ctypes.c_int()
    _lib.call("dn_iunet_debug_buffers", ctypes.byref(net._cfg), N, H, W, 1, desc, 64,
              ctypes.byref(n))
    tr = []
    iunet_ref.forward(flat_cpu, x.cpu(), C, net.out_nc, trace=tr)
    fws = ws.view(torch.float32)
    out = []
    for i, (name, ref) in enumerate(tr):
        off, stride, lvl = desc[3 * i], desc[3 * i + 1], desc[3 * i + 2]
        h, w, ch = H >> lvl, W >> lvl, ref.shape[1]
        got = fws[off:off + N * h * w * stride].view(N, h, w, stride)[..., :ch].permute(0, 3, 1, 2)
        e = rel_err(got.cpu().numpy(), ref.detach().numpy())
        out.append((name, e))
        if e > FP32_TOL:
            return f"first mismatch at {name} (rel err {e:.3e}); before: {out[-4:-1]}"
    return "all intermediates match"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C,name", [(1, "iunet_c1.npz"), (3, "iunet_c3.npz"), (2, "iunet_c2_2.npz"),
                                    (1, "iunet_c1_4.npz"), (3, "iunet_c3_2.npz")])
def test_forward_backward_vs_reference_fixture(golden, C, name, prec):
    g = golden(name)
    OC = g["t"].shape[1]  # (iunet_c<in_nc>_<out_nc>.npz: out_nc != in_nc)
    net = _net(C, prec, OC).to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV)
    t = torch.from_numpy(g["t"]).to(DEV)
    N, _, H, W = x.shape
    ws = net._workspace(N, H, W, with_backward=True, fresh=True)
    y = torch.empty_like(t)
    net._run_forward(x, y, ws)
    err = rel_err(y.cpu().numpy(), g["y"])
    assert err < FP32_TOL, (err, _trace_mismatches(net, x, ws, net.flat_params.cpu(), C))
    dy = (2.0 / y.numel()) * (y - t)
    loss = float(((y - t) ** 2).mean())
    assert abs(loss - float(g["loss"])) <= FP32_TOL * abs(float(g["loss"]))
    if prec == "fp32_x6":
        # the fixture holds torch-fp32 gradients; iunet_c3's input has a LeakyReLU input
        # within 5e-8 (relative) of zero in ups.2, where the split-bf16 arithmetic may take the
        # other slope.  Its gradients are checked against fp64 with the device's own
        # decisions: test_x6_grads_as_accurate_as_fp32_vs_fp64.
        return
    grad = torch.empty_like(net.flat_params)
    net._run_backward(dy.contiguous(), grad, ws, N, H, W)
    gr = grad.cpu().numpy()
    assert rel_err(gr[g["grad_idx"]], g["grad_sample"]) < GRAD_TOL
    norms, off = [], 0
    for _, shape in iunet_ref.layer_table(C, OC):
        k = int(np.prod(shape))
        norms.append(np.linalg.norm(gr[off:off + k]))
        off += k
    ref = g["grad_norms"]
    bad = [(i, norms[i], ref[i]) for i in range(len(ref))
           if abs(norms[i] - ref[i]) > GRAD_TOL * max(abs(ref[i]), 1e-12)]
    assert not bad, bad[:5]


def _pool_gap(x, C, out_nc=None):
    """smallest gap between the two largest values of any 2x2 max-pool window of the fp64
    oracle (iunet_ref.pool_gap).  MaxPool routes the whole gradient to the argmax: where two
    candidates lie within fp32 rounding of each other, any two fp32 implementations (torch CPU
    included) may route differently and every gradient upstream moves by O(1e-3).  The parity
    inputs below are chosen with gaps >= 1e-5 so the comparison is well-posed; ties themselves
    are exercised bit-exactly by the maxpool tests."""
    OC = C if out_nc is None else out_nc
    return iunet_ref.pool_gap(_net(C, out_nc=OC).flat_params, x, C, OC)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,seed", [((1, 1, 32, 48), 14), ((1, 3, 48, 32), 13)])
def test_grads_per_tensor_vs_oracle(shape, seed, prec):
    N, C, H, W = shape
    net = _net(C, prec).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    assert _pool_gap(x, C) >= 1e-5
    dy = torch.randn(shape, generator=gen)
    p = net.flat_params.cpu().clone().requires_grad_(True)
    yr = iunet_ref.forward(p, x, C, C)
    yr.backward(dy)
    ws = net._workspace(N, H, W, with_backward=True, fresh=True)
    y = torch.empty(shape, device=DEV)
    net._run_forward(x.to(DEV), y, ws)
    assert rel_err(y.cpu().numpy(), yr.detach().numpy()) < FP32_TOL
    grad = torch.empty_like(net.flat_params)
    net._run_backward(dy.to(DEV), grad, ws, N, H, W)
    gr, ref = grad.cpu().numpy(), p.grad.numpy()
    off, bad = 0, []
    for key, sh in iunet_ref.layer_table(C, C):
        k = int(np.prod(sh))
        e = rel_err(gr[off:off + k], ref[off:off + k])
        if e > GRAD_TOL:
            bad.append((key, e))
        off += k
    assert not bad, bad[:8]
    # deterministic: a second backward is bit-identical
    grad2 = torch.empty_like(grad)
    net._run_backward(dy.to(DEV), grad2, ws, N, H, W)
    assert torch.equal(grad, grad2)


@pytest.mark.parametrize("prec", PRECS)
def test_backward_side_stream_equals_one_stream(prec):
    """iunet_backward runs the weight gradients on a side stream beside the data-gradient chain;
    with dn_profile_ops on, every launch runs on the caller's stream.  At a size where the two
    streams overlap, both orders give bit-identical gradients (no buffer a weight gradient reads
    is rewritten while it runs), and the batched weight packs of the two passes change nothing."""
    from image_denoising_amd import _lib

    N, C, H, W = 8, 1, 128, 128
    net = _net(C, prec).to(DEV)
    gen = torch.Generator().manual_seed(21)
    x = torch.rand((N, C, H, W), generator=gen).to(DEV)
    dy = torch.randn((N, C, H, W), generator=gen).to(DEV)
    ws = net._workspace(N, H, W, with_backward=True, fresh=True)
    y = torch.empty_like(x)
    grads = []
    try:
        for one_stream in (False, True, False):
            _lib.profile_ops(one_stream)
            net._run_forward(x, y, ws)
            g = torch.empty_like(net.flat_params)
            net._run_backward(dy, g, ws, N, H, W)
            torch.cuda.synchronize()
            grads.append(g)
    finally:
        _lib.profile_ops(False)
    assert torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_module_autograd_and_no_grad_paths():
    net = _net(1).to(DEV)
    x = torch.rand(2, 1, 32, 32, device=DEV)
    with torch.no_grad():
        y0 = net(x)
    y = net(x)
    assert torch.equal(y0, y.detach())
    (y ** 2).mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


@pytest.mark.parametrize("prec", PRECS)
def test_n2n_step_with_improved_unet_vs_oracle(prec):
    """train.py with log_name 'UNetImproved' (train.py:311-313) under the N2N loss"""
    from image_denoising_amd import N2NTrainer

    net = _net(1, prec).to(DEV)
    flat0 = net.flat_params.cpu().clone()
    gen = torch.Generator().manual_seed(7)
    noisy = torch.rand(2, 1, 64, 64, generator=gen)
    rd = torch.randint(0, 8, (2 * 32 * 32,), generator=gen, dtype=torch.uint8)
    s1, _ = n2n_ref.subimages_closed_form(noisy.numpy(), rd.numpy())
    assert _pool_gap(torch.from_numpy(s1), 1) >= 1e-5
    tr = N2NTrainer(net, lr=3e-4)
    loss3 = tr.train_step(noisy.to(DEV), epoch=10, rd_idx=rd.to(DEV), noisy=noisy.to(DEV)).cpu()
    lam = 10 / 100 * 2.0
    p = flat0.clone().requires_grad_(True)
    with torch.no_grad():
        den = iunet_ref.forward(flat0, noisy, 1, 1)
    s1, s2 = n2n_ref.subimages_closed_form(noisy.numpy(), rd.numpy())
    out = iunet_ref.forward(p, torch.from_numpy(s1), 1, 1)
    d1, d2 = n2n_ref.subimages_closed_form(den.numpy(), rd.numpy())
    diff = out - torch.from_numpy(s2)
    l1 = (diff ** 2).mean()
    l2 = lam * ((diff - torch.from_numpy(d1 - d2)) ** 2).mean()
    (l1 + l2).backward()
    assert rel_err(loss3.numpy(), [l1.item(), l2.item(), (l1 + l2).item()]) < FP32_TOL
    assert rel_err(tr.grad.cpu().numpy(), p.grad.numpy()) < GRAD_TOL


def _device_leaky_masks(net, ws, x, C, tr=None):
    """The LeakyReLU decisions the device took in its last forward on ws (its saved
    activations, dn_iunet_debug_buffers), in the order of the oracle's leaky_relu calls:
    noise_estimator.0; per down level: downs.i.0, 4 RDB growth convs, ResBlock a1; bottle: 4
    growth convs, a1; per up block: fuse, 4 growth convs, a1."""
    from image_denoising_amd import _lib

    N, _, H, W = x.shape
    desc = (ctypes.c_int64 * (3 * 64))()
    n = ctypes.c_int()
    _lib.call("dn_iunet_debug_buffers", ctypes.byref(net._cfg), N, H, W, 1, desc, 64,
              ctypes.byref(n))
    if tr is None:  # (name, tensor) of every traced activation: only names and shapes are used
        tr = []
        with torch.no_grad():
            iunet_ref.forward(net.flat_params.cpu().double(), x.double(), C, net.out_nc, trace=tr)
    fws = ws.view(torch.float32)
    dev = {}
    for i, (name, ref) in enumerate(tr):
        off, stride, lvl = desc[3 * i], desc[3 * i + 1], desc[3 * i + 2]
        h, w, ch = H >> lvl, W >> lvl, ref.shape[1]
        t = fws[off:off + N * h * w * stride].view(N, h, w, stride)[..., :ch]
        dev[name] = t.permute(0, 3, 1, 2).cpu().double() > 0
    masks = [dev["h"]]

    def rdb(k, with_input):
        F_ = dev[f"{k}:F"]
        c0 = F_.shape[1] - 4 * 32
        if with_input:
            masks.append(F_[:, :c0])
        masks.extend(F_[:, c0 + 32 * j:c0 + 32 * j + 32] for j in range(4))

    for i in range(4):
        rdb(f"downs.{i}.2", True)
        masks.append(dev[f"downs.{i}.3:a1"])
    rdb("bottle.0", False)
    masks.append(dev["bottle.1:a1"])
    for k in range(4):
        rdb(f"ups.{k}.rdb", True)
        masks.append(dev[f"ups.{k}.res:a1"])
    return masks


class _MaskedF:
    """torch.nn.functional for the oracle, with leaky_relu taking the given decisions"""

    def __init__(self, masks):
        self.masks = list(masks)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def leaky_relu(self, z, slope):
        m = self.masks.pop(0)
        assert m.shape == z.shape, (m.shape, z.shape)
        return torch.where(m, z, z * slope)


@pytest.mark.parametrize("C", [1, 3])
def test_x6_grads_as_accurate_as_fp32_vs_fp64(golden, C, monkeypatch):
    """The split-bf16 3x3 convs against an fp64 oracle run on the golden input that takes the
    device's own LeakyReLU decisions (where a pre-activation lies within fp32 rounding of
    zero, two correct fp32 implementations may take different slopes, and on these small
    images every gradient upstream then moves by up to ~1e-2; iunet_c3 has such a point in
    ups.2).  Per-tensor gradient error must be of the size of the fp32 kernels' own."""
    g = golden(f"iunet_c{C}.npz")
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    N, _, H, W = x.shape
    net = _net(C).to(DEV)
    errs = {}
    for prec in PRECS:
        net.set_precision(prec)
        ws = net._workspace(N, H, W, with_backward=True, fresh=True)
        y = torch.empty(x.shape, device=DEV)
        net._run_forward(x.to(DEV), y, ws)
        masks = _device_leaky_masks(net, ws, x, C)
        mf = _MaskedF(masks)
        monkeypatch.setattr(iunet_ref, "F", mf)
        p = net.flat_params.cpu().double().requires_grad_(True)
        y64 = iunet_ref.forward(p, x.double(), C, C)
        ((y64 - t.double()) ** 2).mean().backward()
        monkeypatch.undo()
        assert not mf.masks
        ref = p.grad.numpy()
        dy = (2.0 / y.numel()) * (y - t.to(DEV))
        gr = torch.empty_like(net.flat_params)
        net._run_backward(dy.contiguous(), gr, ws, N, H, W)
        gr = gr.cpu().numpy()
        off, per = 0, []
        for _, sh in iunet_ref.layer_table(C, C):
            k = int(np.prod(sh))
            per.append(rel_err(gr[off:off + k], ref[off:off + k]))
            off += k
        errs[prec] = (rel_err(y.cpu().numpy(), y64.detach().numpy()), np.array(per))
    (e32, p32), (e6, p6) = errs["fp32"], errs["fp32_x6"]
    print(f"\nC={C} y: fp32 {e32:.2e} x6 {e6:.2e}; grad max: fp32 {p32.max():.2e} x6 "
          f"{p6.max():.2e}; median: fp32 {np.median(p32):.2e} x6 {np.median(p6):.2e}")
    assert e6 < FP32_TOL and e6 < 4 * e32 + 1e-7, (e6, e32)
    assert p6.max() < 4 * p32.max() + 1e-7, (p6.max(), p32.max())
    assert np.median(p6) < 4 * np.median(p32) + 1e-7, (np.median(p6), np.median(p32))


# (in_nc, out_nc), N x H x W, input seed.  The channel counts pick kernels: k_conv3_thin with 2 and
# 4 outputs, the final conv's K = 24 + in_nc behind the stride-28 cf, the sigmoid gradient of 2
# and 4 outputs into the stride-4 buffer, the sigma map's gradient beside 2 input channels.  The
# seeds are the first at which the fp64 oracle's pool windows all have a winner by >= 1e-5.
CHANNEL_CASES = [(2, 2, 2, 32, 48, 7), (1, 4, 1, 32, 48, 2), (3, 2, 1, 48, 32, 3),
                 (2, 1, 1, 32, 32, 1)]


@pytest.mark.parametrize("C,OC,N,H,W,seed", CHANNEL_CASES)
def test_grads_per_tensor_vs_fp64_channel_counts(C, OC, N, H, W, seed, monkeypatch):
    """y and every parameter tensor's gradient at in_nc 2, out_nc 2 and 4 and in_nc != out_nc,
    against the fp64 oracle under the device's own LeakyReLU decisions: y < 1e-4 and each tensor
    < GRAD_TOL for both arithmetics, the bf16x6 errors of the size of the fp32 kernels' own (as
    test_x6_grads_as_accurate_as_fp32_vs_fp64)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((N, C, H, W), generator=gen)
    assert _pool_gap(x, C, OC) >= 1e-5
    dy = torch.randn((N, OC, H, W), generator=gen)
    net = _net(C, out_nc=OC).to(DEV)
    table = iunet_ref.layer_table(C, OC)
    errs, refs = {}, []
    for prec in PRECS:
        net.set_precision(prec)
        ws = net._workspace(N, H, W, with_backward=True, fresh=True)
        y = torch.empty((N, OC, H, W), device=DEV)
        net._run_forward(x.to(DEV), y, ws)
        masks = _device_leaky_masks(net, ws, x, C)
        # the fp64 oracle under this run's LeakyReLU decisions (one reference when both agree)
        ref = next((r for m, r in refs if all(torch.equal(a, b) for a, b in zip(m, masks))), None)
        if ref is None:
            mf = _MaskedF(masks)
            monkeypatch.setattr(iunet_ref, "F", mf)
            p = net.flat_params.cpu().double().requires_grad_(True)
            y64 = iunet_ref.forward(p, x.double(), C, OC)
            y64.backward(dy.double())
            monkeypatch.undo()
            assert not mf.masks
            ref = (y64.detach().numpy(), p.grad.numpy())
            refs.append((masks, ref))
        gr = torch.full_like(net.flat_params, float("nan"))
        net._run_backward(dy.to(DEV), gr, ws, N, H, W)
        gr = gr.cpu().numpy()
        off, per = 0, []
        for _, sh in table:
            k = int(np.prod(sh))
            per.append(rel_err(gr[off:off + k], ref[1][off:off + k]))
            off += k
        assert off == gr.size
        errs[prec] = (rel_err(y.cpu().numpy(), ref[0]), np.array(per))
    (e32, p32), (e6, p6) = errs["fp32"], errs["fp32_x6"]
    print(f"\n{(C, OC)} {(N, H, W)} y: fp32 {e32:.2e} x6 {e6:.2e}; grad max: fp32 {p32.max():.2e} x6 "
          f"{p6.max():.2e}; median: fp32 {np.median(p32):.2e} x6 {np.median(p6):.2e}; "
          f"final.weight: fp32 {p32[-2]:.2e} x6 {p6[-2]:.2e}")
    assert e32 < FP32_TOL and e6 < FP32_TOL and e6 < 4 * e32 + 1e-7, (e6, e32)
    bad = [(table[i][0], p32[i], p6[i]) for i in range(len(table))
           if not (p32[i] < GRAD_TOL and p6[i] < GRAD_TOL)]
    assert not bad, bad[:8]
    assert p6.max() < 4 * p32.max() + 1e-7, (p6.max(), p32.max())
    assert np.median(p6) < 4 * np.median(p32) + 1e-7, (np.median(p6), np.median(p32))


def _profiled_step(net, x, dy, ws, tr=None):
    """forward + backward on ws under the launch profiler -> (y, flat gradient, launch records,
    the device's LeakyReLU decisions when given the oracle's trace `tr`)"""
    from image_denoising_amd import _lib

    N, C, H, W = x.shape
    y = torch.empty(x.shape, device=DEV)
    grad = torch.empty_like(net.flat_params)
    _lib.profile_ops(True)
    try:
        net._run_forward(x.to(DEV), y, ws)
        masks = _device_leaky_masks(net, ws, x, C, tr) if tr is not None else None
        net._run_backward(dy.to(DEV), grad, ws, N, H, W)
        recs = _lib.profile_ops_take()
    finally:
        _lib.profile_ops(False)
    return y, grad, recs, masks


@pytest.mark.parametrize("shape,seed", [((1, 1, 32, 128), 3), ((2, 3, 32, 128), 17)])
def test_wide_levels_take_x6_weight_gradient_vs_fp64(shape, seed, monkeypatch):
    """128 pixels is the smallest width at which the bottleneck (8 wide: k_wgrad3p<3,96>) and
    level 3 (16 wide: k_wgrad3p<4,96>) take the blocked bf16x6 weight gradient, in 2 / 4 / 8
    output-channel blocks for the 192 / 384 / 768-output layers, and their growth convs
    (Cin = 192 .. 480) the 32-wide split kernels.  What ran is asserted from the launch records;
    y and all 174 parameter gradients are compared per tensor with the fp64 oracle under the
    device's own LeakyReLU decisions, the bf16x6 errors held to the size of the fp32 kernels'."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    assert _pool_gap(x, C) >= 1e-5
    dy = torch.randn(shape, generator=gen)
    net = _net(C).to(DEV)
    table = iunet_ref.layer_table(C, C)
    assert len(table) == 174
    wide = [i for i, (_, sh) in enumerate(table) if len(sh) == 4 and sh[0] in (192, 384, 768)]
    monkeypatch.delenv("DN_WG_SLAB_SCALAR", raising=False)
    tr = []  # the oracle's traced activations: their names and shapes locate the device's
    with torch.no_grad():
        iunet_ref.forward(net.flat_params.cpu(), x, C, C, trace=tr)
    errs, refs = {}, []
    for prec in PRECS:
        net.set_precision(prec)
        ws = net._workspace(N, H, W, with_backward=True, fresh=True)
        y, grad, recs, masks = _profiled_step(net, x, dy, ws, tr)
        wg = [r for r in recs if r["op"] == "wgrad3"]
        w96 = [r for r in wg if r["NOUT"] in (192, 384, 768)]
        w32 = [r for r in wg if r["NOUT"] == 32 and r["W"] <= W >> 3]
        assert {r["NOUT"] for r in w96} == {192, 384, 768} and len(w32) == 4 * 3, (w96, w32)
        if prec == "fp32_x6":
            for r in w96:  # 16-pixel stages from 16-wide rows up, 8-pixel ones at the bottleneck
                want = "k_wgrad3p<3,96>" if r["W"] < 16 else "k_wgrad3p<4,96>"
                assert r["kernel"] == want, r
            assert {r["kernel"] for r in w96 if r["NOUT"] == 768} == {"k_wgrad3p<3,96>"}
            assert {"k_wgrad3p<3,96>", "k_wgrad3p<4,96>"} <= {r["kernel"] for r in w96 if r["NOUT"] == 384}
            assert all(r["kernel"].startswith("k_wgrad3s<2,1,") for r in w32), w32
            assert max(r["K"] for r in w32) == 480 and min(r["K"] for r in w32) == 192, w32
        else:
            bad = [r for r in recs if r["kernel"].startswith(("k_wgrad3p", "k_wgrad3s", "k_wgrad3q"))]
            assert not bad, bad
        # the fp64 oracle under this run's LeakyReLU decisions (one reference when both agree)
        ref = next((r for m, r in refs if all(torch.equal(a, b) for a, b in zip(m, masks))), None)
        if ref is None:
            mf = _MaskedF(masks)
            monkeypatch.setattr(iunet_ref, "F", mf)
            p = net.flat_params.cpu().double().requires_grad_(True)
            y64 = iunet_ref.forward(p, x.double(), C, C)
            y64.backward(dy.double())
            monkeypatch.undo()
            assert not mf.masks
            ref = (y64.detach().numpy(), p.grad.numpy())
            refs.append((masks, ref))
        gr = grad.cpu().numpy()
        off, per = 0, []
        for _, sh in table:
            k = int(np.prod(sh))
            per.append(rel_err(gr[off:off + k], ref[1][off:off + k]))
            off += k
        assert off == gr.size
        errs[prec] = (rel_err(y.cpu().numpy(), ref[0]), np.array(per))
        if prec == "fp32_x6":
            # dword slab stores instead of the staged float4 rows: the same bits
            monkeypatch.setenv("DN_WG_SLAB_SCALAR", "1")
            _, grad_sc, recs_sc, _ = _profiled_step(net, x, dy, ws)
            monkeypatch.delenv("DN_WG_SLAB_SCALAR")
            k_sc = [r["kernel"] for r in recs_sc if r["kernel"].startswith("k_wgrad3p")]
            assert len(k_sc) >= len(w96) and all(k.endswith(" dword") for k in k_sc), k_sc
            assert torch.equal(grad.view(torch.int32), grad_sc.view(torch.int32))
    (e32, p32), (e6, p6) = errs["fp32"], errs["fp32_x6"]
    print(f"\n{shape} y: fp32 {e32:.2e} x6 {e6:.2e}; grad max: fp32 {p32.max():.2e} x6 "
          f"{p6.max():.2e}; median: fp32 {np.median(p32):.2e} x6 {np.median(p6):.2e}")
    for i in wide:
        print(f"  {table[i][0]} {tuple(table[i][1])}: fp32 {p32[i]:.2e} x6 {p6[i]:.2e}")
    assert e32 < FP32_TOL and e6 < FP32_TOL and e6 < 4 * e32 + 1e-7, (e6, e32)
    bad = [(table[i][0], p32[i], p6[i]) for i in range(len(table))
           if p32[i] > GRAD_TOL or p6[i] > GRAD_TOL]
    assert not bad, bad[:8]
    assert p6.max() < 4 * p32.max() + 1e-7, (p6.max(), p32.max())
    assert np.median(p6) < 4 * np.median(p32) + 1e-7, (np.median(p6), np.median(p32))
