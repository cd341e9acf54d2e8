"""The staged slab epilogue of the split-bf16 3x3 weight-gradient kernels (k_wgrad3p, k_wgrad3q,
csrc/wgrad_x6p.hip): after the stage loop a workgroup's partial gradients go through LDS as
rows [co][ci * 9 + t] and leave as 16-byte stores.  What such stores could get wrong is a row
end, a masked channel block or a slab row, so every per-kernel case runs with the slab between
NaN-filled guard bands (x6_edge_util) and its inside prefilled with NaN (an element the kernel
skips reaches dwb as NaN through the reduction), checks the gradient against an fp64 numpy
restatement at test_gpu_x6.py's bounds, asserts the kernel from the launch profiler's record,
and calls twice for bit-identical results.  A launch that keeps the dword stores is labelled
"... dword" by the library, so the exact label also says that the staged epilogue ran.
dec_conv1a's launch (96 input channels of a weight with 97: rows of 97 x 9 floats do not start
on 16 B) keeps the dword stores and is only reachable through the executor: the unit-gain
network test covers it and every level from 64^2 down to 2^2.  DN_WG_SLAB_SCALAR=1 (read per
launch) forces the dword stores everywhere; the two epilogues must give the same bits.  Needs
an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from x6_edge_util import guarded, ran_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda"
X6_TOL = 2e-6  # |err| / max|ref| against fp64 (tests/test_gpu_x6.py)
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


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def wgrad_ref(dz, x):
    """fp64 [W (co, ci, ky, kx) | b] of a 3x3 / pad 1 convolution; dz [N, H, W, co], x [N, H, W, ci]"""
    dz = np.asarray(dz, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    N, H, W, cout = dz.shape
    cin = x.shape[3]
    xp = np.zeros((N, H + 2, W + 2, cin))
    xp[:, 1:-1, 1:-1] = x
    g = dz.reshape(-1, cout)
    dw = np.empty((cout, cin, 3, 3))
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = g.T @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, cin)
    return np.concatenate([dw.reshape(-1), g.sum(0)])


def _wgrad(dz, x, x_stride, x6, prefix=None):
    """dz, x NHWC on the CPU -> (dwb, kernel label, splits the slab was sized for).  dwb, x (read
    at x_stride), dz and the slab all sit between NaN guard bands that must come back untouched."""
    _lib = L()
    N, H, W, cout = dz.shape
    cin = x.shape[3]
    n = cout * cin * 9 + cout
    nfl = _lib.lib().dn_conv2d_wgrad_slab_size(N, H, W, cin, cout, 3) // 4
    gs = guarded((1, 1, 1, nfl), nfl, 0, NAN, DEV)
    gd = guarded((1, 1, 1, n), n, 4, NAN, DEV)
    gdz = guarded((N, H, W, cout), cout, 0, NAN, DEV)
    gdz.data.copy_(dz)
    gx = guarded((N, H, W, cin), x_stride, 4 if x_stride > cin else 0, NAN, DEV)
    gx.data.copy_(x)
    if x6:
        with ran_kernel(_lib, prefix) as ran:
            _lib.call("dn_conv2d_backward_weight_x6", gdz.ptr, gx.ptr, x_stride, N, H, W, cin,
                      cout, gd.ptr, gs.ptr, S())
        label = ran.kernel
        assert prefix is None or label == prefix, f"ran {label!r}, expected exactly {prefix!r} (the staged epilogue)"
    else:
        _lib.call("dn_conv2d_backward_weight", gdz.ptr, gx.ptr, x_stride, N, H, W, cin, cout, 3,
                  gd.ptr, gs.ptr, S())
        label = "fp32"
    torch.cuda.synchronize()
    gs.check(what=f"slab ({label})")
    gd.check(what=f"dwb ({label})")
    gx.check(what=f"x ({label})")
    gdz.check(what=f"dz ({label})")
    # the launched split count: what the slab was sized for, capped by the route (wgrad_route.cpp) at one
    # round of 512 workgroups over the input-channel blocks (32 per block at 96 outputs, else 48)
    cib = 32 if cout == 96 else 48
    return gd.data.reshape(-1).cpu().numpy(), label, min((nfl - 64) // n, 512 // -(-cin // cib))


# (cin, cout, N, H, W, x_stride or None = dense, kernel)
CASES = [
    # k_wgrad3p<4,96>: both 48-channel halves, 3 and 5 input blocks (144: a last block of 16)
    (96, 96, 2, 16, 16, None, "k_wgrad3p<4,96>"),
    (144, 96, 2, 16, 16, None, "k_wgrad3p<4,96>"),
    (96, 96, 1, 16, 48, None, "k_wgrad3p<4,96>"),
    (144, 96, 1, 16, 48, None, "k_wgrad3p<4,96>"),
    (96, 96, 2, 8, 8, None, "k_wgrad3p<3,96>"),
    # 48 -> 48: rows of 432 floats
    (48, 48, 2, 16, 16, None, "k_wgrad3p<4,48>"),
    (48, 48, 2, 8, 8, None, "k_wgrad3p<3,48>"),
    (48, 48, 1, 128, 128, None, "k_wgrad3q<4>"),
    # ragged sides: partial stages
    (96, 96, 1, 13, 19, None, "k_wgrad3p<4,96>"),
    (48, 48, 1, 13, 19, None, "k_wgrad3p<4,48>"),
    # x = 96 channels of a 144-channel concat buffer
    (96, 96, 2, 16, 16, 144, "k_wgrad3p<4,96>"),
]


@pytest.mark.parametrize("cin,cout,N,H,W,x_stride,kernel", CASES)
def test_wgrad_slab_epilogue(cin, cout, N, H, W, x_stride, kernel):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, H, W, cin, generator=g)
    dz = torch.randn(N, H, W, cout, generator=g)
    ref = wgrad_ref(dz.numpy(), x.numpy())
    nw = cout * cin * 9
    xs = cin if x_stride is None else x_stride
    o6, label, splits = _wgrad(dz, x, xs, True, kernel)
    o6b, _, _ = _wgrad(dz, x, xs, True, kernel)
    o32, _, _ = _wgrad(dz, x, xs, False)
    assert splits > 1, splits  # more than one slab row
    assert np.isfinite(o6).all(), f"{label}: non-finite or unwritten gradients"
    e6, e32 = rel_err(o6[:nw], ref[:nw]), rel_err(o32[:nw], ref[:nw])
    eb = rel_err(o6[nw:], ref[nw:])
    print(f"wgrad {cin}->{cout} {N}x{H}x{W} stride {xs} {label} splits {splits}: e6 {e6:.3e} "
          f"e32 {e32:.3e} bias {eb:.3e}")
    assert e6 < X6_TOL, (e6, e32)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)
    assert eb < X6_TOL, eb
    assert np.array_equal(o6.view(np.int32), o6b.view(np.int32)), "two calls differ"


# ---- through the executor ----------------------------------------------------------------------
def _net(C):
    from image_denoising_amd import UNet

    torch.manual_seed(0)
    return UNet(in_nc=C, out_nc=C, n_feature=48).to(DEV).set_precision("fp32_x6")


def _unit_gain(net, seed=0):
    """weights x10 (undoing the reference's x0.1 init) and random biases: every level then
    contributes O(1) to the output and to every gradient (tests/test_gpu_parity.py)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(p.device))


ACT_NAMES = ["a0", "a1", "a2", "a3", "a4", "a5", "a6", "d2a", "d3a", "d4a", "d5a", "d2b", "d3b",
             "d4b", "d5b", "d1a", "d1b", "na", "nb"]
# dn_unet_debug_buffers order of the forward buffers
FWD_BUFS = ["c1", "a0", "a1", "c2", "c3", "c4", "c5", "a2", "a3", "a4", "a5", "p5", "a6",
            "d2a", "d3a", "d4a", "d5a", "d2b", "d3b", "d4b", "d5b", "d1a", "d1b", "na", "nb"]


def _fwd_bwd(net, x, r, want_acts=True):
    """the HIP forward + backward on a fresh workspace -> (dflat, saved activations)"""
    N, C, H, W = x.shape
    desc = (ctypes.c_int64 * 300)()
    n = ctypes.c_int()
    L().call("dn_unet_debug_buffers", ctypes.byref(net._cfg), N, H, W, 1, desc, 100,
             ctypes.byref(n))
    ws = net._workspace(N, H, W, True, fresh=True)
    y = torch.empty(N, net.out_nc, H, W, device=DEV)
    net._run_forward(x.to(DEV).contiguous(), y, ws)
    dflat = torch.empty_like(net.flat_params)
    dx = torch.full((N, C, H, W), NAN, device=DEV)
    net._run_backward(r.to(DEV).contiguous(), dflat, ws, N, H, W, dx=dx)
    torch.cuda.synchronize()
    acts = {}
    if want_acts:
        wsf = ws.view(torch.float32)
        for i, name in enumerate(FWD_BUFS):
            off, st, lvl = desc[3 * i], desc[3 * i + 1], desc[3 * i + 2]
            h, w = H >> lvl, W >> lvl
            if name in ACT_NAMES:
                acts[name] = wsf[off:off + N * h * w * st].view(N, h, w, st).permute(0, 3, 1, 2).cpu().clone()
    return dflat.cpu(), acts


@pytest.mark.parametrize("C", [1, 3])
def test_wgrad_slab_unet_unit_gain_vs_fp64(C):
    """All 50 parameter gradients of a 1 x C x 64 x 64 step against the fp64 backward that takes
    LeakyReLU slopes and pool routing from the device's activations: dec_conv1a's unaligned rows
    (the dword stores) and every small-level launch, 64^2 down to 2^2."""
    from oracle.unet_ref import forward, layer_table

    net = _net(C)
    _unit_gain(net)
    x = torch.rand(1, C, 64, 64, generator=torch.Generator().manual_seed(1))
    r = torch.randn(1, C, 64, 64, generator=torch.Generator().manual_seed(2))
    gg, acts = _fwd_bwd(net, x, r)
    p64 = net.flat_params.detach().cpu().double().requires_grad_(True)
    y64 = forward(p64, x.double(), C, C, masks=acts)
    (y64 * r.double()).sum().backward()
    g64, gg = p64.grad.numpy(), gg.numpy()
    off, count = 0, 0
    for name, ws, bl, _ in layer_table(C, C):
        n = int(np.prod(ws)) + bl
        e = rel_err(gg[off:off + n], g64[off:off + n])
        assert e < 2e-5, (name, e)
        off += n
        count += 2 if bl else 1
    assert off == gg.size and count == 50, (off, count)


def test_wgrad_slab_epilogues_agree_bitwise(monkeypatch):
    """the flat gradient of a 2 x 1 x 64 x 64 step: staged float4 rows == dword stores, bit for bit"""
    net = _net(1)
    _unit_gain(net)
    x = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(3))
    r = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(4))
    _lib = L()

    def run():
        """-> (flat gradient, labels of the k_wgrad3p / k_wgrad3q launches) under the launch profiler"""
        _lib.profile_ops(True)
        try:
            g, _ = _fwd_bwd(net, x, r, False)
            recs = _lib.profile_ops_take()
        finally:
            _lib.profile_ops(False)
        return g, [q["kernel"] for q in recs
                   if q["op"] == "wgrad3" and q["kernel"].startswith(("k_wgrad3p", "k_wgrad3q"))]

    monkeypatch.delenv("DN_WG_SLAB_SCALAR", raising=False)
    g_vec, k_vec = run()
    monkeypatch.setenv("DN_WG_SLAB_SCALAR", "1")
    g_sc, k_sc = run()
    monkeypatch.delenv("DN_WG_SLAB_SCALAR")
    # 64^2 .. 8^2: enc_conv1..4, dec_conv1b / 1a, dec_conv2..4 a / b; only dec_conv1a (97 input
    # channels) keeps the dword stores by itself
    assert len(k_vec) == len(k_sc) and len(k_vec) >= 10, (k_vec, k_sc)
    assert sum(k.endswith(" dword") for k in k_vec) == 1, k_vec
    assert all(k.endswith(" dword") for k in k_sc), k_sc
    assert torch.isfinite(g_vec).all()
    assert torch.equal(g_vec.view(torch.int32), g_sc.view(torch.int32))
