"""The ImprovedUNet executor's weight gradient as an op (dn_conv2d_backward_weight_blocked: the
launch sequence of iunet.cpp's wgrad_g -- any Cout in output-channel blocks of 96 / 48 / 32 over
blockIdx.z, views with a channel offset) at the layer shapes of the wide levels, which the
whole-network tests reach only from 128-pixel-wide images up: the 192-channel level 3, the
384-channel bottleneck and the 768-output conv_ps on k_wgrad3p<.,96> with 2 / 4 / 8 blocks
(co_base / cout_total set), the 32-wide growth convs with Cin = 224 .. 480 on k_wgrad3s<2,1,.>,
the 24-channel top level, the KW < 8 fallback and the 1x1 local-feature-fusion convs.  Both
operands are slices (nonzero channel offset) of wider NaN-filled pixels between NaN guard bands
(x6_edge_util), dwb and the slab are NaN-prefilled between guard bands (an element a kernel skips
reaches dwb as NaN through the reduction), the kernel is asserted from the launch profiler's
record, and the result is compared with the fp64 autograd of F.conv2d at test_gpu_x6.py's
bound.  The 96-block launches also run with DN_WG_SLAB_SCALAR=1 (dword slab stores): the two
epilogues must agree bit for bit.  Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from x6_edge_util import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
X6_TOL = 2e-6  # |err| / max|ref| against fp64 (tests/test_gpu_x6.py)
NAN = float("nan")
PREC = {"fp32": 0, "fp32_x6": 2}  # DN_PREC_FP32 / DN_PREC_FP32_X6


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


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _case(ksize, cin, cout, N, H, W):
    """-> (dz NHWC, x NHWC, fp64 dw flat, fp64 db)"""
    g = torch.Generator().manual_seed(1000 * ksize + cin + 7 * cout + H + W)
    x = torch.randn(N, cin, H, W, generator=g)
    dz = torch.randn(N, cout, H, W, generator=g)
    w = torch.zeros(cout, cin, ksize, ksize, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, padding=ksize // 2).backward(dz.double())
    return nhwc(dz), nhwc(x), w.grad.numpy().reshape(-1), b.grad.numpy()


def _run(dz, x, ksize, bias, prec):
    """one call on guarded slices -> (dwb on the CPU, the launch record of the GEMM kernel)"""
    _lib = L()
    N, H, W, cout = dz.shape
    cin = x.shape[3]
    n = cout * cin * ksize * ksize + (cout if bias else 0)
    nfl = _lib.lib().dn_conv2d_wgrad_blocked_slab_size(N, H, W, cin, cout, ksize) // 4
    assert nfl >= 64 + n
    gs = guarded((1, 1, 1, nfl), nfl, 0, NAN, DEV)
    gd = guarded((1, 1, 1, n), n, 4, NAN, DEV)
    # g: channels [4, 4 + cout) of (cout + 8)-channel pixels; x: channels [8, 8 + cin) of
    # (cin + 12)-channel pixels.  The guarded buffer's live channels are the slice, so the base
    # pointer of the view lies `off` floats before it (inside the front guard band's lead).
    g_off, g_stride, x_off, x_stride = 4, cout + 8, 8, cin + 12
    gdz = guarded((N, H, W, cout), g_stride, 8, NAN, DEV)
    gdz.data.copy_(dz)
    gx = guarded((N, H, W, cin), x_stride, 8, NAN, DEV)
    gx.data.copy_(x)
    op = "wgrad3" if ksize == 3 else "wgrad1"
    _lib.profile_ops(True)
    try:
        _lib.call("dn_conv2d_backward_weight_blocked", gdz.ptr - 4 * g_off, g_stride, g_off,
                  gx.ptr - 4 * x_off, x_stride, x_off, N, H, W, cin, cout, ksize, int(bias),
                  PREC[prec], gd.ptr, gs.ptr, S())
        recs = [r for r in _lib.profile_ops_take() if r["op"] == op]
    finally:
        _lib.profile_ops(False)
    torch.cuda.synchronize()
    assert len(recs) == 1, recs
    rec = recs[0]
    assert (rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == (cin, cout, N, H, W), rec
    assert rec["flops"] == 2.0 * cin * cout * ksize * ksize * N * H * W, rec
    what = f"{prec} {rec['kernel']}"
    gs.check(what=f"slab ({what})")
    gd.check(what=f"dwb ({what})")
    gx.check(what=f"x ({what})")
    gdz.check(what=f"g ({what})")
    out = gd.data.reshape(-1).cpu().numpy()
    assert np.isfinite(out).all(), f"{what}: non-finite or unwritten gradients"
    return out, rec


# (cin, cout, N, H, W, bias, the bf16x6 kernel): the stage width (last template argument: 8 / 16
# pixel rows) follows W; k_wgrad3s<2,1,WN,.> takes 16 * WN input channels per workgroup, the
# width that pads Cin least
C3 = [
    # 96-channel blocks: 2 (level 3), 4 (bottleneck), 8 (conv_ps of up block 0)
    (192, 192, 2, 5, 9, 1, "k_wgrad3p<3,96>"),
    (192, 192, 1, 3, 17, 0, "k_wgrad3p<4,96>"),  # a ResBlock conv: no bias row
    (384, 384, 2, 5, 8, 1, "k_wgrad3p<3,96>"),
    (384, 768, 1, 4, 8, 1, "k_wgrad3p<3,96>"),
    (576, 192, 1, 4, 16, 1, "k_wgrad3p<4,96>"),  # the level-3 fuse conv
    (208, 192, 1, 4, 16, 1, "k_wgrad3p<4,96>"),  # Cin % 32 != 0: a last input block of 16
    # 32-wide growth convs of level 3 and the bottleneck
    (224, 32, 2, 5, 9, 1, "k_wgrad3s<2,1,2,3>"),
    (288, 32, 2, 5, 9, 1, "k_wgrad3s<2,1,3,3>"),
    (416, 32, 2, 5, 9, 1, "k_wgrad3s<2,1,2,3>"),
    (480, 32, 2, 5, 9, 1, "k_wgrad3s<2,1,3,3>"),
    (256, 32, 2, 5, 9, 1, "k_wgrad3s<2,1,4,3>"),
    # the 24-channel top level
    (24, 24, 2, 8, 16, 0, "k_wgrad3s<2,1,2,4>"),
    (56, 32, 2, 8, 16, 1, "k_wgrad3s<2,1,4,4>"),
    # rows under 8 pixels: bf16x6 requested, the fp32 kernel runs
    (192, 192, 2, 4, 4, 1, "k_wgrad3"),
]


@pytest.mark.parametrize("cin,cout,N,H,W,bias,kernel", C3)
def test_blocked_weight_gradient_3x3(cin, cout, N, H, W, bias, kernel, monkeypatch):
    monkeypatch.delenv("DN_WG_SLAB_SCALAR", raising=False)
    dz, x, ref_w, ref_b = _case(3, cin, cout, N, H, W)
    nw = ref_w.size
    o32, r32 = _run(dz, x, 3, bias, "fp32")
    o6, r6 = _run(dz, x, 3, bias, "fp32_x6")
    assert r32["kernel"] == "k_wgrad3", r32
    assert r6["kernel"] == kernel, r6
    e32, e6 = rel_err(o32[:nw], ref_w), rel_err(o6[:nw], ref_w)
    eb32 = rel_err(o32[nw:], ref_b) if bias else 0.0
    eb6 = rel_err(o6[nw:], ref_b) if bias else 0.0
    print(f"\nwgrad3 blocked {cin}->{cout} {N}x{H}x{W} {r6['kernel']}: e6 {e6:.3e} e32 {e32:.3e} "
          f"bias e6 {eb6:.3e} e32 {eb32:.3e}")
    assert e32 < X6_TOL and eb32 < X6_TOL, (e32, eb32)
    assert e6 < X6_TOL and eb6 < X6_TOL, (e6, eb6)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)
    if kernel.startswith("k_wgrad3p"):
        monkeypatch.setenv("DN_WG_SLAB_SCALAR", "1")
        osc, rsc = _run(dz, x, 3, bias, "fp32_x6")
        monkeypatch.delenv("DN_WG_SLAB_SCALAR")
        assert rsc["kernel"] == kernel + " dword", rsc
        assert np.array_equal(o6.view(np.int32), osc.view(np.int32)), \
            "staged float4 slab rows and dword stores differ"


# the local-feature-fusion convs of level 0 and of the bottleneck (fp32 kernels in both precisions)
C1 = [
    (152, 24, 2, 8, 16, "k_wgrad1<3,6,1,3>"),
    (512, 384, 2, 2, 8, "k_wgrad1<6,6,2,2>"),
]


@pytest.mark.parametrize("prec", ["fp32", "fp32_x6"])
@pytest.mark.parametrize("cin,cout,N,H,W,kernel", C1)
def test_blocked_weight_gradient_1x1(cin, cout, N, H, W, kernel, prec):
    dz, x, ref_w, ref_b = _case(1, cin, cout, N, H, W)
    nw = ref_w.size
    o, rec = _run(dz, x, 1, 1, prec)
    assert rec["kernel"] == kernel, rec
    e, eb = rel_err(o[:nw], ref_w), rel_err(o[nw:], ref_b)
    print(f"\nwgrad1 blocked {cin}->{cout} {N}x{H}x{W} {prec} {rec['kernel']}: e {e:.3e} "
          f"bias {eb:.3e}")
    assert e < X6_TOL and eb < X6_TOL, (e, eb)
