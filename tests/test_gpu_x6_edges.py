"""The Winograd kernel k_c3w6 (csrc/conv_w6.hip) and the split-bf16 weight-gradient kernels
k_wgrad3p / k_wgrad3q (csrc/wgrad_x6p.hip) where their tiles do not fit: sides that are no
multiple of the 8 x 16 tile (a last tile row of 1 / 3 / 5 rows, a last tile column of 1 / 2 / 8
pixels, half an F(2,3) output pair), widths one past a weight-gradient stage width, and strided
views of wider buffers.  Every operand and result lives in a guarded buffer (x6_edge_util):
input gap channels and guard bands hold NaN, outputs are prefilled with NaN, and after the call
the guard bands and gap channels must be untouched bit for bit and the result finite.  Each case
asserts, from the launch profiler's record, the kernel it means to exercise; the default
dispatcher routes, no environment variable.  Tolerances are test_gpu_x6.py's, against an fp64
PyTorch reference on the CPU, per region (interior, border ring, last partial tile row /
column).  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from x6_edge_util import assert_regions, gemm_flops, guarded, ran_kernel, run_dgrad, run_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
# |err| / max|ref| against fp64 (tests/test_gpu_x6.py)
X6_TOL = 2e-6
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


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- forward -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _fwd_case(cin, cout, N, H, W):
    """inputs (NHWC fp32) and the fp64 pre-activation reference (NHWC), once per shape"""
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    return nhwc(x), w, b, ref, {}


def _forward(case, act, x_stride, y_stride, lead, x6, prefix=None):
    """one forward through the C-ABI on guarded views -> (y [N,H,W,cout] on the CPU, label)"""
    x, w, b = case[:3]
    return run_forward(L(), x, w, b, act, x_stride, y_stride, lead, x6, prefix, DEV)


def _fwd_ref(case, act):
    ref = case[3]
    return (F.leaky_relu(ref, 0.2) if act else ref).numpy()


def _fwd_e32(case, act):
    """the fp32 kernel's own error on this shape (dense views), once per (shape, act); None
    where the fp32 op kernels are not built for the channel counts"""
    cache = case[4]
    if act not in cache:
        cin, cout = case[0].shape[3], case[1].shape[0]
        try:
            y32, _ = _forward(case, act, cin, cout, 0, False)
            cache[act] = rel_err(y32.numpy(), _fwd_ref(case, act))
        except L().DenoiseHipError:
            cache[act] = None
    return cache[act]


def _check_fwd(case, act, y, label):
    ref = _fwd_ref(case, act)
    e6 = assert_regions(y.numpy(), ref, X6_TOL, what=label)
    e32 = _fwd_e32(case, act)
    print(f"fwd {tuple(case[0].shape)} -> {case[1].shape[0]} act {act} {label}: e6 {e6:.3e} "
          f"e32 {e32 if e32 is None else format(e32, '.3e')}")
    if e32 is not None:
        assert e6 < 4 * e32 + 1e-7, (e6, e32)  # fp32-class, not bf16-class


# (cin, cout, N, H, W) -> the instantiation the dispatcher picks (x6_tail_mode of cin)
W6_FWD = [
    # 2 x 2 tiles per image, all on a border; a 1-row second tile row, a 1-pixel second tile
    # column (half an F(2,3) pair); 128 * 2 * 2 = 512 tiles, the smallest Winograd launch
    (96, 96, 128, 9, 17, "k_c3w6<0,96>"),
    # interior tiles, a 3-row and a 1-pixel remainder; 32 * 4 * 4 = 512
    (96, 96, 32, 27, 49, "k_c3w6<0,96>"),
    # one partial tile row only (H < 8), an 8-wide last column; 64 * 1 * 8 = 512
    (96, 96, 64, 5, 120, "k_c3w6<0,96>"),
    # even remainders: a whole pair in the last column
    (96, 96, 32, 26, 50, "k_c3w6<0,96>"),
    # tail modes at 96 outputs (4- and 16-channel last chunks; a 24-channel full-mode one)
    (100, 96, 32, 27, 49, "k_c3w6<1,96>"),
    (144, 96, 32, 27, 49, "k_c3w6<2,96>"),
    (120, 96, 32, 27, 49, "k_c3w6<0,96>"),
    # 48 outputs: one position per wave (tail 2 / full) and the two-position tail-1 layout
    (48, 48, 128, 9, 17, "k_c3w6<2,48>"),
    (96, 48, 32, 27, 49, "k_c3w6<0,48>"),
    (36, 48, 32, 27, 49, "k_c3w6<1,48>"),
    (56, 48, 32, 27, 49, "k_c3w6<0,48>"),
]


# (the shape is the outermost loop: one reference per shape)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("cin,cout,N,H,W,kernel", W6_FWD)
def test_edges_w6_forward(cin, cout, N, H, W, kernel, act, view):
    case = _fwd_case(cin, cout, N, H, W)
    # strided: both views inside wider pixels, both base pointers 4 floats into their buffers
    xs, ys, lead = (cin, cout, 0) if view == "dense" else (cin + 12, cout + 4, 4)
    y, label = _forward(case, act, xs, ys, lead, True, kernel)
    _check_fwd(case, act, y, label)


@pytest.mark.parametrize("act", [0, 1])
def test_edges_forward_unaligned_stride_falls_back(act):
    """x_stride = 97 floats: no 16-byte pixel rows, so the dispatcher must leave the Winograd
    kernel (and every float4-row kernel) for a direct one, which meets the same bound."""
    case = _fwd_case(96, 96, 32, 27, 49)
    y, label = _forward(case, act, 97, 100, 4, True, None)
    assert not label.startswith("k_c3w6"), label
    _check_fwd(case, act, y, label)


# ---- data gradient -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dgrad_case(cin, cout, N, H, W):
    g = torch.Generator().manual_seed(cin + 7 * cout + H)
    x = torch.randn(N, cin, H, W, generator=g).double().requires_grad_(True)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    dz = torch.randn(N, cout, H, W, generator=g)
    mask = torch.randn(N, cin, H, W, generator=g)
    base = torch.randn(N, cin, H, W, generator=g)
    F.conv2d(x, w.double(), None, padding=1).backward(dz.double())
    return nhwc(dz), w, nhwc(mask), nhwc(base), nhwc(x.grad), {}


def _dgrad_ref(case, mode):
    mask, base, grad = case[2], case[3], case[4]
    if mode == "mask":
        grad = torch.where(mask.double() > 0, grad, grad * 0.2)
    if mode == "accum":
        grad = grad + base.double()
    return grad.numpy()


def _dgrad(case, mode, dx_stride, mask_stride, lead, x6, prefix=None):
    dz, w, mask, base = case[:4]
    return run_dgrad(L(), dz, w, mask, base, mode, dx_stride, mask_stride, lead, x6, prefix, DEV)


def _dgrad_e32(case, mode):
    cache = case[5]
    if mode not in cache:
        cin = case[1].shape[1]
        try:
            d32, _ = _dgrad(case, mode, cin, cin, 0, False)
            cache[mode] = rel_err(d32.numpy(), _dgrad_ref(case, mode))
        except L().DenoiseHipError:
            cache[mode] = None
    return cache[mode]


# (cin, cout, N, H, W): K = cout, the outputs are the cin channels (48-channel blocks over
# blockIdx.z above 96)
W6_DGRAD = [
    (96, 96, 128, 9, 17, "k_c3w6<0,96>"),
    (96, 96, 32, 27, 49, "k_c3w6<0,96>"),
    (48, 48, 128, 9, 17, "k_c3w6<2,48>"),
    # three 48-channel output blocks: 11 * 16 * 3 = 528 tiles, the block count carries the launch
    # over the threshold
    (144, 96, 11, 27, 49, "k_c3w6<0,48>"),
    (120, 96, 11, 27, 49, "k_c3w6<0,48>"),  # the last block holds 24 live channels
    (96, 80, 32, 27, 49, "k_c3w6<2,96>"),   # K = 80: a 16-channel tail chunk
    (96, 4, 32, 27, 49, "k_c3w6<1,96>"),    # K = 4: the 4-channel tail chunk alone
]


@pytest.mark.parametrize("mode", ["plain", "mask", "accum"])
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("cin,cout,N,H,W,kernel", W6_DGRAD)
def test_edges_w6_backward_data(cin, cout, N, H, W, kernel, mode, view):
    case = _dgrad_case(cin, cout, N, H, W)
    dxs, ms, lead = (cin, cin, 0) if view == "dense" else (cin + 4, cin + 8, 4)
    dx, label = _dgrad(case, mode, dxs, ms, lead, True, kernel)
    ref = _dgrad_ref(case, mode)
    e6 = assert_regions(dx.numpy(), ref, X6_TOL, what=f"{label} {mode}")
    e32 = _dgrad_e32(case, mode)
    print(f"dgrad {cin}<-{cout} {N}x{H}x{W} {mode} {view} {label}: e6 {e6:.3e} "
          f"e32 {e32 if e32 is None else format(e32, '.3e')}")
    if e32 is not None:
        assert e6 < 4 * e32 + 1e-7, (e6, e32)


# ---- weight gradient ---------------------------------------------------------------------------
def _wgrad(dz, x, x_stride, lead, x6, prefix=None):
    """dz, x NHWC on the CPU; x read at x_stride from `lead` floats into a NaN-filled buffer;
    dwb (NaN-prefilled) between guard bands"""
    _lib = L()
    N, H, W, cout = dz.shape
    cin = x.shape[3]
    n = cout * cin * 9 + cout
    nbytes = _lib.lib().dn_conv2d_wgrad_slab_size(N, H, W, cin, cout, 3)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    gd = guarded((1, 1, 1, n), n, 4, NAN, DEV)
    gdz = guarded((N, H, W, cout), cout, 0, NAN, DEV)
    gdz.data.copy_(dz)
    gx = guarded((N, H, W, cin), x_stride, lead, NAN, DEV)
    gx.data.copy_(x)
    if x6:
        with ran_kernel(_lib, prefix) as ran:
            _lib.call("dn_conv2d_backward_weight_x6", gdz.ptr, gx.ptr, x_stride, N, H, W, cin,
                      cout, gd.ptr, slab.data_ptr(), S())
        rec = ran.record
        assert (rec["op"], rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == \
            ("wgrad3", cin, cout, N, H, W), rec
        assert rec["flops"] == gemm_flops(rec), rec
        label = ran.kernel
    else:
        _lib.call("dn_conv2d_backward_weight", gdz.ptr, gx.ptr, x_stride, N, H, W, cin, cout, 3,
                  gd.ptr, slab.data_ptr(), S())
        label = "fp32"
    torch.cuda.synchronize()
    gd.check(what=f"dwb ({label})")
    gx.check(what=f"x ({label})")
    gdz.check(what=f"dz ({label})")
    return gd.data.reshape(-1).cpu().numpy(), label


# (cin, cout, N, H, W, x_stride or None = dense, lead, kernel): every routing class of
# launch_wgrad3p
WGRAD = [
    # enc_conv4's launch: 256 splits of 2 stages
    (48, 48, 64, 16, 16, None, 0, "k_wgrad3p<4,48>"),
    (96, 96, 64, 8, 8, None, 0, "k_wgrad3p<3,96>"),
    # widths one past a stage width (8, 16, 32, 128)
    (96, 96, 2, 9, 17, None, 0, "k_wgrad3p<4,96>"),
    (96, 96, 4, 10, 11, None, 0, "k_wgrad3p<3,96>"),
    (96, 96, 2, 7, 33, None, 0, "k_wgrad3p<4,96>"),
    (48, 48, 2, 7, 33, None, 0, "k_wgrad3p<4,48>"),
    (48, 48, 2, 6, 130, None, 0, "k_wgrad3q<4>"),  # a ragged last stage
    (48, 48, 4, 5, 9, None, 0, "k_wgrad3p<3,48>"),
    # x = the skip half of a concat buffer: 48 channels into wider NaN-filled pixels
    (96, 96, 2, 20, 36, 96 + 48, 48, "k_wgrad3p<4,96>"),
    (48, 48, 3, 24, 40, 48 + 48, 48, "k_wgrad3p<4,48>"),
    (100, 96, 2, 16, 16, 104, 4, "k_wgrad3p<4,96>"),  # a partial 32-channel block, 4 gap channels
]


@pytest.mark.parametrize("cin,cout,N,H,W,x_stride,lead,kernel", WGRAD)
def test_edges_backward_weight(cin, cout, N, H, W, x_stride, lead, kernel):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, cin, H, W, generator=g)
    dz = torch.randn(N, cout, H, W, generator=g)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, padding=1).backward(dz.double())
    nw = cout * cin * 9
    ref_w, ref_b = w.grad.numpy().reshape(-1), b.grad.numpy()
    xs = cin if x_stride is None else x_stride
    o6, label = _wgrad(nhwc(dz), nhwc(x), xs, lead, True, kernel)
    o32, _ = _wgrad(nhwc(dz), nhwc(x), xs, lead, False)
    assert np.isfinite(o6).all(), f"{label}: non-finite or unwritten gradients"
    e6, e32 = rel_err(o6[:nw], ref_w), rel_err(o32[:nw], ref_w)
    eb = rel_err(o6[nw:], ref_b)
    print(f"wgrad {cin}->{cout} {N}x{H}x{W} stride {xs} {label}: e6 {e6:.3e} e32 {e32:.3e} "
          f"bias {eb:.3e}")
    assert e6 < X6_TOL, (e6, e32)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)
    assert eb < X6_TOL, eb
