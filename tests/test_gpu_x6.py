"""The split-bf16 fp32 3x3 convolution (DN_PREC_FP32_X6, csrc/conv_x6.hip) vs an fp64 reference,
through the C-ABI.  The claim under test is fp32 accuracy: its error against fp64 must be of the
size of the fp32 matrix-core kernel's own (same shapes, same inputs), and within the 1e-4
north-star tolerance by two orders of magnitude.  Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
# |err| / max|ref| against fp64; an fp32 dot product of K ~ 1e3 terms lands near 1e-7
X6_TOL = 2e-6


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


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


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _forward(x, w, b, act, x6):
    _lib = L()
    N, cin, H, W = x.shape
    cout = w.shape[0]
    xg, wg, bg = nhwc(x).to(DEV), w.to(DEV), b.to(DEV)
    y = torch.empty(N, H, W, cout, device=DEV)
    if x6:
        pk = _lib.scratch(_lib.lib().dn_conv2d_x6_pack_size(cin, cout, 0), DEV)
        _lib.call("dn_conv2d_forward_x6", xg.data_ptr(), cin, N, H, W, cin, wg.data_ptr(),
                  bg.data_ptr(), cout, act, y.data_ptr(), cout, pk.data_ptr(), pk.numel(), S())
    else:
        pk = _lib.scratch(_lib.lib().dn_conv2d_pack_size(cin, cout, 3, 0), DEV)
        _lib.call("dn_conv2d_forward", xg.data_ptr(), cin, N, H, W, cin, wg.data_ptr(),
                  bg.data_ptr(), cout, 3, act, y.data_ptr(), cout, pk.data_ptr(), pk.numel(), S())
    return nchw(y.cpu())


@pytest.mark.parametrize("cin,cout,N,H,W", [
    (48, 48, 2, 32, 32), (48, 96, 1, 20, 36), (96, 96, 2, 16, 16), (96, 96, 2, 64, 64),
    (144, 96, 2, 16, 32), (99, 96, 2, 32, 32), (97, 48, 1, 8, 8), (3, 48, 2, 32, 32),
    (96, 96, 64, 32, 32), (48, 48, 8, 4, 4),
    # >= 512 8x16 tiles at exactly 96 / 48 outputs: the Winograd kernel k_c3w6 (tail 0 / 2 / 2);
    # 3 -> 48 is not float4-addressable and stays on the 4-wave k_c3x6.  (Which instantiation a
    # shape runs is asserted in test_gpu_x6_edges.py and test_gpu_x6_direct_edges.py, not here.)
    (96, 96, 8, 128, 128), (48, 48, 8, 128, 128), (144, 96, 8, 128, 128), (3, 48, 2, 256, 256),
    # k_c3w6 with a partial last chunk packed over fewer stages (x6_tail_mode 1 / 2)
    (100, 96, 2, 256, 256), (36, 48, 4, 128, 128), (80, 96, 8, 128, 128), (16, 48, 8, 128, 128),
    # 32 outputs (ImprovedUNet RDB growth convs): the small-grid 3-slot ring k_c3x6h<2,0,1,3>,
    # then 512 tiles on k_c3x6h<2,2,2> (a 16-channel tail chunk)
    (48, 32, 2, 32, 32), (144, 32, 1, 24, 40), (80, 32, 8, 128, 128), (112, 32, 8, 128, 128),
    # ImprovedUNet routes on large grids (k_c3x6h<2,T,2>): K 48..79 at 32 outputs, zero-padded
    # 32-wide K (88, 120), and 72 -> 24
    (48, 32, 8, 128, 128), (88, 32, 8, 128, 128), (120, 32, 8, 128, 128), (72, 24, 8, 128, 128),
])
@pytest.mark.parametrize("act", [0, 1])
def test_x6_forward_vs_fp64(cin, cout, N, H, W, act):
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    y6 = _forward(x, w, b, act, True)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if act:
        ref = F.leaky_relu(ref, 0.2)
    e6 = rel_err(y6.numpy(), ref.numpy())
    try:
        y32 = _forward(x, w, b, act, False)
    except L().DenoiseHipError:  # channel counts the fp32 op kernels are not built for
        assert e6 < X6_TOL, e6
        return
    e32 = rel_err(y32.numpy(), ref.numpy())
    assert e6 < X6_TOL, (e6, e32)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)  # fp32-class, not bf16-class (~4e-3)


def _dgrad(dz, w, cin, mode, mask, base, x6):
    _lib = L()
    N, cout, H, W = dz.shape
    dx = nhwc(base).to(DEV) if mode == "accum" else torch.zeros(N, H, W, cin, device=DEV)
    mg, dzg, wg = nhwc(mask).to(DEV), nhwc(dz).to(DEV), w.to(DEV)
    name = "dn_conv2d_backward_data_x6" if x6 else "dn_conv2d_backward_data"
    size = (_lib.lib().dn_conv2d_x6_pack_size(cin, cout, 1) if x6
            else _lib.lib().dn_conv2d_pack_size(cin, cout, 3, 1))
    pk = _lib.scratch(size, DEV)
    args = [dzg.data_ptr(), N, H, W, cout, wg.data_ptr(), cin]
    if not x6:
        args.append(3)
    args += [mg.data_ptr() if mode == "mask" else None, cin, 1 if mode == "accum" else 0,
             dx.data_ptr(), cin, pk.data_ptr(), pk.numel(), S()]
    _lib.call(name, *args)
    return nchw(dx.cpu())


@pytest.mark.parametrize("cin,cout,N,H,W", [
    (48, 48, 2, 32, 32), (96, 96, 2, 16, 16), (144, 96, 2, 16, 16), (48, 96, 2, 8, 8),
    (96, 48, 1, 20, 36), (144, 96, 1, 64, 32),
    # large grids into 96 / 48 channels or 48-channel blocks: the Winograd kernel k_c3w6
    (96, 96, 8, 128, 128), (144, 96, 3, 128, 112), (48, 48, 8, 128, 128),
    (96, 80, 8, 128, 128), (48, 16, 8, 128, 128), (96, 4, 8, 128, 128),  # ... with a tail chunk
    # 32 outputs: k_c3x6h<2,0,1,3> (small grid) and k_c3x6h<2,2,2> (512 tiles, K = 48)
    (32, 96, 2, 32, 32), (32, 48, 8, 128, 128),
    # ImprovedUNet shapes: final conv (K = out_nc), RDB growth convs (K = 32, wide outputs)
    (24, 3, 1, 32, 32), (24, 1, 2, 32, 32), (144, 32, 1, 16, 16), (112, 32, 1, 16, 16),
    (80, 32, 2, 16, 16), (120, 32, 1, 32, 32), (72, 24, 1, 32, 32),
    # ... on large grids: K = 32 data gradients into 80 / 112 / 144 channels (48-channel blocks,
    # a partial last one) and 72 -> 24
    (80, 32, 8, 128, 128), (112, 32, 8, 128, 128), (144, 32, 8, 128, 128), (72, 24, 8, 128, 128),
    # ImprovedUNet's wide levels on grids over the Winograd threshold: data gradients into 192 /
    # 384 channels in 96-channel output blocks (blockIdx.z, the per-block image stride)
    (192, 96, 8, 64, 64), (384, 96, 4, 64, 64), (192, 192, 8, 64, 64),
])
@pytest.mark.parametrize("mode", ["plain", "mask", "accum"])
def test_x6_backward_data_vs_fp64(cin, cout, N, H, W, mode):
    g = torch.Generator().manual_seed(cin + 7 * cout + H)
    x = torch.randn(N, cin, H, W, generator=g).double().requires_grad_(True)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    dz = torch.randn(N, cout, H, W, generator=g)
    mask = torch.randn(N, cin, H, W, generator=g)
    base = torch.randn(N, cin, H, W, generator=g)
    F.conv2d(x, w.double(), None, padding=1).backward(dz.double())
    ref = x.grad
    if mode == "mask":
        ref = torch.where(mask.double() > 0, ref, ref * 0.2)
    if mode == "accum":
        ref = ref + base.double()
    d6 = _dgrad(dz, w, cin, mode, mask, base, True)
    e6 = rel_err(d6.numpy(), ref.numpy())
    try:
        d32 = _dgrad(dz, w, cin, mode, mask, base, False)
    except L().DenoiseHipError:  # channel counts the fp32 op kernels are not built for
        assert e6 < X6_TOL, e6
        return
    e32 = rel_err(d32.numpy(), ref.numpy())
    assert e6 < X6_TOL, (e6, e32)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)


def test_x6_exact_on_bf16_representable_inputs():
    """Operands that are exact in bf16 leave pieces 1 and 2 zero: the result is then the exact
    product sum rounded once per MFMA accumulation, equal to fp64 to fp32 rounding."""
    g = torch.Generator().manual_seed(5)
    q = lambda t: t.to(torch.bfloat16).float()
    x = q(torch.randn(1, 96, 16, 16, generator=g))
    w = q(torch.randn(96, 96, 3, 3, generator=g) * 0.1)
    b = torch.zeros(96)
    y6 = _forward(x, w, b, 0, True)
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    assert rel_err(y6.numpy(), ref.numpy()) < 1e-6


def _wgrad(dz, x, x6):
    _lib = L()
    N, cout, H, W = dz.shape
    cin = x.shape[1]
    nbytes = _lib.lib().dn_conv2d_wgrad_slab_size(N, H, W, cin, cout, 3)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dwb = torch.full((cout * cin * 9 + cout,), float("nan"), device=DEV)
    dzg, xg = nhwc(dz).to(DEV), nhwc(x).to(DEV)
    if x6:
        _lib.call("dn_conv2d_backward_weight_x6", dzg.data_ptr(), xg.data_ptr(), cin, N, H, W,
                  cin, cout, dwb.data_ptr(), slab.data_ptr(), S())
    else:
        _lib.call("dn_conv2d_backward_weight", dzg.data_ptr(), xg.data_ptr(), cin, N, H, W, cin,
                  cout, 3, dwb.data_ptr(), slab.data_ptr(), S())
    return dwb.cpu().numpy()


# k_wgrad3p (96 / 48 outputs; operands split once per stage into LDS planes): 32-wide rows and the 16/8/4-wide
# multi-row K stages;
# Cin 96 / 144 (concat) / 48 / 97 (a partial 32-channel block); long pixel sums (64 x 128^2)
@pytest.mark.parametrize("cin,cout,N,H,W", [
    (96, 96, 2, 32, 32), (144, 96, 2, 16, 32), (48, 96, 2, 64, 64), (97, 96, 1, 32, 32),
    (96, 96, 4, 16, 16), (96, 96, 8, 8, 8), (96, 96, 16, 4, 4), (96, 96, 64, 128, 128),
    (48, 48, 2, 32, 32), (144, 48, 4, 16, 16), (48, 48, 64, 128, 128),  # 48 outputs
    (48, 48, 8, 8, 8), (100, 48, 2, 16, 16),  # (k_wgrad3p<.., 48>: 8-wide rows, a partial block)
    # sides that are not whole stage blocks (the generic DMA addressing) and an exact 8-wide one
    (96, 96, 2, 20, 36), (48, 48, 3, 24, 40), (96, 96, 2, 13, 16), (96, 96, 2, 12, 8),
])
def test_x6_backward_weight_vs_fp64(cin, cout, N, H, W):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, cin, H, W, generator=g)
    dz = torch.randn(N, cout, H, W, generator=g)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, padding=1).backward(dz.double())
    nw = cout * cin * 9
    ref_w, ref_b = w.grad.numpy().reshape(-1), b.grad.numpy()
    o6, o32 = _wgrad(dz, x, True), _wgrad(dz, x, False)
    assert np.isfinite(o6).all()
    e6, e32 = rel_err(o6[:nw], ref_w), rel_err(o32[:nw], ref_w)
    assert e6 < X6_TOL, (e6, e32)
    assert e6 < 4 * e32 + 1e-7, (e6, e32)
    assert rel_err(o6[nw:], ref_b) < X6_TOL


def test_x6_forward_single_image_past_2gib():
    """k_c3x6p reads its input tile through a 32-bit buffer resource: one 96-channel image of
    2400 x 2432 pixels is 2.24 GB, past 2^31 bytes, so the resource is based at the tile's own
    rows (a whole-image resource overflowed there).  The x6 output must equal the
    fp32 kernel's (which addresses with 64-bit offsets) everywhere, bottom rows included."""
    _lib = L()
    N, H, W, C = 1, 2400, 2432, 96
    assert H * W * C * 4 > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, H, W, C, device=DEV, generator=g)
    w = (torch.randn(C, C, 3, 3, device=DEV, generator=g) * 0.05).contiguous()
    b = torch.randn(C, device=DEV, generator=g) * 0.1
    outs = []
    for x6 in (True, False):
        y = torch.full((N, H, W, C), float("nan"), device=DEV)
        if x6:
            pk = _lib.scratch(_lib.lib().dn_conv2d_x6_pack_size(C, C, 0), DEV)
            _lib.call("dn_conv2d_forward_x6", x.data_ptr(), C, N, H, W, C, w.data_ptr(),
                      b.data_ptr(), C, 0, y.data_ptr(), C, pk.data_ptr(), pk.numel(), S())
        else:
            pk = _lib.scratch(_lib.lib().dn_conv2d_pack_size(C, C, 3, 0), DEV)
            _lib.call("dn_conv2d_forward", x.data_ptr(), C, N, H, W, C, w.data_ptr(),
                      b.data_ptr(), C, 3, 0, y.data_ptr(), C, pk.data_ptr(), pk.numel(), S())
        outs.append(y)
    y6, y32 = outs
    assert bool(torch.isfinite(y6).all())
    scale = float(y32.abs().max())
    # both are fp32-accurate (~1e-6 of max against fp64); a mis-addressed tile is O(1) off
    for r0, r1 in ((0, 32), (H // 2 - 16, H // 2 + 16), (H - 48, H)):
        d = float((y6[:, r0:r1] - y32[:, r0:r1]).abs().max())
        assert d < 1e-5 * scale, (r0, d, scale)
    assert float((y6 - y32).abs().max()) < 1e-5 * scale
    # and against fp64 on the last rows, the part past 2 GiB
    xs = x[:, H - 18:].permute(0, 3, 1, 2).double().cpu()
    ref = F.conv2d(F.pad(xs, (1, 1, 0, 1)), w.double().cpu(), b.double().cpu())[:, :, -16:]
    got = y6[:, H - 16:].permute(0, 3, 1, 2).cpu()
    assert rel_err(got.numpy(), ref.numpy()) < X6_TOL


@pytest.mark.parametrize("scale", [1e-20, 1e-30, 1e-34, 1e-36, 1e-38])
def test_x6_tiny_magnitude_operands(scale):
    """The exact split needs every piece to be a normal bf16: |v| >= 2^-110 keeps even the
    third piece (>= 2^-16 |v|) normal.  Below that the third and then the second piece become
    subnormal, and whatever the matrix core does with them, the result may keep only the pieces
    that survive (2^-16, then 2^-8 relative per operand).  Activations scaled by `scale`
    against O(0.1) weights: the result is compared with fp64 relative to its own max."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 96, 32, 32, generator=g) * scale
    w = torch.randn(96, 96, 3, 3, generator=g) * 0.1
    b = torch.zeros(96)
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    y6 = _forward(x, w, b, 0, True)
    y32 = _forward(x, w, b, 0, False)
    e6, e32 = rel_err(y6.numpy(), ref.numpy()), rel_err(y32.numpy(), ref.numpy())
    print(f"scale {scale:g}: x6 {e6:.3e}  fp32 {e32:.3e}  max|ref| {float(ref.abs().max()):.3e}")
    if scale >= 2.0 ** -100:  # every piece normal: the full fp32-class bound
        assert e6 < X6_TOL, (e6, e32)
    else:  # documented degradation: no worse than losing the subnormal pieces
        assert e6 < 2.0 ** -7 or e6 < 4 * e32 + 1e-7, (e6, e32)


@pytest.mark.parametrize("N,H,W", [(2, 8, 8), (3, 13, 37), (4, 64, 64)])
def test_x6_deconv_forward_vs_fp64_and_deterministic(N, H, W):
    """ConvTranspose2d(96, 96, 2, 2) on the bf16 matrix cores (k_deconv_x6, persistent, per-row
    buffer loads / stores): fp32 accuracy against fp64, written into a strided concat buffer
    without touching the other channels, and bit-identical across repeated launches."""
    _lib = L()
    torch.manual_seed(N * 100 + H)
    x = torch.randn(N, 96, H, W, dtype=torch.float64)
    w = torch.randn(96, 96, 2, 2, dtype=torch.float64) * 0.1
    b = torch.randn(96, dtype=torch.float64) * 0.1
    ref = F.conv_transpose2d(x, w, b, stride=2)
    stride, off = 104, 4  # output at channels [4, 100) of a 104-channel concat buffer
    xg = nhwc(x.float()).to(DEV)
    wg, bg = w.float().to(DEV), b.float().to(DEV)
    pk = _lib.scratch(_lib.lib().dn_deconv2x2_x6_pack_size(), DEV)
    outs = []
    for _ in range(3):
        yg = torch.full((N, 2 * H, 2 * W, stride), 7.0, device=DEV)
        _lib.call("dn_deconv2x2_forward_x6", xg.data_ptr(), N, H, W, wg.data_ptr(), bg.data_ptr(),
                  yg.data_ptr(), stride, off, pk.data_ptr(), pk.numel(), S())
        outs.append(yg)
    torch.cuda.synchronize()
    y = outs[0]
    assert rel_err(y[..., off:off + 96].permute(0, 3, 1, 2).cpu().numpy(), ref.numpy()) < X6_TOL
    assert bool((y[..., :off] == 7.0).all()) and bool((y[..., off + 96:] == 7.0).all())
    for o in outs[1:]:
        assert torch.equal(o, y)


@pytest.mark.parametrize("N,H,W,dy_stride,masked", [(2, 8, 8, 96, True), (3, 13, 37, 144, True),
                                                    (2, 16, 40, 100, False)])
def test_x6_deconv_backward_data_vs_fp64(N, H, W, dy_stride, masked):
    """Data gradient of ConvTranspose2d(96, 96, 2, 2) on the bf16 matrix cores
    (k_deconv_dgrad_x6): fp32 accuracy against fp64 with and without the LeakyReLU' mask, from a
    strided concat-buffer gradient, bit-identical across repeated launches."""
    _lib = L()
    torch.manual_seed(N * 10 + W)
    x = torch.randn(N, 96, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(96, 96, 2, 2, dtype=torch.float64) * 0.1
    y = F.conv_transpose2d(x, w, None, stride=2)
    dy = torch.randn_like(y)
    y.backward(dy)
    mask = torch.randn(N, 96, H, W, dtype=torch.float64)
    ref = torch.where(mask > 0, x.grad, x.grad * 0.2) if masked else x.grad
    dyg = torch.zeros(N, 2 * H, 2 * W, dy_stride, device=DEV)
    dyg[..., :96] = nhwc(dy.float()).to(DEV)
    mg = nhwc(mask.float()).to(DEV)
    wg = w.float().to(DEV)
    pk = _lib.scratch(_lib.lib().dn_deconv2x2_x6_pack_size(), DEV)
    outs = []
    for _ in range(3):
        dx = torch.full((N, H, W, 96), 7.0, device=DEV)
        _lib.call("dn_deconv2x2_backward_data_x6", dyg.data_ptr(), dy_stride, N, H, W, wg.data_ptr(),
                  mg.data_ptr() if masked else None, dx.data_ptr(), pk.data_ptr(), pk.numel(), S())
        outs.append(dx)
    torch.cuda.synchronize()
    assert rel_err(outs[0].permute(0, 3, 1, 2).cpu().numpy(), ref.detach().numpy()) < X6_TOL
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
