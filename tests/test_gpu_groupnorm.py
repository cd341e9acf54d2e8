"""GroupNorm of ImprovedUNet's ResBlocks as an op (dn_groupnorm_forward / dn_groupnorm_backward:
the launch sequences of iunet.cpp's gn_fwd / gn_bwd -- k_chan_sums, k_gn_fwd_fin / k_gn_bwd_fin +
k_gn_dparams, k_affine in csrc/iunet_ops.hip) against torch.nn.functional.group_norm in fp64 and
its autograd, at the edges the whole-network tests never reach: more than 64 images (k_gn_dparams'
lane l sums images l, l + 64, ...), pixel splits that do not divide the image (23 x 23: S = 2;
16 x 48: S = 3), fewer pixels than k_chan_sums has pixel lanes (1 x 2), a large mean with a small
spread, and a constant group (variance 0: the clamp, rstd = eps^-1/2).  Operands sit on guarded
views (x6_edge_util): input gap channels and guard bands hold NaN, outputs are NaN-prefilled, and
after the call guards and gaps must be untouched bit for bit and the results finite.

Tolerance: the suite's relation between a kernel and an fp32 reference implementation -- the
device's error as a fraction of max |fp64 reference| stays below 4 x (torch's fp32 CPU GroupNorm
error on the same inputs) + 1e-7, for y, dz, dgamma and dbeta.  The saved statistics are compared
with fp64 directly: the mean is an fp64 mean rounded to fp32 (2^-24 relative, plus the fp64
summation error), rstd an fp64 (var + eps)^-1/2 rounded to fp32 whose variance E[z^2] - mean^2
loses at most mean^2 / var x 2^-52 ~ 2e-8 relative in the large-mean cases: 3e-7 bounds both.
Needs an MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from x6_edge_util import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
EPS = 1e-5
CONST = 1.7  # the constant group's value


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


def frac_err(a, b):
    """max |a - b| / max |b|"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _inputs(C, G, N, H, W, stat):
    g = torch.Generator().manual_seed(C + 3 * N + 5 * H + 7 * W + len(stat))
    z = torch.randn(N, C, H, W, generator=g)
    if stat == "bigmean":
        z = 100.0 + 1e-2 * z
    elif stat == "const":
        cpg = C // G
        z[:, cpg:2 * cpg] = CONST  # group 1 of every image
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    res = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, C, H, W, generator=g)
    return z, gamma, beta, res, dy


def _torch_gn(z, gamma, beta, res, dy, G, act, use_res, dtype):
    """-> y, dz, dgamma, dbeta of torch's GroupNorm in dtype (dy = the gradient of the
    normalisation's own output, before the activation and the residual), as fp64 numpy"""
    z = z.to(dtype).clone().requires_grad_(True)
    gamma = gamma.to(dtype).clone().requires_grad_(True)
    beta = beta.to(dtype).clone().requires_grad_(True)
    gn = F.group_norm(z, G, gamma, beta, EPS)
    y = F.leaky_relu(gn, 0.2) if act else gn
    if use_res:
        y = y + res.to(dtype)
    gn.backward(dy.to(dtype))
    return [t.detach().double().numpy() for t in (y, z.grad, gamma.grad, beta.grad)]


def _view(shape, strided, fill_from=None):
    """-> (Guarded, base pointer, stride, off): dense, or channels [4, 4 + C) of (C + 8)-channel
    pixels with the base pointer 4 floats into the buffer"""
    C = shape[3]
    stride, off, lead = (C + 8, 4, 8) if strided else (C, 0, 0)
    gd = guarded(shape, stride, lead, NAN, DEV)
    if fill_from is not None:
        gd.data.copy_(fill_from)
    return gd, gd.ptr - 4 * off, stride, off


def _flat(n):
    return guarded((1, 1, 1, n), n, 4, NAN, DEV)


# (C, G, N, H, W, view, input statistics, act, residual)
CASES = [
    # 1 x 2: fewer pixels than pixel lanes
    (24, 24, 1, 1, 2, "dense", "normal", 0, 0),
    (48, 24, 3, 1, 2, "strided", "normal", 1, 0),
    (96, 32, 1, 1, 2, "dense", "normal", 0, 1),
    (192, 32, 3, 1, 2, "strided", "normal", 1, 0),
    (384, 32, 1, 1, 2, "dense", "normal", 0, 1),
    (24, 24, 3, 1, 2, "dense", "const", 0, 0),
    # 23 x 23: P = 529, two pixel splits of 264 and 265
    (24, 24, 1, 23, 23, "strided", "normal", 1, 0),
    (48, 24, 3, 23, 23, "dense", "normal", 0, 1),
    (96, 32, 1, 23, 23, "strided", "bigmean", 0, 0),
    (192, 32, 3, 23, 23, "dense", "normal", 1, 0),
    (384, 32, 1, 23, 23, "strided", "normal", 0, 1),
    (48, 24, 1, 23, 23, "dense", "const", 1, 0),
    (384, 32, 1, 23, 23, "dense", "bigmean", 0, 0),
    # 16 x 48: three pixel splits
    (24, 24, 3, 16, 48, "dense", "normal", 0, 1),
    (48, 24, 1, 16, 48, "strided", "bigmean", 1, 0),
    (96, 32, 3, 16, 48, "dense", "const", 0, 0),
    (192, 32, 1, 16, 48, "strided", "normal", 0, 1),
    (384, 32, 3, 16, 48, "dense", "normal", 1, 0),
    # more than 64 images (4 x 4): k_gn_dparams' second and third round
    (24, 24, 65, 4, 4, "dense", "normal", 1, 0),
    (48, 24, 65, 4, 4, "strided", "normal", 0, 1),
    (96, 32, 65, 4, 4, "dense", "bigmean", 0, 0),
    (192, 32, 65, 4, 4, "strided", "const", 1, 0),
    (384, 32, 65, 4, 4, "dense", "normal", 0, 1),
    (24, 24, 130, 4, 4, "strided", "normal", 0, 1),
    (48, 24, 130, 4, 4, "dense", "const", 1, 0),
    (96, 32, 130, 4, 4, "strided", "normal", 1, 0),
    (192, 32, 130, 4, 4, "dense", "normal", 0, 0),
    (384, 32, 130, 4, 4, "strided", "bigmean", 0, 1),
    (96, 32, 130, 4, 4, "dense", "bigmean", 1, 0),
]


@pytest.mark.parametrize("C,G,N,H,W,view,stat,act,use_res", CASES)
def test_groupnorm_forward_backward_vs_fp64(C, G, N, H, W, view, stat, act, use_res):
    _lib = L()
    z, gamma, beta, res, dy = _inputs(C, G, N, H, W, stat)
    ref = _torch_gn(z, gamma, beta, res, dy, G, act, use_res, torch.float64)
    t32 = _torch_gn(z, gamma, beta, res, dy, G, act, use_res, torch.float32)
    zg = z.double().reshape(N, G, -1)
    mean64 = zg.mean(-1).numpy()
    rstd64 = (zg.var(-1, unbiased=False) + EPS).rsqrt().numpy()
    if stat == "const":  # the fp64 reference itself: variance 0, rstd = eps^-1/2
        assert np.array_equal(mean64[:, 1], np.full(N, np.float64(np.float32(CONST))))
        assert np.allclose(rstd64[:, 1], EPS ** -0.5, rtol=1e-12)

    strided = view == "strided"
    shape = (N, H, W, C)
    gz, pz, zs, zo = _view(shape, strided, nhwc(z))
    gr, pr, rs, ro = _view(shape, strided, nhwc(res))
    gy, py, ys, yo = _view(shape, strided)
    gdy, pdy, dys, dyo = _view(shape, strided, nhwc(dy))
    gdz, pdz, dzs, dzo = _view(shape, strided)
    gst, gdg, gdb = _flat(2 * N * G), _flat(C), _flat(C)
    nfl = _lib.lib().dn_groupnorm_scratch_size(N, H, W, C) // 4
    assert nfl > 0
    gsc = guarded((1, 1, 1, nfl), nfl, 0, NAN, DEV)
    gam, bet = gamma.to(DEV), beta.to(DEV)
    _lib.call("dn_groupnorm_forward", pz, zs, zo, pr if use_res else None, rs, ro, py, ys, yo,
              N, H, W, C, G, gam.data_ptr(), bet.data_ptr(), act, gst.ptr, gsc.ptr, 4 * nfl, S())
    torch.cuda.synchronize()
    y = gy.data.cpu()
    stats = gst.data.reshape(N, G, 2).cpu().double().numpy()
    _lib.call("dn_groupnorm_backward", pdy, dys, dyo, pz, zs, zo, pdz, dzs, dzo, N, H, W, C, G,
              gam.data_ptr(), gst.ptr, gdg.ptr, gdb.ptr, gsc.ptr, 4 * nfl, S())
    torch.cuda.synchronize()
    for gd, what in ((gz, "z"), (gr, "res"), (gy, "y"), (gdy, "dy"), (gdz, "dz"), (gst, "stats"),
                     (gdg, "dgamma"), (gdb, "dbeta"), (gsc, "scratch")):
        gd.check(what=what)
    got = [y.permute(0, 3, 1, 2).double().numpy(),
           gdz.data.cpu().permute(0, 3, 1, 2).double().numpy(),
           gdg.data.reshape(-1).cpu().double().numpy(), gdb.data.reshape(-1).cpu().double().numpy()]
    names = ("y", "dz", "dgamma", "dbeta")
    for name, a in zip(names, got):
        assert np.isfinite(a).all(), f"{name}: non-finite or unwritten values"

    # the saved statistics against fp64 directly
    zmax = float(z.abs().max())
    em = np.abs(stats[..., 0] - mean64)
    assert (em <= 1.2e-7 * np.abs(mean64) + 1e-9 * zmax).all(), float(em.max())
    er = float(np.abs(stats[..., 1] / rstd64 - 1.0).max())
    assert er < 3e-7, er

    e_dev = [frac_err(a, r) for a, r in zip(got, ref)]
    e_t32 = [frac_err(a, r) for a, r in zip(t32, ref)]
    print(f"\ngroupnorm C{C} G{G} {N}x{H}x{W} {view} {stat} act{act} res{use_res}: "
          + "; ".join(f"{n} dev {d:.2e} torch32 {t:.2e}" for n, d, t in zip(names, e_dev, e_t32))
          + f"; rstd {er:.1e}")
    for name, d, t in zip(names, e_dev, e_t32):
        assert d < 4 * t + 1e-7, (name, d, t)
