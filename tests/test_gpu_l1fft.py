"""The L1FFT loss (csrc/fft_loss.hip: k_l1fft_rows_fwd, k_l1fft_cols, k_l1fft_rows_inv,
k_l1fft_pixel, k_l1fft_finalize), its Python surface (util.L1FFT, l1fft_loss_into) and
SupervisedTrainer.  Needs an MI355X.

Buffers handed to the C entry point are the guarded views of tests/test_gpu_step_ops.py (256
bytes of 0xA5 on each side that must survive).

Shapes: 2x1x8x8 and 1x1x8x1024 are the size bounds (8x1024: 4 row pairs in a tile of 4, one
lane group = 8 butterflies, the deepest LDS swizzle); 1x3x16x64 and 2x1x64x16 have H != W both
ways and C > 1; 3x1x32x32 has 17 spectrum columns in tiles of 32 and 48 row pairs in tiles of 32
(both ragged); 2x1x256x256 runs 129 columns in tiles of 16 (ragged, swizzled, several blocks).

Bounds: loss parts 1e-4 relative against the fp64 restatement.  Gradient:
e_hip <= K e_ref, both max-abs distances to the fp64 restatement on the same inputs, e_ref that
of the reference's own formulation in fp32 on the CPU (torch fft2 + autograd); K = 4 allows for
another butterfly order and twiddle rounding drawing another sample of the same log2(H W) eps
error class (measured e_hip / e_ref: 0.69 .. 1.05 over these shapes).
"""
import numpy as np
import pytest
import torch

import l1fft_ref as R
from test_gpu_step_ops import ERR_ARG, Buf, L, S, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
K_GRAD = 4.0
SHAPES = list(R.SEEDS)
ERR_WS = r"status -2\)"  # DN_ERR_WORKSPACE


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L().lib()


@pytest.fixture(scope="module")
def refs():
    """per shape, computed once and left unchanged: inputs, fp64 restatement, fp32 CPU torch"""
    cache = {}

    def get(shape, alpha=1.0, beta=1.0):
        key = (tuple(shape), alpha, beta)
        if key not in cache:
            pred, target = R.inputs(shape)
            cache[key] = (pred, target, R.restatement(pred, target, alpha, beta),
                          R.torch_fp32(pred, target, alpha, beta))
        return cache[key]

    return get


def _call(pred, target, alpha, beta, red_sum=0, ws_bytes=None, expect=None):
    """dn_l1fft_loss on guarded buffers -> (loss3 np, dpred np)"""
    N, C, H, W = pred.shape
    p, t = Buf(pred.shape, init=pred), Buf(pred.shape, init=target)
    d, l3 = Buf(pred.shape), Buf((3,))
    need = int(L().lib().dn_l1fft_ws_size(N, C, H, W))
    ws = Buf((max(need, 16),), torch.uint8)
    args = (p.ptr, t.ptr, N, C, H, W, float(alpha), float(beta), red_sum, d.ptr, l3.ptr, ws.ptr,
            need if ws_bytes is None else ws_bytes, S())
    if expect is not None:
        with pytest.raises(L().DenoiseHipError, match=expect):
            L().call("dn_l1fft_loss", *args)
        torch.cuda.synchronize()
        assert d.untouched() and l3.untouched() and ws.untouched()
        return None
    L().call("dn_l1fft_loss", *args)
    torch.cuda.synchronize()
    for b, what in ((p, "pred"), (t, "target"), (d, "dpred"), (l3, "loss3"), (ws, "workspace")):
        b.check(what)
    assert np.array_equal(p.np(), pred.numpy()) and np.array_equal(t.np(), target.numpy())
    return l3.np().copy(), d.np().copy()


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_against_fp64(refs, shape):
    pred, target, (l3r, dr), (_, d32) = refs(shape)
    mn, med = R.conditioning(pred, target)
    assert mn > 1e-3 * med, "ill-conditioned spectrum: choose another seed"
    l3, d = _call(pred, target, 1.0, 1.0)
    print("loss3", l3, "restatement", l3r.numpy())
    assert np.abs(l3 - l3r.numpy()).max() <= TOL * np.abs(l3r.numpy()).max()
    assert np.all(np.abs(l3 - l3r.numpy()) <= TOL * np.abs(l3r.numpy()))
    e_ref = float((d32.double() - dr).abs().max())
    e_hip = float(np.abs(d.astype(np.float64) - dr.numpy()).max())
    print(f"shape {shape}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / e_ref:.2f} "
          f"max|grad| {float(dr.abs().max()):.3e}")
    assert e_hip <= K_GRAD * e_ref


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (1, 3, 16, 64), (2, 1, 64, 16)])
@pytest.mark.parametrize("at", ["interior", "origin"])
def test_delta_difference(shape, at):
    """D = d at one pixel: |F_k| = |d| everywhere, so loss_freq = |d| H W / n and the spectrum
    term of the gradient is beta sgn(d) H W / n at that pixel and 0 elsewhere (a wrong transform
    direction, a missing conjugate or a wrong scale moves or rescales the peak)"""
    N, C, H, W = shape
    n = N * C * H * W
    target = torch.rand(shape, generator=torch.Generator().manual_seed(5))
    target = (target * 256).round() / 256  # target + d exact in fp32
    pos = (N - 1, C - 1, H // 2 + 1, W // 2 - 3) if at == "interior" else (0, 0, 0, 0)
    dval, alpha, beta = -0.375, 0.5, 2.0
    pred = target.clone()
    pred[pos] += dval
    l3, d = _call(pred, target, alpha, beta)
    assert abs(l3[0] - abs(dval) / n) <= TOL * abs(dval) / n
    assert abs(l3[1] - abs(dval) * H * W / n) <= TOL * abs(dval) * H * W / n
    peak = beta * np.sign(dval) * H * W / n
    want = np.zeros(shape)
    want[pos] = alpha * np.sign(dval) / n + peak
    # four fp32 transforms of <= 10 radix-2 stages, each stage ~1 ulp (6e-8) of the peak
    assert np.abs(d - want).max() <= 1e-5 * abs(peak)


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (1, 3, 16, 64), (3, 1, 32, 32)])
def test_nyquist_difference(shape):
    """D = a (-1)^x along W: the one nonzero bin of every plane is (0, W/2), |F| = a H W; a
    column-W/2 weight of 2 doubles the loss"""
    N, C, H, W = shape
    a = 0.25
    pred = a * torch.tensor([1.0, -1.0]).repeat(W // 2).expand(shape).contiguous()
    l3, d = _call(pred, torch.zeros(shape), 1.0, 1.0)
    n = N * C * H * W
    want = a * H * W * (N * C) / n
    assert abs(l3[1] - want) <= TOL * want
    assert abs(l3[0] - a) <= TOL * a
    assert np.isfinite(d).all()


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (2, 1, 64, 16)])
def test_zero_difference(refs, shape):
    pred, _, _, _ = refs(shape)
    l3, d = _call(pred, pred.clone(), 1.0, 1.0)
    assert same_bits(l3, np.zeros(3, np.float32))
    assert not np.isnan(d).any() and np.all(d == 0.0)


@pytest.mark.parametrize("shape", [(1, 3, 16, 64), (2, 1, 256, 256)])
def test_beta_zero_is_plain_l1(refs, shape):
    pred, target, _, _ = refs(shape)
    alpha = 0.75
    l3, d = _call(pred, target, alpha, 0.0)
    n = pred.numel()
    want = (torch.tensor(alpha, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
            * torch.sign(pred - target))
    assert same_bits(d, want.numpy())
    pix = float((pred.double() - target.double()).abs().mean())
    assert abs(l3[0] - pix) <= TOL * pix and l3[1] == 0.0
    assert abs(l3[2] - alpha * pix) <= TOL * alpha * pix


@pytest.mark.parametrize("shape", [(1, 3, 16, 64), (2, 1, 256, 256)])
def test_deterministic_bits(refs, shape):
    pred, target, _, _ = refs(shape)
    l3a, da = _call(pred, target, 1.0, 0.7)
    l3b, db = _call(pred, target, 1.0, 0.7)
    assert same_bits(l3a, l3b) and same_bits(da, db)


@pytest.mark.parametrize("shape", [(2, 1, 8, 8), (3, 1, 32, 32)])
def test_sum_is_n_times_mean(refs, shape):
    pred, target, _, _ = refs(shape)
    n = pred.numel()
    l3m, dm = _call(pred, target, 1.0, 0.7)
    l3s, ds = _call(pred, target, 1.0, 0.7, red_sum=1)
    assert np.all(np.abs(l3s - n * l3m) <= 1e-6 * np.abs(l3s))
    assert np.abs(ds - n * dm).max() <= 1e-6 * np.abs(ds).max()
    l3r, dr = R.restatement(pred, target, 1.0, 0.7, reduction="sum")
    assert np.all(np.abs(l3s - l3r.numpy()) <= TOL * np.abs(l3r.numpy()))


@pytest.mark.parametrize("H,W", [(12, 16), (16, 12), (4, 16), (16, 4), (2048, 8), (8, 2048)])
def test_bad_sizes_are_errors(H, W):
    from image_denoising_amd import util

    assert L().lib().dn_l1fft_ws_size(1, 1, H, W) == 0
    x = torch.zeros(1, 1, H, W)
    _call(x, x, 1.0, 1.0, expect=ERR_ARG)
    xg = x.to(DEV)
    with pytest.raises(ValueError):
        util.l1fft_loss(xg, xg)
    with pytest.raises(ValueError):
        util.L1FFT()(xg, xg)


def test_small_workspace_is_refused(refs):
    pred, target, _, _ = refs((2, 1, 8, 8))
    need = int(L().lib().dn_l1fft_ws_size(2, 1, 8, 8))
    assert need >= 2 * 8 * 5 * 8
    _call(pred, target, 1.0, 1.0, ws_bytes=need - 1, expect=ERR_WS)


def test_module_matches_into(refs):
    from image_denoising_amd import util

    pred, target, (l3r, _), _ = refs((1, 3, 16, 64))
    p = pred.to(DEV).requires_grad_(True)
    t = target.to(DEV)
    loss = util.L1FFT()(p, t)
    loss.backward()
    dp, l3 = torch.empty_like(t), torch.empty(3, device=DEV)
    util.l1fft_loss_into(p.detach(), t, 1.0, 1.0, dp, l3)
    assert torch.equal(p.grad, dp) and loss.item() == l3[2].item()
    assert abs(loss.item() - l3r[2].item()) <= TOL * l3r[2].item()
    with pytest.raises(NotImplementedError):
        util.L1FFT(reduction="none")
    s = util.L1FFT(0.5, 0.25, reduction="sum")(p.detach(), t)
    want = R.restatement(pred, target, 0.5, 0.25, reduction="sum")[0][2].item()
    assert abs(s.item() - want) <= TOL * want


def _net(kind):
    from image_denoising_amd import RESNET, UNet

    torch.manual_seed(11)
    return (UNet(1, 1, 48) if kind == "unet" else RESNET(1, 1, 48)).to(DEV)


@pytest.mark.parametrize("kind,shape,criterion", [("unet", (2, 1, 32, 32), "l1fft"),
                                                  ("unet", (2, 1, 32, 32), "l1"),
                                                  ("resnet", (2, 1, 16, 16), "l1fft")])
def test_supervised_trainer_gradient_and_step(kind, shape, criterion):
    """SupervisedTrainer.grad / loss3 equal net(x) -> criterion -> .backward() through the
    module's autograd, to 1e-6 of max|grad|; one step changes the parameters"""
    from image_denoising_amd import SupervisedTrainer, util

    g = torch.Generator().manual_seed(21)
    clean = torch.rand(shape, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(shape, generator=g).to(DEV)).contiguous()
    net = _net(kind)
    alpha, beta = 1.0, 0.5
    tr = SupervisedTrainer(net, criterion=criterion, alpha=alpha, beta=beta, lr=1e-3,
                           distributed=False)
    before = net.flat_params.detach().clone()
    net.zero_grad()
    out = net(noisy)
    if criterion == "l1fft":
        loss = util.L1FFT(alpha, beta)(out, clean)
    else:
        loss = torch.nn.functional.l1_loss(out, clean)
    loss.backward()
    want = torch.zeros_like(before)  # the flat layout: every parameter is a view at its offset
    for off, p in net._param_views():
        if p.grad is not None:
            want[off:off + p.numel()] = p.grad.reshape(-1)
    assert torch.equal(net.flat_params.detach(), before)
    l3 = tr.train_step(clean, noisy)
    gmax = float(want.abs().max())
    assert gmax > 0
    assert float((tr.grad - want).abs().max()) <= 1e-6 * gmax
    assert abs(l3[2].item() - loss.item()) <= 1e-6 * abs(loss.item())
    if criterion == "l1":
        assert l3[1].item() == 0.0 and l3[0].item() == l3[2].item()
    assert not torch.equal(net.flat_params.detach(), before)
