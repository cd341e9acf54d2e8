"""The L1FFT loss at mixed-radix sizes (csrc/fft_loss.hip): H and W of the form
m 2^k with m odd, 1 <= m <= 31, k >= 3, at most 1024.  Needs an MI355X.  Every test here fails
before the odd stage existed (DN_ERR_ARG / ValueError at these sizes).

Buffers handed to the C entry point are the guarded views of tests/test_gpu_step_ops.py.
Inputs are l1fft_ref.inputs(shape, seed=0); on the CPU that seed gives min|F| / median|F| between
4.1e-3 and 5.0e-2 over the shapes below (asserted > 1e-3), which keeps F / |F| well conditioned.

Shapes: 24 = 3 * 8 is the smallest mixed length; 24x16 and 16x24 mix an odd factor with a power
of two each way and have ragged row-pair tiles; 40x96 has C > 1, m = 5 and 3 and 32 lanes per
tile; 8x992 and 992x8 are the largest length (m = 31, P = 32, 4 lanes per tile, the deepest LDS
swizzle); 248 = 31 * 8 is m = 31 on the smallest P; 352 and 704 are the evaluation lengths (8 and
4 lanes per tile); 704x704 is the workload's plane once (353 columns in ragged tiles of 4).
ODD_SHAPES runs every m = 3 .. 31 along H and along W.

Bounds (those of tests/test_gpu_l1fft.py): loss parts 1e-4 relative against the fp64
restatement; gradient e_hip <= 4 e_ref, both max-abs distances to the fp64 restatement, e_ref
that of torch fft2 + autograd in fp32 on the CPU.
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
ERR_WS = r"status -2\)"  # DN_ERR_WORKSPACE
SHAPES = [(2, 1, 24, 24), (3, 1, 24, 16), (3, 1, 16, 24), (1, 3, 40, 96), (2, 1, 96, 56),
          (1, 1, 8, 992), (1, 1, 992, 8), (1, 1, 248, 16), (1, 1, 16, 248), (1, 1, 352, 64),
          (1, 1, 64, 704), (1, 1, 704, 704)]
ODD_SHAPES = [(1, 1, 8 * m, 8 * (34 - m)) for m in range(3, 32, 2)]
INVARIANT_SHAPES = [(2, 1, 24, 24), (1, 3, 40, 96), (1, 1, 64, 704)]


def rule(v: int) -> bool:
    """v = m 2^k with m odd, m <= 31, k >= 3, v <= 1024, by factoring"""
    if v < 8 or v > 1024:
        return False
    k = 0
    while v % 2 == 0:
        v //= 2
        k += 1
    return k >= 3 and v <= 31


def split(v: int):
    m = v
    while m % 2 == 0:
        m //= 2
    return m, v // m


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L().lib()


@pytest.fixture(scope="module")
def refs():
    """per shape, computed once and left unchanged: inputs, fp64 restatement, fp32 CPU torch"""
    cache = {}

    def get(shape, alpha=1.0, beta=1.0, fp32=True):
        key = (tuple(shape), alpha, beta)
        if key not in cache:
            pred, target = R.inputs(shape, seed=0)
            cache[key] = [pred, target, R.restatement(pred, target, alpha, beta), None]
        if fp32 and cache[key][3] is None:
            cache[key][3] = R.torch_fp32(cache[key][0], cache[key][1], alpha, beta)
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


def _against_fp64(refs, shape):
    pred, target, (l3r, dr), (_, d32) = refs(shape)
    mn, med = R.conditioning(pred, target)
    print(f"shape {shape}: min|F| / median|F| = {mn / med:.2e}")
    assert mn > 1e-3 * med, "ill-conditioned spectrum: choose another seed"
    l3, d = _call(pred, target, 1.0, 1.0)
    print("loss3", l3, "restatement", l3r.numpy())
    e_ref = float((d32.double() - dr).abs().max())
    e_hip = float(np.abs(d.astype(np.float64) - dr.numpy()).max())
    print(f"shape {shape}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / e_ref:.2f} "
          f"max|grad| {float(dr.abs().max()):.3e}")
    assert np.all(np.abs(l3 - l3r.numpy()) <= TOL * np.abs(l3r.numpy()))
    assert e_hip <= K_GRAD * e_ref


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_against_fp64(refs, shape):
    _against_fp64(refs, shape)


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=[f"m{m}" for m in range(3, 32, 2)])
def test_every_odd_factor(refs, shape):
    """m = 3 .. 31 along H (8 m) with m' = 34 - m along W"""
    assert split(shape[2])[0] + split(shape[3])[0] == 34 and split(shape[2])[1] == 8
    _against_fp64(refs, shape)


@pytest.mark.parametrize("shape", [(2, 1, 24, 40), (1, 1, 704, 24)])
@pytest.mark.parametrize("at", ["origin", "last", "interior"])
def test_delta_difference(shape, at):
    """D = d at one pixel: |F_k| = |d| everywhere, so loss_freq = |d| H W / n and the spectrum
    term of the gradient is beta sgn(d) H W / n at that pixel and 0 elsewhere (a wrong pos(k), a
    wrong twiddle sign or swapped n1 / n2 moves the peak)"""
    N, C, H, W = shape
    n = N * C * H * W
    target = torch.rand(shape, generator=torch.Generator().manual_seed(5))
    target = (target * 256).round() / 256  # target + d exact in fp32
    PH, PW = split(H)[1], split(W)[1]
    y, x = H // 2 + 1, W // 2 - 3
    assert y % PH and x % PW  # not on a multiple of P along either axis
    pos = {"origin": (0, 0, 0, 0), "last": (N - 1, C - 1, H - 1, W - 1),
           "interior": (N - 1, C - 1, y, x)}[at]
    dval, alpha, beta = -0.375, 0.5, 2.0
    pred = target.clone()
    pred[pos] += dval
    l3, d = _call(pred, target, alpha, beta)
    assert abs(l3[0] - abs(dval) / n) <= TOL * abs(dval) / n
    assert abs(l3[1] - abs(dval) * H * W / n) <= TOL * abs(dval) * H * W / n
    peak = beta * np.sign(dval) * H * W / n
    want = np.zeros(shape)
    want[pos] = alpha * np.sign(dval) / n + peak
    assert np.abs(d - want).max() <= 1e-5 * abs(peak)


def _single_bin_cases():
    out = []
    for shape in [(1, 1, 24, 40), (1, 1, 96, 352)]:
        (mh, _), (_, pw) = split(shape[2]), split(shape[3])
        v = pw + 1 if (pw + 1) % split(shape[3])[0] else pw + 2  # not a multiple of m_W
        out += [(shape, 1, 1), (shape, mh + 1, v)]
    return out


@pytest.mark.parametrize("shape,u,v", _single_bin_cases())
def test_single_bin_difference(shape, u, v):
    """D = a cos(2 pi (u y / H + v x / W)): bins (u, v) and (H-u, W-v) hold a H W / 2 each and
    every other bin 0, so loss_freq = a H W / n"""
    N, C, H, W = shape
    assert u % split(H)[0] and v % split(W)[0] and 0 < v < W // 2
    a = 0.25
    yy = torch.arange(H, dtype=torch.float64).view(H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, W)
    # the phase reduced mod 1 in integers first, so the fp64 cosine sees an exact argument
    ph = ((u * yy * W + v * xx * H) % (H * W)) / (H * W)
    D = (a * torch.cos(2 * np.pi * ph)).float().expand(shape).contiguous()
    l3, d = _call(D, torch.zeros(shape), 1.0, 1.0)
    n = N * C * H * W
    want = a * H * W * (N * C) / n
    print(f"{shape} (u, v) = ({u}, {v}): loss_freq {l3[1]:.8g} want {want:.8g}")
    assert abs(l3[1] - want) <= TOL * want
    assert np.isfinite(d).all()


@pytest.mark.parametrize("shape", [(2, 1, 24, 24), (1, 1, 16, 704)])
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


@pytest.mark.parametrize("shape", INVARIANT_SHAPES)
def test_zero_difference(refs, shape):
    pred = refs(shape, fp32=False)[0]
    l3, d = _call(pred, pred.clone(), 1.0, 1.0)
    assert same_bits(l3, np.zeros(3, np.float32))
    assert not np.isnan(d).any() and np.all(d == 0.0)


@pytest.mark.parametrize("shape", INVARIANT_SHAPES)
def test_beta_zero_is_plain_l1(refs, shape):
    pred, target = refs(shape, fp32=False)[:2]
    alpha = 0.75
    l3, d = _call(pred, target, alpha, 0.0)
    n = pred.numel()
    want = (torch.tensor(alpha, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
            * torch.sign(pred - target))
    assert same_bits(d, want.numpy())
    pix = float((pred.double() - target.double()).abs().mean())
    assert abs(l3[0] - pix) <= TOL * pix and l3[1] == 0.0
    assert abs(l3[2] - alpha * pix) <= TOL * alpha * pix


@pytest.mark.parametrize("shape", INVARIANT_SHAPES)
def test_deterministic_bits(refs, shape):
    pred, target = refs(shape, fp32=False)[:2]
    l3a, da = _call(pred, target, 1.0, 0.7)
    l3b, db = _call(pred, target, 1.0, 0.7)
    assert same_bits(l3a, l3b) and same_bits(da, db)


@pytest.mark.parametrize("shape", INVARIANT_SHAPES)
def test_sum_is_n_times_mean(refs, shape):
    pred, target = refs(shape, fp32=False)[:2]
    n = pred.numel()
    l3m, dm = _call(pred, target, 1.0, 0.7)
    l3s, ds = _call(pred, target, 1.0, 0.7, red_sum=1)
    assert np.all(np.abs(l3s - n * l3m) <= 1e-6 * np.abs(l3s))
    assert np.abs(ds - n * dm).max() <= 1e-6 * np.abs(ds).max()
    l3r, _ = R.restatement(pred, target, 1.0, 0.7, reduction="sum")
    assert np.all(np.abs(l3s - l3r.numpy()) <= TOL * np.abs(l3r.numpy()))


def test_ws_size_follows_the_rule():
    lib = L().lib()
    for v in range(1, 1101):
        a, b = lib.dn_l1fft_ws_size(1, 1, v, 8) != 0, lib.dn_l1fft_ws_size(1, 1, 8, v) != 0
        assert a == b == rule(v), v


def test_l1fft_supported_agrees_on_pairs():
    from image_denoising_amd import util

    lengths = [8, 16, 24, 40, 56, 64, 72, 88, 96, 104, 136, 152, 184, 232, 248, 352, 480, 704,
               992, 1024,                                                    # accepted
               0, 1, 4, 12, 20, 25, 28, 36, 100, 264, 280, 296, 330, 528, 1000, 1023, 1025, 1032,
               1056, 2048]                                                    # refused
    assert len(lengths) == 40 and sum(map(rule, lengths)) == 20
    lib = L().lib()
    for h in lengths:
        for w in lengths:
            ok = rule(h) and rule(w)
            assert util.l1fft_supported(h, w) == ok, (h, w)
            assert (lib.dn_l1fft_ws_size(1, 1, h, w) != 0) == ok, (h, w)


@pytest.mark.parametrize("bad", [264, 296, 20, 1032, 25])
def test_refused_lengths_are_errors(bad):
    from image_denoising_amd import util

    for H, W in ((bad, 24), (24, bad)):
        assert L().lib().dn_l1fft_ws_size(1, 1, H, W) == 0
        x = torch.zeros(1, 1, H, W)
        _call(x, x, 1.0, 1.0, expect=ERR_ARG)
        xg = x.to(DEV)
        with pytest.raises(ValueError, match="m odd"):
            util.l1fft_loss(xg, xg)
        with pytest.raises(ValueError, match="m odd"):
            util.L1FFT()(xg, xg)


def test_small_workspace_is_refused(refs):
    pred, target = refs((2, 1, 24, 40), fp32=False)[:2]
    need = int(L().lib().dn_l1fft_ws_size(2, 1, 24, 40))
    assert need >= 2 * 1 * 24 * 21 * 8
    _call(pred, target, 1.0, 1.0, ws_bytes=need - 1, expect=ERR_WS)


def test_module_matches_into(refs):
    from image_denoising_amd import util

    pred, target, (l3r, _), _ = refs((1, 3, 40, 96))
    p = pred.to(DEV).requires_grad_(True)
    t = target.to(DEV)
    loss = util.L1FFT()(p, t)
    loss.backward()
    dp, l3 = torch.empty_like(t), torch.empty(3, device=DEV)
    util.l1fft_loss_into(p.detach(), t, 1.0, 1.0, dp, l3)
    assert torch.equal(p.grad, dp) and loss.item() == l3[2].item()
    assert abs(loss.item() - l3r[2].item()) <= TOL * l3r[2].item()


def _net(kind):
    from image_denoising_amd import RESNET, UNet

    torch.manual_seed(11)
    return (UNet(1, 1, 48) if kind == "unet" else RESNET(1, 1, 48)).to(DEV)


@pytest.mark.parametrize("kind,shape", [("unet", (2, 1, 96, 96)), ("resnet", (2, 1, 24, 40))])
def test_supervised_trainer_gradient_and_step(kind, shape):
    """SupervisedTrainer.grad / loss3 equal net(x) -> L1FFT -> .backward() through the module's
    autograd, to 1e-6 of max|grad|; one step changes the parameters"""
    from image_denoising_amd import SupervisedTrainer, util

    g = torch.Generator().manual_seed(21)
    clean = torch.rand(shape, generator=g).to(DEV)
    noisy = (clean + 0.1 * torch.randn(shape, generator=g).to(DEV)).contiguous()
    net = _net(kind)
    alpha, beta = 1.0, 0.5
    tr = SupervisedTrainer(net, "l1fft", alpha=alpha, beta=beta, lr=1e-3, distributed=False)
    before = net.flat_params.detach().clone()
    net.zero_grad()
    loss = util.L1FFT(alpha, beta)(net(noisy), clean)
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
    assert not torch.equal(net.flat_params.detach(), before)
