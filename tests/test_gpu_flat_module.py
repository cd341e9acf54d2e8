"""image_denoising_amd/flat_module.py on the GPU: for each of the five flat-parameter classes, at
N = 1 and the smallest shape that runs its kernels, what autograd delivers through the shared
machinery (the one network Function / the adapters' Functions on the shared gradient slicer) is
BITWISE what a direct _run_forward + _run_backward on a fresh workspace writes.  Every one of
these backwards is deterministic (their own suites assert bit-identical repeats), so no tolerance.
Needs an MI355X."""
import pytest
import torch

from image_denoising_amd.flat_module import HipNet

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _make(name):
    from image_denoising_amd import RESNET, ImprovedUNet, OutputAdapter, UNet
    from image_denoising_amd.memory import HyperGatedResidualAdapter_FFT

    make, shape, n_in = {
        "UNet": (lambda: UNet(1, 1, 48), (1, 1, 32, 32), 1),
        "ImprovedUNet": (lambda: ImprovedUNet(1, 1, 48), (1, 1, 16, 16), 1),
        # in_nc != out_nc: the output and its gradient have out_nc channels, dL/dx has in_nc
        "UNet(2,5)": (lambda: UNet(2, 5, 48), (1, 2, 32, 32), 1),
        "ImprovedUNet(2,4)": (lambda: ImprovedUNet(2, 4, 48), (1, 2, 16, 16), 1),
        "RESNET": (lambda: RESNET(1, 1, 48), (1, 1, 9, 17), 1),  # ragged: test_gpu_resnet's size
        "OutputAdapter": (lambda: OutputAdapter(1, 16), (1, 1, 8, 8), 2),
        "HyperGatedResidualAdapter_FFT": (lambda: HyperGatedResidualAdapter_FFT(1, 16),
                                          (1, 1, 8, 8), 3),
    }[name]
    torch.manual_seed(0)
    m = make()
    g = torch.Generator().manual_seed(7)
    if not isinstance(m, HipNet):  # adapters (the memory one zeroes layers): every gradient live
        with torch.no_grad():
            m.flat_params.copy_(0.2 * torch.randn(m.flat_params.shape, generator=g))
    inputs = [torch.rand(shape, generator=g).to(DEV) for _ in range(n_in)]
    out_shape = (shape[0], m.out_nc) + shape[2:] if isinstance(m, HipNet) else shape
    dy = torch.randn(out_shape, generator=g).to(DEV)
    return m.to(DEV), inputs, dy


def _direct(m, inputs, dy, want_dx=False):
    """(dflat, dx or None) of the module's own _run_forward + _run_backward"""
    dflat = torch.full_like(m.flat_params, float("nan"))
    out = torch.empty_like(dy)
    if isinstance(m, HipNet):
        (x,) = inputs
        N, _, H, W = x.shape
        ws = m._workspace(N, H, W, with_backward=True, fresh=True)
        m._run_forward(x, out, ws)
        dx = torch.full_like(x, float("nan")) if want_dx else None
        m._run_backward(dy, dflat, ws, N, H, W, dx=dx)
        return dflat, dx
    if len(inputs) == 2:
        m._run_forward(*inputs, out)
        m._run_backward(*inputs, dy, dflat)
    else:
        feat = m._run_forward(*inputs, out)
        m._run_backward(inputs[0], inputs[1], feat, dy, dflat)
    return dflat, None


def _autograd(m, inputs, dy):
    """the flat gradient loss.backward() leaves in the parameters' .grad (None where none)"""
    m.zero_grad(set_to_none=True)
    loss = (m(*inputs) * dy).sum()  # dloss/dy is dy, bit for bit
    loss.backward()
    return [p.grad for p in m._params()]


NAMES = ["UNet", "RESNET", "OutputAdapter", "HyperGatedResidualAdapter_FFT", "ImprovedUNet",
         "UNet(2,5)", "ImprovedUNet(2,4)"]


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    m, inputs, dy = _make(request.param)
    dflat, _ = _direct(m, inputs, dy)
    assert torch.isfinite(dflat).all() and float(dflat.abs().max()) > 0
    return request.param, m, inputs, dy, dflat


def test_views_share_the_flat_buffer_on_the_gpu(case):
    _, m, *_ = case
    assert m.flat_params.device.type == "cuda"
    base, n = m.flat_params.data_ptr(), 0
    for off, p in m._param_views():
        assert p.device == m.flat_params.device and p.data_ptr() == base + 4 * off and off == n
        n += p.numel()
    assert n == m.flat_params.numel()


def test_autograd_gradients_equal_the_direct_backward_bitwise(case):
    _, m, inputs, dy, dflat = case
    grads = _autograd(m, inputs, dy)
    assert all(g is not None for g in grads)
    assert torch.equal(torch.cat([g.reshape(-1) for g in grads]), dflat)


def test_frozen_parameter_gets_no_grad_and_the_others_are_unchanged(case):
    _, m, inputs, dy, dflat = case
    views = m._param_views()
    k = len(views) // 2
    views[k][1].requires_grad_(False)
    try:
        grads = _autograd(m, inputs, dy)
    finally:
        views[k][1].requires_grad_(True)
    assert grads[k] is None
    for i, ((off, p), g) in enumerate(zip(views, grads)):
        if i != k:
            assert torch.equal(g.reshape(-1), dflat[off:off + p.numel()]), i


def test_input_gradient(case):
    """UNet / RESNET: dL/dx and the parameter gradients of the same backward equal the direct
    call's with a dx buffer; ImprovedUNet and the adapters compute no input gradient and say so"""
    name, m, inputs, dy, _ = case
    x = inputs[0].clone().requires_grad_(True)
    if name not in ("UNet", "RESNET", "UNet(2,5)"):
        with pytest.raises(NotImplementedError):
            m(x, *inputs[1:])
        return
    dflat, dx = _direct(m, inputs, dy, want_dx=True)
    grads = _autograd(m, [x], dy)
    assert torch.equal(x.grad, dx) and torch.isfinite(dx).all() and float(dx.abs().max()) > 0
    assert torch.equal(torch.cat([g.reshape(-1) for g in grads]), dflat)


@pytest.mark.parametrize("name,shape,multiple", [("UNet", (48, 32), 32),
                                                 ("ImprovedUNet", (24, 16), 16)])
def test_wrong_multiple_raises_value_error_through_forward(name, shape, multiple):
    m, _, _ = _make(name)
    with pytest.raises(ValueError, match=f"multiples of {multiple}"):
        m(torch.zeros(1, 1, *shape, device=DEV))
