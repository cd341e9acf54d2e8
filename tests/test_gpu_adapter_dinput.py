"""dn_adapter_backward_input (csrc/adapter.hip k_adapter_dinput): the adapter's gradient with
respect to base_out and noisy, through the C-ABI, against fp64 torch-CPU autograd
(tests/joint_ref.py).  Needs an MI355X.

Shapes: the smallest at which the tile kernel can go wrong (one pixel; one ragged tile in which
every pixel touches a border; exactly one tile; one row / column spilling into a second tile at
C = 3; interior tile borders, where a neighbour tile's dpre feeds this one).

Bound (DESIGN.md §14's convention): max error relative to the tensor's largest magnitude, at most
4x the error torch's own fp32 CPU autograd makes against fp64 on the same inputs; the fp32 error
is computed here.  Measured on an MI355X (kernel / fp32 CPU): see DESIGN.md §17."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import joint_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-4  # test_gpu_adapter.py's, for the parameter gradient against the fixture
SHAPES = [(1, 1, 1, 1), (1, 1, 5, 7), (1, 1, 16, 16), (2, 3, 17, 33), (2, 1, 32, 48)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _adapter(C, flat):
    from image_denoising_amd.adapter import OutputAdapter

    ad = OutputAdapter(in_channels=C, hidden_channels=16)
    ad.flat_params.copy_(torch.as_tensor(flat))
    return ad.to(DEV)


_cases = {}


def _case(shape):
    """inputs, the fp64 reference and the fp32 CPU error of a shape, computed once"""
    if shape not in _cases:
        from image_denoising_amd.adapter import adapter_reference_init

        N, C, H, W = shape
        gen = torch.Generator().manual_seed(sum(shape))
        torch.manual_seed(3)
        # 3x the reference initialisation on zero-mean inputs: about half the hidden units are off
        flat = adapter_reference_init(C) * 3.0
        noisy, base, dout = (torch.randn(N, C, H, W, generator=gen) for _ in range(3))
        dn64, db64, off = joint_ref.adapter_input_grads(flat, noisy, base, dout)
        dn32, db32, _ = joint_ref.adapter_input_grads(flat, noisy, base, dout, dtype=torch.float32)
        _cases[shape] = dict(flat=flat, noisy=noisy, base=base, dout=dout, dn64=dn64, db64=db64,
                             off=off, e32=(rel_err(dn32, dn64), rel_err(db32, db64)))
    return _cases[shape]


def _run(ad, c, with_noisy):
    n, b, d = (c[k].to(DEV) for k in ("noisy", "base", "dout"))
    dbase = torch.full_like(b, float("nan"))
    dnoisy = torch.full_like(n, float("nan")) if with_noisy else None
    ad._run_backward_input(n, b, d, dbase, dnoisy)
    return dbase, dnoisy


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_input_gradients_vs_fp64(shape):
    c = _case(shape)
    assert 0.2 <= c["off"] <= 0.8, c["off"]  # relu' is exercised both ways
    ad = _adapter(shape[1], c["flat"])
    dbase, dnoisy = _run(ad, c, True)
    e_n, e_b = rel_err(dnoisy.cpu(), c["dn64"]), rel_err(dbase.cpu(), c["db64"])
    print(f"\n{shape}: off {c['off']:.3f}  dnoisy {e_n:.3e} (fp32 CPU {c['e32'][0]:.3e})  "
          f"dbase {e_b:.3e} (fp32 CPU {c['e32'][1]:.3e})")
    assert e_n <= 4 * c["e32"][0], (e_n, c["e32"][0])
    assert e_b <= 4 * c["e32"][1], (e_b, c["e32"][1])
    # dnoisy null: the same dbase bits; a second call: identical bits
    dbase_only, none = _run(ad, c, False)
    assert none is None and torch.equal(dbase_only, dbase)
    dbase2, dnoisy2 = _run(ad, c, True)
    assert torch.equal(dbase2, dbase) and torch.equal(dnoisy2, dnoisy)


def test_autograd_function_returns_what_is_asked_for():
    """_AdapterFunction.backward: dnoisy / dbase by needs_input_grad, bits of the direct call"""
    from image_denoising_amd.adapter import _AdapterFunction

    c = _case((2, 1, 32, 48))
    ad = _adapter(1, c["flat"])
    dbase, dnoisy = _run(ad, c, True)
    for need_n, need_b in ((True, True), (False, True), (True, False)):
        n = c["noisy"].to(DEV).requires_grad_(need_n)
        b = c["base"].to(DEV).requires_grad_(need_b)
        ad.zero_grad(set_to_none=True)
        _AdapterFunction.apply(n, b, ad, *ad._params()).backward(c["dout"].to(DEV))
        assert (n.grad is None) == (not need_n) and (b.grad is None) == (not need_b)
        assert n.grad is None or torch.equal(n.grad, dnoisy)
        assert b.grad is None or torch.equal(b.grad, dbase)
        assert all(p.grad is not None for p in ad._params())


# sha256 of dn_adapter_backward's 449 / 1315 floats on the adapter.npz inputs (dout = the finetune
# loss's gradient there), recorded on an MI355X from the commit before k_adapter_dinput existed
PARAM_GRAD_SHA = {1: "165a0f4e0e70ffd26195a6741f9cedb86c818f9a3076d6bb617fdb4c3b913ce9",
                  3: "0545d4b51547c9fae09d7eadea7a339a2dda3868da73f30ddcc21b9293304c38"}


@pytest.mark.parametrize("C", [1, 3])
def test_parameter_gradient_is_untouched(golden, C):
    """dn_adapter_backward on test_gpu_adapter.py's fixture inputs: the bits of the build before
    this kernel, before and after a dn_adapter_backward_input launch on the same buffers"""
    from image_denoising_amd.finetune import finetune_loss

    g = golden("adapter.npz")
    k = f"c{C}_"
    ad = _adapter(C, g[k + "params"])
    noisy, base, clean = (torch.from_numpy(g[k + n]).to(DEV) for n in ("noisy", "base", "clean"))
    out = torch.empty_like(base)
    ad._run_forward(noisy, base, out)
    _, dpred = finetune_loss(out, clean, 0.1)
    grad = torch.empty_like(ad.flat_params)
    ad._run_backward(noisy, base, dpred, grad)
    dbase, dnoisy = torch.empty_like(base), torch.empty_like(base)
    ad._run_backward_input(noisy, base, dpred, dbase, dnoisy)
    grad2 = torch.empty_like(grad)
    ad._run_backward(noisy, base, dpred, grad2)
    assert torch.equal(grad, grad2)
    got = grad.cpu().numpy()
    assert np.abs(got - g[k + "grad"]).max() < FP32_TOL * np.abs(g[k + "grad"]).max()
    assert hashlib.sha256(got.tobytes()).hexdigest() == PARAM_GRAD_SHA[C]


def test_bad_arguments_are_dn_err_arg():
    from image_denoising_amd import _lib

    L = _lib.lib()
    ad = _adapter(1, torch.zeros(449))
    t = [torch.zeros(1, 1, 8, 8, device=DEV) for _ in range(5)]
    noisy, base, dout, dbase, dnoisy = (_lib.ptr(v) for v in t)
    prm, s = _lib.ptr(ad.flat_params), _lib.stream_of(t[0])

    def call(*a, C=1, hid=16, N=1):
        return L.dn_adapter_backward_input(*a, N, C, 8, 8, hid, s)

    assert call(prm, noisy, base, dout, dbase, dnoisy) == 0
    assert call(prm, noisy, base, dout, dbase, None) == 0
    torch.cuda.synchronize()
    assert call(prm, noisy, base, dout, None, dnoisy) == -1  # DN_ERR_ARG
    assert "null" in _lib.last_error()
    assert call(prm, noisy, base, dout, dout, dnoisy) == -1
    assert "alias" in _lib.last_error()
    assert call(prm, noisy, base, dout, dbase, dout) == -1
    assert call(prm, noisy, base, dout, dbase, dbase) == -1
    assert call(None, noisy, base, dout, dbase, dnoisy) == -1
    assert call(prm, noisy, base, None, dbase, dnoisy) == -1
    assert call(prm, noisy, base, dout, dbase, dnoisy, C=2) == -1
    assert "in_channels" in _lib.last_error()
    assert call(prm, noisy, base, dout, dbase, dnoisy, hid=8) == -1
    assert call(prm, noisy, base, dout, dbase, dnoisy, N=0) == -1
    n = ctypes.c_size_t()
    assert L.dn_adapter_param_count(2, 16, ctypes.byref(n)) == -1  # the same C as the other calls
