"""dn_memadapter_backward_input (csrc/memory.hip): the gradient of HyperGatedResidualAdapter(_FFT)
with respect to base_out, against fp64 torch-CPU autograd (tests/memory_joint_ref.py).  Needs an
MI355X.

Tolerance, DESIGN.md §14's convention: max error over the tensor's largest magnitude against
fp64, at most 4 x the error torch's own fp32 CPU autograd makes on the same inputs, computed here.
The hyper route is only 1e-4 .. 2e-2 of dbase's magnitude, so it is also pinned on its own
(dn_memadapter_feature_adjoint), where an error in it cannot hide."""
import numpy as np
import pytest
import torch

import memory_joint_ref as J
import memory_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _adapter(C, Hc, nb, clamp, params=None):
    from image_denoising_amd.memory import HyperGatedResidualAdapter, HyperGatedResidualAdapter_FFT

    ad = (HyperGatedResidualAdapter_FFT(C, Hc, nb, clamp) if nb > 0
          else HyperGatedResidualAdapter(C, Hc, clamp))
    if params is not None:
        ad.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return ad.to(DEV)


# ---- the feature adjoint alone ------------------------------------------------------------------
@pytest.mark.parametrize("shape", J.FEATURE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feature_adjoint_alone_vs_fp64(shape):
    B, C, H, W, nb = shape
    x, cot = J.feature_inputs(shape)
    want = J.feature_adjoint_autograd(x, cot, nb, torch.float64).numpy()
    ref32 = J.feature_adjoint_autograd(x, cot, nb, torch.float32).numpy()
    ad = _adapter(C, 16, nb, True)
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cot).to(DEV)
    got = ad._feature_adjoint(xd, cd)
    err, tol = rel(got.cpu().numpy(), want), 4 * rel(ref32, want)
    print(f"\nfeature adjoint {shape}: err {err:.2e} fp32-autograd {tol / 4:.2e}")
    assert err <= tol
    assert torch.equal(ad._feature_adjoint(xd, cd), got)  # bit-identical from run to run


# ---- the whole dbase ----------------------------------------------------------------------------
EXTRA_CASES = {  # name -> (B, C, H, W, hidden, nb, clamp)
    "one_row_1x1x1x2": (1, 1, 1, 2, 16, 2, True),   # one row, one tile, the smallest M with a std
                                                    # (F = 2: nb = 2, a DC and a Nyquist band)
    "c3_2x3x17x33": (2, 3, 17, 33, 16, 3, True),    # interior tile borders at C = 3
}
_extra = {}


def _case(name):
    """(cfg, params, noisy, base, mem, dout) of an ADAPTER_CASES or EXTRA_CASES entry"""
    if name in R.ADAPTER_CASES:
        return (R.ADAPTER_CASES[name], *R.adapter_case(name))
    if name not in _extra:
        B, C, H, W, Hc, nb, clamp = cfg = EXTRA_CASES[name]
        seed = 3000 + 19 * list(EXTRA_CASES).index(name)
        params = {}
        for k, (key, shp) in enumerate(zip(R.KEYS, R.shapes_of(C, Hc, nb))):
            fan = int(np.prod(shp[1:])) if len(shp) > 1 else 4
            params[key] = ((R.uniform(np.prod(shp), seed + k) * 2 - 1) * 0.7 / np.sqrt(fan)) \
                .reshape(shp).astype(np.float32)
        n = B * C * H * W
        noisy = R.uniform(n, seed + 20).reshape(B, C, H, W).astype(np.float32)
        base = (R.uniform(n, seed + 21) * 1.4 - 0.2).reshape(B, C, H, W).astype(np.float32)
        mem = R.uniform(n, seed + 22).reshape(B, C, H, W).astype(np.float32)
        dout = (R.uniform(n, seed + 23) * 2 - 1).reshape(B, C, H, W).astype(np.float32)
        p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
        for _ in range(20):  # memory_ref.adapter_case's rule: no pixel within 1e-4 of a clamp bound
            pre = R.forward(p64, *(torch.from_numpy(v).double() for v in (noisy, base, mem)), nb,
                            clamp, keep=True)[1]["pre"].numpy()
            near = (np.abs(pre) < 1e-4) | (np.abs(pre - 1) < 1e-4)
            if not near.any():
                break
            base = np.where(near, base + np.float32(2e-3), base).astype(np.float32)
        else:
            raise AssertionError(name)
        _extra[name] = (cfg, params, noisy, base, mem, dout)
    return _extra[name]


def _run(name, with_params=True):
    """(ad, dbase, dparams or None, tensors) of one dn_memadapter_backward_input call"""
    (B, C, H, W, Hc, nb, clamp), params, noisy, base, mem, dout = _case(name)
    ad = _adapter(C, Hc, nb, clamp, params)
    n, b, m, d = (torch.from_numpy(v).to(DEV) for v in (noisy, base, mem, dout))
    feat = ad._run_forward(n, b, m, torch.empty_like(b))
    dbase = torch.empty_like(b)
    dflat = torch.empty_like(ad.flat_params) if with_params else None
    ad._run_backward_input(n, b, feat, d, dflat, dbase)
    return ad, dbase, dflat, (n, b, m, d, feat)


@pytest.mark.parametrize("name", list(R.ADAPTER_CASES) + list(EXTRA_CASES))
def test_whole_dbase_vs_fp64(name):
    (B, C, H, W, Hc, nb, clamp), params, noisy, base, mem, dout = _case(name)
    want, hyper = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp, torch.float64)
    ref32, _ = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp, torch.float32)
    share = float(hyper.abs().max() / want.abs().max())
    assert share > 1e-5, share  # the hyper route is live in these inputs
    _, dbase, _, _ = _run(name)
    err, tol = rel(dbase.cpu().numpy(), want.numpy()), 4 * rel(ref32.numpy(), want.numpy())
    print(f"\ndbase {name}: err {err:.2e} fp32-autograd {tol / 4:.2e} hyper share {share:.1e}")
    assert err <= tol


def test_autograd_function_returns_dbase_and_parameter_gradients():
    """through _MemAdapterFunction, as DenoiserWithMemoryAdapter enters it: base_out.grad and the
    parameter gradients are the C call's, and the module itself keeps refusing such an input"""
    from image_denoising_amd.memory import _MemAdapterFunction

    ad, dbase, dflat, (n, b, m, d, _) = _run("b3c1_17x23")
    bb = b.clone().requires_grad_(True)
    _MemAdapterFunction.apply(n, bb, m, ad, *ad._params()).backward(d)
    assert torch.equal(bb.grad, dbase)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in ad._params()]), dflat)
    for p in ad._params():
        p.requires_grad_(False)
    bb = b.clone().requires_grad_(True)
    _MemAdapterFunction.apply(n, bb, m, ad, *ad._params()).backward(d)
    assert torch.equal(bb.grad, dbase)
    with pytest.raises(NotImplementedError):
        ad(n, b.clone().requires_grad_(True), m)


# ---- dparams bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b3c1_17x23", "b2c3_16x20", "hid8", "v4", "noclamp"])
def test_dparams_bits_and_repeatability(name):
    ad, dbase, dflat, (n, b, m, d, feat) = _run(name)
    old = torch.empty_like(ad.flat_params)
    ad._run_backward(n, b, feat, d, old)
    assert torch.equal(dflat, old)  # exactly dn_memadapter_backward's bits
    dbase2 = torch.empty_like(b)
    ad._run_backward_input(n, b, feat, d, None, dbase2)  # dparams null
    assert torch.equal(dbase2, dbase)
    dbase3, dflat3 = torch.empty_like(b), torch.empty_like(dflat)
    ad._run_backward_input(n, b, feat, d, dflat3, dbase3)  # a second call
    assert torch.equal(dbase3, dbase) and torch.equal(dflat3, dflat)


# ---- argument errors ----------------------------------------------------------------------------
def test_argument_errors():
    from image_denoising_amd import _lib

    L = _lib.lib()
    DN_ERR_ARG = -1
    ad, dbase, dflat, (n, b, m, d, feat) = _run("b3c1_17x23")
    N, C, H, W = n.shape
    ws = _lib.scratch(L.dn_memadapter_ws_size(N, C, H, W, 16, 3, 2), n.device)
    s = _lib.stream_of(n)

    def call(dparams=dflat, out=dbase, C_=C, hid=16, nb=3, nbytes=ws.numel()):
        return L.dn_memadapter_backward_input(
            _lib.ptr(ad.flat_params), _lib.ptr(n), _lib.ptr(b), _lib.ptr(feat), _lib.ptr(d),
            _lib.ptr(dparams), _lib.ptr(out), N, C_, H, W, hid, nb, 1, ws.data_ptr(), nbytes, s)

    assert call() == 0
    assert call(out=None) == DN_ERR_ARG
    for alias in (n, b, d):
        assert call(out=alias) == DN_ERR_ARG
    assert call(out=ad.flat_params[:dbase.numel()].view_as(dbase)) == DN_ERR_ARG  # params
    wide = torch.empty(dbase.numel() + feat.numel(), dtype=torch.float32, device=n.device)
    f2 = wide[dbase.numel() - 1:dbase.numel() - 1 + feat.numel()].view_as(feat).copy_(feat)
    assert L.dn_memadapter_backward_input(  # features: its first float is dbase's last
        _lib.ptr(ad.flat_params), _lib.ptr(n), _lib.ptr(b), _lib.ptr(f2), _lib.ptr(d), None,
        _lib.ptr(wide[:dbase.numel()].view_as(dbase)), N, C, H, W, 16, 3, 1, ws.data_ptr(),
        ws.numel(), s) == DN_ERR_ARG
    big = torch.empty(max(dflat.numel(), dbase.numel()), dtype=torch.float32, device=n.device)
    assert call(dparams=big[:dflat.numel()], out=big[:dbase.numel()].view_as(dbase)) == DN_ERR_ARG
    assert call(C_=2) == DN_ERR_ARG
    assert call(hid=12) == DN_ERR_ARG
    assert call(nb=9) == DN_ERR_ARG
    assert call(nbytes=ws.numel() - 1) == DN_ERR_ARG
    assert call(nbytes=L.dn_memadapter_ws_size(N, C, H, W, 16, 3, 1)) == DN_ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 1, 1, 2, 16, 0), (3, 1, 17, 23, 16, 3), (2, 3, 16, 20, 8, 3),
                                   (1, 1, 2, 1030, 16, 3), (16, 1, 512, 512, 16, 3)])
def test_workspace_sizes(shape):
    from image_denoising_amd import _lib

    L = _lib.lib()
    N, C, H, W, hid, nb = shape
    s0, s1, s2 = (L.dn_memadapter_ws_size(N, C, H, W, hid, nb, k) for k in (0, 1, 2))
    assert 0 < s0 <= s1 < s2
    assert L.dn_memadapter_ws_size(N, C, H, W, hid, nb, 3) == s1  # any other non-zero: as today
    assert L.dn_memadapter_ws_size(N, 2, H, W, hid, nb, 2) == 0
