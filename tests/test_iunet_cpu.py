"""ImprovedUNet (arch_unet.py:421-531) on the CPU: the oracle (oracle/iunet_ref.py) and the
host mirror's init / state_dict keys pinned to fixtures the reference produced
(tests/golden/make_golden.py --only iunet)."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import iunet_ref


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# (in_nc, fixture): the reference's two usual channel counts (out_nc = in_nc), then in_nc 2,
# out_nc 2 and 4 and in_nc != out_nc (make_golden.py iunet_pairs_main:
# iunet_c<in_nc>_<out_nc>.npz); out_nc is the fixture output's channel count
FIXTURES = [(1, "iunet_c1.npz"), (3, "iunet_c3.npz"), (2, "iunet_c2_2.npz"),
            (1, "iunet_c1_4.npz"), (3, "iunet_c3_2.npz")]


@pytest.mark.parametrize("C,name", FIXTURES)
def test_init_and_keys_match_reference(golden, C, name):
    from image_denoising_amd.improved_unet import ImprovedUNet

    g = golden(name)
    OC = g["y"].shape[1]
    assert name in ("iunet_c1.npz", "iunet_c3.npz") or name == f"iunet_c{C}_{OC}.npz"
    torch.manual_seed(0)
    net = ImprovedUNet(in_nc=C, out_nc=OC, n_feature=48)
    flat = net.flat_params.numpy()
    assert flat.size == int(g["params_count"])
    assert hashlib.sha256(flat.tobytes()).hexdigest() == str(g["params_sha"])
    assert list(net.state_dict().keys()) == [str(k) for k in g["keys"]]
    # every state_dict tensor is a view of the flat buffer, in order
    off = 0
    for k, v in net.state_dict().items():
        assert v.data_ptr() == net.flat_params.data_ptr() + 4 * off, k
        off += v.numel()
    assert [k for k, _ in iunet_ref.layer_table(C, OC)] == list(net.state_dict().keys())


@pytest.mark.parametrize("C,name", FIXTURES)
def test_oracle_forward_backward_matches_reference(golden, C, name):
    """The oracle runs in float64 on the fixture's fp32 weights and inputs, so the result does
    not depend on the host's thread count: the fp32 run's C=3 gradient moves with it (447 of the
    16384 sampled entries by up to 1.856e-3 of the largest one at 2, 4 and 16 threads, 1e-6 at
    one thread; at 8 it depends on the CPU), while the float64 run sits 1.5e-6 from the reference's fp32 fixture
    (forward 7e-7) at any thread count."""
    from image_denoising_amd.improved_unet import ImprovedUNet

    g = golden(name)
    OC = g["y"].shape[1]
    torch.manual_seed(0)
    flat = ImprovedUNet(in_nc=C, out_nc=OC, n_feature=48).flat_params.clone().double().requires_grad_(True)
    if "pool_gap" in g:  # the channel-count fixtures' inputs: every 2x2 pool has a clear winner
        assert iunet_ref.pool_gap(flat.detach(), torch.from_numpy(g["x"]), C, OC) >= 1e-5
    y = iunet_ref.forward(flat, torch.from_numpy(g["x"]).double(), C, OC)
    assert y.shape == g["t"].shape
    assert rel_err(y.detach().numpy(), g["y"]) < 1e-5
    loss = ((y - torch.from_numpy(g["t"]).double()) ** 2).mean()
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    grad = flat.grad.numpy()
    assert rel_err(grad[g["grad_idx"]], g["grad_sample"]) < 1e-4
    norms, off = [], 0
    for _, shape in iunet_ref.layer_table(C, OC):
        n = int(np.prod(shape))
        norms.append(np.linalg.norm(grad[off:off + n]))
        off += n
    assert rel_err(norms, g["grad_norms"]) < 1e-4


@pytest.mark.parametrize("in_nc,out_nc,names", [(4, 1, "in_nc"), (0, 1, "in_nc"), (1, 5, "out_nc"),
                                                (3, 0, "out_nc")])
def test_channel_counts_outside_the_built_range_are_rejected(in_nc, out_nc, names):
    """ImprovedUNet takes in_nc 1..3 and out_nc 1..4: anything else is a ValueError from the
    constructor (the library's own check, before a module is built) and DN_ERR_ARG from every
    entry point that plans, with a message that names the argument; nothing is launched"""
    import ctypes

    from image_denoising_amd import _lib
    from image_denoising_amd.improved_unet import ImprovedUNet

    with pytest.raises(ValueError, match=names):
        ImprovedUNet(in_nc=in_nc, out_nc=out_nc)
    n = ctypes.c_size_t()
    cfg = _lib.cfg(in_nc, out_nc, 48)
    L = _lib.lib()
    assert L.dn_iunet_param_count(ctypes.byref(cfg), ctypes.byref(n)) == -1  # DN_ERR_ARG
    assert names in _lib.last_error()
    assert L.dn_iunet_workspace_size(ctypes.byref(cfg), 1, 32, 32, 1, ctypes.byref(n)) == -1
    assert names in _lib.last_error()
    host = (ctypes.c_float * 4)()  # never read: the plan is refused first
    buf = ctypes.addressof(host)
    assert L.dn_iunet_forward_prec(ctypes.byref(cfg), buf, buf, buf, 1, 32, 32, buf, 16, 0, None) == -1
    assert names in _lib.last_error()


def test_workspace_plan_rejects_bad_shapes():
    import ctypes

    from image_denoising_amd import _lib

    cfg = _lib.cfg(1, 1, 48)
    nb = ctypes.c_size_t()
    assert _lib.lib().dn_iunet_workspace_size(ctypes.byref(cfg), 2, 40, 64, 1, ctypes.byref(nb)) != 0
    assert "multiples of 16" in _lib.last_error()
    assert _lib.lib().dn_iunet_workspace_size(ctypes.byref(cfg), 2, 64, 64, 1, ctypes.byref(nb)) == 0
    fwd = ctypes.c_size_t()
    assert _lib.lib().dn_iunet_workspace_size(ctypes.byref(cfg), 2, 64, 64, 0, ctypes.byref(fwd)) == 0
    assert 0 < fwd.value < nb.value
    bad = _lib.cfg(1, 1, 32)
    assert _lib.lib().dn_iunet_param_count(ctypes.byref(bad), ctypes.byref(nb)) != 0
