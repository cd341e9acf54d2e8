"""RESNET without a GPU: the CPU restatement (tests/resnet_ref.py) against the reference
fixtures, the module's state_dict layout and reference_init replay, the C-ABI's host logic."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resnet_ref

from resnet_ref import FIX, GOLD, fixture_params, rel, sha, tensor_ranges


@pytest.mark.parametrize("C", [1, 3, 2, 4])
def test_restatement_matches_reference_fixture(C):
    g = np.load(os.path.join(GOLD, FIX[C]))
    p = fixture_params(g, C).requires_grad_(True)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = resnet_ref.forward(p, x, C, C)
    loss = (y ** 2).mean()
    loss.backward()
    assert float(g["residual_max"]) >= 0.1 * float(np.abs(g["x"]).max())
    assert rel(y.detach().numpy(), g["y"]) < 1e-5
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * float(g["loss"])
    assert rel(x.grad.numpy(), g["dx"]) < 1e-5
    gs = p.grad.numpy()[g["grad_idx"]]
    assert rel(gs, g["grad_sample"]) < 1e-5
    # the unused up5.deconv has no gradient
    b, e = resnet_ref.ranges(C, C)["up5.deconv"]
    assert not p.grad[b:e].any()
    norms = [float(p.grad[o:o + n].double().norm()) for _, o, n in tensor_ranges(C)]
    np.testing.assert_allclose(norms, g["grad_norms"], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("C,count", [(1, 1108849), (3, 1111635), (2, 1110242), (4, 1113028)])
def test_module_keys_shapes_and_init_replay(C, count):
    from image_denoising_amd import RESNET, _lib

    g = np.load(os.path.join(GOLD, FIX[C]))
    torch.manual_seed(0)
    net = RESNET(C, C, 48)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in g["key_shapes"]]
    assert not any(k.startswith(("up4", "up3", "up2", "up1")) for k in sd)
    assert net.flat_params.numel() == count
    assert sha(net.flat_params.numpy()) == str(g["params_sha"])
    np.testing.assert_array_equal(net.flat_params.numpy()[:64], g["params_head"])
    torch.manual_seed(0)
    assert sha(RESNET(C, C, 48, zero_last=True).flat_params.numpy()) == str(g["params_sha_zero_last"])
    assert str(g["params_sha_zero_last"]) != str(g["params_sha"])
    # the C-ABI's layout is the state_dict's
    cfg = _lib.cfg(C, C, 48)
    off = 0
    for i, (name, ws, bl, _) in enumerate(resnet_ref.layer_table(C, C)):
        wo, wc, bc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _lib.call("dn_resnet_param_info", ctypes.byref(cfg), i, ctypes.byref(wo), ctypes.byref(wc),
                  ctypes.byref(bc))
        assert (wo.value, wc.value, bc.value) == (off, int(np.prod(ws)), bl), name
        off += int(np.prod(ws)) + bl
    assert off == count


def test_state_dict_roundtrip_with_module_prefix(tmp_path):
    from image_denoising_amd import RESNET
    from image_denoising_amd.checkpoint import load_checkpoint, save_checkpoint

    torch.manual_seed(1)
    a = RESNET(1, 1, 48)
    ck = save_checkpoint(a, str(tmp_path / "r.pth"), data_parallel=True)
    assert all(k.startswith("module.") for k in torch.load(ck, weights_only=True))
    b = RESNET(1, 1, 48)
    assert not torch.equal(a.flat_params, b.flat_params)
    load_checkpoint(b, ck)
    assert torch.equal(a.flat_params, b.flat_params)
    assert b.enc_conv0.weight.data_ptr() == b.flat_params.data_ptr()  # still views of one buffer


def test_host_side_rejections_and_any_size_workspace():
    from image_denoising_amd import RESNET, _lib

    with pytest.raises(NotImplementedError):
        RESNET(1, 1, 48, blindspot=True)
    with pytest.raises(ValueError):
        RESNET(1, 3, 48)
    with pytest.raises(ValueError):
        RESNET(1, 1, 32)
    n = ctypes.c_size_t()
    L = _lib.lib()
    assert L.dn_resnet_param_count(ctypes.byref(_lib.cfg(1, 3, 48)), ctypes.byref(n)) == -1  # DN_ERR_ARG
    assert "out_nc" in _lib.last_error()
    assert L.dn_resnet_param_count(ctypes.byref(_lib.cfg(1, 1, 32)), ctypes.byref(n)) == -1
    cfg = _lib.cfg(1, 1, 48)
    for N, H, W, ok in [(1, 1, 5, True), (2, 13, 22, True), (1, 0, 8, False), (0, 8, 8, False)]:
        assert (L.dn_resnet_workspace_size(ctypes.byref(cfg), N, H, W, 1, ctypes.byref(n)) == 0) == ok
    # bf16 is refused before any pointer is touched
    assert L.dn_resnet_forward_prec(ctypes.byref(cfg), None, None, None, 1, 8, 8, None, 0, 1, None) == -1
    assert "precision" in _lib.last_error()
    with pytest.raises(RuntimeError):
        RESNET(1, 1, 48)(torch.zeros(1, 1, 8, 8))


@pytest.mark.parametrize("in_nc,out_nc,names", [(2, 3, "out_nc"), (5, 5, "in_nc"), (0, 0, "in_nc")])
def test_channel_counts_outside_the_built_range_are_rejected(in_nc, out_nc, names):
    """in_nc == out_nc in 1..4 is what the kernels are instantiated for: anything else is a
    ValueError from the constructor and DN_ERR_ARG from the C-ABI's own check, whose message
    names the argument, before any workspace is sized or anything is launched"""
    from image_denoising_amd import RESNET, _lib

    with pytest.raises(ValueError, match=names):
        RESNET(in_nc=in_nc, out_nc=out_nc)
    n = ctypes.c_size_t()
    cfg = _lib.cfg(in_nc, out_nc, 48)
    assert _lib.lib().dn_resnet_param_count(ctypes.byref(cfg), ctypes.byref(n)) == -1
    assert names in _lib.last_error()
    assert _lib.lib().dn_resnet_workspace_size(ctypes.byref(cfg), 1, 8, 8, 1, ctypes.byref(n)) == -1
    assert names in _lib.last_error()


def test_name_dispatch_builds_resnet():
    from image_denoising_amd import RESNET, evaluation_adapter, finetune

    assert isinstance(finetune.build_base_model("RESNET", 1, 48), RESNET)
    m = evaluation_adapter.build_model("RESNET", 1, 48, 16)
    assert isinstance(m.base, RESNET) and not any(p.requires_grad for p in m.base.parameters())
