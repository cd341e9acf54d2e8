"""The joint finetune on the GPU: DenoiserWithAdapter(freeze_base=False,
use_no_grad_for_base=False) through loss.backward(), and FinetuneTrainer's fused joint step.
Reference truth: fp64 torch-CPU autograd (tests/joint_ref.py), and the fixture the reference
produced (tests/golden/joint_c1.npz).  Needs an MI355X.

Gradient tolerance: test_gpu_parity.py::test_unet_forward_backward_vs_reference's -- per layer,
max error relative to the layer's largest gradient below 1e-3 (fp64 without matched masks: a
LeakyReLU / ReLU slope within rounding of zero may flip); outputs and losses at its FP32_TOL."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import joint_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FP32_TOL = 1e-4   # test_gpu_parity.py
LAYER_TOL = 1e-3  # test_gpu_parity.py::test_unet_forward_backward_vs_reference, per layer
PRECS = ["fp32", "fp32_x6"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _model(arch="UNet", C=1, prec="fp32", freeze_base=False):
    from image_denoising_amd import RESNET, ImprovedUNet, UNet
    from image_denoising_amd.adapter import DenoiserWithAdapter

    torch.manual_seed(0)
    base = {"UNet": UNet, "RESNET": RESNET, "ImprovedUNet": ImprovedUNet}[arch](C, C, 48)
    base.set_precision(prec)
    torch.manual_seed(1)
    return DenoiserWithAdapter(base, in_channels=C, hidden_channels=16, freeze_base=freeze_base,
                               use_no_grad_for_base=freeze_base).to(DEV)


def _batch(shape, seed=6):
    gen = torch.Generator().manual_seed(seed)
    clean = torch.rand(shape, generator=gen)
    return clean, clean + 0.1 * torch.randn(shape, generator=gen)


def _flat_grad(mod):
    return torch.cat([p.grad.reshape(-1) for p in mod.parameters()])


CASES = {"UNet-c1": ("UNet", (2, 1, 32, 32)), "RESNET-c1": ("RESNET", (2, 1, 20, 36)),
         "UNet-c3": ("UNet", (1, 3, 32, 64))}
_refs = {}


def _reference(case):
    """the fp64 loss and gradients of a case, computed once"""
    if case not in _refs:
        arch, shape = CASES[case]
        m = _model(arch, shape[1])
        clean, noisy = _batch(shape)
        _refs[case] = joint_ref.loss_and_grads(m.base.flat_params.cpu(), m.adapter.flat_params.cpu(),
                                               clean, noisy, arch)
    return _refs[case]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(CASES))
def test_loss_backward_trains_base_and_adapter_vs_fp64(case, prec):
    from image_denoising_amd.finetune import FinetuneLoss

    arch, shape = CASES[case]
    C = shape[1]
    ref = _reference(case)
    model = _model(arch, C, prec)
    clean, noisy = _batch(shape)
    pred = model(noisy.to(DEV))
    loss = FinetuneLoss(0.1)(pred, clean.to(DEV))
    loss.backward()
    assert rel_err(pred.detach().cpu().numpy(), ref["pred"].numpy()) < FP32_TOL
    assert abs(float(loss.detach()) - ref["loss3"][2]) <= FP32_TOL * ref["loss3"][2]
    gad, gbase = _flat_grad(model.adapter).cpu().numpy(), _flat_grad(model.base).cpu().numpy()
    worst = {}
    for off, p in model.adapter._param_views():
        s = slice(off, off + p.numel())
        worst[f"adapter@{off}"] = rel_err(gad[s], ref["gad"].numpy()[s])
    assert np.abs(ref["gbase"].numpy()).max() > 0
    for name, b, e in joint_ref.layer_ranges(arch, C):
        # (RESNET's up5.deconv is in its state_dict and unused: an exact zero on both sides)
        worst[name] = rel_err(gbase[b:e], ref["gbase"].numpy()[b:e])
    print(f"\n{case} {prec}: worst layer {max(worst, key=worst.get)} {max(worst.values()):.3e}")
    for name, e in worst.items():
        assert e < LAYER_TOL, (name, e)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("arch,shape", [("UNet", (2, 1, 32, 32)), ("RESNET", (2, 1, 20, 36)),
                                        ("ImprovedUNet", (1, 1, 16, 16))])
def test_fused_joint_step_equals_autograd_path_bitwise(arch, shape, prec):
    """loss, both gradients and both buffers after Adam: FinetuneTrainer's joint step against
    loss.backward() followed by the same FlatAdam on each buffer"""
    from image_denoising_amd.finetune import FinetuneLoss, FinetuneTrainer
    from image_denoising_amd.optim import FlatAdam

    clean, noisy = (t.to(DEV) for t in _batch(shape))
    auto = _model(arch, 1, prec)
    loss = FinetuneLoss(0.1)(auto(noisy), clean)
    loss.backward()
    g_ad, g_base = _flat_grad(auto.adapter), _flat_grad(auto.base)
    FlatAdam(auto.adapter.flat_params, lr=1e-4).step(g_ad)
    FlatAdam(auto.base.flat_params, lr=1e-4).step(g_base)
    fused = _model(arch, 1, prec)
    tr = FinetuneTrainer(fused, lr=1e-4, lambda_grad=0.1)
    assert tr.joint
    l3 = tr.train_step(clean, noisy)
    assert float(l3[2]) == float(loss)
    assert torch.equal(tr.grad, g_ad) and torch.equal(tr.base_grad, g_base)
    assert float(g_base.abs().max()) > 0 and torch.isfinite(g_base).all()
    assert torch.equal(fused.adapter.flat_params, auto.adapter.flat_params)
    assert torch.equal(fused.base.flat_params, auto.base.flat_params)


@pytest.mark.parametrize("prec", PRECS)
def test_two_joint_steps_vs_reference_fixture(golden, prec):
    from image_denoising_amd.finetune import FinetuneTrainer

    g = golden("joint_c1.npz")
    model = _model("UNet", 1, prec)
    assert np.array_equal(model.adapter.flat_params.cpu().numpy(), g["adapter_pre"])
    tr = FinetuneTrainer(model, lr=1e-4, lambda_grad=0.1)
    for s in (1, 2):
        l3 = tr.train_step(torch.from_numpy(g[f"clean{s}"]).to(DEV),
                           torch.from_numpy(g[f"noisy{s}"]).to(DEV)).cpu().numpy()
        assert rel_err(l3, g[f"loss{s}"]) < FP32_TOL
        if s == 1:
            assert rel_err(tr.grad.cpu().numpy(), g["adapter_grad"]) < FP32_TOL
            gb = tr.base_grad.cpu().numpy()
            norms = [float(np.linalg.norm(gb[b:e])) for _, b, e in joint_ref.layer_ranges("UNet", 1)]
            assert rel_err(norms, g["base_grad_norms"]) < FP32_TOL
    # test_gpu_adapter.py::test_finetune_step_vs_reference_fixture's bound on parameters after Adam
    assert np.abs(model.adapter.flat_params.cpu().numpy() - g["adapter_post2"]).max() < 1e-6
    assert np.abs(model.base.flat_params.cpu().numpy()[g["base_idx"]] - g["base_post2"]).max() < 1e-6
    assert tr.opt.step_count == tr.base_opt.step_count == 2


def test_frozen_default_is_unchanged_by_the_joint_path():
    from image_denoising_amd.finetune import FinetuneTrainer

    clean, noisy = (t.to(DEV) for t in _batch((2, 1, 32, 32)))

    def frozen_step():
        m = _model("UNet", 1, "fp32", freeze_base=True)
        base0 = m.base.flat_params.clone()
        tr = FinetuneTrainer(m, lr=1e-4, lambda_grad=0.1)
        assert not tr.joint and not hasattr(tr, "base_grad")
        l3 = tr.train_step(clean, noisy)
        assert torch.equal(m.base.flat_params, base0)  # the base's buffer: bit-unchanged
        assert all(p.grad is None for p in m.base.parameters())
        return l3.clone(), tr.grad.clone(), m.adapter.flat_params.clone()

    before = frozen_step()
    joint = _model("UNet", 1, "fp32")
    FinetuneTrainer(joint, lr=1e-4, lambda_grad=0.1).train_step(clean, noisy)
    after = frozen_step()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_guard_with_a_trained_base_is_refused():
    from image_denoising_amd.finetune import FinetuneTrainer
    from image_denoising_amd.optim import GradGuard

    with pytest.raises(ValueError, match="both flat buffers"):
        FinetuneTrainer(_model(), guard=GradGuard())
    FinetuneTrainer(_model(freeze_base=True), guard=GradGuard())  # the frozen path keeps it


def test_base_out_gradient_alone_with_frozen_adapter_parameters():
    from image_denoising_amd.adapter import OutputAdapter

    torch.manual_seed(2)
    ad = OutputAdapter(1, 16).to(DEV)
    for p in ad.parameters():
        p.requires_grad_(False)
    gen = torch.Generator().manual_seed(8)
    noisy, base, dout = (torch.randn(2, 1, 20, 36, generator=gen).to(DEV) for _ in range(3))
    b = base.clone().requires_grad_(True)
    ad(noisy, b).backward(dout)
    want = torch.empty_like(base)
    ad._run_backward_input(noisy, base, dout, want)
    assert torch.equal(b.grad, want) and all(p.grad is None for p in ad.parameters())
    _, db64, _ = joint_ref.adapter_input_grads(ad.flat_params.cpu(), noisy.cpu(), base.cpu(), dout.cpu())
    assert rel_err(b.grad.cpu().numpy(), db64.numpy()) < FP32_TOL


def test_one_rank_distributed_joint_step_bit_exact(tmp_path):
    """distributed=True on a one-rank RCCL group (both gradients all-reduced, the sum the identity)
    equals the distributed=False joint step bit for bit; a fresh process, as test_gpu_dist.py's"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "joint_dp.npz")
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), PYTHONUNBUFFERED="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "joint_dp_worker.py"), out], env=env,
                       cwd=ROOT, timeout=240)
    assert p.returncode == 0
    r = np.load(out)
    assert str(r["backend"]) == "nccl"
    for k in ("losses", "grad", "base_grad", "adapter", "base"):
        assert np.array_equal(r[k], r[k + "_local"]), k
