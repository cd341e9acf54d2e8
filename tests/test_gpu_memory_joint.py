"""The joint finetune through the memory-bank adapter on the GPU:
DenoiserWithMemoryAdapter(freeze_base=False, use_no_grad_for_base=False) through loss.backward(),
and MemoryFinetuneTrainer's fused joint step.  Reference truth: fp64 torch-CPU autograd
(tests/memory_joint_ref.py).  Needs an MI355X.

Gradient tolerance: test_gpu_joint_finetune.py's -- per layer, max error relative to the layer's
largest gradient below 1e-3; outputs and losses at its FP32_TOL.

The bank's selection kernel takes square P x P queries.  The rectangular cases (RESNET 2x1x20x36,
UNet 1x3x32x64) therefore carry a small tensor bank `[K,C,H,W]` whose nearest entry is picked by
a torch argmin in the test (`_select_memory_patch` of that one model instance); the selection is
a constant of the gradient either way and is pinned by test_gpu_memory.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import joint_ref
import memory_joint_ref as J
import memory_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FP32_TOL = 1e-4   # test_gpu_parity.py
LAYER_TOL = 1e-3  # test_gpu_joint_finetune.py, per layer
PRECS = ["fp32", "fp32_x6"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class _Identity(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x


def _centre(base):
    """an untrained UNet answers near 0, where the adapter's clamp kills every gradient: move its
    output to 0.5 (test_gpu_memory.py's _step_setup does the same)"""
    sd = base.state_dict()
    for last in ("nin_c", "final"):
        if last + ".weight" in sd and type(base).__name__ != "RESNET":  # RESNET adds its input
            sd[last + ".weight"] = sd[last + ".weight"] * 0.05
            sd[last + ".bias"] = torch.full_like(sd[last + ".bias"], 0.5)
    base.load_state_dict(sd)


def _adapter_params(C):
    params, *_ = R.adapter_case("b3c1_17x23" if C == 1 else "b2c3_16x20")
    return {k: torch.from_numpy(v) for k, v in params.items()}


def _model(arch="UNet", shape=(2, 1, 32, 32), prec="fp32", freeze_base=False, base=None):
    """non-zero adapter parameters: at the reference initialisation local_net.4 and the hyper MLP
    are zero and two of the three routes are dead"""
    from image_denoising_amd import RESNET, ImprovedUNet, UNet
    from image_denoising_amd.memory import DenoiserWithMemoryAdapter, MemoryBank

    _, C, H, W = shape
    if base is None:
        torch.manual_seed(0)
        base = {"UNet": UNet, "RESNET": RESNET, "ImprovedUNet": ImprovedUNet}[arch](C, C, 48)
        base.set_precision(prec)
        _centre(base)
    P = min(H, W)
    noise = torch.from_numpy(R.bank_images((P, 4, P + 8, P + 12, 2, C), 310))
    bank = MemoryBank(noise, noise * 0.8 + 0.1, P, 4)
    model = DenoiserWithMemoryAdapter(base, C, 16, bank, freeze_base=freeze_base,
                                      use_no_grad_for_base=freeze_base).to(DEV)
    model.adapter.load_state_dict(_adapter_params(C))
    if H != W:  # a tensor bank of whole H x W entries, nearest by squared distance
        tn = torch.from_numpy(R.uniform(5 * C * H * W, 311).reshape(5, C, H, W).astype(np.float32))
        tn, tc = tn.to(DEV), (tn * 0.8 + 0.1).to(DEV)

        def select(noisy):
            with torch.no_grad():
                d = ((noisy[:, None] - tn[None]) ** 2).flatten(2).sum(-1)
                return tc[d.argmin(1)].contiguous()

        model._select_memory_patch = select
    return model


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
        m = _model(arch, shape)
        clean, noisy = _batch(shape)
        mem = m._select_memory_patch(noisy.to(DEV)).cpu()
        _refs[case] = J.joint_loss_and_grads(m.base.flat_params.cpu(), m.adapter.flat_params.cpu(),
                                             clean, noisy, mem, arch)
    return _refs[case]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(CASES))
def test_loss_backward_trains_base_and_adapter_vs_fp64(case, prec):
    from image_denoising_amd.finetune import FinetuneLoss

    arch, shape = CASES[case]
    C = shape[1]
    ref = _reference(case)
    model = _model(arch, shape, prec)
    clean, noisy = _batch(shape)
    pred = model(noisy.to(DEV))
    loss = FinetuneLoss(0.1)(pred, clean.to(DEV))
    loss.backward()
    assert rel_err(pred.detach().cpu().numpy(), ref["pred"].numpy()) < FP32_TOL
    assert abs(float(loss.detach()) - ref["loss3"][2]) <= FP32_TOL * ref["loss3"][2]
    gad, gbase = _flat_grad(model.adapter).cpu().numpy(), _flat_grad(model.base).cpu().numpy()
    worst = {}
    for key, (off, p) in zip(R.KEYS, model.adapter._param_views()):
        s = slice(off, off + p.numel())
        assert np.abs(ref["gad"].numpy()[s]).max() > 0, key
        worst["adapter." + key] = rel_err(gad[s], ref["gad"].numpy()[s])
    assert np.abs(ref["gbase"].numpy()).max() > 0
    for name, b, e in joint_ref.layer_ranges(arch, C):
        worst[name] = rel_err(gbase[b:e], ref["gbase"].numpy()[b:e])
    print(f"\n{case} {prec}: worst layer {max(worst, key=worst.get)} {max(worst.values()):.3e}")
    for name, e in worst.items():
        assert e < LAYER_TOL, (name, e)


@pytest.mark.parametrize("arch,shape,prec,lam_iq", [
    ("UNet", (2, 1, 32, 32), "fp32", 0.0), ("UNet", (2, 1, 32, 32), "fp32_x6", 0.1),
    ("RESNET", (2, 1, 20, 20), "fp32", 0.0), ("RESNET", (2, 1, 20, 20), "fp32_x6", 0.1),
    ("ImprovedUNet", (1, 1, 16, 16), "fp32", 0.1), ("ImprovedUNet", (1, 1, 16, 16), "fp32_x6", 0.0)])
def test_fused_joint_step_equals_autograd_path_bitwise(arch, shape, prec, lam_iq):
    """loss, both gradients and both buffers after Adam: MemoryFinetuneTrainer's joint step
    against loss.backward() followed by the same FlatAdam on each buffer"""
    from image_denoising_amd.finetune import finetune_iqsl_loss, finetune_loss
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer
    from image_denoising_amd.optim import FlatAdam

    clean, noisy = (t.to(DEV) for t in _batch(shape))
    iq = dict(t1=0.3, t2=0.7)
    auto = _model(arch, shape, prec)
    pred = auto(noisy)
    if lam_iq > 0:
        loss, dpred = finetune_iqsl_loss(pred.detach(), clean, 0.1, lam_iq, **iq)
    else:
        loss, dpred = finetune_loss(pred.detach(), clean, 0.1)
    pred.backward(dpred)
    g_ad, g_base = _flat_grad(auto.adapter), _flat_grad(auto.base)
    FlatAdam(auto.adapter.flat_params, lr=1e-4).step(g_ad)
    FlatAdam(auto.base.flat_params, lr=1e-4).step(g_base)
    fused = _model(arch, shape, prec)
    tr = MemoryFinetuneTrainer(fused, lr=1e-4, lambda_grad=0.1, lambda_iqsl=lam_iq,
                               iqsl=iq if lam_iq > 0 else None)
    assert tr.joint
    got = tr.train_step(clean, noisy)
    assert got.numel() == (4 if lam_iq > 0 else 3)
    assert torch.equal(got, loss)
    assert torch.equal(tr.grad, g_ad) and torch.equal(tr.base_grad, g_base)
    assert float(g_base.abs().max()) > 0 and torch.isfinite(g_base).all()
    assert torch.equal(fused.adapter.flat_params, auto.adapter.flat_params)
    assert torch.equal(fused.base.flat_params, auto.base.flat_params)
    assert tr.opt.step_count == tr.base_opt.step_count == 1


def test_guard_and_foreign_base_are_refused():
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer
    from image_denoising_amd.optim import GradGuard

    with pytest.raises(ValueError, match="both flat buffers"):
        MemoryFinetuneTrainer(_model(), guard=GradGuard())
    MemoryFinetuneTrainer(_model(freeze_base=True), guard=GradGuard())  # the frozen path keeps it
    with pytest.raises(TypeError, match="HIP backward"):
        MemoryFinetuneTrainer(_model(base=_Identity()))
    MemoryFinetuneTrainer(_model(base=_Identity(), freeze_base=True))


def test_frozen_path_and_module_refusals_are_unchanged():
    """use_no_grad_for_base=False with a frozen base still takes the frozen code; the adapter
    module itself keeps refusing an input that requires grad"""
    from image_denoising_amd.memory import DenoiserWithMemoryAdapter

    m = _model(freeze_base=True)
    m2 = DenoiserWithMemoryAdapter(m.base, 1, 16, m.bank, freeze_base=True,
                                   use_no_grad_for_base=False).to(DEV)
    m2.adapter.load_state_dict(_adapter_params(1))
    _, noisy = _batch((2, 1, 32, 32))
    a, b = m(noisy.to(DEV)), m2(noisy.to(DEV))
    assert torch.equal(a, b)
    b.sum().backward()
    assert all(p.grad is None for p in m2.base.parameters())
    assert all(p.grad is not None for p in m2.adapter.parameters())


def _worker(args, env_extra=None, n=1):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, PYTHONUNBUFFERED="1")
        if n > 1:
            env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable,
                                       os.path.join(HERE, "memory_joint_dp_worker.py"), *args],
                                      env=env, cwd=ROOT))
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0] * n, codes


def test_frozen_step_is_unchanged_by_the_joint_path(tmp_path):
    """two frozen steps in a fresh process before any joint object exists, then a joint step, then
    the two frozen steps again: losses and parameters bit-equal (no state leaks between paths)"""
    out = str(tmp_path / "frozen.npz")
    _worker([out, "frozen"])
    r = np.load(out)
    assert np.isfinite(r["losses_before"]).all()
    assert np.array_equal(r["losses_before"], r["losses_after"])
    assert np.array_equal(r["adapter_before"], r["adapter_after"])


def test_checkpoint_roundtrip_base_and_adapter(tmp_path):
    from image_denoising_amd import checkpoint
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer

    model = _model()
    clean, noisy = (t.to(DEV) for t in _batch((2, 1, 32, 32)))
    MemoryFinetuneTrainer(model, lr=1e-3).train_step(clean, noisy)
    path = checkpoint.save_finetune_checkpoint(model, str(tmp_path / "joint.pth"))
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert any(k.startswith("base.") for k in state)
    assert [k for k in state if k.startswith("adapter.")] == ["adapter." + k for k in R.KEYS]
    assert not any("bank" in k for k in state)  # the bank is not in the file
    other = _model()
    with torch.no_grad():
        other.base.flat_params.zero_()
        other.adapter.flat_params.zero_()
    missing, unexpected = checkpoint.load_checkpoint(other, path)
    assert not missing and not unexpected
    assert torch.equal(other.base.flat_params, model.base.flat_params)
    assert torch.equal(other.adapter.flat_params, model.adapter.flat_params)
    assert torch.equal(other(noisy), model(noisy))
    # a frozen model keeps writing the adapter-only file
    frozen = _model(freeze_base=True)
    state = torch.load(checkpoint.save_finetune_checkpoint(frozen, str(tmp_path / "ad.pth")),
                       map_location="cpu", weights_only=True)
    assert list(state) == R.KEYS


def test_two_rank_joint_step_equals_full_batch(tmp_path):
    """two ranks (gloo, one GPU) of the distributed joint step on the halves of a batch against
    the single-process step on the whole batch, test_gpu_dist.py's tolerances; rank 1 starts from
    perturbed weights, so the broadcast of both buffers is under test"""
    sys.path.insert(0, HERE)
    import memory_joint_dp_worker as Wk

    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer

    out = str(tmp_path / "dp.npz")
    _worker([out], n=2)
    r = np.load(out)
    assert np.array_equal(r["adapter0"], r["adapter1"]) and np.array_equal(r["base0"], r["base1"])
    model = Wk.build()
    tr = MemoryFinetuneTrainer(model, lr=1e-4, distributed=False)
    losses = Wk.run(tr, 0, 1).cpu().numpy()
    assert np.abs(r["losses"][0] - losses[0]).max() <= 1e-6 * np.abs(losses[0]).max()
    assert np.abs(r["losses"][1] - losses[1]).max() <= 1e-4 * np.abs(losses[1]).max()
    for k, g in (("grad", tr.grad), ("base_grad", tr.base_grad)):
        g = g.cpu().numpy()
        assert np.abs(r[k] - g).max() <= 1e-4 * np.abs(g).max(), k
    for k, flat in (("adapter0", model.adapter.flat_params), ("base0", model.base.flat_params)):
        d = np.abs(r[k] - flat.detach().cpu().numpy())
        assert (d > 1e-6).mean() < 2e-3, (k, (d > 1e-6).mean())
        assert d.max() <= 2 * 2 * 1e-4 + 1e-6, k


@pytest.mark.parametrize("prec", PRECS)
def test_two_joint_steps_vs_reference_fixture(golden, prec):
    """two steps of the reference's own DenoiserWithMemoryAdapter(freeze_base=False,
    use_no_grad_for_base=False) under its Adam (tests/golden/make_golden_memory_joint.py),
    test_gpu_joint_finetune.py's bounds: losses and first-step gradients at FP32_TOL, parameters
    after the second step within 1e-6"""
    from image_denoising_amd import UNet
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer
    from image_denoising_amd.memory import DenoiserWithMemoryAdapter, MemoryBank

    g = golden("memory_joint_c1.npz")
    s = J.golden_setup()
    torch.manual_seed(0)
    base = UNet(1, 1, 48)
    base.set_precision(prec)
    J.centre_state(base)
    bank = MemoryBank(s["bank_noise"], s["bank_clean"], s["patch"], s["stride"])
    model = DenoiserWithMemoryAdapter(base, 1, 16, bank, freeze_base=False,
                                      use_no_grad_for_base=False).to(DEV)
    model.adapter.load_state_dict(s["adapter"])
    assert np.array_equal(model.adapter.flat_params.cpu().numpy(), g["adapter_pre"])
    tr = MemoryFinetuneTrainer(model, lr=1e-4, lambda_grad=0.1)
    assert tr.joint
    for k in (1, 2):
        clean, noisy = (torch.from_numpy(g[f"{n}{k}"]).to(DEV) for n in ("clean", "noisy"))
        assert np.array_equal(model.bank.select(noisy).cpu().numpy(), g[f"idx{k}"])
        l3 = tr.train_step(clean, noisy).cpu().numpy()
        assert rel_err(l3, g[f"loss{k}"]) < FP32_TOL
        if k == 1:
            assert rel_err(tr.grad.cpu().numpy(), g["adapter_grad"]) < FP32_TOL
            gb = tr.base_grad.cpu().numpy()
            norms = [float(np.linalg.norm(gb[b:e])) for _, b, e in joint_ref.layer_ranges("UNet", 1)]
            assert rel_err(norms, g["base_grad_norms"]) < FP32_TOL
    assert np.abs(model.adapter.flat_params.cpu().numpy() - g["adapter_post2"]).max() < 1e-6
    assert np.abs(model.base.flat_params.cpu().numpy()[g["base_idx"]] - g["base_post2"]).max() < 1e-6
    assert tr.opt.step_count == tr.base_opt.step_count == 2

