"""The joint finetune on the CPU: tests/joint_ref.py (base and adapter trained through one
loss.backward(), one Adam) pinned to the fixture the reference produced
(tests/golden/make_golden_joint.py -> joint_c1.npz), at the tolerances the other oracle-vs-fixture
tests use (test_adapter_cpu.py, test_oracle_golden.py: losses 1e-5, gradients and their norms
1e-4 of the largest, parameters after Adam 1e-6 absolute).  And the host side of the feature:
the constructor flags, and the checkpoint of a finetune with a trained base."""
import hashlib

import numpy as np
import pytest
import torch

import joint_ref


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _model(freeze_base=False):
    from image_denoising_amd.adapter import DenoiserWithAdapter
    from image_denoising_amd.arch_unet import UNet

    torch.manual_seed(0)
    base = UNet(in_nc=1, out_nc=1, n_feature=48)
    torch.manual_seed(1)
    return DenoiserWithAdapter(base, in_channels=1, hidden_channels=16, freeze_base=freeze_base,
                               use_no_grad_for_base=freeze_base)


@pytest.fixture(scope="module")
def ref_steps(golden):
    g = golden("joint_c1.npz")
    model = _model()
    batches = [(torch.from_numpy(g[f"clean{s}"]), torch.from_numpy(g[f"noisy{s}"])) for s in (1, 2)]
    one = joint_ref.steps(model.base.flat_params, model.adapter.flat_params, batches[:1])
    two = joint_ref.steps(model.base.flat_params, model.adapter.flat_params, batches)
    return model, one, two


def test_fixture_starts_from_this_package_s_initialisation(golden):
    g = golden("joint_c1.npz")
    model = _model()
    assert hashlib.sha256(model.base.flat_params.numpy().tobytes()).hexdigest() == str(g["base_sha"])
    assert np.array_equal(model.adapter.flat_params.numpy(), g["adapter_pre"])
    assert all(p.requires_grad for p in model.parameters())
    assert [n for n, _, _ in joint_ref.layer_ranges("UNet", 1)] == list(g["layer_names"])
    assert g["adapter_grad"].size == 449


def test_joint_ref_first_step_matches_reference(golden, ref_steps):
    g = golden("joint_c1.npz")
    _, one, _ = ref_steps
    assert rel_err(one["losses"][0], g["loss1"]) < 1e-5
    assert rel_err(one["gad"].numpy(), g["adapter_grad"]) < 1e-4
    gb = one["gbase"].numpy()
    idx = g["base_idx"]
    # samples of every layer against the largest gradient of the base (test_oracle_golden.py's
    # convention for a sampled gradient), and every layer's norm
    assert np.abs(gb[idx] - g["base_grad_sample"]).max() < 1e-4 * float(g["base_grad_max"])
    norms = [float(np.linalg.norm(gb[b:e])) for _, b, e in joint_ref.layer_ranges("UNet", 1)]
    assert rel_err(norms, g["base_grad_norms"]) < 1e-4
    for (name, b, e), want in zip(joint_ref.layer_ranges("UNet", 1), g["base_grad_norms"]):
        assert want > 0, name  # the gradient reaches every layer of the base
    assert np.abs(one["adapter"].numpy() - g["adapter_post1"]).max() < 1e-6
    assert np.abs(one["base"].numpy()[idx] - g["base_post1"]).max() < 1e-6


def test_joint_ref_second_step_matches_reference(golden, ref_steps):
    g = golden("joint_c1.npz")
    _, _, two = ref_steps
    assert rel_err(two["losses"][1], g["loss2"]) < 1e-5
    assert np.abs(two["adapter"].numpy() - g["adapter_post2"]).max() < 1e-6
    assert np.abs(two["base"].numpy()[g["base_idx"]] - g["base_post2"]).max() < 1e-6
    # the base did move: Adam's first two updates are ~lr each where |g| >> eps = 1e-8 (the head;
    # at the reference initialisation the deep layers' gradients are far below eps)
    moved = np.abs(g["base_post2"] - _model().base.flat_params.numpy()[g["base_idx"]])
    assert moved.max() > 1e-4


def test_flags_are_kept_and_the_frozen_default_is_unchanged():
    joint, frozen = _model(False), _model(True)
    assert not joint.freeze_base and not joint.use_no_grad_for_base
    assert all(p.requires_grad for p in joint.base.parameters())
    assert frozen.freeze_base and not any(p.requires_grad for p in frozen.base.parameters())
    assert list(joint.state_dict()) == list(frozen.state_dict())


def test_finetune_checkpoint_round_trip(tmp_path):
    """a finetune with a trained base saves base.* and adapter.*; evaluation_adapter's --ckpt
    loader reads the file back into a freshly built model.  With a frozen base the file stays
    adapter-only."""
    from image_denoising_amd import checkpoint, evaluation_adapter

    model = _model(False)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():  # "trained": both buffers differ from every fresh initialisation
        model.base.flat_params.add_(0.01 * torch.randn(model.base.flat_params.shape, generator=gen))
        model.adapter.flat_params.add_(0.01 * torch.randn(449, generator=gen))
    for dp in (False, True):
        path = checkpoint.save_finetune_checkpoint(model, str(tmp_path / f"joint{int(dp)}.pth"),
                                                   data_parallel=dp)
        state = torch.load(path, map_location="cpu", weights_only=True)
        keys = [k[len("module."):] if dp else k for k in state]
        assert keys == list(model.state_dict())
        assert any(k.startswith("base.") for k in keys) and any(k.startswith("adapter.") for k in keys)
        fresh = evaluation_adapter.build_model("UNet", 1, 48, 16)
        assert not torch.equal(fresh.base.flat_params, model.base.flat_params)
        evaluation_adapter.load_adapter_weights(fresh, path)
        assert torch.equal(fresh.base.flat_params, model.base.flat_params)
        assert torch.equal(fresh.adapter.flat_params, model.adapter.flat_params)
    frozen = _model(True)
    path = checkpoint.save_finetune_checkpoint(frozen, str(tmp_path / "frozen.pth"))
    assert list(torch.load(path, map_location="cpu", weights_only=True)) == \
        list(frozen.adapter.state_dict())
