"""tests/memory_joint_ref.py against itself on the CPU: the closed form of the hyper route (what
csrc/memory.hip computes) equals fp64 autograd of memory_ref.features at every pinned feature
shape, and the hyper share of the whole input gradient is what the closed form gives for the
cotangent the hyper MLP hands back.  The fixture tests/golden/memory_joint_c1.npz (recorded from
the reference's own classes by tests/golden/make_golden_memory_joint.py) ties both to the
reference: its HyperGatedResidualAdapter(_FFT)'s dbase, and the first step of its joint run."""
import numpy as np
import pytest
import torch

import memory_joint_ref as J
import memory_ref as R


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("shape", J.FEATURE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_closed_form_equals_fp64_autograd_of_features(shape):
    x, cot = J.feature_inputs(shape)
    want = J.feature_adjoint_autograd(x, cot, shape[4]).numpy()
    got = J.hyper_closed_form(x, cot, shape[4])
    assert rel(got, want) <= 1e-12


def test_base_features_are_the_base_columns_of_memory_ref_features():
    x, _ = J.feature_inputs((2, 3, 16, 20, 3))
    t = torch.from_numpy(x).double()
    full = R.features(t * 0.5, t, t * 2.0, 3)
    mine = J.base_features(t, 3)
    assert torch.equal(full[:, [2, 3, 9, 10, 11]], mine)


@pytest.mark.parametrize("name", ["b3c1_17x23", "b2c3_16x20", "v4"])
def test_hyper_share_of_the_whole_gradient_is_the_closed_form(name):
    """dbase - (direct + local routes) == closed form at dfeat = W0^T dz0"""
    B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
    params, noisy, base, mem, dout = R.adapter_case(name)
    dbase, hyper = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp)
    p = {k: torch.from_numpy(v).double() for k, v in params.items()}
    n, b, m, d = (torch.from_numpy(v).double() for v in (noisy, base, mem, dout))
    _, k = R.forward(p, n, b, m, nb, clamp, keep=True)
    dpre = d * ((k["pre"] >= 0) & (k["pre"] <= 1)).double() if clamp else d
    g = k["gamma"][:, :, 0, 0]
    dhy = torch.cat([(k["r"] * dpre).sum((2, 3)) * g * (1 - g),
                     dpre.sum((2, 3)) * 0.1 * (1 - k["th"] ** 2)], 1)
    dz0 = (dhy @ p["hyper_mlp.2.weight"]) * (k["hh"] > 0).double()
    dfeat = dz0 @ p["hyper_mlp.0.weight"]
    cols = [2, 3] + [6 + nb + j for j in range(nb)]
    got = J.hyper_closed_form(base, dfeat[:, cols].numpy(), nb)
    assert rel(got, hyper.numpy()) <= 1e-9  # `hyper` is a difference of two O(1) gradients
    assert np.abs(hyper.numpy()).max() / np.abs(dbase.numpy()).max() > 1e-5


@pytest.mark.parametrize("name", J.DBASE_CASES)
def test_reference_adapter_agrees_with_memory_ref_on_dbase(name, golden):
    """the reference's own adapter (torch fp32, recorded) against memory_ref in fp64: within 4 x
    the error memory_ref itself makes in fp32 on the same inputs (the same arithmetic in the same
    format; the recorded errors are 7.6e-8 .. 8.3e-8)"""
    fx = golden("memory_joint_c1.npz")
    B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
    params, noisy, base, mem, dout = R.adapter_case(name)
    insum = [v.astype(np.float64).sum() for v in (noisy, base, mem, dout)] \
        + [R.flat_of(params).astype(np.float64).sum()]
    assert np.array_equal(fx[name + "_insum"], np.array(insum))  # the generators have not drifted
    want, _ = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp, torch.float64)
    own32, _ = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp, torch.float32)
    err, tol = rel(fx[name + "_dbase"], want.numpy()), 4 * rel(own32.numpy(), want.numpy())
    print(f"\n{name}: reference dbase err {err:.2e} tol {tol:.2e}")
    assert err <= tol


def test_fp64_restatement_reproduces_the_reference_joint_step(golden):
    """loss, prediction, adapter gradient and per-layer base gradient norms of the reference's
    first joint step (fp32) against memory_joint_ref in fp64, at test_gpu_parity.py's FP32_TOL"""
    import joint_ref
    from oracle import unet_ref  # noqa: F401  (joint_ref's UNet restatement)

    g = golden("memory_joint_c1.npz")
    s = J.golden_setup()
    clean, noisy = s["batches"][0]
    assert np.array_equal(clean.numpy(), g["clean1"]) and np.array_equal(noisy.numpy(), g["noisy1"])
    P, st = s["patch"], s["stride"]
    nbank, cbank = R.bank_patches(s["bank_noise"], P, st), R.bank_patches(s["bank_clean"], P, st)
    idx = R.select(noisy.double(), nbank.double())[0]
    assert np.array_equal(idx.numpy(), g["idx1"])
    base_flat = J.golden_base_flat()
    ad_flat = torch.from_numpy(g["adapter_pre"])
    ref = J.joint_loss_and_grads(base_flat, ad_flat, clean, noisy, cbank[idx], "UNet")
    tol = 1e-4
    assert rel(ref["loss3"], g["loss1"]) < tol
    assert rel(ref["pred"].numpy(), g["pred1"]) < tol
    assert rel(ref["gad"].numpy(), g["adapter_grad"]) < tol
    gb = ref["gbase"].numpy()
    norms = [float(np.linalg.norm(gb[b:e])) for _, b, e in joint_ref.layer_ranges("UNet", 1)]
    assert rel(norms, g["base_grad_norms"]) < tol
    assert rel(gb[g["base_idx"]], g["base_grad_sample"]) < tol

