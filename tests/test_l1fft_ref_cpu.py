"""tests/l1fft_ref.py (the fp64 restatement the GPU tests compare with) against the reference
program's fixture tests/golden/l1fft.npz, and its half-spectrum weights against the direct sum
over the full spectrum.  No GPU."""
import numpy as np
import pytest
import torch

import l1fft_ref as R

TOL = 1e-12


def _key(shape):
    return "x".join(map(str, shape)) + "_"


@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES)
def test_restatement_equals_reference_fixture(golden, shape):
    fx = golden("l1fft.npz")
    k = _key(shape)
    pred, target = R.inputs(shape)
    got = np.array([pred.double().sum().item(), target.double().sum().item()])
    assert np.array_equal(got, fx[k + "insum"]), "the input generator drifted from the fixture's"
    l3, d = R.restatement(pred, target, R.GOLDEN_ALPHA, R.GOLDEN_BETA)
    assert abs(l3[0].item() - fx[k + "pix"]) <= TOL
    assert abs(l3[1].item() - fx[k + "frq"]) <= TOL
    assert abs(l3[2].item() - fx[k + "mean"]) <= TOL
    assert np.abs(d.numpy() - fx[k + "dmean"]).max() <= TOL
    l3s, ds = R.restatement(pred, target, R.GOLDEN_ALPHA, R.GOLDEN_BETA, reduction="sum")
    n = pred.numel()
    assert abs(l3s[2].item() - fx[k + "sum"]) <= TOL * n  # the sum is n times the mean
    assert np.abs(ds.numpy() - n * fx[k + "dmean"]).max() <= TOL * n


@pytest.mark.parametrize("shape", [s for s in R.SEEDS if np.prod(s) <= 8192])
def test_half_spectrum_weights_equal_full_spectrum_sum(shape):
    pred, target = R.inputs(shape)
    l3, _ = R.restatement(pred, target)
    full = R.full_spectrum_parts(pred, target)
    assert torch.allclose(l3[:2], full, rtol=1e-13, atol=0)
    # a column-W/2 (or column-0) weight of 2 is seen: the alternating image has only that bin
    N, C, H, W = shape
    alt = torch.tensor([1.0, -1.0]).repeat(W // 2).expand(shape).contiguous()
    l3, _ = R.restatement(0.25 * alt, torch.zeros(shape))
    assert abs(l3[1].item() - 0.25 * H * W * N * C / alt.numel()) <= 1e-13
    l3, _ = R.restatement(torch.full(shape, 0.5), torch.zeros(shape))
    assert abs(l3[1].item() - 0.5) <= 1e-13


def test_zero_bins_carry_no_gradient():
    shape = (1, 1, 8, 8)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3))
    l3, d = R.restatement(x, x.clone())
    assert float(l3.abs().max()) == 0.0 and float(d.abs().max()) == 0.0
    assert not torch.isnan(d).any()


def test_seeds_are_well_conditioned():
    for shape in R.SEEDS:
        mn, med = R.conditioning(*R.inputs(shape))
        assert mn > 1e-3 * med, (shape, mn, med)
