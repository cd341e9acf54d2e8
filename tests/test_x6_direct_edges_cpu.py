"""What tests/test_gpu_x6_direct_edges.py rests on, checked without a GPU: the operands of its
exact cases really are exact (torch's fp32 conv2d on the CPU equals fp64 bit for bit at the
largest K of the tables, so the reference alone meets the condition, and one unit planted in one
tap is caught), its closed-form data-gradient reference is autograd's, and its tables hold the
tile geometry and the K values they claim per kernel and tile height."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_x6_direct_edges as T
from x6_edge_util import assert_bit_equal, exact_operands


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


KMAX = max([r[0] for r in T.FWD] + [r[1] for r in T.DGRAD])


def _exact(K, cout=8):
    g = torch.Generator().manual_seed(K)
    return exact_operands(g, (2, K, 9, 17), (cout, K, 3, 3), cout)


def test_exact_operands_are_what_they_claim():
    x, w, b = _exact(KMAX)
    assert x.abs().max() == 4 and set(x.unique().tolist()) == set(range(-4, 5))
    assert set((w * 8).unique().tolist()) == {-2, -1, 0, 1, 2}
    assert bool(((b * 8) == (b * 8).round()).all()) and b.abs().max() <= 1
    for t in (x, w, b):  # exact in bf16: the low pieces of the three-way split are zero
        assert torch.equal(t.to(torch.bfloat16).float(), t)


def test_fp32_conv_equals_fp64_on_exact_operands_at_the_largest_k():
    assert KMAX >= 96
    x, w, b = _exact(KMAX)
    got = nhwc(F.conv2d(x, w, b, padding=1))
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    assert float(ref.abs().max()) > 16  # sums that a dropped or doubled term would move
    assert_bit_equal(got, ref, "fp32 conv2d")
    # the same on the data gradient's accumulate form (an integer base)
    base = torch.randint(-4, 5, got.shape, generator=torch.Generator().manual_seed(1)).float()
    assert_bit_equal(got + base, ref + base.double(), "fp32 conv2d + base")


def test_one_unit_in_one_tap_is_caught():
    x, w, b = _exact(KMAX)
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    w1 = w.clone()
    w1[5, KMAX - 1, 2, 0] += 0.125  # one unit of the weight grid, the last channel's corner tap
    got = nhwc(F.conv2d(x, w1, b, padding=1))
    with pytest.raises(AssertionError, match="differ from fp64"):
        assert_bit_equal(got, ref, "planted")
    # ... and it is an error the max-norm bound of the random cases would not see at one pixel
    one = nhwc(F.conv2d(x, w, b, padding=1))
    one[1, 8, 16, 5] += 2.0 ** -19 * float(one[1, 8, 16, 5].abs().clamp(min=1))
    assert float((one.double() - ref).abs().max() / ref.abs().max()) < T.X6_TOL
    with pytest.raises(AssertionError, match=r"first at \(1, 8, 16, 5\)"):
        assert_bit_equal(one, ref, "one ulp-sized slip")


def test_bit_equal_ignores_the_sign_of_zero_only():
    ref = torch.tensor([0.0, -0.0, 1.0], dtype=torch.float64)
    assert_bit_equal(torch.tensor([-0.0, 0.0, 1.0]), ref)
    with pytest.raises(AssertionError):
        assert_bit_equal(torch.tensor([0.0, 0.0, float("nan")]), ref)
    with pytest.raises(AssertionError, match="not exact in fp32"):
        assert_bit_equal(torch.tensor([0.0]), torch.tensor([1.0 + 2.0 ** -40], dtype=torch.float64))


def test_dgrad_closed_form_is_autograd():
    for exact in (False, True):
        dz, w, _, _, grad, _ = T._dgrad_case(24, 3, 2, 11, 31, exact)
        x = torch.zeros(2, 24, 11, 31, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w.double(), None, padding=1).backward(dz.permute(0, 3, 1, 2).double())
        assert float((nhwc(x.grad) - grad).abs().max()) <= 1e-13 * float(grad.abs().max())


def _family(label):
    if label.startswith("k_c3x6h<") and label.endswith(",3>"):
        return "k_c3x6h ring3"
    return label[:label.index("<")]


def test_tables_hold_the_geometry_per_kernel_and_tile_height():
    """"Kernel" here is the kernel template -- k_c3x6, the 3-slot-ring k_c3x6h, k_c3x6h, k_c3x6p --
    at one tile height, not each NT / TAIL instantiation: the remainders are spread over a
    family's instantiations, so one instantiation need not see every remainder.  The image below
    one tile is checked as H < TH and W < 16 together (a single partial tile on all four
    borders)."""
    rows = {}
    for r in T.FWD + T.DGRAD:
        rows.setdefault((_family(r[7]), T.tile_rows(r[7])), []).append((r[3], r[4]))
    assert set(rows) == {("k_c3x6", 4), ("k_c3x6", 8), ("k_c3x6h ring3", 4), ("k_c3x6h ring3", 8),
                         ("k_c3x6h", 8), ("k_c3x6h", 16), ("k_c3x6p", 16)}
    for (fam, TH), hw in rows.items():
        have = {
            "last tile row of 1": any(H > TH and H % TH == 1 for H, _ in hw),
            "last tile row of TH - 1": any(H > TH and H % TH == TH - 1 for H, _ in hw),
            "last tile column of 1": any(W > 16 and W % 16 == 1 for _, W in hw),
            "last tile column of 15": any(W > 16 and W % 16 == 15 for _, W in hw),
            "one partial tile": any(H < TH and W < 16 for H, W in hw),
        }
        assert all(have.values()), (fam, TH, have)


def test_rows_without_an_fp32_kernel_are_the_listed_ones():
    """dn_conv2d_pack_size (host code, no GPU) answers 0 exactly for the rows the GPU file lists
    as having no fp32 op kernel, so its 4 x e32 bound applies to every other row"""
    from image_denoising_amd import _lib

    assert {(r[0], r[1]) for r in T.FWD if not T.fp32_built(_lib, r[0], r[1], 0)} == T.FWD_NO_FP32
    assert ({(r[0], r[1]) for r in T.DGRAD if not T.fp32_built(_lib, r[0], r[1], 1)}
            == T.DGRAD_NO_FP32)
    assert len(T.FWD_NO_FP32) + len(T.DGRAD_NO_FP32) <= 4


def test_tables_hold_the_k_values_and_views():
    ks = {r[0] for r in T.FWD} | {r[1] for r in T.DGRAD}
    assert any(k % 32 == 0 for k in ks) and any(k > 32 and k % 32 == 4 for k in ks)
    assert any(k > 32 and k % 32 == 16 for k in ks) and any(k > 32 and k % 32 == 24 for k in ks)
    assert any(k % 4 for k in ks)
    # the three routes no other test takes: an odd output stride behind an aligned input on a
    # large grid; outputs that are no multiple of 4 on the aligned kernels; 48-channel blocks
    # (a last one of 24) off the Winograd kernel
    assert any(r[5] is not None and r[5] % 4 == 0 and r[6] % 4 and r[7].startswith("k_c3x6p<")
               for r in T.FWD)
    assert any(r[1] % 4 and r[7].endswith(",3>") for r in T.FWD)
    assert any(r[1] % 4 and r[7].startswith("k_c3x6h<") and not r[7].endswith(",3>") for r in T.FWD)
    assert any(r[0] % 4 and r[7].startswith("k_c3x6h<") for r in T.DGRAD)
    assert any(r[0] == 120 and r[7].startswith("k_c3x6h<3,") for r in T.DGRAD)
    assert any(r[0] > 96 and r[7].startswith("k_c3x6<3,") for r in T.DGRAD)
    assert {r[7] for r in T.FWD + T.DGRAD} == T.LABELS and len(T.LABELS) == 26
    for r in T.FWD + T.DGRAD:  # small grids are small images
        if r[7].endswith(",3>") and not (r[3] < 8 and r[4] < 16):
            assert r[2] <= 4, r
