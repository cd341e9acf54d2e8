"""The comparators of tests/test_gpu_x6_edges.py (x6_edge_util) fail when they should: on CPU
tensors, with an fp32 F.conv2d playing the kernel, every planted defect is flagged in the right
region or guard, and the untouched result passes.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from x6_edge_util import GUARD, REGIONS, assert_regions, guarded, ran_kernel, region_errors

TOL = 2e-6  # tests/test_gpu_x6.py's X6_TOL
N, H, W, CIN, COUT = 2, 11, 19, 8, 12  # a 3-row last tile row, a 3-pixel last tile column
STRIDE = COUT + 4
INTERIOR, RING, ROWS, COLS = REGIONS


@pytest.fixture(scope="module")
def conv():
    """(fp32 'kernel' result, fp64 reference), NHWC"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, CIN, H, W, generator=g)
    w = torch.randn(COUT, CIN, 3, 3, generator=g) * 0.1
    got = F.conv2d(x, w, None, padding=1).permute(0, 2, 3, 1).contiguous()
    ref = F.conv2d(x.double(), w.double(), None, padding=1).permute(0, 2, 3, 1).contiguous()
    return got, ref


def stored(got, fill=float("nan"), base=None):
    """the result as a kernel would leave it in a guarded strided view"""
    g = guarded((N, H, W, COUT), STRIDE, 4, fill)
    if base is not None:
        g.full.copy_(base)
    g.data.copy_(got)
    return g


def test_untouched_result_passes(conv):
    got, ref = conv
    g = stored(got)
    g.check()
    assert g.ptr % 16 == 0 and g.ptr == g.buf.data_ptr() + 4 * (GUARD + 4)
    assert torch.equal(g.data, got)
    errs = region_errors(g.data.numpy(), ref.numpy())
    assert set(errs) == set(REGIONS) and all(0 < e < TOL for e in errs.values()), errs
    assert assert_regions(g.data.numpy(), ref.numpy(), TOL) == max(errs.values())


def flagged(got, ref):
    errs = region_errors(got.numpy(), ref.numpy())
    return {k for k, v in errs.items() if not v < TOL}


def test_wrong_pixel_in_last_partial_column(conv):
    got, ref = conv
    bad = got.clone()
    bad[1, 4, 17, 3] += 1e-4 * float(ref.abs().max())  # column 17 of 16..18, off the ring
    assert flagged(bad, ref) == {COLS}
    with pytest.raises(AssertionError, match="last partial tile column"):
        assert_regions(bad.numpy(), ref.numpy(), TOL)


def test_wrong_pixel_in_last_partial_row(conv):
    got, ref = conv
    bad = got.clone()
    bad[0, 9, 5, 0] += 1e-4 * float(ref.abs().max())  # row 9 of 8..10, off the ring
    assert flagged(bad, ref) == {ROWS}


def test_wrong_border_pixel(conv):
    got, ref = conv
    bad = got.clone()
    bad[0, 0, 6, 2] += 1e-4 * float(ref.abs().max())
    assert flagged(bad, ref) == {RING}
    with pytest.raises(AssertionError, match="border ring"):
        assert_regions(bad.numpy(), ref.numpy(), TOL)
    bad = got.clone()
    bad[1, 5, 0, 2] = float("nan")  # an unwritten pixel of the left column
    assert flagged(bad, ref) == {RING}


def test_wrong_interior_pixel_and_global_scale(conv):
    got, ref = conv
    bad = got.clone()
    bad[1, 3, 7, 1] += 1e-4 * float(ref.abs().max())
    assert flagged(bad, ref) == {INTERIOR}
    # the denominator is the global max: a region where the reference is ~0 is not inflated
    ref0, got0 = ref.clone(), got.clone()
    ref0[:, :, 16:] *= 1e-9
    got0[:, :, 16:] = ref0[:, :, 16:].float()
    assert region_errors(got0.numpy(), ref0.numpy())[COLS] < TOL


def test_exact_tiles_have_no_partial_regions(conv):
    got, ref = conv
    errs = region_errors(got[:, :8, :16].numpy(), ref[:, :8, :16].numpy())
    assert errs[ROWS] == 0.0 and errs[COLS] == 0.0 and errs[INTERIOR] > 0 and errs[RING] > 0


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_touched_gap_channel(conv, fill):
    g = stored(conv[0], fill)
    g.full[1, 10, 18, COUT] = fill  # the same bits: not a touch
    g.check()
    g.full[1, 10, 18, COUT] = 0.0
    with pytest.raises(AssertionError, match=r"gap channel touched.*\(1, 10, 18\) \+ \(12,\)"):
        g.check()


def test_gap_nan_with_another_payload_is_a_touch(conv):
    g = stored(conv[0])
    g.full.view(torch.int32)[0, 0, 0, COUT + 1] ^= 1  # still a NaN, other bits
    with pytest.raises(AssertionError, match="gap channel touched"):
        g.check()


def test_touched_guard_before_and_after(conv):
    g = stored(conv[0])
    g.buf[GUARD + 3] = 0.0  # the last float before the inner pointer (the lead)
    with pytest.raises(AssertionError, match="front guard band touched"):
        g.check()
    g = stored(conv[0])
    g.buf[0] = 1.0
    with pytest.raises(AssertionError, match="front guard band touched"):
        g.check()
    g = stored(conv[0])
    g.buf[GUARD + 4 + N * H * W * STRIDE] = 0.0  # the first float past the last pixel's gap
    with pytest.raises(AssertionError, match="back guard band touched"):
        g.check()
    g = stored(conv[0])
    g.buf[-1] = 0.0
    with pytest.raises(AssertionError, match="back guard band touched"):
        g.check()


def test_accum_gap_keeps_its_base(conv):
    base = torch.randn(N, H, W, STRIDE, generator=torch.Generator().manual_seed(2))
    g = stored(conv[0], base=base)
    g.check(base=base)
    with pytest.raises(AssertionError, match="gap channel touched"):
        g.check()  # the gap holds the base, not the filler
    g.full[0, 3, 4, COUT + 2] += 1.0  # an accumulation that ran into the gap
    with pytest.raises(AssertionError, match=r"gap channel touched.*\(0, 3, 4\) \+ \(14,\)"):
        g.check(base=base)


def test_dense_view_has_guards_only(conv):
    g = guarded((N, H, W, COUT), COUT, 0)
    g.data.copy_(conv[0])
    g.check()
    g.buf[GUARD + N * H * W * COUT] = 0.0
    with pytest.raises(AssertionError, match="back guard band touched"):
        g.check()


class FakeLib:
    """the three profiler calls of image_denoising_amd._lib"""

    def __init__(self, recs):
        self.recs, self.calls = recs, []

    def profile_ops(self, on):
        self.calls.append(bool(on))

    def profile_ops_take(self):
        return self.recs


def rec(op, kernel):
    return dict(op=op, kernel=kernel, K=96, NOUT=96, H=9, W=17, N=128, flops=0.0, ms=0.1)


def test_ran_kernel_label_and_count():
    lib = FakeLib([rec("fwd3", "k_c3w6<0,96>")])
    with ran_kernel(lib, "k_c3w6<") as ran:
        pass
    assert ran.kernel == "k_c3w6<0,96>" and lib.calls == [True, False]
    with pytest.raises(AssertionError, match="expected 'k_c3w6<1,96>'"):
        with ran_kernel(lib, "k_c3w6<1,96>"):
            pass
    with ran_kernel(FakeLib([rec("fwd3", "k_c3x6<6,1>")])) as ran:  # a fallback: label only
        pass
    assert not ran.kernel.startswith("k_c3w6")
    # other ops' records do not count; none, two, or an unlabelled GEMM record fail
    with ran_kernel(FakeLib([rec("pack", ""), rec("wgrad3", "k_wgrad3p<4,48>")]), "k_wgrad3p<4,48>"):
        pass
    for recs in ([], [rec("pack", "")], [rec("fwd3", "k_c3w6<0,96>"), rec("fwd3", "k_c3w6<0,96>")],
                 [rec("dgrad3", "")]):
        with pytest.raises(AssertionError):
            with ran_kernel(FakeLib(recs)):
                pass


def test_ran_kernel_takes_the_op_names_to_look_for():
    fwd1 = rec("fwd1", "k_fwd<G_C1,3,1>")
    # the default set does not know the 1x1 / deconv records
    with pytest.raises(AssertionError, match="expected one GEMM launch record"):
        with ran_kernel(FakeLib([fwd1])):
            pass
    with ran_kernel(FakeLib([rec("pack", ""), fwd1]), "k_fwd<G_C1,3,1>", ops=("fwd1",)) as ran:
        pass
    assert ran.kernel == "k_fwd<G_C1,3,1>" and ran.record["op"] == "fwd1"
    with ran_kernel(FakeLib([rec("deconv", "k_fwd<G_UP,6,4>")]), "k_fwd<G_UP,", ops="deconv") as ran:
        pass
    assert ran.record["op"] == "deconv"
    # a record of the default set is NOT counted once the caller names its own set ...
    with pytest.raises(AssertionError, match=r"record of \('deconv_dgrad',\)"):
        with ran_kernel(FakeLib([rec("fwd3", "k_fwd<G_C3,6,4>")]), ops=("deconv_dgrad",)):
            pass
    # ... two records of the named set fail, and the prefix is still checked
    with pytest.raises(AssertionError):
        with ran_kernel(FakeLib([fwd1, rec("dgrad1", "k_fwd<G_C1,6,1>")]), ops=("fwd1", "dgrad1")):
            pass
    with pytest.raises(AssertionError, match="expected 'k_fwd<G_C1,6,'"):
        with ran_kernel(FakeLib([fwd1]), "k_fwd<G_C1,6,", ops=("fwd1",)):
            pass
    with pytest.raises(AssertionError, match="no op name"):
        with ran_kernel(FakeLib([fwd1]), ops=()):
            pass


def test_ran_kernel_disables_the_profiler_when_the_call_raises():
    lib = FakeLib([])
    with pytest.raises(RuntimeError, match="boom"):
        with ran_kernel(lib, "k_"):
            raise RuntimeError("boom")
    assert lib.calls == [True, False]
