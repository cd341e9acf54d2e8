"""gemm_bound's per-element bound is neither too tight nor too loose: at the MT = 1 and small
shapes of tests/test_gpu_gemm_edges.py, with torch's own fp32 op playing the kernel, every element
of the fp32 result lies inside the bound, and each of four planted kernel errors -- one tap
dropped at one border pixel, one tile column shifted by a pixel, two adjacent channels swapped in
one 16-channel fragment, the last ragged row copied from the row above -- leaves it.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import gemm_bound as gb

TH, TW = 4, 16  # the MT = 1 tile


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


class Case:
    """one op at one shape: .ref / .bound (gemm_bound), .got (torch fp32), and .dropped, the fp32
    result of the same op with one tap (or, for a one-tap op, the first four input channels) of
    the weights zeroed"""

    def __init__(self, name, bound_fn, fp32_fn, w, drop):
        self.name = name
        self.ref, self.bound = bound_fn(w)
        self.got = fp32_fn(w)
        w0 = w.clone()
        w0[drop] = 0.0
        self.dropped = fp32_fn(w0)


def fwd_case(k, cin, cout, N, H, W, bf16=False):
    g = gen(k, cin, cout, N, H, W)
    x = torch.randn(N, H, W, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    r = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    drop = (slice(None), slice(None), 1, 2) if k == 3 else (slice(None), slice(0, 4))
    return Case(f"{'bf16' if bf16 else 'fwd'}{k} {cin}->{cout} {N}x{H}x{W}",
                lambda w_: gb.conv_forward(x, w_, b, 1, bf16=bf16),
                lambda w_: nhwc(F.leaky_relu(F.conv2d(nchw(r(x)), r(w_), b, padding=k // 2), 0.2)),
                w, drop)


def dgrad_case(k, cin, cout, N, H, W, mode):
    g = gen(k, cin, cout, N, H, W, 1)
    dz = torch.randn(N, H, W, cout, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1
    mask = torch.randn(N, H, W, cin, generator=g)
    base = torch.randn(N, H, W, cin, generator=g)

    def fp32(w_):
        d = nhwc(F.conv_transpose2d(nchw(dz), w_, None, padding=k // 2))
        if mode == "mask":
            d = torch.where(mask > 0, d, d * 0.2)
        return d + base if mode == "accum" else d

    drop = (slice(None), slice(None), 1, 2) if k == 3 else (slice(0, 4),)
    return Case(f"dgrad{k} {cin}<-{cout} {N}x{H}x{W} {mode}",
                lambda w_: gb.conv_dgrad(dz, w_, mode, mask, base), fp32, w, drop)


def deconv_fwd_case(cin, cout, N, H, W):
    g = gen(cin, cout, N, H, W, 2)
    x = torch.randn(N, H, W, cin, generator=g)
    w = torch.randn(cin, cout, 2, 2, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    return Case(f"deconv {cin}->{cout} {N}x{H}x{W}",
                lambda w_: gb.deconv_forward(x, w_, b),
                lambda w_: nhwc(F.conv_transpose2d(nchw(x), w_, b, stride=2)), w, (slice(0, 4),))


def deconv_dgrad_case(cin, cout, N, H, W, masked):
    g = gen(cin, cout, N, H, W, 3)
    dy = torch.randn(N, 2 * H, 2 * W, cout, generator=g)
    w = torch.randn(cin, cout, 2, 2, generator=g) * 0.1
    mask = torch.randn(N, H, W, cin, generator=g)

    def fp32(w_):
        d = nhwc(F.conv2d(nchw(dy), w_, None, stride=2))
        return torch.where(mask > 0, d, d * 0.2) if masked else d

    return Case(f"deconv_dgrad {cin}<-{cout} {N}x{H}x{W} masked {masked}",
                lambda w_: gb.deconv_dgrad(dy, w_, mask if masked else None), fp32, w,
                (slice(None), slice(None), 0, 1))


BUILDERS = (
    # fp32 3x3 forward, MT = 1: every (Cin, Cout) of the GPU file, the partial K chunks and N fragments
    [(fwd_case, (3, cin, cout, 3, 5, 35)) for cin, cout in
     [(48, 32), (48, 48), (96, 96), (96, 144), (50, 48), (97, 96), (48, 40), (96, 90), (96, 130)]]
    + [(dgrad_case, (3, cin, cout, 3, 5, 35, mode))
       for cin, cout in [(48, 48), (96, 96), (144, 96), (96, 48)]
       for mode in ("plain", "mask", "accum")]
    + [(fwd_case, (1, cin, cout, 2, 19, 21)) for cout in (1, 3, 24, 48, 96) for cin in (96, 40)]
    + [(dgrad_case, (1, cin, cout, 2, 19, 21, mode)) for cout in (1, 3, 24, 48, 96)
       for cin in (96, 40) for mode in ("plain", "mask")]
    + [(deconv_fwd_case, (cin, cout) + nhw) for cin, cout in [(48, 48), (96, 96), (96, 48)]
       for nhw in [(2, 5, 7), (3, 19, 21)]]
    + [(deconv_dgrad_case, (cin, cout) + nhw + (m,)) for cin, cout in [(48, 48), (96, 96), (96, 48)]
       for nhw in [(2, 5, 7), (3, 19, 21)] for m in (0, 1)]
    + [(fwd_case, (3, cin, cout, 2, 19, 21, True)) for cin, cout in [(96, 96), (48, 48), (97, 96)]]
)


_CASES = {}


def build(param):
    """the case of a BUILDERS entry, built once"""
    if param not in _CASES:
        _CASES[param] = param[0](*param[1])
    return _CASES[param]


def ident(p):
    return p[0].__name__ + "-" + "-".join(str(v) for v in p[1])


def out_shape(p):
    """(H, W, C) of the output of a BUILDERS entry"""
    fn, a = p
    if fn is fwd_case:
        return a[4], a[5], a[2]
    if fn is dgrad_case:
        return a[4], a[5], a[1]
    if fn is deconv_fwd_case:
        return 2 * a[3], 2 * a[4], a[1]
    return a[3], a[4], a[0]


every = pytest.mark.parametrize("param", BUILDERS, ids=ident)
# a second tile column / a second output channel, where the planted error needs one
two_columns = pytest.mark.parametrize("param", [p for p in BUILDERS if out_shape(p)[1] > TW], ids=ident)
two_channels = pytest.mark.parametrize("param", [p for p in BUILDERS if out_shape(p)[2] >= 2], ids=ident)


def outside(case, got):
    """the planted result leaves the bound: the ratio says so and the assertion raises"""
    r = gb.worst_ratio(got, case.ref, case.bound)
    with pytest.raises(AssertionError, match="outside the bound"):
        gb.assert_within(got, case.ref, case.bound, case.name)
    return r > 1.0


@every
def test_torch_fp32_is_inside_the_bound(param):
    case = build(param)
    assert tuple(case.got.shape[1:]) == out_shape(param)
    r = gb.assert_within(case.got, case.ref, case.bound, case.name)
    assert 0.0 < r <= 1.0, r
    assert bool((case.bound > 0).all())


@every
def test_dropped_tap_at_one_border_pixel(param):
    case = build(param)
    bad = case.got.clone()
    bad[0, 0, 5] = case.dropped[0, 0, 5]  # one pixel of the top row, all channels
    assert not torch.equal(bad, case.got)
    assert outside(case, bad), case.name


@two_columns
def test_tile_column_shifted_by_a_pixel(param):
    case = build(param)
    W = case.got.shape[2]
    bad = case.got.clone()
    bad[:, :, TW:] = case.got[:, :, TW - 1:W - 1]
    assert outside(case, bad), case.name


@two_channels
def test_adjacent_channels_swapped_in_one_fragment(param):
    case = build(param)
    C = case.got.shape[3]
    c0 = min(6, C - 2)
    bad = case.got.clone()
    bad[0, :TH, :TW, c0] = case.got[0, :TH, :TW, c0 + 1]
    bad[0, :TH, :TW, c0 + 1] = case.got[0, :TH, :TW, c0]
    assert outside(case, bad), case.name


@every
def test_last_ragged_row_copied_from_the_row_above(param):
    case = build(param)
    H = case.got.shape[1]
    assert H % TH, "the shapes have a ragged last tile row"
    bad = case.got.clone()
    bad[:, H - 1] = case.got[:, H - 2]
    assert outside(case, bad), case.name


def test_bf16_store_adds_half_an_ulp():
    g = gen(5)
    x = torch.randn(1, 5, 7, 16, generator=g)
    w = torch.randn(16, 16, 3, 3, generator=g) * 0.1
    b = torch.randn(16, generator=g) * 0.1
    ref, bound = gb.conv_forward(x, w, b, 1, bf16=True)
    ref2, bound2 = gb.conv_forward(x, w, b, 1, bf16=True, bf16_store=True)
    assert torch.equal(ref, ref2)
    assert torch.equal(bound2, bound + 2.0 ** -8 * ref.abs())
    got = nhwc(F.leaky_relu(F.conv2d(nchw(x.bfloat16().float()), w.bfloat16().float(), b,
                                     padding=1), 0.2))
    assert gb.worst_ratio(got.bfloat16().float(), ref, bound) > 1.0  # the store's own rounding
    gb.assert_within(got.bfloat16().float(), ref2, bound2, "bf16 store")


def test_constant_and_non_finite_results():
    case = fwd_case(3, 48, 48, 1, 5, 19)
    r1 = gb.worst_ratio(case.got, case.ref, case.bound)
    assert gb.worst_ratio(case.got, case.ref, 2 * case.bound) == pytest.approx(r1 / 2)
    bad = case.got.clone()
    bad[0, 2, 3, 4] = float("nan")  # an unwritten element
    assert gb.worst_ratio(bad, case.ref, case.bound) == float("inf")
    with pytest.raises(AssertionError, match=r"\(0, 2, 3, 4\)"):
        gb.assert_within(bad, case.ref, case.bound)
