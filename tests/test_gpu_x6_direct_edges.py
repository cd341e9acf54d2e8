"""The direct split-bf16 3x3 kernels of csrc/conv_x6.hip -- k_c3x6<NT,MT>, k_c3x6h<NT,TAIL,MT>,
the 3-slot-ring k_c3x6h<NT,0,MT,3> and k_c3x6p<6,TAIL,false> -- pinned per instantiation the way
test_gpu_x6_edges.py pins the Winograd kernel: one table maps a shape and its strides to the
instantiation the default dispatcher (no environment variable) picks, and every case asserts that
label from the launch profiler's record.  Operands and results live in NaN-filled guarded
buffers (x6_edge_util): guard bands and gap channels must come back bit for bit, every live
output finite.  Errors are taken per region with the kernel's own tile height against an fp64
PyTorch reference on the CPU, under test_gpu_x6.py's bounds; one case per instantiation runs on
operands for which the arithmetic is exact and must equal fp64 bit for bit.  Needs an MI355X.

How launch_fwd_x6 routes a launch that is not Winograd (np = 32 / 48 / 96 output channels per
workgroup, nz = output-channel blocks, tiles16 = N * ceil(H/16) * ceil(W/16) * nz):
  * input not float4-addressable (in_stride % 4 or K % 4)          -> k_c3x6<np/16, MT>
  * aligned, tiles16 < 512 (x6_pipelined false): the 3-slot ring  -> k_c3x6h<np/16, 0, MT, 3>
    (MT = 1 at 96 channels)
  * aligned, tiles16 >= 512: np <= 48 or a tail-1 image            -> k_c3x6h<np/16, T, 2 or 4>
    (MT = 4 from 1024 tiles at np <= 48), else                     -> k_c3x6p<6, T, false>
MT of the first two is x6_pick_mt: 8-row tiles when the 4-row blocks need more rounds of the 512
resident workgroups than the 8-row blocks (here: more than 512 four-row blocks, at most 512
eight-row ones).  T is x6_tail_mode(K) when the C entry point found every view float4-aligned
(x6_image_mode), else 0: then the last chunk is plainly zero padded and the generic scalar
epilogue of conv_epi.h writes the result.  Winograd takes an aligned launch of exactly 48 or 96
outputs (or 48-channel blocks) from 512 8 x 16 tiles, so the aligned large-grid rows here have
33..47 or 49..95 outputs, or an odd output stride.

Instantiated but out of reach of the two op entry points at test sizes:
  * k_c3x6h<6,0,2> and k_c3x6h<6,2,2>: `half` in launch_fwd_x6 is np <= 48 || x6_tail == 1;
  * k_c3x6p<6,1,false>: the same line sends a tail-1 image to k_c3x6h<6,1,2>;
  * k_c3x6p<2,...> / k_c3x6p<3,...>: only when `half_fits` fails, a tile's 10 input rows past
    2 GiB."""
import functools

import pytest
import torch
import torch.nn.functional as F

from x6_edge_util import (assert_bit_equal, assert_regions, exact_operands, region_errors,
                          run_dgrad, run_forward)

pytestmark = pytest.mark.gpu
DEV = "cuda"
# |err| / max|ref| against fp64 (tests/test_gpu_x6.py)
X6_TOL = 2e-6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def L():
    from image_denoising_amd import _lib

    return _lib


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def tile_rows(label):
    """the tile height of an instantiation, from its label"""
    a = [int(v) for v in label[label.index("<") + 1:-1].replace("false", "0").split(",")]
    if label.startswith("k_c3x6p<"):
        return 16
    return 4 * (a[2] if label.startswith("k_c3x6h<") else a[1])


# (cin, cout, N, H, W, x_stride, y_stride, label).  Strides None: the row runs in two views,
# "dense" and "strided" (cin + 12 / cout + 4 floats per pixel, base pointers 4 floats in), which
# route alike; given: that one view ("odd"), base pointers 4 floats in.  Per kernel and tile
# height TH the rows hold a last tile row of 1 and of TH - 1 rows, a last tile column of 1 and of
# 15 pixels, and one image below TH x 16 (a single partial tile on all four borders).  K covers
# 32k, 32k + 4 / + 16 (tail modes 1 / 2), 32k + 24 (a full-mode partial chunk) and K % 4 != 0.
# Large grids take their tile count from N.
FWD = [
    # -- aligned, below 512 16 x 16 tiles: the 3-slot ring, 4-row tiles
    (96, 96, 2, 9, 17, None, None, "k_c3x6h<6,0,1,3>"),
    (56, 88, 3, 7, 31, None, None, "k_c3x6h<6,0,1,3>"),
    (36, 48, 4, 3, 5, None, None, "k_c3x6h<3,0,1,3>"),  # (tail modes need a large grid: plain)
    (48, 32, 2, 13, 33, None, None, "k_c3x6h<2,0,1,3>"),
    (32, 3, 2, 9, 17, None, None, "k_c3x6h<2,0,1,3>"),  # Cout % 4: the scalar epilogue
    (96, 96, 2, 9, 17, 96, 97, "k_c3x6h<6,0,1,3>"),     # an odd output stride: the same
    # ... 8-row tiles: more than 512 4-row blocks, fewer than 512 8 x 16 tiles (no Winograd)
    (32, 48, 4, 257, 17, None, None, "k_c3x6h<3,0,2,3>"),
    (36, 24, 4, 263, 31, None, None, "k_c3x6h<2,0,2,3>"),
    (32, 32, 260, 7, 5, None, None, "k_c3x6h<2,0,2,3>"),  # (one tile per image: N carries it)
    # -- an input that is not float4-addressable: K % 4 or x_stride % 4
    (3, 48, 2, 9, 17, None, None, "k_c3x6<3,1>"),
    (50, 96, 2, 7, 31, None, None, "k_c3x6<6,1>"),
    (33, 32, 2, 3, 5, None, None, "k_c3x6<2,1>"),
    (32, 30, 2, 9, 17, 33, 31, "k_c3x6<2,1>"),  # odd strides alone, Cout % 4
    (3, 96, 4, 257, 17, None, None, "k_c3x6<6,2>"),
    (6, 40, 4, 263, 31, None, None, "k_c3x6<3,2>"),
    (5, 20, 260, 7, 5, None, None, "k_c3x6<2,2>"),
    # -- aligned, 512..1023 tiles, at most 48 outputs (not exactly 48), or a 4-channel tail at
    # 49..95: two workgroups per CU, 8-row tiles
    (32, 32, 128, 17, 17, None, None, "k_c3x6h<2,0,2>"),
    (36, 32, 128, 23, 31, None, None, "k_c3x6h<2,1,2>"),
    (48, 24, 512, 7, 5, None, None, "k_c3x6h<2,2,2>"),
    (64, 40, 128, 17, 17, None, None, "k_c3x6h<3,0,2>"),
    (36, 36, 128, 23, 31, None, None, "k_c3x6h<3,1,2>"),
    (16, 44, 256, 3, 17, None, None, "k_c3x6h<3,2,2>"),
    (36, 88, 128, 17, 17, None, None, "k_c3x6h<6,1,2>"),
    # Cout % 4 with float4 strides: the tail image AND the scalar epilogue
    (36, 30, 128, 17, 17, 48, 32, "k_c3x6h<2,1,2>"),
    # -- from 1024 tiles: 16-row tiles
    (32, 32, 128, 17, 49, None, None, "k_c3x6h<2,0,4>"),
    (36, 20, 256, 31, 31, None, None, "k_c3x6h<2,1,4>"),
    (48, 28, 1024, 5, 7, None, None, "k_c3x6h<2,2,4>"),
    (56, 40, 128, 17, 49, None, None, "k_c3x6h<3,0,4>"),
    (4, 36, 256, 31, 31, None, None, "k_c3x6h<3,1,4>"),
    (80, 44, 1024, 5, 7, None, None, "k_c3x6h<3,2,4>"),
    # -- 49..95 outputs on a large grid: one workgroup per CU, 16-row tiles
    (32, 88, 128, 17, 17, None, None, "k_c3x6p<6,0,false>"),
    (16, 84, 128, 31, 31, None, None, "k_c3x6p<6,2,false>"),
    (56, 92, 512, 5, 7, None, None, "k_c3x6p<6,0,false>"),
    # y_stride % 4 with an aligned input on a large grid: dn_conv2d_forward_x6 asks for no tail
    # image and no Winograd, launch_fwd_x6 still finds the input aligned: the pipelined kernel on
    # a zero-padded 4-channel last chunk and the scalar epilogue
    (36, 96, 128, 17, 17, 36, 97, "k_c3x6p<6,0,false>"),
]

# (cin, cout, N, H, W, dx_stride, mask_stride, label): K = cout, the outputs are the cin
# channels, in 48-channel blocks over blockIdx.z above 96 (x6_dgrad_zc); dz is dense.  Strides
# None: "dense" and "strided" (cin + 4 / cin + 8, 4 floats in).
DGRAD = [
    # 48-channel output blocks off the Winograd kernel: below 512 8 x 16 tiles * blocks ...
    (144, 64, 2, 9, 17, None, None, "k_c3x6h<3,0,1,3>"),
    (120, 36, 4, 87, 17, None, None, "k_c3x6h<3,0,2,3>"),  # the last block holds 24 live channels
    # ... on a large grid with an odd dx_stride (no tail image, no Winograd; scalar epilogue) ...
    (120, 32, 44, 17, 17, 121, 128, "k_c3x6h<3,0,2>"),
    (144, 36, 128, 17, 17, 145, 152, "k_c3x6h<3,0,4>"),
    # ... and behind K % 4 (out_nc = 3 / 1 as the data gradient's K: dz is not float4-addressable)
    (120, 3, 2, 9, 17, None, None, "k_c3x6<3,1>"),
    (24, 3, 2, 11, 31, None, None, "k_c3x6<2,1>"),
    (24, 1, 4, 257, 17, None, None, "k_c3x6<2,2>"),
    (96, 50, 2, 7, 31, None, None, "k_c3x6<6,1>"),
    (96, 56, 3, 7, 31, None, None, "k_c3x6h<6,0,1,3>"),
    # large grids
    (30, 64, 128, 17, 17, None, None, "k_c3x6h<2,0,2>"),   # 30 outputs: the scalar epilogue
    (40, 36, 128, 23, 31, None, None, "k_c3x6h<3,1,2>"),
    (32, 4, 128, 17, 49, None, None, "k_c3x6h<2,1,4>"),
    (88, 16, 128, 31, 31, None, None, "k_c3x6p<6,2,false>"),
]

# every instantiation the default routes reach from the two entry points at test sizes
LABELS = {
    "k_c3x6<2,1>", "k_c3x6<3,1>", "k_c3x6<6,1>", "k_c3x6<2,2>", "k_c3x6<3,2>", "k_c3x6<6,2>",
    "k_c3x6h<6,0,1,3>", "k_c3x6h<3,0,1,3>", "k_c3x6h<3,0,2,3>", "k_c3x6h<2,0,1,3>",
    "k_c3x6h<2,0,2,3>",
    "k_c3x6h<2,0,2>", "k_c3x6h<2,1,2>", "k_c3x6h<2,2,2>", "k_c3x6h<2,0,4>", "k_c3x6h<2,1,4>",
    "k_c3x6h<2,2,4>",
    "k_c3x6h<3,0,2>", "k_c3x6h<3,1,2>", "k_c3x6h<3,2,2>", "k_c3x6h<3,0,4>", "k_c3x6h<3,1,4>",
    "k_c3x6h<3,2,4>",
    "k_c3x6h<6,1,2>",
    "k_c3x6p<6,0,false>", "k_c3x6p<6,2,false>",
}


def views(row):
    """(name, x_stride, y_stride, lead) of a FWD row"""
    cin, cout, xs, ys = row[0], row[1], row[5], row[6]
    if xs is None:
        return [("dense", cin, cout, 0), ("strided", cin + 12, cout + 4, 4)]
    return [("odd", xs, ys, 4)]


def dviews(row):
    """(name, dx_stride, mask_stride, lead) of a DGRAD row"""
    cin, dxs, ms = row[0], row[5], row[6]
    if dxs is None:
        return [("dense", cin, cin, 0), ("strided", cin + 4, cin + 8, 4)]
    return [("odd", dxs, ms, 4)]


def _id(row, *more):
    return "-".join([row[7], f"{row[0]}to{row[1]}", "x".join(map(str, row[2:5])), *map(str, more)])


@pytest.mark.parametrize("label", sorted(LABELS | {r[7] for r in FWD + DGRAD}))
def test_tables_reach_every_instantiation(label):
    """the labels of the two tables are exactly the set written out above: a dropped row, or a
    route that no longer reaches its kernel (the cases below assert each row's label), fails"""
    assert label in LABELS, f"{label} is in a table and not in the expected set"
    assert label in {r[7] for r in FWD + DGRAD}, f"no row reaches {label}"


# ---- forward -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _fwd_case(cin, cout, N, H, W, exact=False):
    """inputs (NHWC fp32) and the fp64 pre-activation reference (NHWC), once per shape"""
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    if exact:
        x, w, b = exact_operands(g, (N, cin, H, W), (cout, cin, 3, 3), cout)
    else:
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
        b = torch.randn(cout, generator=g) * 0.1
    ref = nhwc(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    return nhwc(x), w, b, ref, {}


def _fwd_ref(case, act):
    return (F.leaky_relu(case[3], 0.2) if act else case[3]).numpy()


# The (cin, cout) of the rows for which the fp32 op kernel is not built (dn_conv2d_pack_size
# answers 0: it is built for 17..48, 81..96 and 129..144 outputs), written out so that the
# 4 x e32 bound cannot quietly stop applying: every other row must have an e32, and an error of
# the fp32 op itself is an error of the test.  The rows' output counts are chosen inside those
# ranges wherever the route allows; 3 outputs and the 120-channel gradient (a last block of 24
# live channels) cannot be.
FWD_NO_FP32 = {(32, 3)}
DGRAD_NO_FP32 = {(120, 36), (120, 32), (120, 3)}


def fp32_built(lib, cin, cout, backward_data):
    return lib.lib().dn_conv2d_pack_size(cin, cout, 3, backward_data) != 0


def _fwd_e32(case, act):
    """the fp32 kernel's own error on this shape (dense views), once per (shape, act); None
    where the fp32 op kernel is not built for the channel counts (FWD_NO_FP32)"""
    cache = case[4]
    if act not in cache:
        x, w, b = case[:3]
        cin, cout = x.shape[3], w.shape[0]
        built = fp32_built(L(), cin, cout, 0)
        assert built == ((cin, cout) not in FWD_NO_FP32), (cin, cout, built)
        cache[act] = None
        if built:
            y32, _ = run_forward(L(), x, w, b, act, cin, cout, 0, False, None, DEV)
            cache[act] = max(region_errors(y32.numpy(), _fwd_ref(case, act)).values())
    return cache[act]


# (the row is the outermost loop: one reference per shape)
@pytest.mark.parametrize("row,view,act", [
    pytest.param(r, v, act, id=_id(r, v[0], f"act{act}"))
    for r in FWD for v in views(r) for act in (0, 1)])
def test_direct_forward(row, view, act):
    cin, cout, N, H, W, _, _, kernel = row
    case = _fwd_case(cin, cout, N, H, W)
    x, w, b = case[:3]
    y, label = run_forward(L(), x, w, b, act, view[1], view[2], view[3], True, kernel, DEV)
    assert label == kernel, (label, kernel)
    ref = _fwd_ref(case, act)
    e6 = assert_regions(y.numpy(), ref, X6_TOL, what=label, TH=tile_rows(kernel), TW=16)
    e32 = _fwd_e32(case, act)
    print(f"fwd {cin}->{cout} {N}x{H}x{W} {view[0]} act {act} {label}: e6 {e6:.3e} "
          f"e32 {e32 if e32 is None else format(e32, '.3e')}")
    if e32 is not None:
        assert e6 < 4 * e32 + 1e-7, (e6, e32)  # fp32-class, not bf16-class


# ---- data gradient -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dgrad_case(cin, cout, N, H, W, exact=False):
    """dz, mask, base (NHWC fp32), w, and the fp64 gradient: the correlation of dz with the
    flipped, transposed weights, which is what autograd computes for a stride-1 padded conv"""
    g = torch.Generator().manual_seed(cin + 7 * cout + H)
    if exact:
        dz, w, _ = exact_operands(g, (N, cout, H, W), (cout, cin, 3, 3))
        base = torch.randint(-4, 5, (N, cin, H, W), generator=g).float()
    else:
        dz = torch.randn(N, cout, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
        base = torch.randn(N, cin, H, W, generator=g)
    mask = torch.randn(N, cin, H, W, generator=g)
    grad = F.conv2d(dz.double(), w.double().flip(2, 3).transpose(0, 1).contiguous(), None,
                    padding=1)
    return nhwc(dz), w, nhwc(mask), nhwc(base), nhwc(grad), {}


def _dgrad_ref(case, mode):
    mask, base, grad = case[2], case[3], case[4]
    if mode == "mask":
        grad = torch.where(mask.double() > 0, grad, grad * 0.2)
    if mode == "accum":
        grad = grad + base.double()
    return grad.numpy()


def _dgrad_e32(case, mode):
    cache = case[5]
    if mode not in cache:
        dz, w, mask, base = case[:4]
        cout, cin = w.shape[:2]
        built = fp32_built(L(), cin, cout, 1)
        assert built == ((cin, cout) not in DGRAD_NO_FP32), (cin, cout, built)
        cache[mode] = None
        if built:
            d32, _ = run_dgrad(L(), dz, w, mask, base, mode, cin, cin, 0, False, None, DEV)
            cache[mode] = max(region_errors(d32.numpy(), _dgrad_ref(case, mode)).values())
    return cache[mode]


@pytest.mark.parametrize("row,view,mode", [
    pytest.param(r, v, mode, id=_id(r, v[0], mode))
    for r in DGRAD for v in dviews(r) for mode in ("plain", "mask", "accum")])
def test_direct_backward_data(row, view, mode):
    cin, cout, N, H, W, _, _, kernel = row
    case = _dgrad_case(cin, cout, N, H, W)
    dz, w, mask, base = case[:4]
    dx, label = run_dgrad(L(), dz, w, mask, base, mode, view[1], view[2], view[3], True, kernel,
                          DEV)
    assert label == kernel, (label, kernel)
    ref = _dgrad_ref(case, mode)
    e6 = assert_regions(dx.numpy(), ref, X6_TOL, what=f"{label} {mode}", TH=tile_rows(kernel),
                        TW=16)
    e32 = _dgrad_e32(case, mode)
    print(f"dgrad {cin}<-{cout} {N}x{H}x{W} {view[0]} {mode} {label}: e6 {e6:.3e} "
          f"e32 {e32 if e32 is None else format(e32, '.3e')}")
    if e32 is not None:
        assert e6 < 4 * e32 + 1e-7, (e6, e32)


# ---- exact operands: bit for bit ---------------------------------------------------------------
def _first_row(table, label):
    return next((r for r in table if r[7] == label), None)


@pytest.mark.parametrize("label", sorted(LABELS))
def test_direct_exact_bit_for_bit(label):
    """One row per instantiation (a forward row where there is one, in its strided or odd view)
    on x6_edge_util.exact_operands: every product and partial sum is exact in fp32 and the low
    bf16 pieces are zero, so whatever the order of summation the result must equal the fp64
    reference at every element -- an element off by less than the max-norm bound shows."""
    row = _first_row(FWD, label)
    if row is not None:
        cin, cout, N, H, W = row[:5]
        case = _fwd_case(cin, cout, N, H, W, True)
        v = views(row)[-1]
        y, got = run_forward(L(), case[0], case[1], case[2], 0, v[1], v[2], v[3], True, label, DEV)
        assert got == label
        assert_bit_equal(y, case[3], what=f"fwd {label}")
    row = _first_row(DGRAD, label)
    assert row is not None or _first_row(FWD, label) is not None, label
    if row is not None:
        cin, cout, N, H, W = row[:5]
        case = _dgrad_case(cin, cout, N, H, W, True)
        v = dviews(row)[-1]
        for mode in ("plain", "accum"):
            dx, got = run_dgrad(L(), case[0], case[1], case[2], case[3], mode, v[1], v[2], v[3],
                                True, label, DEV)
            assert got == label
            assert_bit_equal(dx, torch.from_numpy(_dgrad_ref(case, mode)),
                             what=f"dgrad {label} {mode}")
