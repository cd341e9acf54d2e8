"""The fp32 implicit-GEMM family k_fwd<GATHER, NT, MT> (csrc/conv.hip) and the bf16 kernels
k_fwd_bf16 / k_fwd_bf16p (csrc/conv_bf16.hip) through their op-level entry points, at every tile
height the launchers can select and where the tiles do not fit: one whole tile plus a ragged
remainder in H, a ragged last tile column, strided and odd-strided views, partial last K chunks
and N fragments, and grids of >= 16 blocks that are no multiple of 8 (xcd_tile's uneven runs).

Every buffer a kernel reads or writes is an x6_edge_util.guarded buffer filled with NaN: both
guard bands and every gap channel must survive bit for bit (for the accumulating epilogue the
gap holds the base's bits), and the whole output must have been written.  Each case asserts,
from the launch profiler's record, the instance it means to exercise -- the label decides
whether a case is valid, not the shape.  The result is compared element by element with an fp64
reference on the CPU under gemm_bound's derived bound c * (T + 3) * 2^-24 * A with c = C_BOUND;
no element is exempt and nothing is divided by a maximum.  Needs an MI355X."""
import functools

import pytest
import torch

import gemm_bound as gb
from x6_edge_util import guarded, ran_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
C_BOUND = 1  # every add rounds to nearest


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def L():
    from image_denoising_amd import _lib

    return _lib


def S():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _in(t, stride, lead=4):
    """a guarded device copy of the NHWC tensor t, read at `stride` floats per pixel"""
    gbuf = guarded(tuple(t.shape), stride, lead if stride > t.shape[3] else 0, NAN, DEV)
    gbuf.data.copy_(t)
    return gbuf


def _record(ran, op, K, NOUT, N, H, W, flops):
    rec = ran.record
    assert (rec["op"], rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == \
        (op, K, NOUT, N, H, W), rec
    assert rec["flops"] == flops, rec


def _report(family, what, ratio):
    print(f"RATIO {family} {ratio:.4f} {what}")


# ---- conv forward (3x3 and 1x1) ----------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _fwd_case(k, cin, cout, N, H, W, bf16=False):
    """inputs (NHWC fp32) and (ref, bound) of the activated forward, once per shape"""
    g = _gen(k, cin, cout, N, H, W)
    x = _randn(g, N, H, W, cin)
    w = _randn(g, cout, cin, k, k) * 0.1
    b = _randn(g, cout) * 0.1
    ref, bound = gb.conv_forward(x, w, b, 1, c=C_BOUND, bf16=bf16)
    return x, w, b, ref, bound


def _forward(case, k, x_stride, y_stride, kernel, bf16=False):
    """one activated forward through the C-ABI on guarded views -> y [N,H,W,cout] on the CPU"""
    _lib = L()
    x, w, b = case[:3]
    N, H, W, cin = x.shape
    cout = w.shape[0]
    gx = _in(x, x_stride)
    gy = guarded((N, H, W, cout), y_stride, 4 if y_stride > cout else 0, NAN, DEV)
    wg, bg = w.to(DEV), b.to(DEV)
    op = "fwd3" if k == 3 else "fwd1"
    with ran_kernel(_lib, kernel, ops=(op,)) as ran:
        if bf16:
            pk = _lib.scratch(_lib.lib().dn_conv2d_bf16_pack_size(cin, cout), DEV)
            _lib.call("dn_conv2d_forward_bf16", gx.ptr, x_stride, N, H, W, cin, wg.data_ptr(),
                      bg.data_ptr(), cout, 1, gy.ptr, y_stride, pk.data_ptr(), pk.numel(), S())
        else:
            pk = _lib.scratch(_lib.lib().dn_conv2d_pack_size(cin, cout, k, 0), DEV)
            _lib.call("dn_conv2d_forward", gx.ptr, x_stride, N, H, W, cin, wg.data_ptr(),
                      bg.data_ptr(), cout, k, 1, gy.ptr, y_stride, pk.data_ptr(), pk.numel(), S())
    torch.cuda.synchronize()
    _record(ran, op, cin, cout, N, H, W, 2.0 * cin * cout * k * k * N * H * W)
    gy.check(what=f"y ({ran.kernel})")
    gx.check(what=f"x ({ran.kernel})")
    return gy.data.cpu()


VIEWS = {"dense": (0, 0), "vec": (4, 8), "odd": (3, 1)}  # (x_stride - Cin, y_stride - Cout)

# Cout -> (Cin, {MT: (N, H, W)}): one whole tile plus a ragged remainder in H, a ragged last tile
# column, a block count >= 16 that is no multiple of 8 -- from pick_mt() restated on the CPU
C3_SHAPES = {
    32: (48, {4: (117, 41, 21), 2: (107, 21, 21), 1: (3, 5, 35)}),
    48: (48, {4: (117, 41, 21), 2: (107, 21, 21), 1: (3, 5, 35)}),
    96: (96, {4: (114, 33, 21), 2: (114, 9, 35), 1: (3, 5, 35)}),
    144: (96, {2: (97, 13, 21), 1: (3, 5, 35)}),
}
C3_FWD = [(cin, cout, mt) + nhw for cout, (cin, by_mt) in C3_SHAPES.items()
          for mt, nhw in by_mt.items()]
# MT = 1: a partial last K chunk (of 8 resp. 4 channels), a partial last N fragment
C3_FWD += [(50, 48, 1, 3, 5, 35), (97, 96, 1, 3, 5, 35), (48, 40, 1, 3, 5, 35),
           (96, 90, 1, 3, 5, 35), (96, 130, 1, 3, 5, 35)]


@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("cin,cout,mt,N,H,W", C3_FWD)
def test_c3_forward(cin, cout, mt, N, H, W, view):
    case = _fwd_case(3, cin, cout, N, H, W)
    kernel = f"k_fwd<G_C3,{(cout + 15) // 16},{mt}>"
    y = _forward(case, 3, cin + VIEWS[view][0], cout + VIEWS[view][1], kernel)
    what = f"fwd3 {cin}->{cout} {N}x{H}x{W} {view} {kernel}"
    _report("c3_fwd", what, gb.assert_within(y, case[3], case[4], what))


C1_SIZES = {"small": (2, 19, 21), "large": (65, 50, 53)}


def _c1_kernel(nout, size):
    nt = (nout + 15) // 16
    mt = 4 if nt == 1 else (1 if size == "small" else (2 if nt == 6 else 4))
    return f"k_fwd<G_C1,{nt},{mt}>"


@pytest.mark.parametrize("view", ["dense", "vec"])
@pytest.mark.parametrize("size", list(C1_SIZES))
@pytest.mark.parametrize("cin", [96, 40])
@pytest.mark.parametrize("cout", [1, 3, 24, 48, 96])
def test_c1_forward(cout, cin, size, view):
    N, H, W = C1_SIZES[size]
    case = _fwd_case(1, cin, cout, N, H, W)
    kernel = _c1_kernel(cout, size)
    y = _forward(case, 1, cin + VIEWS[view][0], cout + VIEWS[view][1], kernel)
    what = f"fwd1 {cin}->{cout} {N}x{H}x{W} {view} {kernel}"
    _report("c1_fwd", what, gb.assert_within(y, case[3], case[4], what))


# ---- conv data gradient (3x3 and 1x1) ----------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dgrad_case(k, cin, cout, N, H, W):
    g = _gen(k, cin, cout, N, H, W, 1)
    dz = _randn(g, N, H, W, cout)
    w = _randn(g, cout, cin, k, k) * 0.1
    mask = _randn(g, N, H, W, cin)
    base = _randn(g, N, H, W, cin)
    out = gb.conv_dgrad_modes(dz, w, ("plain", "mask", "accum"), mask, base, c=C_BOUND)
    return dz, w, mask, base, out


def _dgrad(case, k, mode, dx_stride, mask_stride, kernel):
    _lib = L()
    dz, w, mask, base = case[:4]
    N, H, W, cout = dz.shape
    cin = w.shape[1]
    gdz = _in(dz, cout)
    gm = _in(mask, mask_stride)
    gdx = guarded((N, H, W, cin), dx_stride, 4 if dx_stride > cin else 0, NAN, DEV)
    base_full = None
    if mode == "accum":  # a random base under the live channels AND the gap
        base_full = _randn(_gen(dx_stride), N, H, W, dx_stride)
        base_full[..., :cin] = base
        gdx.full.copy_(base_full)
    wg = w.to(DEV)
    pk = _lib.scratch(_lib.lib().dn_conv2d_pack_size(cin, cout, k, 1), DEV)
    op = "dgrad3" if k == 3 else "dgrad1"
    with ran_kernel(_lib, kernel, ops=(op,)) as ran:
        _lib.call("dn_conv2d_backward_data", gdz.ptr, N, H, W, cout, wg.data_ptr(), cin, k,
                  gm.ptr if mode == "mask" else None, mask_stride, 1 if mode == "accum" else 0,
                  gdx.ptr, dx_stride, pk.data_ptr(), pk.numel(), S())
    torch.cuda.synchronize()
    _record(ran, op, cout, cin, N, H, W, 2.0 * cout * cin * k * k * N * H * W)
    gdx.check(base=base_full, what=f"dx ({ran.kernel}, {mode})")
    gdz.check(what=f"dz ({ran.kernel})")
    gm.check(what=f"mask ({ran.kernel})")
    return gdx.data.cpu()


# (Cin, Cout, MT): the outputs are the Cin channels, K = Cout; the shape is C3_SHAPES' of nout = Cin
C3_DGRAD = [(48, 48, 4), (48, 48, 1), (96, 96, 4), (96, 96, 1), (144, 96, 2), (144, 96, 1),
            (96, 48, 2), (96, 48, 1)]
# (epilogue, mask_stride - Cin)
DGRAD_MODES = [("plain", 0), ("mask", 0), ("mask", 4), ("accum", 0)]


@pytest.mark.parametrize("mode,mgap", DGRAD_MODES)
@pytest.mark.parametrize("cin,cout,mt", C3_DGRAD)
def test_c3_backward_data(cin, cout, mt, mode, mgap):
    N, H, W = C3_SHAPES[cin][1][mt]
    case = _dgrad_case(3, cin, cout, N, H, W)
    kernel = f"k_fwd<G_C3,{(cin + 15) // 16},{mt}>"
    dx = _dgrad(case, 3, mode, cin + 8, cin + mgap, kernel)
    ref, bound = case[4][mode]
    what = f"dgrad3 {cin}<-{cout} {N}x{H}x{W} {mode} mask+{mgap} {kernel}"
    _report("c3_dgrad", what, gb.assert_within(dx, ref, bound, what))


@pytest.mark.parametrize("mode,mgap", [("plain", 0), ("mask", 4)])
@pytest.mark.parametrize("size", list(C1_SIZES))
@pytest.mark.parametrize("cin", [96, 40])
@pytest.mark.parametrize("cout", [1, 3, 24, 48, 96])
def test_c1_backward_data(cout, cin, size, mode, mgap):
    N, H, W = C1_SIZES[size]
    case = _dgrad_case(1, cin, cout, N, H, W)
    kernel = _c1_kernel(cin, size)
    dx = _dgrad(case, 1, mode, cin + 8, cin + mgap, kernel)
    ref, bound = case[4][mode]
    what = f"dgrad1 {cin}<-{cout} {N}x{H}x{W} {mode} {kernel}"
    _report("c1_dgrad", what, gb.assert_within(dx, ref, bound, what))


# ---- 2x2 deconvolution -------------------------------------------------------------------------
DECONV_SMALL = [(2, 5, 7), (3, 19, 21)]


@pytest.mark.parametrize("y_off", [0, 8])
@pytest.mark.parametrize("N,H,W", DECONV_SMALL)
@pytest.mark.parametrize("cin,cout", [(48, 48), (96, 96), (96, 48)])
def test_deconv_forward(cin, cout, N, H, W, y_off):
    _lib = L()
    g = _gen(cin, cout, N, H, W, 2)
    x = _randn(g, N, H, W, cin)
    w = _randn(g, cin, cout, 2, 2) * 0.1
    b = _randn(g, cout) * 0.1
    ref, bound = gb.deconv_forward(x, w, b, c=C_BOUND)
    stride = cout + 16
    gx = _in(x, cin)
    # the live channels are [y_off, y_off + cout) of each pixel: the gap is checked below
    gy = guarded((N, 2 * H, 2 * W, stride), stride, 4, NAN, DEV)
    wg, bg = w.to(DEV), b.to(DEV)
    pk = _lib.scratch(_lib.lib().dn_deconv2x2_pack_size(cin, cout, 0), DEV)
    kernel = f"k_fwd<G_UP,{cout // 16},4>"
    with ran_kernel(_lib, kernel, ops=("deconv",)) as ran:
        _lib.call("dn_deconv2x2_forward", gx.ptr, N, H, W, cin, wg.data_ptr(), bg.data_ptr(), cout,
                  gy.ptr, stride, y_off, pk.data_ptr(), pk.numel(), S())
    torch.cuda.synchronize()
    _record(ran, "deconv", cin, cout, N, H, W, 2.0 * N * H * W * cin * cout * 4)
    gy.check(what="y")
    gx.check(what="x")
    full = gy.data.cpu()
    live = torch.zeros(stride, dtype=torch.bool)
    live[y_off:y_off + cout] = True
    gap = full[..., ~live].contiguous().view(torch.int32)
    assert bool((gap == gy.fill_bits).all()), f"gap channels outside [{y_off}, {y_off + cout}) touched"
    y = full[..., live]
    worst = 0.0
    for a in (0, 1):  # parity by parity: a swapped (a, b) names itself
        for bb in (0, 1):
            what = f"deconv {cin}->{cout} {N}x{H}x{W} y_off {y_off} {kernel} parity ({a},{bb})"
            worst = max(worst, gb.assert_within(y[:, a::2, bb::2], ref[:, a::2, bb::2],
                                                bound[:, a::2, bb::2], what))
    _report("deconv_fwd", f"deconv {cin}->{cout} {N}x{H}x{W} y_off {y_off} {kernel}", worst)


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("N,H,W", DECONV_SMALL + [(65, 50, 53)])
@pytest.mark.parametrize("cin,cout", [(48, 48), (96, 96), (96, 48)])
def test_deconv_backward_data(cin, cout, N, H, W, masked):
    _lib = L()
    g = _gen(cin, cout, N, H, W, 3)
    dy = _randn(g, N, 2 * H, 2 * W, cout)
    w = _randn(g, cin, cout, 2, 2) * 0.1
    mask = _randn(g, N, H, W, cin)
    ref, bound = gb.deconv_dgrad(dy, w, mask if masked else None, c=C_BOUND)
    gdy = _in(dy, cout + 8)
    gm = _in(mask, cin)
    gdx = guarded((N, H, W, cin), cin, 0, NAN, DEV)
    wg = w.to(DEV)
    pk = _lib.scratch(_lib.lib().dn_deconv2x2_pack_size(cin, cout, 1), DEV)
    tiles = N * ((H + 15) // 16) * ((W + 15) // 16)
    kernel = f"k_fwd<G_DN2,{cin // 16},{1 if tiles < 1024 else 4}>"
    with ran_kernel(_lib, kernel, ops=("deconv_dgrad",)) as ran:
        _lib.call("dn_deconv2x2_backward_data", gdy.ptr, cout + 8, N, H, W, cout, wg.data_ptr(),
                  cin, gm.ptr if masked else None, gdx.ptr, pk.data_ptr(), pk.numel(), S())
    torch.cuda.synchronize()
    _record(ran, "deconv_dgrad", cout, cin, N, H, W, 2.0 * N * H * W * cin * cout * 4)
    gdx.check(what="dx")
    gdy.check(what="dy")
    gm.check(what="mask")
    what = f"deconv_dgrad {cin}<-{cout} {N}x{H}x{W} masked {masked} {kernel}"
    _report("deconv_dgrad", what, gb.assert_within(gdx.data.cpu(), ref, bound, what))


# ---- bf16 forward ------------------------------------------------------------------------------
# (Cin, Cout, N, H, W, x_stride - Cin, kernel)
BF16 = [
    (96, 96, 2, 19, 21, 0, "k_fwd_bf16<6,1,true>"),
    (48, 48, 2, 19, 21, 4, "k_fwd_bf16<3,1,true>"),
    # K % 4 != 0, or a view that is no multiple of 4 floats: off the pipelined kernel
    (97, 96, 65, 50, 53, 0, "k_fwd_bf16<6,4,true>"),
    (97, 48, 65, 50, 53, 0, "k_fwd_bf16<3,4,true>"),
    (96, 96, 65, 50, 53, 2, "k_fwd_bf16<6,4,true>"),
    (96, 96, 65, 50, 53, 4, "k_fwd_bf16p<6,4,false>"),  # (the same reference as the line above)
    (48, 48, 65, 50, 53, 2, "k_fwd_bf16<3,4,true>"),
    (48, 48, 65, 50, 53, 4, "k_fwd_bf16p<3,4,false>"),
]


@pytest.mark.parametrize("cin,cout,N,H,W,xgap,kernel", BF16)
def test_bf16_forward(cin, cout, N, H, W, xgap, kernel):
    case = _fwd_case(3, cin, cout, N, H, W, True)
    y = _forward(case, 3, cin + xgap, cout + 8, kernel, bf16=True)
    what = f"bf16 {cin}->{cout} {N}x{H}x{W} x+{xgap} {kernel}"
    _report("bf16", what, gb.assert_within(y, case[3], case[4], what))


def test_bf16_rows8_tile_equals_rows4():
    """k_fwd_bf16p<3,8> (>= 4096 tiles of 32 rows, H % 32 != 0, W % 16 != 0): the accumulation
    order does not depend on MT, so the whole output equals, bit for bit, the same images run as
    sub-batches that select <3,4>; the derived bound on the first, a middle and the last image."""
    _lib = L()
    cin = cout = 48
    N, H, W, sub = 128, 70, 170, 32
    g = _gen(cin, cout, N, H, W, 4)
    x = _randn(g, N, H, W, cin)
    w = _randn(g, cout, cin, 3, 3) * 0.1
    b = _randn(g, cout) * 0.1
    y8 = _forward((x, w, b), 3, cin + 4, cout + 8, "k_fwd_bf16p<3,8,false>", bf16=True)
    for n0 in range(0, N, sub):
        y4 = _forward((x[n0:n0 + sub], w, b), 3, cin + 4, cout + 8, "k_fwd_bf16p<3,4,false>",
                      bf16=True)
        assert torch.equal(y8[n0:n0 + sub].view(torch.int32), y4.view(torch.int32)), \
            f"images [{n0}, {n0 + sub}) differ between the 8- and the 4-row tile"
    worst = 0.0
    for n in (0, N // 2, N - 1):
        ref, bound = gb.conv_forward(x[n:n + 1], w, b, 1, c=C_BOUND, bf16=True)
        worst = max(worst, gb.assert_within(y8[n:n + 1], ref, bound, f"bf16p<3,8> image {n}"))
    _report("bf16", f"bf16 48->48 {N}x{H}x{W} k_fwd_bf16p<3,8,false>", worst)
