"""Helpers of tests/test_gpu_x6_edges.py and tests/test_gpu_x6_direct_edges.py (plain numpy /
torch): guarded strided NHWC buffers, per-region errors against a reference and the launch
profiler's record of the one GEMM kernel a call ran (these three checked on CPU tensors by
tests/test_x6_edge_util_cpu.py); the operands of the exact cases, exact_operands /
assert_bit_equal (checked by tests/test_x6_direct_edges_cpu.py); and the two op runners on
guarded views, run_forward / run_dgrad, which need the GPU and are exercised by the two GPU
files only."""
import contextlib

import numpy as np
import torch

GUARD = 4096  # floats of each guard band
GEMM_OPS = ("fwd3", "dgrad3", "wgrad3")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """One flat fp32 buffer [guard band | lead | N*H*W*stride floats | guard band], every float
    prefilled with `fill`.  The NHWC view of C live channels per pixel starts `lead` floats past
    the front guard band (the lead belongs to the front guard); channels [C, stride) of every
    pixel are the gap."""

    def __init__(self, shape_nhwc, stride, lead=4, fill=float("nan"), device="cpu", guard=GUARD):
        N, H, W, C = shape_nhwc
        assert stride >= C and lead >= 0 and lead % 4 == 0 and guard >= 4096 and guard % 4 == 0
        self.shape, self.stride, self.C = (N, H, W, C), stride, C
        self.off, self.inner = guard + lead, N * H * W * stride
        self.buf = torch.full((self.off + self.inner + guard,), fill, dtype=torch.float32,
                              device=device)
        self.fill_bits = int(_bits(torch.tensor([fill], dtype=torch.float32))[0])
        self.ptr = self.buf.data_ptr() + 4 * self.off
        assert self.ptr % 16 == 0, "inner pointer must be 16-byte aligned"

    @property
    def full(self):
        """[N, H, W, stride] view of the inner range (live channels and gap)"""
        N, H, W, _ = self.shape
        return self.buf[self.off:self.off + self.inner].view(N, H, W, self.stride)

    @property
    def data(self):
        """[N, H, W, C] view of the live channels"""
        return self.full[..., :self.C]

    def check(self, base=None, what="buffer"):
        """Both guard bands, and the gap channels of every pixel, hold what they were given, bit
        for bit: `fill`, or for the gap the values of `base` ([N, H, W, stride], what an
        accumulating call started from)."""
        b = _bits(self.buf)
        front, back = b[:self.off], b[self.off + self.inner:]
        for name, band, at in (("front", front, 0), ("back", back, self.off + self.inner)):
            bad = torch.nonzero(band != self.fill_bits)
            assert bad.numel() == 0, (
                f"{what}: {name} guard band touched: {bad.shape[0]} floats, first at flat index "
                f"{at + int(bad[0])} (inner range [{self.off}, {self.off + self.inner}))")
        if self.stride > self.C:
            N, H, W, _ = self.shape
            gap = b[self.off:self.off + self.inner].view(N, H, W, self.stride)[..., self.C:]
            if base is None:
                bad = torch.nonzero(gap != self.fill_bits)
            else:
                want = _bits(base.to(self.buf.device))[..., self.C:]
                bad = torch.nonzero(gap != want)
            assert bad.numel() == 0, (
                f"{what}: gap channel touched: {bad.shape[0]} floats, first at (n, y, x, c) = "
                f"{tuple(int(v) for v in bad[0][:3])} + ({self.C + int(bad[0][3])},)")


def guarded(shape_nhwc, stride, lead=4, fill=float("nan"), device="cpu"):
    """-> Guarded: .ptr is the 16-byte-aligned inner pointer, .check() the checker"""
    return Guarded(shape_nhwc, stride, lead, fill, device)


REGIONS = ("interior", "border ring", "last partial tile row", "last partial tile column")


def region_errors(got, ref, TH=8, TW=16):
    """max |got - ref| / max |ref| over four pixel regions of [N, H, W, C] arrays: the one-pixel
    image border ring, the rows of the last partial TH-row tile, the columns of the last partial
    TW-column tile, and the interior (pixels in none of the three).  The denominator is the
    global max of the reference, so a near-zero region cannot inflate its own ratio; an empty
    region gives 0.  A non-finite difference gives inf."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and got.ndim == 4, (got.shape, ref.shape)
    _, H, W, _ = ref.shape
    scale = max(float(np.abs(ref).max()), 1e-30)
    d = np.abs(got - ref).max(axis=(0, 3))  # [H, W]
    d = np.where(np.isfinite(d), d, np.inf)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ring = (yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)
    rows = yy >= H - H % TH if H % TH else np.zeros_like(ring)
    cols = xx >= W - W % TW if W % TW else np.zeros_like(ring)
    masks = (~(ring | rows | cols), ring, rows, cols)
    return {name: (float(d[m].max()) / scale if m.any() else 0.0) for name, m in zip(REGIONS, masks)}


def assert_regions(got, ref, bound, what="", TH=8, TW=16):
    """every region's error below `bound`; the message names the regions that fail"""
    errs = region_errors(got, ref, TH, TW)
    bad = {k: v for k, v in errs.items() if not v < bound}
    assert not bad, f"{what}: over {bound:.3g} of max|ref| in {sorted(bad)}: {errs}"
    return max(errs.values())


class _Ran:
    kernel = None
    record = None


@contextlib.contextmanager
def ran_kernel(lib, prefix=None, ops=GEMM_OPS):
    """Runs the body under the launch profiler and asserts that it took exactly one GEMM record
    (an op of `ops`; by default fwd3 / dgrad3 / wgrad3) whose kernel label starts with `prefix`
    (None: any label; the yielded object's .kernel / .record hold it after the block)."""
    ops = (ops,) if isinstance(ops, str) else tuple(ops)
    assert ops, "ran_kernel: no op name to look for"
    out = _Ran()
    lib.profile_ops(True)
    try:
        yield out
        recs = lib.profile_ops_take()
    finally:
        lib.profile_ops(False)
    gemm = [r for r in recs if r["op"] in ops]
    assert len(gemm) == 1, f"expected one GEMM launch record of {ops}, got {recs}"
    out.record, out.kernel = gemm[0], gemm[0]["kernel"]
    assert out.kernel, f"the GEMM record carries no kernel label: {gemm[0]}"
    if prefix is not None:
        assert out.kernel.startswith(prefix), f"ran {out.kernel!r}, expected {prefix!r}..."


# ---- the 3x3 ops through the C-ABI on guarded views ---------------------------------------------
NAN = float("nan")


def gemm_flops(rec):
    return 2.0 * rec["K"] * rec["NOUT"] * 9 * rec["N"] * rec["H"] * rec["W"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_forward(lib, x, w, b, act, x_stride, y_stride, lead, x6, prefix=None, device="cuda"):
    """One 3x3 forward (x NHWC, w OIHW, b on the CPU) through the C-ABI: x read at x_stride and y
    written at y_stride, both `lead` floats into NaN-filled guarded buffers.  x6: the split-bf16
    op, its one GEMM record checked against the shape and its label against `prefix`; else the
    fp32 op.  Guard bands and gap channels of x and y must come back untouched and y finite.
    -> (y [N, H, W, cout] on the CPU, label)"""
    N, H, W, cin = x.shape
    cout = w.shape[0]
    gx = guarded((N, H, W, cin), x_stride, lead, NAN, device)
    gx.data.copy_(x)
    gy = guarded((N, H, W, cout), y_stride, lead, NAN, device)
    wg, bg = w.to(device), b.to(device)
    if x6:
        pk = lib.scratch(lib.lib().dn_conv2d_x6_pack_size(cin, cout, 0), device)
        with ran_kernel(lib, prefix) as ran:
            lib.call("dn_conv2d_forward_x6", gx.ptr, x_stride, N, H, W, cin, wg.data_ptr(),
                     bg.data_ptr(), cout, act, gy.ptr, y_stride, pk.data_ptr(), pk.numel(),
                     _stream())
        rec = ran.record
        assert (rec["op"], rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == \
            ("fwd3", cin, cout, N, H, W), rec
        assert rec["flops"] == gemm_flops(rec), rec
        label = ran.kernel
    else:
        pk = lib.scratch(lib.lib().dn_conv2d_pack_size(cin, cout, 3, 0), device)
        lib.call("dn_conv2d_forward", gx.ptr, x_stride, N, H, W, cin, wg.data_ptr(),
                 bg.data_ptr(), cout, 3, act, gy.ptr, y_stride, pk.data_ptr(), pk.numel(),
                 _stream())
        label = "fp32"
    torch.cuda.synchronize()
    gy.check(what=f"y ({label})")
    gx.check(what=f"x ({label})")
    y = gy.data.cpu()
    assert bool(torch.isfinite(y).all()), f"{label}: non-finite or unwritten outputs"
    return y, label


def run_dgrad(lib, dz, w, mask, base, mode, dx_stride, mask_stride, lead, x6, prefix=None,
              device="cuda"):
    """One 3x3 data gradient (dz, mask, base NHWC, w OIHW on the CPU; mode plain / mask / accum)
    through the C-ABI: dz dense, the mask read at mask_stride and dx written at dx_stride, all in
    NaN-filled guarded buffers; accum starts from `base` under the live channels and a random
    base in the gap, which must come back bit for bit.  -> (dx [N, H, W, cin] on the CPU, label)"""
    N, H, W, cout = dz.shape
    cin = w.shape[1]
    gdz = guarded((N, H, W, cout), cout, lead, NAN, device)
    gdz.data.copy_(dz)
    gm = guarded((N, H, W, cin), mask_stride, lead, NAN, device)
    gm.data.copy_(mask)
    gdx = guarded((N, H, W, cin), dx_stride, lead, NAN, device)
    base_full = None
    if mode == "accum":  # a random base under the live channels AND the gap
        g = torch.Generator().manual_seed(dx_stride)
        base_full = torch.randn(N, H, W, dx_stride, generator=g)
        base_full[..., :cin] = base
        gdx.full.copy_(base_full)
    wg = w.to(device)
    name = "dn_conv2d_backward_data_x6" if x6 else "dn_conv2d_backward_data"
    size = (lib.lib().dn_conv2d_x6_pack_size(cin, cout, 1) if x6
            else lib.lib().dn_conv2d_pack_size(cin, cout, 3, 1))
    pk = lib.scratch(size, device)
    args = [gdz.ptr, N, H, W, cout, wg.data_ptr(), cin]
    if not x6:
        args.append(3)
    args += [gm.ptr if mode == "mask" else None, mask_stride, 1 if mode == "accum" else 0,
             gdx.ptr, dx_stride, pk.data_ptr(), pk.numel(), _stream()]
    if x6:
        with ran_kernel(lib, prefix) as ran:
            lib.call(name, *args)
        rec = ran.record
        assert (rec["op"], rec["K"], rec["NOUT"], rec["N"], rec["H"], rec["W"]) == \
            ("dgrad3", cout, cin, N, H, W), rec
        assert rec["flops"] == gemm_flops(rec), rec
        label = ran.kernel
    else:
        lib.call(name, *args)
        label = "fp32"
    torch.cuda.synchronize()
    gdx.check(base=base_full, what=f"dx ({label}, {mode})")
    gdz.check(what=f"dz ({label})")
    gm.check(what=f"mask ({label})")
    dx = gdx.data.cpu()
    assert bool(torch.isfinite(dx).all()), f"{label}: non-finite or unwritten outputs"
    return dx, label


# ---- operands on which the split-bf16 arithmetic is exact ---------------------------------------
def exact_operands(gen, x_shape, w_shape, nb=0):
    """(x, w, b): x integers -4..4, w from {-2..2} / 8, b multiples of 1/8 in [-1, 1].  Each
    value has at most 3 significant bits, so it is exact in bf16 (the low pieces of the split
    are zero), every product is a multiple of 1/8 of magnitude at most 1, and a sum of
    9 * K <= 9 * 4096 of them stays a multiple of 1/8 far below 2^24 / 8: exact in fp32 in any
    order of summation."""
    x = torch.randint(-4, 5, x_shape, generator=gen).float()
    w = torch.randint(-2, 3, w_shape, generator=gen).float() / 8
    b = torch.randint(-8, 9, (nb,), generator=gen).float() / 8
    return x, w, b


def assert_bit_equal(got, ref64, what=""):
    """got (fp32) equals the fp64 reference bit for bit at every element (the sign of a zero
    aside: x + 0.0 makes every zero +0)"""
    got = torch.as_tensor(got)
    ref = torch.as_tensor(ref64)
    assert got.dtype == torch.float32 and ref.dtype == torch.float64 and got.shape == ref.shape
    assert bool((ref.float().double() == ref).all()), f"{what}: the reference is not exact in fp32"
    bad = torch.nonzero(_bits(got + 0.0) != _bits(ref.float() + 0.0))
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} elements differ from fp64, first at {tuple(int(v) for v in bad[0])}: "
        f"{float(got[tuple(bad[0])])!r} vs {float(ref[tuple(bad[0])])!r}")
