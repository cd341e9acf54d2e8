"""Helpers of tests/test_gpu_x6_edges.py (plain numpy / torch, checked on CPU tensors by
tests/test_x6_edge_util_cpu.py): guarded strided NHWC buffers, per-region errors against a
reference, and the launch profiler's record of the one GEMM kernel a call ran."""
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
                f"{what}: {name} guard band touched: {bad.numel()} floats, first at flat index "
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
                f"{what}: gap channel touched: {bad.numel()} floats, first at (n, y, x, c) = "
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
