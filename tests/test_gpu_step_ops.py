"""The training step's elementwise kernels (csrc/elementwise.hip, and dn_l1_mean_batched of
eval.hip), op by op, on every path their launchers choose.  Needs an MI355X.

Conventions of this module:

* Guard bands.  Every buffer a kernel is handed is a view (`Buf`) into a larger byte allocation
  filled with 0xA5: 256 bytes (64 floats) in front, the view, 256 bytes behind.  After the call
  both bands must be unchanged bit for bit.  256 bytes keep the view 16-byte aligned.
* Misaligned views.  `shift=1` moves the view one element further (4 bytes for fp32, 1 byte for
  uint8).  The float4 / uchar4 kernels are gated on pointer alignment, so this is how their scalar
  twins are reached at vector-friendly shapes.
* Calling route.  The Python wrappers allocate their outputs themselves, so a guarded output needs
  `_lib.call`; every test here calls the C entry point directly except Adam, which goes through
  `FlatAdam` (it takes its buffers from the caller).
* Route proof.  Each test names the kernel each case takes and the launcher condition that sends
  it there.  The launch profiler records only the op name for these ops (no kernel name), so the
  comment is the proof.
* Tolerances.  Each is bit-equality, a bound tests/step_ops_ref.py derives from the reference's
  magnitudes, or the number an existing test of this project uses for the same op; each says
  which.  Seeds are fixed, nothing is statistical.

`k_nchw_to_slice` and `k_add_slice` have no C entry point and stay covered through the network
tests (test_gpu_parity.py, test_gpu_resnet.py).  Left out for their size: the second trip of the
max-pool kernels' grid-stride loop (a 268 MB input).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_ops_ref as R
from oracle import n2n_ref, philox

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0xA5
SENT32 = int(np.array([SENT] * 4, np.uint8).view(np.int32)[0])
GUARD_BYTES = 256
ERR_ARG = r"status -1\)"  # DN_ERR_ARG


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_denoising_amd import _lib

    _lib.lib()
    torch.manual_seed(1234)


def L():
    from image_denoising_amd import _lib

    return _lib


def S():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """[256 guard bytes | shift elements | view of `shape` | 256 guard bytes (+ pad)], all 0xA5"""

    def __init__(self, shape, dtype=torch.float32, shift=0, init=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        self.lo = GUARD_BYTES + shift * item
        self.hi = self.lo + int(np.prod(shape)) * item
        total = self.hi + GUARD_BYTES
        self.raw = torch.full((total + (-total) % 16,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)
        assert self.raw.data_ptr() % 256 == 0
        assert self.t.data_ptr() % 16 == (shift * item) % 16
        if init is not None:
            self.t.copy_(torch.as_tensor(init).reshape(shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what="buffer"):
        for name, band in (("front", self.raw[:self.lo]), ("back", self.raw[self.hi:])):
            assert bool((band == SENT).all()), f"{what}: {name} guard band was written"

    def untouched(self):
        return bool((self.raw == SENT).all())

    def np(self):
        return self.t.cpu().numpy()

    def bits(self):
        return self.t.cpu().numpy().reshape(-1).view(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.int32), b.reshape(-1).view(np.int32))


# =============================================================================================
# Gaussian noise: k_noise4 when per_image % 4 == 0, elem_base % 4 == 0 and both pointers are
# 16-byte aligned (launch_noise); the scalar k_noise otherwise.
# =============================================================================================
SIG = float(np.float32(25.0 / 255.0))


def _gauss(clean, N, per, sig, sig_img, seed, off, base, shift_in=0, shift_out=0):
    """-> (clean Buf, noisy Buf); the guard bands of both are checked"""
    c = Buf((N, per), shift=shift_in, init=clean)
    out = Buf((N, per), shift=shift_out)
    s = None if sig_img is None else Buf((N,), init=np.asarray(sig_img, np.float32))
    L().call("dn_add_gauss_noise", c.ptr, N, per, float(sig), None if s is None else s.ptr, seed,
             off, base, out.ptr, S())
    torch.cuda.synchronize()
    c.check("clean")
    out.check("noisy")
    assert np.array_equal(c.np(), np.asarray(clean, np.float32).reshape(N, per)), "input changed"
    return c, out


def _gauss_check(noisy, clean, sig, seed, off, base, per, idx=None):
    """assertion 1: |noisy - (clean + sigma z)| <= 2e-6 sigma / (25/255), z the fp64 Box-Muller
    normals of oracle.philox.  2e-6 at sigma = 25/255 is test_gauss_noise_matches_philox_oracle's
    bound; the issue scales it by sigma.  `idx`: flat indices of a sampled check."""
    clean = np.asarray(clean, np.float64).reshape(-1)
    noisy = np.asarray(noisy, np.float64).reshape(-1)
    e = np.arange(clean.size, dtype=np.uint64) if idx is None else np.asarray(idx, np.uint64)
    z = philox.normal(seed, off, e + np.uint64(base))
    sig = np.asarray(sig, np.float32).astype(np.float64).reshape(-1)
    sig_e = sig[(e // np.uint64(per)).astype(np.int64)] if sig.size > 1 else sig[0]
    err = np.abs(noisy - (clean + sig_e * z))
    bound = 2e-6 * sig_e / (25.0 / 255.0)
    worst = float((err / bound).max())
    print(f"gauss worst err/bound {worst:.3f} over {e.size} elements")
    assert (err <= bound).all(), worst


GAUSS_CASES = {
    # name: (N, per_image, elem_base, shift_in, shift_out, per-image sigmas)
    "a_3x35_scalar": (3, 35, 0, 0, 0, None),            # per_image % 4 != 0      -> k_noise
    "b_4096_base6_scalar": (1, 4096, 6, 0, 0, None),    # elem_base % 4 != 0      -> k_noise
    "c_2x128_base8_vector": (2, 128, 8, 0, 0, None),    # all three conditions    -> k_noise4
    "e_3x64_sigmas_vector": (3, 64, 0, 0, 0, (5 / 255, 25 / 255, 50 / 255)),   # -> k_noise4
    "e_3x35_sigmas_scalar": (3, 35, 0, 0, 0, (5 / 255, 25 / 255, 50 / 255)),   # -> k_noise
    "e_3x64_sigmas_misaligned_scalar": (3, 64, 0, 1, 1, (5 / 255, 25 / 255, 50 / 255)),  # -> k_noise
    "f_base_2p34_4_vector": (2, 128, 2 ** 34 + 4, 0, 0, None),   # high counter word -> k_noise4
    "f_base_2p34_6_scalar": (2, 128, 2 ** 34 + 6, 0, 0, None),   # high counter word -> k_noise
}


@pytest.mark.parametrize("case", list(GAUSS_CASES))
def test_gauss_noise_paths_vs_philox_oracle(case):
    N, per, base, si, so, sigs = GAUSS_CASES[case]
    clean = np.random.default_rng(1).random((N, per)).astype(np.float32)
    _, out = _gauss(clean, N, per, SIG, sigs, 9, 4, base, si, so)
    _gauss_check(out.np(), clean, SIG if sigs is None else sigs, 9, 4, base, per)


def test_gauss_noise_misaligned_views_equal_aligned_bits():
    """case (d): 2x1x8x16 at elem_base 8 is k_noise4; the same data in views one float off 16-byte
    alignment (either or both) is k_noise.  "The same values" (kernel comment): bit-equal."""
    clean = np.random.default_rng(2).random((2, 128)).astype(np.float32)
    _, ref = _gauss(clean, 2, 128, SIG, None, 9, 4, 8)
    _gauss_check(ref.np(), clean, SIG, 9, 4, 8, 128)
    for si, so in ((1, 1), (1, 0), (0, 1)):
        _, out = _gauss(clean, 2, 128, SIG, None, 9, 4, 8, si, so)
        assert np.array_equal(out.bits(), ref.bits()), (si, so)


def test_gauss_noise_rank_slice_equals_stream_slice_bits():
    """assertion 2: a run over [0, n) restricted to [b, n) equals a run with elem_base = b on the
    slice.  b = 8: k_noise4 against k_noise4 (the slice starts 32 bytes in: still aligned).
    b = 6: k_noise4 against k_noise (elem_base % 4 = 2).  No tolerance."""
    n = 4096
    clean = np.random.default_rng(3).random((1, n)).astype(np.float32)
    _, full = _gauss(clean, 1, n, SIG, None, 9, 4, 0)
    for b in (8, 6):
        _, part = _gauss(clean[:, b:], 1, n - b, SIG, None, 9, 4, b)
        assert np.array_equal(part.bits(), full.bits()[b:]), b


# (g): beyond the 65536 x 256 grid cap, the grid-stride loop's second trip.  Scalar: per_image odd,
# 1029 elements in the second trip.  Vector: 4 (16777216 + 257) elements, 257 quads in the second.
@pytest.mark.parametrize("per,tail", [(16777216 + 1029, 1029), (4 * (16777216 + 257), 4 * 257)],
                         ids=["scalar_k_noise", "vector_k_noise4"])
def test_gauss_noise_second_grid_trip_sampled(per, tail):
    c = Buf((1, per))
    c.t.uniform_()
    out = Buf((1, per))
    L().call("dn_add_gauss_noise", c.ptr, 1, per, SIG, None, 9, 4, 0, out.ptr, S())
    torch.cuda.synchronize()
    c.check("clean")
    out.check("noisy")
    rng = np.random.default_rng(4)
    idx = np.unique(np.concatenate([[0, per - tail - 1], rng.integers(0, per - tail, 4096 - tail - 2),
                                    np.arange(per - tail, per)])).astype(np.int64)
    it = torch.from_numpy(idx).to(DEV)
    _gauss_check(out.t.view(-1)[it].cpu().numpy(), c.t.view(-1)[it].cpu().numpy(), SIG, 9, 4, 0,
                 per, idx=idx)


# =============================================================================================
# Poisson noise: one kernel (k_poisson).  Bit-exact against oracle.philox.poisson_noise: the
# same Philox draw, the same fp64 inversion, an integer count divided in fp32.
# =============================================================================================
def _poisson(clean, N, per, lam, lam_img, seed, off, base):
    c = Buf((N, per), init=clean)
    out = Buf((N, per))
    li = None if lam_img is None else Buf((N,), init=np.asarray(lam_img, np.float32))
    L().call("dn_add_poisson_noise", c.ptr, N, per, float(lam), None if li is None else li.ptr,
             seed, off, base, out.ptr, S())
    torch.cuda.synchronize()
    c.check("clean")
    out.check("noisy")
    return out


def _poisson_clean(N, per):
    clean = np.random.default_rng(5).random((N, per)).astype(np.float32)
    clean[:, 0], clean[:, 1], clean[:, 2] = 0.0, -0.25, 1.0  # mu = 0, mu < 0 -> 0, mu = lam
    return clean


@pytest.mark.parametrize("lam", [500.0, 5.0])
@pytest.mark.parametrize("base", [1, 7, 2 ** 33 + 1])
def test_poisson_noise_bases_and_cap_bitexact(base, lam):
    """odd bases (the 53-bit draw is words (2p, 2p + 1), p = q & 1, of block q >> 1), a base whose
    block index needs the high counter word, mu at the 500 cap (clean = 1, lam = 500), clean <= 0"""
    clean = _poisson_clean(2, 60)
    out = _poisson(clean, 2, 60, lam, None, 21, 3, base).np()
    ref = philox.poisson_noise(clean, lam, seed=21, offset=3, elem_base=base)
    assert same_bits(out, ref)
    assert (out[:, :2] == 0).all()


def test_poisson_noise_per_image_lam_nan_branch():
    """per-image lam [30, 0, 600, 50]: the host cannot check device values, so images 1 and 2 come
    out NaN; images 0 and 3 are bit-exact at their own stream positions"""
    clean = _poisson_clean(4, 60)
    out = _poisson(clean, 4, 60, 30.0, [30.0, 0.0, 600.0, 50.0], 21, 3, 7).np()
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all()
    for i, lam in ((0, 30.0), (3, 50.0)):
        ref = philox.poisson_noise(clean[i], lam, seed=21, offset=3, elem_base=7 + 60 * i)
        assert same_bits(out[i], ref), i


@pytest.mark.parametrize("lam", [0.0, 600.0])
def test_poisson_noise_scalar_lam_out_of_range_raises(lam):
    c = Buf((2, 60), init=_poisson_clean(2, 60))
    out = Buf((2, 60))
    with pytest.raises(L().DenoiseHipError, match=ERR_ARG + r": lam must be in \(0, 500\]"):
        L().call("dn_add_poisson_noise", c.ptr, 2, 60, lam, None, 21, 3, 0, out.ptr, S())
    torch.cuda.synchronize()
    assert out.untouched()


# =============================================================================================
# Sub-sampler, masks, sub-image from mask.  Bit-exact: these kernels only move values.
# k_subsample4 when w % 4 == 0, cell_base % 4 == 0 and img, sub1, sub2, rd_in, rd_out are all
# 16-byte aligned (launch_subsample); the scalar k_subsample otherwise.  k_masks and
# k_subimage_from_mask have one path each.
# =============================================================================================
def _subsample(img, rd, seed=0, off=0, base=0, shifts=()):
    """dn_n2n_subsample through _lib.call (misaligned rd_in / sub / rd_out views cannot be made
    through n2n.n2n_subsample).  `shifts`: names among img, rd_in, sub1, sub2, rd_out to move one
    element off alignment.  rd None: Philox draws, rd_out returned.  -> (sub1, sub2, rd) numpy"""
    N, C, H, W = img.shape
    cells = N * (H // 2) * (W // 2)
    sh = lambda k: 1 if k in shifts else 0  # noqa: E731
    bi = Buf(img.shape, shift=sh("img"), init=img)
    s1 = Buf((N, C, H // 2, W // 2), shift=sh("sub1"))
    s2 = Buf((N, C, H // 2, W // 2), shift=sh("sub2"))
    rin = None if rd is None else Buf((cells,), torch.uint8, shift=sh("rd_in"), init=rd)
    rout = Buf((cells,), torch.uint8, shift=sh("rd_out")) if rd is None else None
    L().call("dn_n2n_subsample", bi.ptr, N, C, H, W, None if rin is None else rin.ptr, seed, off,
             base, s1.ptr, s2.ptr, None if rout is None else rout.ptr, S())
    torch.cuda.synchronize()
    for b, what in ((bi, "img"), (s1, "sub1"), (s2, "sub2"), (rin, "rd_in"), (rout, "rd_out")):
        if b is not None:
            b.check(what)
    return s1.np(), s2.np(), (rin if rout is None else rout).np()


def _masks(rd):
    """dn_n2n_masks into guarded uint8 buffers -> (m1, m2) bool numpy"""
    r = Buf((rd.size,), torch.uint8, init=rd)
    m1, m2 = Buf((4 * rd.size,), torch.uint8), Buf((4 * rd.size,), torch.uint8)
    L().call("dn_n2n_masks", r.ptr, rd.size, m1.ptr, m2.ptr, S())
    torch.cuda.synchronize()
    m1.check("mask1")
    m2.check("mask2")
    a, b = m1.np(), m2.np()
    assert set(np.unique(a)) <= {0, 1} and set(np.unique(b)) <= {0, 1}
    return a.astype(bool), b.astype(bool)


def _sub_from_mask(img, mask):
    N, C, H, W = img.shape
    bi = Buf(img.shape, init=img)
    m = Buf((mask.size,), torch.uint8, init=mask.astype(np.uint8))
    sub = Buf((N, C, H // 2, W // 2))
    L().call("dn_n2n_subimage_from_mask", bi.ptr, N, C, H, W, m.ptr, sub.ptr, S())
    torch.cuda.synchronize()
    sub.check("sub")
    return sub.np()


def _img(shape, seed):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


def _check_sampler_family(img, s1, s2, rd):
    """sub-images against the closed form, masks against train.py's table, and the drop-in
    generate_subimages(img, mask) against the literal restatement: all bit-exact"""
    c1, c2 = n2n_ref.subimages_closed_form(img, rd)
    assert same_bits(s1, c1) and same_bits(s2, c2)
    m1, m2 = _masks(rd)
    o1, o2 = n2n_ref.masks_from_rd(rd)
    assert np.array_equal(m1, o1) and np.array_equal(m2, o2)
    assert same_bits(_sub_from_mask(img, m1), n2n_ref.generate_subimages(img, o1))
    assert same_bits(_sub_from_mask(img, m2), n2n_ref.generate_subimages(img, o2))
    assert same_bits(_sub_from_mask(img, m1), s1) and same_bits(_sub_from_mask(img, m2), s2)


@pytest.mark.parametrize("rd0", range(8))
def test_subsample_one_cell_image(rd0):
    """1x1x2x2: one cell, w = 1 -> k_subsample; each of the eight pair-table rows"""
    img = _img((1, 1, 2, 2), 6)
    rd = np.array([rd0], np.uint8)
    s1, s2, _ = _subsample(img, rd)
    _check_sampler_family(img, s1, s2, rd)


def test_subsample_one_cell_image_philox():
    img = _img((1, 1, 2, 2), 6)
    s1, s2, rd = _subsample(img, None, seed=11, off=5, base=2 ** 34 + 5)
    assert np.array_equal(rd, philox.rd_idx(11, 5, 1, cell_base=2 ** 34 + 5))
    _check_sampler_family(img, s1, s2, rd)


def test_subsample_vector_path_given_rd():
    """2x3x2x8: w = 4, everything aligned -> k_subsample4 (uchar4 read of rd_in), three channels"""
    img = _img((2, 3, 2, 8), 7)
    rd = np.arange(8, dtype=np.uint8)[::-1].copy()
    s1, s2, _ = _subsample(img, rd)
    _check_sampler_family(img, s1, s2, rd)


@pytest.mark.parametrize("shape,base,kernel", [
    ((1, 3, 6, 12), 2 ** 34 + 4, "k_subsample"),    # w = 6: w % 4 != 0
    ((2, 3, 2, 8), 2 ** 34 + 4, "k_subsample4"),    # w = 4, cell_base % 4 == 0, aligned
    ((2, 3, 2, 8), 2 ** 34 + 5, "k_subsample"),     # cell_base % 4 != 0
])
def test_subsample_philox_draws_high_counter_word(shape, base, kernel):
    """Philox draws at a cell_base past 2^34 (block index past 2^32: the counter's high word) on
    both kernels; the rd values emitted equal oracle.philox.rd_idx"""
    img = _img(shape, 8)
    cells = shape[0] * (shape[2] // 2) * (shape[3] // 2)
    s1, s2, rd = _subsample(img, None, seed=11, off=5, base=base)
    assert np.array_equal(rd, philox.rd_idx(11, 5, cells, cell_base=base)), kernel
    _check_sampler_family(img, s1, s2, rd)


@pytest.mark.parametrize("philox_draws", [False, True])
def test_subsample_misaligned_views_equal_aligned(philox_draws):
    """2x1x8x16 (w = 8, cell_base = 0): aligned is k_subsample4; with any one of img, rd_in /
    rd_out, sub1, sub2 one element off alignment it is k_subsample.  Equal bits either way."""
    img = _img((2, 1, 8, 16), 9)
    rd = None if philox_draws else (np.random.default_rng(10).integers(0, 8, 64)).astype(np.uint8)
    a1, a2, ard = _subsample(img, rd, seed=11, off=5)
    if philox_draws:
        assert np.array_equal(ard, philox.rd_idx(11, 5, 64))
    _check_sampler_family(img, a1, a2, ard)
    for name in ("img", "rd_out" if philox_draws else "rd_in", "sub1", "sub2"):
        s1, s2, r = _subsample(img, rd, seed=11, off=5, shifts=(name,))
        assert same_bits(s1, a1) and same_bits(s2, a2) and np.array_equal(r, ard), name


@pytest.mark.parametrize("kind", ["random_one_hot", "slot3_everywhere"])
def test_subimage_from_arbitrary_one_hot_mask(kind):
    """generate_subimages with a mask that no pair-table row produced, 2x3x6x10"""
    img = _img((2, 3, 6, 10), 12)
    cells = 2 * 3 * 5
    slot = np.random.default_rng(13).integers(0, 4, cells) if kind == "random_one_hot" \
        else np.full(cells, 3)
    mask = np.zeros((cells, 4), bool)
    mask[np.arange(cells), slot] = True
    assert same_bits(_sub_from_mask(img, mask.reshape(-1)),
                     n2n_ref.generate_subimages(img, mask.reshape(-1)))


# =============================================================================================
# N2N loss: k_n2n_loss (1024 blocks x 256 threads, grid-stride) + k_n2n_finalize.  fp64 reference
# from the fp32 inputs; bounds derived in tests/step_ops_ref.py, twice the first-order bound.
# =============================================================================================
def _partials():
    return Buf((int(L().lib().dn_loss_partials_size()),), torch.uint8)


@pytest.mark.parametrize("lam", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 3, 300, 300)],
                         ids=["1x1x1x1", "2x3x5x7", "1x3x300x300"])
def test_n2n_loss_vs_fp64_with_derived_bounds(shape, lam):
    """1x1x1x1: one thread has work, 1023 blocks store zero partials.  2x3x5x7: the n, c, i, j
    decomposition and the den plane stride at C = 3, odd sizes.  1x3x300x300: 270000 > 262144
    elements, the loop's second trip with every partial live.  rd covers all eight values."""
    N, C, h, w = shape
    rng = np.random.default_rng(14)
    out = rng.standard_normal(shape).astype(np.float32)
    sub2 = rng.standard_normal(shape).astype(np.float32)   # diff = out - sub2 is O(1)
    den = rng.standard_normal((N, C, 2 * h, 2 * w)).astype(np.float32)
    rd = rng.permutation(np.arange(N * h * w) % 8).astype(np.uint8)
    if rd.size == 1:
        rd[0] = 6
    bo, bs, bd = Buf(shape, init=out), Buf(shape, init=sub2), Buf(den.shape, init=den)
    br = Buf((rd.size,), torch.uint8, init=rd)
    dout, loss3, part = Buf(shape), Buf((3,)), _partials()
    L().call("dn_n2n_loss", bo.ptr, bs.ptr, bd.ptr, br.ptr, N, C, h, w, lam, dout.ptr, loss3.ptr,
             part.ptr, S())
    torch.cuda.synchronize()
    for b, what in ((bo, "out"), (bs, "sub2"), (bd, "den"), (br, "rd"), (dout, "dout"),
                    (loss3, "loss3"), (part, "partials")):
        b.check(what)
    r = R.n2n_loss_ref(out, sub2, den, rd, lam)
    got = loss3.np().astype(np.float64)
    for i, k in enumerate(("loss1", "loss2", "loss")):
        err = abs(got[i] - r[k])
        print(f"{k}: {got[i]!r} ref {r[k]!r} err {err:.3e} bound {r['b_' + k]:.3e}")
        assert err <= r["b_" + k], k
    err = np.abs(dout.np().astype(np.float64) - r["dout"])
    print("dout worst err/bound", float((err / r["b_dout"]).max()))
    assert (err <= r["b_dout"]).all()
    if lam == 0.0:
        assert got[1] == 0.0 and got[2] == got[0]


# =============================================================================================
# Structure loss: k_structure_loss + k_structure_finalize, same grid.
# =============================================================================================
def _structure(pred, pred2, tgt, alpha=1.0, beta=0.5, gamma=0.5):
    N, C, H, W = pred.shape
    bp, bp2, bt = Buf(pred.shape, init=pred), Buf(pred.shape, init=pred2), Buf(pred.shape, init=tgt)
    dp, dp2, loss5, part = Buf(pred.shape), Buf(pred.shape), Buf((5,)), _partials()
    L().call("dn_structure_loss", bp.ptr, bp2.ptr, bt.ptr, N, C, H, W, alpha, beta, gamma, dp.ptr,
             dp2.ptr, loss5.ptr, part.ptr, S())
    torch.cuda.synchronize()
    for b, what in ((bp, "pred"), (bp2, "pred2"), (bt, "target"), (dp, "dpred"), (dp2, "dpred2"),
                    (loss5, "loss5"), (part, "partials")):
        b.check(what)
    return dp, dp2, loss5


@pytest.mark.parametrize("shape,quantised", [
    ((1, 1, 2, 2), True),       # the smallest legal image: every element is on two borders
    ((2, 3, 5, 7), True),       # C = 3, odd sizes
    ((2, 3, 5, 7), False),      # no ties
    ((1, 1, 520, 512), True),   # 266240 > 262144 elements: the loop's second trip
], ids=["1x1x2x2", "2x3x5x7", "2x3x5x7_unquantised", "1x1x520x512"])
def test_structure_loss_vs_fp64(shape, quantised):
    """inputs quantised to multiples of 1/8 tie often (pred == target, equal TV neighbours), where
    sgnf must give 0 as torch.sign does.  dpred: bit-exact.  dpred2: 5 u sum |term|.  The four
    means: 2 u relative; the total: the same combination of those bounds (step_ops_ref.py)."""
    rng = np.random.default_rng(15)
    if quantised:
        draw = lambda: (rng.integers(-4, 5, shape) / 8.0).astype(np.float32)  # noqa: E731
    else:
        draw = lambda: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    pred, pred2, tgt = draw(), draw(), draw()
    if quantised and pred.size > 4:
        assert (pred == tgt).any() and (pred2[..., 1:] == pred2[..., :-1]).any()
    if shape == (1, 1, 2, 2):
        pred[0, 0, 0, 0] = tgt[0, 0, 0, 0]       # a tie in d0
        pred2[0, 0, 0, 1] = pred2[0, 0, 0, 0]    # a tie between horizontal neighbours
    dp, dp2, loss5 = _structure(pred, pred2, tgt)
    r = R.structure_loss_ref(pred, pred2, tgt)
    assert same_bits(dp.np(), r["dpred"])
    err = np.abs(dp2.np().astype(np.float64) - r["dpred2"])
    assert (err <= r["b_dpred2"]).all(), float(err.max())
    got = loss5.np().astype(np.float64)
    for i, k in enumerate(("pixel", "tv1", "tv2", "consistency", "total")):
        e = abs(got[i] - r["parts"][i])
        print(f"{k}: {got[i]!r} ref {r['parts'][i]!r} err {e:.3e} bound {r['b_parts'][i]:.3e}")
        assert e <= r["b_parts"][i], k


@pytest.mark.parametrize("H,W", [(1, 8), (8, 1)])
def test_structure_loss_rejects_one_row_or_column(H, W):
    z = np.zeros((1, 1, H, W), np.float32)
    bp, bp2, bt = Buf(z.shape, init=z), Buf(z.shape, init=z), Buf(z.shape, init=z)
    dp, dp2, loss5, part = Buf(z.shape), Buf(z.shape), Buf((5,)), _partials()
    with pytest.raises(L().DenoiseHipError, match=ERR_ARG + ": Structure_loss needs H, W >= 2"):
        L().call("dn_structure_loss", bp.ptr, bp2.ptr, bt.ptr, 1, 1, H, W, 1.0, 0.5, 0.5, dp.ptr,
                 dp2.ptr, loss5.ptr, part.ptr, S())
    torch.cuda.synchronize()
    assert dp.untouched() and dp2.untouched() and loss5.untouched()


# =============================================================================================
# Adam: k_adam through FlatAdam (the wrapper takes the caller's buffers, so they can be guarded).
# One kernel; grid capped at 8192 x 256.  Reference: torch.optim.Adam on the CPU fed
# g * float32(scale) formed in fp32.  Bounds are test_adam_matches_torch_adam's own: atol 1e-7 on
# the parameters, at most 5 % of elements off in the last bit; the same atol scaled by
# max |state| / max |p| on exp_avg and exp_avg_sq (the parameters' 1e-7 is 1e-7 / max |p| of their
# range; the states get the same fraction of theirs).  The state check is what found that
# dn_adam_step formed 1 - beta2 from (double)0.999f: exp_avg_sq was 1.3e-5 (relative) off torch's in
# every element while the parameters stayed inside 1e-7.
# =============================================================================================
def _adam_compare(n, scale, steps, step0=0, seed=16):
    from image_denoising_amd.optim import FlatAdam

    g0 = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g0) * 0.05
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=3e-4)
    bp, bm, bv = Buf((n,), init=p0), Buf((n,)), Buf((n,))
    fa = FlatAdam(bp.t, lr=3e-4)
    fa.exp_avg, fa.exp_avg_sq = bm.t.zero_(), bv.t.zero_()
    if step0:  # a late step: both bias corrections are ~ 1, the state is not zero
        m0 = torch.randn(n, generator=g0) * 0.01
        v0 = torch.rand(n, generator=g0) * 1e-4
        opt.state[pt] = dict(step=torch.tensor(float(step0)), exp_avg=m0.clone(),
                             exp_avg_sq=v0.clone())
        fa.exp_avg.copy_(m0)
        fa.exp_avg_sq.copy_(v0)
        fa.step_count = step0
    s32 = torch.tensor(scale, dtype=torch.float32)
    for _ in range(steps):
        g = torch.randn(n, generator=g0) * torch.logspace(-9, 0, n)   # 1e-9 .. 1, as the old test
        pt.grad = g.clone() if scale == 1.0 else g * s32
        opt.step()
        bg = Buf((n,), init=g)
        fa.step(bg.t, grad_scale=scale)
        torch.cuda.synchronize()
        bg.check("grad")
        assert torch.equal(bg.t.cpu(), g), "the gradient buffer was written"
    for b, what in ((bp, "param"), (bm, "exp_avg"), (bv, "exp_avg_sq")):
        b.check(what)
    st = opt.state[pt]
    p_ref = pt.detach()
    pmax = float(p_ref.abs().max())
    for got, ref, what in ((bp.t.cpu(), p_ref, "param"), (bm.t.cpu(), st["exp_avg"], "exp_avg"),
                           (bv.t.cpu(), st["exp_avg_sq"], "exp_avg_sq")):
        atol = 1e-7 if what == "param" else 1e-7 * float(ref.abs().max()) / pmax
        err = float((got - ref).abs().max())
        frac = float((got != ref).float().mean())
        print(f"{what}: max err {err:.3e} atol {atol:.3e}, {100 * frac:.2f} % differ")
        assert err <= atol, what
        if what == "param":
            assert frac < 0.05


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["scale1", "scale_half", "scale_third"])
@pytest.mark.parametrize("n", [1, 255, 257, 2097152 + 257])
def test_adam_grad_scale_and_sizes_vs_torch(n, scale):
    """grad_scale != 1 is every data-parallel and finetune step; n = 2097152 + 257 is past the
    8192 x 256 grid (second trip of the loop); n = 1, 255, 257: one thread, a partly filled block,
    one element into a second block"""
    _adam_compare(n, scale, steps=3)


def test_adam_late_step_vs_torch():
    """step_count = 100000 before stepping: bias corrections ~ 1, non-zero state"""
    _adam_compare(4099, 0.5, steps=2, step0=100000)


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_adam_zero_gradient_zero_state_keeps_params_bits(scale):
    from image_denoising_amd.optim import FlatAdam

    p0 = torch.randn(257, generator=torch.Generator().manual_seed(17)) * 0.05
    bp, bm, bv, bg = Buf((257,), init=p0), Buf((257,)), Buf((257,)), Buf((257,))
    fa = FlatAdam(bp.t, lr=3e-4)
    fa.exp_avg, fa.exp_avg_sq = bm.t.zero_(), bv.t.zero_()
    bg.t.zero_()
    fa.step(bg.t, grad_scale=scale)
    torch.cuda.synchronize()
    assert same_bits(bp.np(), p0.numpy())
    assert not bm.np().any() and not bv.np().any()
    for b in (bp, bm, bv, bg):
        b.check()


# =============================================================================================
# Accumulate (dst += src), through _lib.call: no Python wrapper exists.  k_accumulate (float4 body
# + scalar tail in the same kernel) when dst and src are both 16-byte aligned, k_accumulate_tail
# (scalar over everything) otherwise (launch_accumulate); grid capped at 4096 x 256.
# =============================================================================================
@pytest.mark.parametrize("shifts", [(0, 0), (1, 0), (0, 1), (1, 1)],
                         ids=["aligned_k_accumulate", "dst+1_tail", "src+1_tail", "both+1_tail"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 4096 * 256 + 5])
def test_accumulate_bitexact(n, shifts):
    """n < 4: only the tail loop has work.  4, 5, 1023: float4 body with 0, 1, 3 tail elements.
    4 * 4096 * 256 + 5: one float4 past the vector grid (second trip) plus the tail; on the
    scalar route four trips.  fp32 a + b has one correct rounding: bit-exact against numpy."""
    rng = np.random.default_rng(18)
    d0 = rng.standard_normal(n).astype(np.float32)
    s0 = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    dst, src = Buf((n,), shift=shifts[0], init=d0), Buf((n,), shift=shifts[1], init=s0)
    L().call("dn_accumulate", dst.ptr, src.ptr, n, S())
    torch.cuda.synchronize()
    dst.check("dst")
    src.check("src")
    assert same_bits(src.np(), s0)
    assert same_bits(dst.np(), d0 + s0)


def test_accumulate_empty_and_negative():
    d0 = np.arange(8, dtype=np.float32)
    dst, src = Buf((8,), init=d0), Buf((8,), init=d0)
    L().call("dn_accumulate", dst.ptr, src.ptr, 0, S())
    with pytest.raises(L().DenoiseHipError, match=ERR_ARG + ": n < 0"):
        L().call("dn_accumulate", dst.ptr, src.ptr, -1, S())
    torch.cuda.synchronize()
    assert same_bits(dst.np(), d0)
    dst.check()


# =============================================================================================
# Max-pool 2x2 (NHWC, float4 over channels): k_pool_fwd / k_pool_bwd, one path each.  Bit-exact
# against F.max_pool2d and its autograd on the CPU (ATen's max_pool2d_with_indices: NaN
# propagates, the first maximum in TL, TR, BL, BR order wins, a later NaN replaces an earlier one).
# =============================================================================================
def _nhwc(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


@pytest.mark.parametrize("N,C,H,W,stride,off", [(1, 4, 2, 2, 4, 0), (2, 8, 6, 10, 24, 8)],
                         ids=["1x4x2x2_compact", "2x8x6x10_into_ch8_16_of_24"])
def test_maxpool_edge_values_and_concat_slice(N, C, H, W, stride, off):
    """1x4x2x2: one thread, one window per channel, NaN in each of the four slots.  2x8x6x10: NaN
    in each slot, two and four NaNs, -inf windows, all-equal windows, exact zeros (act = 1 takes
    the 0.2 slope at 0), written into channels [8, 16) of a 24-channel buffer whose other channels
    hold the sentinel, which must survive."""
    x = R.pool_edge_input(N, C, H, W, seed=19)
    xr = torch.from_numpy(x).requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(20))
    y.backward(dy)
    grad = xr.grad
    H2, W2 = H // 2, W // 2
    bx = Buf((N, H, W, C), init=_nhwc(x))
    by = Buf((N, H2, W2, stride))
    L().call("dn_maxpool2x2_forward", bx.ptr, N, H, W, C, by.ptr, stride, off, S())
    torch.cuda.synchronize()
    bx.check("x")
    by.check("y")
    got = by.np()
    others = np.delete(got, np.s_[off:off + C], axis=3)
    assert (others.reshape(-1).view(np.int32) == SENT32).all(), "channels outside the slice written"
    gy, ry = got[..., off:off + C], _nhwc(y.detach().numpy())
    assert np.array_equal(np.isnan(gy), np.isnan(ry))
    assert np.isnan(ry).any()
    fin = ~np.isnan(ry)
    assert same_bits(gy[fin], ry[fin])
    # backward: dy read from the same slice; the other channels hold NaN, which a wrong offset
    # or stride would route into dx
    dyb = np.full((N, H2, W2, stride), np.nan, np.float32)
    dyb[..., off:off + C] = _nhwc(dy.numpy())
    bdy = Buf(dyb.shape, init=dyb)
    for act in (0, 1):
        dx = Buf((N, H, W, C))
        L().call("dn_maxpool2x2_backward", bx.ptr, N, H, W, C, bdy.ptr, stride, off, act, dx.ptr,
                 S())
        torch.cuda.synchronize()
        dx.check("dx")
        bdy.check("dy")
        # act = 1: LeakyReLU' through the saved activation, test_maxpool_forward_backward's rule
        ref = grad if not act else torch.where(xr.detach() > 0, grad, grad * 0.2)
        assert same_bits(dx.np(), _nhwc(ref.numpy())), f"act={act}"


# =============================================================================================
# Batched L1 (eval.hip k_l1_batched): one block per item, per-thread fp64 sums of
# |double(a) - double(b)|, a fixed fp64 tree, one fp64 division; the output is fp64.  Any order of
# n fp64 additions is within (n - 1) 2^-53 of the exact sum of non-negative terms; the difference,
# the division and the reference's own rounding add one 2^-53 each: (n + 3) 2^-53 relative, far
# inside the 2 u (u = 2^-24) an fp64 accumulation was asked to meet.
# =============================================================================================
@pytest.mark.parametrize("P,n", [(3, 1), (3, 255), (3, 1027), (1, 262144 + 3)])
def test_l1_mean_batched_vs_fp64(P, n):
    """n = 1: 255 idle threads; 255 and 1027: not a multiple of 4 or 256, so items 1 and 2 start
    off 16-byte alignment; 262144 + 3: 1024 full trips of the 256-thread loop and a ragged one"""
    rng = np.random.default_rng(21)
    a, b = rng.random((P, n)).astype(np.float32), rng.random((P, n)).astype(np.float32)
    ba, bb, out = Buf((P, n), init=a), Buf((P, n), init=b), Buf((P,), torch.float64)
    L().call("dn_l1_mean_batched", ba.ptr, bb.ptr, P, n, out.ptr, S())
    torch.cuda.synchronize()
    for buf, what in ((ba, "a"), (bb, "b"), (out, "l1")):
        buf.check(what)
    ref = R.l1_batched_ref(a, b)
    err = np.abs(out.np() - ref)
    print("l1 rel err", (err / ref).max(), "bound", (n + 3) * 2.0 ** -53)
    assert (err <= (n + 3) * 2.0 ** -53 * ref).all()
    assert (err <= 2 * R.U * ref).all()
