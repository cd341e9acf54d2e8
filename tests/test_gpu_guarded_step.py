"""The guarded optimizer step on the GPU (csrc/guard.hip): k_grad_sumsq (float4 and
its scalar twin), k_guard_decide and k_adam_guarded through dn_grad_norm / dn_adam_step_guarded,
FlatAdam(guard=...) and the trainers.  Needs an MI355X.

Every buffer a kernel is handed, the guard state included, is a guard-banded `Buf` of
test_gpu_step_ops.py: the bands must be intact after every call and the gradient buffer unchanged
bit for bit.  References: tests/guard_ref.py (clip_grad_norm_ + torch.optim.Adam behind the
reference's tests) and torch.optim.Adam itself.

Bounds.  Norm: squares of floats are exact in fp64, so the error is summation only, at most
n * 2^-53 relative (2.3e-10 at the largest n here); 1e-9 is asserted.  Parameters and Adam state:
test_gpu_step_ops._adam_compare's own (atol 1e-7 on the parameters, fewer than 5 % of the elements
different at all, the same atol scaled by max |state| / max |p| on exp_avg and exp_avg_sq).
Skipped steps: bit equality.

One pass of k_grad_sumsq's full grid covers kLossBlocks * 256 threads * 4 elements = 1048576
(guard.hip guard_norm_blocks), one block 1024."""
import math

import numpy as np
import pytest
import torch

import guard_ref
from test_gpu_step_ops import Buf, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
PASS = 1024 * 256 * 4      # elements one pass of the norm kernel's full grid covers
BIG = 2097152 + 257        # past k_adam's 8192 x 256 grid; the norm loop's third trip
LR = 3e-4


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


def _state_buf(step=0):
    st = Buf((int(L().lib().dn_guard_state_size()),), torch.uint8)
    L().call("dn_guard_state_init", st.ptr, step, S())
    return st


def _read(st):
    out = L().DnGuardStats()
    L().call("dn_guard_state_read", st.ptr, out, S())
    return {k: getattr(out, k) for k, _ in out._fields_}


def _grad(n, seed, norm=None):
    """randn * logspace(-9, 0, n), as the Adam tests use; rescaled to `norm` when given"""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * torch.logspace(-9, 0, n)
    if norm is not None:
        g = (g.double() * (norm / guard_ref.norm64(g))).float()
    return g


# =============================================================================================
# 1. the norm
# =============================================================================================
@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0], ids=["scale1", "scale_third"])
@pytest.mark.parametrize("shift", [0, 1], ids=["float4", "scalar_twin"])
@pytest.mark.parametrize("n", [1, 255, 257, PASS + 1, BIG])
def test_grad_norm_vs_fp64_and_same_bits(n, shift, scale):
    """n = 1: one thread; 255 / 257: a ragged last quad; PASS + 1: one element into the loop's
    second trip; BIG: every partial live, three trips.  shift = 1 moves the view 4 bytes off
    16-byte alignment: launch_grad_sumsq takes k_grad_sumsq<false>."""
    g = _grad(n, 30)
    bg, st, out = Buf((n,), shift=shift, init=g), _state_buf(), Buf((1,), torch.float64)
    got = []
    for _ in range(2):
        out.t.fill_(-1.0)
        L().call("dn_grad_norm", bg.ptr, n, scale, st.ptr, out.ptr, S())
        torch.cuda.synchronize()
        for b, what in ((bg, "grad"), (st, "state"), (out, "norm_out")):
            b.check(what)
        assert same_bits(bg.np(), g.numpy()), "the gradient buffer was written"
        got.append(out.np().copy())
        assert _read(st)["last_norm"] == float(got[-1][0])
    assert got[0].view(np.int64)[0] == got[1].view(np.int64)[0], "two runs differ"
    ref = guard_ref.norm64(g, scale)
    rel = abs(float(got[0][0]) - ref) / ref
    print(f"norm {float(got[0][0])!r} ref {ref!r} rel err {rel:.3e} (n 2^-53 = {n * 2.0 ** -53:.3e})")
    assert rel <= 1e-9
    # without norm_out the state alone receives it
    L().call("dn_grad_norm", bg.ptr, n, scale, st.ptr, None, S())
    assert _read(st)["last_norm"] == float(got[0][0])
    st.check("state")


def test_grad_norm_scalar_twin_equals_float4_bits():
    """both kernels give thread t the same quads and add a quad's terms in index order"""
    n = PASS + 1027
    g = _grad(n, 31)
    bits = []
    for shift in (0, 1):
        bg, st, out = Buf((n,), shift=shift, init=g), _state_buf(), Buf((1,), torch.float64)
        L().call("dn_grad_norm", bg.ptr, n, 1.0 / 3.0, st.ptr, out.ptr, S())
        torch.cuda.synchronize()
        bits.append(int(out.np().view(np.int64)[0]))
    assert bits[0] == bits[1]


def test_guard_entry_points_validate():
    st, bg = _state_buf(), Buf((8,), init=np.ones(8, np.float32))
    err = L().DenoiseHipError
    with pytest.raises(err, match=r"status -1\)"):
        L().call("dn_grad_norm", bg.ptr, -1, 1.0, st.ptr, None, S())
    with pytest.raises(err, match=r"status -1\)"):
        L().call("dn_grad_norm", None, 8, 1.0, st.ptr, None, S())
    with pytest.raises(err, match=r"status -1\)"):
        L().call("dn_adam_step_guarded", bg.ptr, bg.ptr, bg.ptr, bg.ptr, 8, LR, .9, .999, 1e-8,
                 1.0, None, 5.0, 200.0, 1.0, None, S())
    with pytest.raises(err, match=r"status -1\)"):
        L().call("dn_adam_step_guarded", bg.ptr, None, bg.ptr, bg.ptr, 8, LR, .9, .999, 1e-8,
                 1.0, None, 5.0, 200.0, 1.0, st.ptr, S())
    L().call("dn_adam_step_guarded", None, None, None, None, 0, LR, .9, .999, 1e-8, 1.0, None,
             5.0, 200.0, 1.0, st.ptr, S())        # n == 0: DN_OK, no launch
    s = _read(st)
    assert (s["step"], s["applied"], s["skipped_loss"], s["skipped_norm"]) == (0, 0, 0, 0)
    assert same_bits(bg.np(), np.ones(8, np.float32))
    st.check("state")


# =============================================================================================
# the guarded optimizer on guard-banded buffers
# =============================================================================================
class Opt:
    """FlatAdam(guard=...) whose parameters, state tensors and guard state are all `Buf`s"""

    def __init__(self, n, guard, seed=16, warm=False):
        from image_denoising_amd.optim import FlatAdam

        g0 = torch.Generator().manual_seed(seed)
        self.n = n
        self.p0 = torch.randn(n, generator=g0) * 0.05
        self.m0, self.v0 = torch.zeros(n), torch.zeros(n)
        if warm:  # a non-zero Adam state, so that a skipped step has something to preserve
            self.m0 = torch.randn(n, generator=g0) * 0.01
            self.v0 = torch.rand(n, generator=g0) * 1e-4
        self.bp, self.bm, self.bv = Buf((n,), init=self.p0), Buf((n,), init=self.m0), \
            Buf((n,), init=self.v0)
        self.fa = FlatAdam(self.bp.t, lr=LR, guard=guard)
        self.fa.exp_avg, self.fa.exp_avg_sq = self.bm.t, self.bv.t
        self.st = _state_buf()
        self.fa._guard_state = self.st.t
        self.lossbuf = Buf((1,))

    def step(self, g, scale=1.0, loss=None, shift=0):
        bg = Buf((self.n,), shift=shift, init=g)
        lt = None
        if loss is not None:
            self.lossbuf.t.fill_(loss)
            lt = self.lossbuf.t
        self.fa.step(bg.t, grad_scale=scale, loss=lt)
        torch.cuda.synchronize()
        for b, what in ((bg, "grad"), (self.bp, "param"), (self.bm, "exp_avg"),
                        (self.bv, "exp_avg_sq"), (self.st, "state"), (self.lossbuf, "loss")):
            b.check(what)
        assert same_bits(bg.np(), g.numpy()), "the gradient buffer was written"
        return self.fa.guard_stats()

    def bits(self):
        return self.bp.bits().copy(), self.bm.bits().copy(), self.bv.bits().copy()

    def unchanged_since(self, before):
        return all(np.array_equal(a, b) for a, b in zip(self.bits(), before))


def _assert_adam_close(got, ref):
    """got / ref: (param, exp_avg, exp_avg_sq) CPU tensors; _adam_compare's bounds"""
    pmax = float(ref[0].abs().max())
    for g, r, what in zip(got, ref, ("param", "exp_avg", "exp_avg_sq")):
        g, r = g.reshape(-1), r.detach().reshape(-1)
        atol = 1e-7 if what == "param" else 1e-7 * float(r.abs().max()) / pmax
        err = float((g - r).abs().max())
        frac = float((g != r).float().mean())
        print(f"{what}: max err {err:.3e} atol {atol:.3e}, {100 * frac:.2f} % differ")
        assert err <= atol, what
        if what == "param":
            assert frac < 0.05


def _torch_adam(p0):
    pt = torch.nn.Parameter(p0.clone())
    return pt, torch.optim.Adam([pt], lr=LR)


def _state_of(opt, pt):
    return pt.detach(), opt.state[pt]["exp_avg"], opt.state[pt]["exp_avg_sq"]


def _got(o):
    return o.bp.t.cpu(), o.bm.t.cpu(), o.bv.t.cpu()


# 2. apply, no clip -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4099, BIG])
def test_apply_below_the_clip_equals_torch_adam(n):
    """norm 0.5 < grad_clip: coef == 1, three steps of plain torch.optim.Adam"""
    from image_denoising_amd.optim import GradGuard

    o = Opt(n, GradGuard())
    pt, opt = _torch_adam(o.p0)
    for k in range(3):
        g = _grad(n, 40 + k, norm=0.5)
        pt.grad = g.clone()
        opt.step()
        s = o.step(g, loss=0.3)
        assert s["apply"] == 1 and s["last_coef"] == 1.0 and s["gscale"] == 1.0
        assert (s["step"], s["applied"]) == (k + 1, k + 1)
        assert abs(s["last_norm"] - 0.5) <= 1e-6 and s["last_loss"] == np.float32(0.3)
    assert s["skipped_loss"] == 0 and s["skipped_norm"] == 0
    _assert_adam_close(_got(o), _state_of(opt, pt))


# 3. clip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5], ids=["scale1", "scale_half"])
def test_clip_equals_guard_ref(scale):
    """the scaled gradient has norm ~7.3 > grad_clip = 1: clipped inside the Adam pass, the
    gradient buffer untouched.  scale 0.5: the raw norm is ~14.6, the clip acts on the scaled one."""
    from image_denoising_amd.optim import GradGuard

    n = 4099
    o = Opt(n, GradGuard())
    ref = guard_ref.GuardRef(o.p0, GradGuard(), lr=LR)
    for k in range(3):
        g = _grad(n, 50 + k, norm=7.3 / scale)
        assert ref.step(g, scale, 0.3) == "applied"
        s = o.step(g, scale=scale, loss=0.3)
        n64 = guard_ref.norm64(g, scale)
        assert abs(n64 - 7.3) < 1e-5 and abs(s["last_norm"] - n64) <= 1e-9 * n64
        want = np.float32(guard_ref.clip_coef(n64, 1.0))
        assert abs(np.float32(s["last_coef"]) - want) <= np.spacing(want), (s["last_coef"], want)
        assert abs(s["gscale"] - float(want) * scale) <= 2 * np.spacing(np.float32(want * scale))
        assert s["apply"] == 1 and s["applied"] == k + 1
    _assert_adam_close(_got(o), (ref.params, ref.exp_avg, ref.exp_avg_sq))


# 4. skip on norm -------------------------------------------------------------------------------
def test_skip_on_norm_then_step_one_of_torch_adam():
    """norm 201 > 10 * max_grad_norm = 200: nothing moves.  The next ordinary step is torch's step
    1 (bc1 = 0.1): the step count lives on the device and the skipped batch did not advance it."""
    from image_denoising_amd.optim import GradGuard

    n = 4099
    o = Opt(n, GradGuard(max_grad_norm=20.0))
    before = o.bits()
    s = o.step(_grad(n, 60, norm=201.0), loss=0.3)
    assert o.unchanged_since(before)
    assert (s["apply"], s["applied"], s["skipped_norm"], s["skipped_loss"], s["step"]) == \
        (0, 0, 1, 0, 0)
    assert abs(s["last_norm"] - 201.0) < 1e-3
    g = _grad(n, 61, norm=0.5)
    pt, opt = _torch_adam(o.p0)
    pt.grad = g.clone()
    opt.step()
    s = o.step(g, loss=0.3)
    assert (s["apply"], s["applied"], s["skipped_norm"], s["step"]) == (1, 1, 1, 1)
    assert abs(s["step_size"] - LR / 0.1) <= 1e-6 * LR / 0.1
    _assert_adam_close(_got(o), _state_of(opt, pt))
    # the device step count goes through state_dict / load_state_dict
    sd = o.fa.state_dict()
    assert sd["step"] == 1
    o.fa.load_state_dict(dict(sd, step=7))
    s = o.fa.guard_stats()
    assert (s["step"], s["applied"], s["skipped_norm"]) == (7, 0, 0)
    o.st.check("state")


# 5. skip on non-finite -------------------------------------------------------------------------
@pytest.mark.parametrize("n,shift", [(257, 0), (257, 1), (1025, 0), (PASS + 1, 1), (BIG, 0),
                                     (BIG, 1)])
def test_nonfinite_gradient_skips_bit_for_bit(n, shift):
    """one NaN, then one +inf, in the last element: 257 is k_adam's second block, 1025 the norm
    kernel's second block, PASS + 1 its loop's second trip, BIG past both grids; shift = 1 is the
    scalar twin.  Parameters and a non-zero Adam state keep their bits."""
    from image_denoising_amd.optim import GradGuard

    o = Opt(n, GradGuard(), warm=True)
    before = o.bits()
    for k, bad in enumerate((float("nan"), float("inf"))):
        g = _grad(n, 70, norm=0.5)
        g[-1] = bad
        s = o.step(g, loss=0.3, shift=shift)
        assert o.unchanged_since(before), bad
        assert (s["apply"], s["applied"], s["skipped_norm"], s["skipped_loss"], s["step"]) == \
            (0, 0, k + 1, 0, 0)
        assert not math.isfinite(s["last_norm"])


def test_loss_guard_and_counters():
    """a finite gradient with loss NaN, +inf and the float just above 5 skips on the loss; exactly
    5.0 applies (the comparison is strict, train_opt.py:136); the counters name each cause, and
    the loss test comes first"""
    from image_denoising_amd.optim import GradGuard

    n = 1025
    o = Opt(n, GradGuard(), warm=True)
    g = _grad(n, 80, norm=0.5)
    before = o.bits()
    above5 = float(np.nextafter(np.float32(5.0), np.float32(np.inf)))
    for k, loss in enumerate((float("nan"), float("inf"), above5)):
        s = o.step(g, loss=loss)
        assert o.unchanged_since(before), loss
        assert (s["apply"], s["applied"], s["skipped_loss"], s["skipped_norm"]) == (0, 0, k + 1, 0)
    s = o.step(g, loss=5.0)
    assert (s["apply"], s["applied"], s["skipped_loss"], s["skipped_norm"]) == (1, 1, 3, 0)
    assert not o.unchanged_since(before)
    before = o.bits()
    bad = g.clone()
    bad[3] = float("nan")
    s = o.step(bad, loss=0.3)
    assert (s["applied"], s["skipped_loss"], s["skipped_norm"]) == (1, 3, 1)
    s = o.step(bad, loss=float("nan"))     # both bad: attributed to the loss
    assert (s["applied"], s["skipped_loss"], s["skipped_norm"], s["step"]) == (1, 4, 1, 1)
    assert o.unchanged_since(before)


# 6. disabled guards ----------------------------------------------------------------------------
def test_each_guard_off_on_its_own():
    from image_denoising_amd.optim import GradGuard

    n = 4099
    # loss guard off: a NaN behind the loss pointer is ignored
    o = Opt(n, GradGuard(max_loss_skip=None))
    g = _grad(n, 90, norm=0.5)
    pt, opt = _torch_adam(o.p0)
    pt.grad = g.clone()
    opt.step()
    s = o.step(g, loss=float("nan"))
    assert (s["apply"], s["applied"], s["skipped_loss"]) == (1, 1, 0)
    _assert_adam_close(_got(o), _state_of(opt, pt))
    # clip off: norm 7.3 is applied unclipped
    o = Opt(n, GradGuard(grad_clip=None))
    g = _grad(n, 91, norm=7.3)
    pt, opt = _torch_adam(o.p0)
    pt.grad = g.clone()
    opt.step()
    s = o.step(g, loss=0.3)
    assert s["apply"] == 1 and s["last_coef"] == 1.0 and s["gscale"] == 1.0
    _assert_adam_close(_got(o), _state_of(opt, pt))
    # loss guard on, no loss pointer: applies
    o = Opt(n, GradGuard())
    s = o.step(_grad(n, 92, norm=0.5), loss=None)
    assert (s["apply"], s["applied"], s["skipped_loss"]) == (1, 1, 0)
    # norm skip off: norm 201 is clipped and applied, as guard_ref does
    gd = GradGuard(max_grad_norm=None)
    o = Opt(n, gd)
    ref = guard_ref.GuardRef(o.p0, gd, lr=LR)
    g = _grad(n, 93, norm=201.0)
    assert ref.step(g, 1.0, 0.3) == "applied"
    s = o.step(g, loss=0.3)
    assert (s["apply"], s["skipped_norm"]) == (1, 0)
    want = np.float32(guard_ref.clip_coef(guard_ref.norm64(g), 1.0))
    assert abs(np.float32(s["last_coef"]) - want) <= np.spacing(want)
    _assert_adam_close(_got(o), (ref.params, ref.exp_avg, ref.exp_avg_sq))
    # ... but a non-finite norm still skips while the clip is on
    before = o.bits()
    g[0] = float("nan")
    s = o.step(g, loss=0.3)
    assert (s["apply"], s["skipped_norm"]) == (0, 1) and o.unchanged_since(before)


def test_unguarded_flat_adam_is_unchanged():
    """guard=None: no guard state, the loss argument is refused, step_count counts on the host"""
    from image_denoising_amd.optim import FlatAdam

    bp = Buf((257,), init=np.zeros(257, np.float32))
    fa = FlatAdam(bp.t)
    fa.step(torch.ones(257, device=DEV))
    assert fa.step_count == 1 and fa._guard_state is None
    with pytest.raises(ValueError):
        fa.step(torch.ones(257, device=DEV), loss=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):
        fa.guard_stats()


# =============================================================================================
# 7. the trainers, at the smallest network shapes
# =============================================================================================
def _unet():
    from image_denoising_amd import UNet

    torch.manual_seed(0)
    return UNet(1, 1, 48).to(DEV)


def _pairs(H, W, steps=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        clean = torch.rand(2, 1, H, W, generator=g)
        out.append((clean.to(DEV), (clean + 0.1 * torch.randn(2, 1, H, W, generator=g)).to(DEV)))
    return out


def _flat(net):
    return net.flat_params.detach().cpu().clone()


def test_supervised_trainer_skips_the_nan_batch():
    """three steps, the middle one with clean[0, 0, 0, 0] = nan: one NaN in the target makes the
    loss non-finite (no separate test of prediction and target is needed), the update is withheld,
    and the run equals an unguarded trainer that only saw steps 1 and 3"""
    from image_denoising_amd.optim import GradGuard
    from image_denoising_amd.trainer import SupervisedTrainer

    data = _pairs(32, 32)
    tr = SupervisedTrainer(_unet(), "l1", guard=GradGuard(grad_clip=None))
    for k, (clean, noisy) in enumerate(data):
        if k == 1:
            clean = clean.clone()
            clean[0, 0, 0, 0] = float("nan")
        loss3 = tr.train_step(clean, noisy)
        assert bool(torch.isfinite(loss3[2])) == (k != 1)
    s = tr.guard_stats()
    print("supervised guard stats", s)
    assert (s["applied"], s["skipped_loss"], s["skipped_norm"], s["step"]) == (2, 1, 0, 2)
    plain = SupervisedTrainer(_unet(), "l1")
    for k in (0, 2):
        plain.train_step(*data[k])
    torch.cuda.synchronize()
    _assert_adam_close((_flat(tr.net), tr.opt.exp_avg.cpu(), tr.opt.exp_avg_sq.cpu()),
                       (_flat(plain.net), plain.opt.exp_avg.cpu(), plain.opt.exp_avg_sq.cpu()))
    assert torch.isfinite(tr.net.flat_params).all()


def test_n2n_trainer_skips_the_inf_batch():
    """N2NTrainer (sub-images of 32 x 32 need 64 x 64 patches) handed a `noisy` with one inf in
    the middle step; the pair choices and the noisy images are given, so the unguarded run of
    steps 1 and 3 sees the same batches"""
    from image_denoising_amd.optim import GradGuard
    from image_denoising_amd.trainer import N2NTrainer
    from oracle import philox

    data = _pairs(64, 64)
    rds = [torch.from_numpy(philox.rd_idx(1, k, 2 * 32 * 32)).to(DEV) for k in range(3)]
    tr = N2NTrainer(_unet(), guard=GradGuard(grad_clip=None))
    for k, (clean, noisy) in enumerate(data):
        if k == 1:
            noisy = noisy.clone()
            noisy[1, 0, 17, 40] = float("inf")
        loss3 = tr.train_step(clean, epoch=1, rd_idx=rds[k], noisy=noisy)
        assert bool(torch.isfinite(loss3[2])) == (k != 1)
    s = tr.guard_stats()
    print("n2n guard stats", s)
    assert (s["applied"], s["skipped_loss"], s["skipped_norm"], s["step"]) == (2, 1, 0, 2)
    plain = N2NTrainer(_unet())
    for k in (0, 2):
        plain.train_step(data[k][0], epoch=1, rd_idx=rds[k], noisy=data[k][1])
    torch.cuda.synchronize()
    _assert_adam_close((_flat(tr.net), tr.opt.exp_avg.cpu(), tr.opt.exp_avg_sq.cpu()),
                       (_flat(plain.net), plain.opt.exp_avg.cpu(), plain.opt.exp_avg_sq.cpu()))
    assert torch.isfinite(tr.net.flat_params).all()


def test_supervised_trainer_default_guard_equals_guard_ref_on_its_own_gradient():
    """GradGuard() and clean data: one step's parameters are guard_ref's, fed the trainer's own
    flat gradient buffer and loss"""
    from image_denoising_amd.optim import GradGuard
    from image_denoising_amd.trainer import SupervisedTrainer

    clean, noisy = _pairs(32, 32, steps=1)[0]
    tr = SupervisedTrainer(_unet(), "l1", guard=GradGuard())
    p0 = _flat(tr.net)
    loss3 = tr.train_step(clean, noisy)
    s = tr.guard_stats()
    ref = guard_ref.GuardRef(p0, GradGuard(), lr=tr.opt.lr)
    taken = ref.step(tr.grad.cpu(), 1.0, float(loss3[2]))
    print("default guard: stats", s, "reference", taken, ref.stats)
    assert taken == "applied" and (s["apply"], s["applied"]) == (1, 1)
    assert abs(s["last_norm"] - ref.stats["last_norm"]) <= 1e-9 * ref.stats["last_norm"]
    _assert_adam_close((_flat(tr.net), tr.opt.exp_avg.cpu(), tr.opt.exp_avg_sq.cpu()),
                       (ref.params, ref.exp_avg, ref.exp_avg_sq))
