"""A derived per-element error bound for the GEMM-style ops of csrc/conv.hip and
csrc/conv_bf16.hip (plain torch fp64 on the CPU; checked by tests/test_gemm_bound_cpu.py, used by
tests/test_gpu_gemm_edges.py).

An output element of such an op is a sum of T = taps x K products plus a bias (or nothing).  The
matrix cores form fp32 x fp32 (and bf16 x bf16) products exactly and add them in fp32 in some
order, so with u = 2^-24 the computed sum s' of the exact sum s obeys |s' - s| <= (T u + O(T^2
u^2)) * sum |terms|, whatever the order.  The epilogues add at most three more roundings (the
bias add, the 0.2 multiply of the LeakyReLU or of its masked derivative, the add onto the old
output), each relative to a magnitude that the sum of the absolute terms also bounds.  Hence for
every output element

    |got - ref| <= c * (T + 3) * 2^-24 * A

where `ref` is the op in fp64 and A the same op in fp64 on |x|, |w|, |b| (and |base| for the
accumulating epilogue): the sum of the absolute terms.  (T^2 u^2 < 3 u up to T = 7000.)
LeakyReLU is 1-Lipschitz, so the activation leaves the bound of the pre-activation as it is; the
mask epilogue scales A with the derivative it applies.  c = 1 holds if every add rounds to
nearest; c = 2 is the ceiling should the MFMA's inner add truncate instead.  For the bf16 kernels
`ref` and A are taken on the bf16-rounded operands (bf16=True), and a result stored as bf16 adds
half a bf16 ulp of `ref`, taken as its ceiling 2^-8 |ref| (bf16_store=True).  No element is
exempt; nothing is normalised by a maximum.

All activations are NHWC torch tensors; weights keep PyTorch's layouts.  Every function returns
(ref, bound), fp64, shaped like the op's output."""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24   # unit roundoff of fp32
UBF16 = 2.0 ** -8  # half a bf16 ulp of v is at most 2^-8 |v| (8 significand bits)
SLOPE = 0.2


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _rb(t, bf16):
    """the operand as the kernel sees it: rounded to bf16 (nearest even) or as it is"""
    return t.bfloat16().double() if bf16 else t.double()


def _finish(ref, A, T, c, bf16_store=False):
    bound = c * (T + 3) * U32 * A
    if bf16_store:
        bound = bound + UBF16 * ref.abs()
    return ref, bound


def conv_forward(x, w, b, act, c=1, bf16=False, bf16_store=False):
    """Conv2d(k, padding=k//2) + bias (+ LeakyReLU(0.2) if act): x [N,H,W,Cin], w [Cout,Cin,k,k]
    (k = 1 or 3), b [Cout] -> [N,H,W,Cout]; T = k*k*Cin"""
    k = w.shape[2]
    xd, wd, bd = _nchw(_rb(x, bf16)), _rb(w, bf16), b.double()
    ref = F.conv2d(xd, wd, bd, padding=k // 2)
    A = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=k // 2)
    if act:
        ref = F.leaky_relu(ref, SLOPE)
    return _finish(_nhwc(ref), _nhwc(A), k * k * w.shape[1], c, bf16_store)


def conv_dgrad(dz, w, mode="plain", mask=None, base=None, c=1):
    """data gradient of Conv2d(k, padding=k//2): dz [N,H,W,Cout], w [Cout,Cin,k,k] -> dx
    [N,H,W,Cin]; mode "plain", "mask" (dx * (mask > 0 ? 1 : 0.2), mask [N,H,W,Cin]) or "accum"
    (base + dx, base [N,H,W,Cin]); T = k*k*Cout"""
    return conv_dgrad_modes(dz, w, (mode,), mask, base, c)[mode]


def conv_dgrad_modes(dz, w, modes, mask=None, base=None, c=1):
    """conv_dgrad for several epilogues from one evaluation of the gradient: {mode: (ref, bound)}"""
    k = w.shape[2]
    g, wd = _nchw(dz), w.double()
    ref0 = _nhwc(F.conv_transpose2d(g, wd, None, padding=k // 2))
    A0 = _nhwc(F.conv_transpose2d(g.abs(), wd.abs(), None, padding=k // 2))
    out = {}
    for mode in modes:
        assert mode in ("plain", "mask", "accum"), mode
        ref, A = ref0, A0
        if mode == "mask":
            keep = mask.double() > 0
            ref, A = torch.where(keep, ref, ref * SLOPE), torch.where(keep, A, A * SLOPE)
        elif mode == "accum":
            ref, A = ref + base.double(), A + base.double().abs()
        out[mode] = _finish(ref, A, k * k * w.shape[0], c)
    return out


def deconv_forward(x, w, b, c=1):
    """ConvTranspose2d(Cin, Cout, 2, 2) + bias: x [N,H,W,Cin], w [Cin,Cout,2,2], b [Cout] ->
    [N,2H,2W,Cout]; T = Cin"""
    xd, wd, bd = _nchw(x), w.double(), b.double()
    ref = F.conv_transpose2d(xd, wd, bd, stride=2)
    A = F.conv_transpose2d(xd.abs(), wd.abs(), bd.abs(), stride=2)
    return _finish(_nhwc(ref), _nhwc(A), w.shape[0], c)


def deconv_dgrad(dy, w, mask=None, c=1):
    """data gradient of ConvTranspose2d(Cin, Cout, 2, 2): dy [N,2H,2W,Cout], w [Cin,Cout,2,2] ->
    dx [N,H,W,Cin] (optionally * (mask > 0 ? 1 : 0.2)); T = 4*Cout"""
    g, wd = _nchw(dy), w.double()
    ref = _nhwc(F.conv2d(g, wd, None, stride=2))
    A = _nhwc(F.conv2d(g.abs(), wd.abs(), None, stride=2))
    if mask is not None:
        keep = mask.double() > 0
        ref, A = torch.where(keep, ref, ref * SLOPE), torch.where(keep, A, A * SLOPE)
    return _finish(ref, A, 4 * w.shape[1], c)


def worst_ratio(got, ref, bound):
    """max over all elements of |got - ref| / bound (inf for a non-finite result or an error
    over a zero bound; 0 for an exact result where the bound is 0)"""
    got = torch.as_tensor(got).double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (x / 0 = inf)
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within(got, ref, bound, what=""):
    """every element within its bound; the message names the worst element -> the worst ratio"""
    got = torch.as_tensor(got).double()
    r = worst_ratio(got, ref, bound)
    if not r <= 1.0:
        err = (got - ref).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        over = err > bound
        ratio = torch.where(over, err / bound, torch.zeros_like(err))
        at = [int(v) for v in torch.unravel_index(torch.argmax(ratio), ratio.shape)]
        raise AssertionError(
            f"{what}: {int(over.sum())} of {over.numel()} elements outside the bound, worst "
            f"|err| / bound = {r:.3g} at (n, y, x, c) = {tuple(at)}: got {float(got[tuple(at)])!r}, "
            f"ref {float(ref[tuple(at)])!r}, bound {float(bound[tuple(at)]):.3g}")
    return r
