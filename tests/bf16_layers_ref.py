"""fp64 restatement of every kind of layer of the forward-only bf16 plan (dn_unet_forward_bf16).

Shared by tests/test_gpu_bf16_layers.py (each layer of the device pass against these, computed
from the device's own input to that layer) and tests/test_bf16_layers_ref_cpu.py (these against
oracle.unet_ref and against planted faults).  torch only, NCHW fp64 in and out.

What the plan rounds (unet.cpp fwd_routes, the kernels named per function below):
  * every 3x3 layer after enc_conv0, the deconvs and nin_a / nin_b multiply bf16-rounded
    activations by bf16-rounded weights; the products are exact in fp32, the sums, the bias and
    LeakyReLU(0.2) are fp32;
  * enc_conv0 and nin_c are fp32 arithmetic on unrounded operands;
  * a0, d{1..5}a and d1b are STORED as bf16 (round to nearest even); their only readers round
    to bf16 anyway, so the storage changes no later value.
The bounds of check() come from the number formats alone; nothing is fitted to a kernel's output.
"""
from __future__ import annotations

from collections import namedtuple
from functools import partial

import torch
import torch.nn.functional as F

from oracle.unet_ref import layer_table

REL_ACC = 1e-5  # fp32 accumulation order, relative to max |ref| (test_conv_bf16_vs_fp64_of_rounded_operands)


def rb(t: torch.Tensor) -> torch.Tensor:
    """round to nearest even to bf16, back in fp64"""
    return t.float().bfloat16().double()


def _leaky(t):
    return F.leaky_relu(t, 0.2)


def params(flat: torch.Tensor, in_nc: int, out_nc: int, nf: int = 48):
    """{layer name: (weight, bias)} as fp64 views of the flat parameters (state_dict order)"""
    flat = flat.detach().cpu().double()
    out, off = {}, 0
    for name, ws, bl, _ in layer_table(in_nc, out_nc, nf):
        n = 1
        for d in ws:
            n *= d
        out[name] = (flat[off:off + n].view(ws), flat[off + n:off + n + bl])
        off += n + bl
    assert off == flat.numel(), (off, flat.numel())
    return out


# ---------------------------------------------------------------------------------------------
# the layers
# ---------------------------------------------------------------------------------------------
def enc0(x, w, b):
    """enc_conv0 (k_enc0_fwd, first_layer.hip): fp32 FMAs on the unrounded input and weights;
    only its store is bf16, which check(stored_bf16=True) accounts for"""
    return _leaky(F.conv2d(x, w, b, padding=1))


def conv3(xin, w, b):
    """a 3x3 layer on the bf16 matrix cores (k_fwd_bf16 / k_fwd_bf16p, conv_bf16.hip): the staged
    input tile and the packed weights rounded to bf16, fp32 bias and LeakyReLU"""
    return _leaky(F.conv2d(rb(xin), rb(w), b, padding=1))


def conv3_pool(xin, w, b):
    """conv3 with the 2x2 max-pool of the activated output (conv_epi.h fwd_epilogue_vec_at)"""
    return F.max_pool2d(conv3(xin, w, b), 2)


def deconv(xin, w, b):
    """ConvTranspose2d(2, 2) in plain bf16 products, no activation: k_deconv_x6<true> (the 96-channel
    deconvs: input rounded in registers, the image's leading plane = the weight rounded to bf16) and
    k_fwd_bf16<3, ., false> with OUT_UP2 (upsample5, 48 channels: one 1x1 bf16 image per parity)"""
    return F.conv_transpose2d(rb(xin), rb(w), b, stride=2)


def head(d1b, wa, ba, wb, bb, wc, bc, acc32: bool = False, round_na: bool = True):
    """nin_a -> nin_b -> nin_c as k_nin_head_x6<false, false, B1 = true, IBF = true> computes them
    (head_x6.hip):
      * the input is taken as stored: bf16 bits loaded by load() under IBF (l. 70-73) and used as the
        MFMA operand without conversion (gemm96, INB branch, l. 107-110) -- rb() of a value that is
        already bf16 changes nothing;
      * nin_a and nin_b multiply by the images' leading planes (l. 116-119 read plane 0 only), which
        pk_head_x6 fills with split3()'s h = (__bf16)w (x6_core.h l. 25-26): the weights rounded to
        bf16, round to nearest even;
      * na IS rounded to bf16 before nin_b: tile() passes h = bias_act(nin_a) to
        gemm96(std::false_type, ...) (l. 154), whose B1 branch converts each value with
        (__bf16)v8[j] (l. 112-113);
      * bias and LeakyReLU are fp32 (bias_act, l. 85-89);
      * nin_c is fp32 FMAs on the unrounded nb and the unrounded wc (l. 175-188).
    acc32: the two 96x96 products accumulated in fp32 (torch .float() matmuls) instead of fp64, the
    measure of how far two legitimate accumulation orders may disagree (head_bound).
    round_na = False plants the fault of a head that skips the rounding of na."""
    N, K, H, W = d1b.shape
    x = rb(d1b).permute(0, 2, 3, 1).reshape(-1, K)

    def mm(t, w):
        w = rb(w).reshape(w.shape[0], -1)
        if acc32:
            return (t.float() @ w.float().t()).double()
        return t @ w.t()

    na = _leaky(mm(x, wa) + ba)
    nb = _leaky(mm(rb(na) if round_na else na, wb) + bb)
    y = nb @ wc.reshape(wc.shape[0], -1).t() + bc
    return y.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def bind(layer, *prm, **kw):
    """a layer with its parameters bound: a function of the input alone (what windowed() takes)"""
    assert len(prm) == len(_ARGS[layer]), (layer.__name__, len(prm))
    return partial(layer, **dict(zip(_ARGS[layer], prm)), **kw)


_ARGS = {enc0: ("w", "b"), conv3: ("w", "b"), conv3_pool: ("w", "b"), deconv: ("w", "b"),
         head: ("wa", "ba", "wb", "bb", "wc", "bc")}
# (input pixels of halo per side, output pixels computed per side and dropped, output / input
# scale as num, den).  conv + pool takes a halo of 2 input pixels, not the minimal 1, so that the
# patch starts on a pool window; the extra pooled ring is dropped.
_GEOM = {enc0: (1, 1, 1, 1), conv3: (1, 1, 1, 1), conv3_pool: (2, 1, 1, 2), deconv: (0, 0, 2, 1),
         head: (0, 0, 1, 1)}


def _patch(x, ya, yb, xa, xb):
    """x[:, :, ya:yb, xa:xb] as CPU fp64, zeros where the rectangle leaves the image (the layers'
    own zero padding).  x may live on any device in any float type: only the rectangle is read."""
    H, W = x.shape[-2:]
    y0, y1, x0, x1 = max(ya, 0), min(yb, H), max(xa, 0), min(xb, W)
    core = x[:, :, y0:y1, x0:x1].cpu().double()
    return F.pad(core, (x0 - xa, xb - x1, y0 - ya, yb - y1))


def windowed(fn, xin, y0, y1, x0, x1):
    """fn(xin)[:, :, y0:y1, x0:x1] from the input window plus its halo only.  fn is a bind()
    of one of the layers above; xin the layer's whole NCHW input (any device / float type)."""
    halo, drop, num, den = _GEOM[fn.func]
    if num == 2:  # the deconv: output pixel 2y + a comes from input pixel y alone
        ya, yb, xa, xb = y0 // 2, (y1 + 1) // 2, x0 // 2, (x1 + 1) // 2
        out = fn(_patch(xin, ya, yb, xa, xb))
        return out[:, :, y0 - 2 * ya:y1 - 2 * ya, x0 - 2 * xa:x1 - 2 * xa]
    out = fn(_patch(xin, den * y0 - halo, den * y1 + halo, den * x0 - halo, den * x1 + halo))
    return out[:, :, drop:out.shape[2] - drop, drop:out.shape[3] - drop]


def chain(flat, x, in_nc, out_nc, nf: int = 48):
    """the layers above in the network's order (unet.cpp run_forward), fp64 throughout: y and
    the intermediate tensors by workspace name.  Without the bf16 stores: their readers round."""
    P = params(flat, in_nc, out_nc, nf)
    t = {"x": x.double()}
    t["a0"] = enc0(t["x"], *P["enc_conv0"])
    t["p1"] = conv3_pool(t["a0"], *P["enc_conv1"])
    for l in range(2, 6):
        t[f"p{l}"] = conv3_pool(t[f"p{l - 1}"], *P[f"enc_conv{l}"])
    t["a6"] = conv3(t["p5"], *P["enc_conv6"])
    h = t["a6"]
    for l in range(5, 0, -1):  # c_l = [up_l | skip]; the skip of level 1 is the network input
        skip = t[f"p{l - 1}"] if l > 1 else t["x"]
        t[f"c{l}"] = torch.cat([deconv(h, *P[f"up{l}.deconv"]), skip], 1)
        t[f"d{l}a"] = conv3(t[f"c{l}"], *P[f"dec_conv{l}a"])
        h = t[f"d{l}b"] = conv3(t[f"d{l}a"], *P[f"dec_conv{l}b"])
    t["y"] = head(h, *P["nin_a"], *P["nin_b"], *P["nin_c"])
    return t["y"], t


# ---------------------------------------------------------------------------------------------
# the workspace
# ---------------------------------------------------------------------------------------------
def read_buffer(ws, desc_entry, N, H, W, bf16, c0=0, c1=None):
    """The NHWC view [N, H >> level, W >> level, c0:c1] of one activation buffer of a workspace
    (a byte tensor), without copying: the caller slices what it needs and moves that to the CPU.
    desc_entry = (offset in floats, pixel stride in channels, level) as dn_unet_debug_buffers
    reports it.  bf16: the buffer holds bf16 -- element pix * stride + c of the __bf16 array that
    starts at the same byte offset (conv_epi.h fwd_epilogue_vec_at's out_bf16 store), i.e. the first
    half of the float buffer with the same stride counted in elements."""
    off, stride, level = (int(v) for v in desc_entry)
    h, w = H >> level, W >> level
    n = N * h * w * stride
    if bf16:
        flat = ws[4 * off:4 * off + 2 * n].view(torch.bfloat16)
    else:
        flat = ws[4 * off:4 * off + 4 * n].view(torch.float32)
    return flat.view(N, h, w, stride)[..., c0:stride if c1 is None else c1]


def nchw(t):
    """an NHWC view (read_buffer) as NCHW; still a view"""
    return t.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 |v|) - 7); below the smallest normal 2^-126, that one's ulp"""
    _, e = torch.frexp(v.double().abs())  # |v| = m 2^e, m in [0.5, 1); frexp(0) = (0, 0)
    e = torch.where(v == 0, torch.full_like(e, -126), torch.clamp(e - 1, min=-126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 7)


Check = namedtuple("Check", "ok worst index err bound")
Check.__doc__ = """ok: every element finite and within its bound; worst: the largest error / bound;
index: where; err, bound: that element's |dev - ref| and bound"""


def check(dev, ref, stored_bf16, rel=REL_ACC):
    """Every element of dev against ref (same shape):
      |dev - ref| <= rel * max|ref|                        for an fp32-stored output,
      |dev - ref| <= 0.5 ulp_bf16(ref) + rel * max|ref|    for a bf16-stored one
    (round-to-nearest-even's own error on top of the accumulation order's).  A non-finite device
    value fails.  No element is exempt."""
    dev, ref = dev.detach().cpu().double(), ref.detach().cpu().double()
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    bound = torch.full_like(ref, rel * float(ref.abs().max()))
    if stored_bf16:
        bound = bound + 0.5 * ulp_bf16(ref)
    err = (dev - ref).abs()
    err = torch.where(torch.isfinite(dev), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    i = int(torch.argmax(ratio))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return Check(bool((err <= bound).all()), float(ratio.flatten()[i]), idx,
                 float(err.flatten()[i]), float(bound.flatten()[i]))


def head_bound(d1b, prm):
    """(fp64 head, rel): the bound the device's head is held to.  The head rounds na to bf16
    inside, so a value at a rounding boundary may legitimately land on either side depending on the
    accumulation order.  floor = the largest difference between the head with fp64 and with fp32
    accumulation of the two 96x96 products, relative to max|ref|; the device (a third order) may
    differ from the fp64 head by 4 x floor and never by more than 1e-3."""
    ref = head(d1b, *prm)
    floor = float((head(d1b, *prm, acc32=True) - ref).abs().max() / ref.abs().max())
    return ref, min(4.0 * floor, 1e-3), floor
