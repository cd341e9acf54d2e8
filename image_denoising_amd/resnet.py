"""Drop-in `RESNET` for arch_unet.py:263-409, computed by libdenoise_hip.so on gfx950.

The reference's full-resolution residual network: the UNet's layers without pooling or
upsampling (any H, W), skip concatenations of the encoder activations, and the network input
added to nin_c's output.  Same constructor, same `state_dict` keys / shapes (21 layers;
`up5.deconv` is constructed and initialised but never used, so its gradient is zero), all
parameters views of ONE flat fp32 buffer, forward / backward through dn_resnet_forward_prec /
dn_resnet_backward_prec.

Deviation: the residual needs out_nc == in_nc (torch would broadcast a one-channel side).
The blind-spot variant raises.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib
from .arch_unet import _Holder, _kaiming01

# state_dict order of arch_unet.py:279-346
LAYER_NAMES = [
    "enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5", "enc_conv6",
    "up5.deconv", "dec_conv5a", "dec_conv5b", "dec_conv4a", "dec_conv4b", "dec_conv3a",
    "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "nin_a", "nin_b", "nin_c",
]


def layer_shapes(in_nc: int, out_nc: int, nf: int):
    """[(name, weight_shape, bias_len, is_deconv)] in state_dict order"""
    C, OC = in_nc, out_nc
    s = []
    conv = lambda name, co, ci, k: s.append((name, (co, ci, k, k), co, False))
    conv("enc_conv0", nf, C, 3)
    for i in range(1, 7):
        conv(f"enc_conv{i}", nf, nf, 3)
    s.append(("up5.deconv", (nf, nf, 2, 2), nf, True))
    conv("dec_conv5a", 2 * nf, 2 * nf, 3)
    conv("dec_conv5b", 2 * nf, 2 * nf, 3)
    for lvl in (4, 3, 2):
        conv(f"dec_conv{lvl}a", 2 * nf, 3 * nf, 3)
        conv(f"dec_conv{lvl}b", 2 * nf, 2 * nf, 3)
    conv("dec_conv1a", 96, 2 * nf + C, 3)
    conv("dec_conv1b", 96, 96, 3)
    conv("nin_a", 96, 96, 1)
    conv("nin_b", 96, 96, 1)
    conv("nin_c", OC, 96, 1)
    return s


def param_count(in_nc: int, out_nc: int, nf: int) -> int:
    return sum(int(torch.Size(w).numel()) + b for _, w, b, _ in layer_shapes(in_nc, out_nc, nf))


def reference_init(in_nc: int, out_nc: int, nf: int = 48, zero_last: bool = False) -> torch.Tensor:
    """Flat CPU fp32 parameters drawn exactly like the reference RESNET.__init__: every module's
    construction (its reset_parameters) and re-initialisation consume the global CPU RNG in the
    order of arch_unet.py:279-346 -- enc_conv0 and enc_conv1 are both constructed before either is
    re-initialised, likewise each dec_conv{k}a/b pair and nin_a/b; nin_c keeps torch's default
    init under zero_last."""
    C, OC = in_nc, out_nc
    mods = {}

    def conv(name, ci, co, k):
        mods[name] = nn.Conv2d(ci, co, k, 1, (k - 1) // 2)

    def pair(a, cia, b, cib, co, k=3):
        conv(a, cia, co, k)
        conv(b, cib, co, k)
        _kaiming01(mods[a])
        _kaiming01(mods[b])

    with torch.no_grad():
        pair("enc_conv0", C, "enc_conv1", nf, nf)
        for i in range(2, 7):
            conv(f"enc_conv{i}", nf, nf, 3)
            _kaiming01(mods[f"enc_conv{i}"])
        mods["up5.deconv"] = nn.ConvTranspose2d(nf, nf, 2, 2, 0, 0)  # UpsampleCat.__init__
        _kaiming01(mods["up5.deconv"])
        pair("dec_conv5a", 2 * nf, "dec_conv5b", 2 * nf, 2 * nf)
        for lvl in (4, 3, 2):
            pair(f"dec_conv{lvl}a", 3 * nf, f"dec_conv{lvl}b", 2 * nf, 2 * nf)
        conv("dec_conv1a", 2 * nf + C, 96, 3)
        _kaiming01(mods["dec_conv1a"])
        conv("dec_conv1b", 96, 96, 3)
        _kaiming01(mods["dec_conv1b"])
        pair("nin_a", 96, "nin_b", 96, 96, 1)
        conv("nin_c", 96, OC, 1)
        if not zero_last:
            _kaiming01(mods["nin_c"])
        parts = []
        for name in LAYER_NAMES:
            parts += [mods[name].weight.reshape(-1), mods[name].bias.reshape(-1)]
        return torch.cat(parts).float().contiguous()


class _ResnetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net, *params):
        N, C, H, W = x.shape
        y = torch.empty((N, net.out_nc, H, W), dtype=torch.float32, device=x.device)
        ws = net._workspace(N, H, W, with_backward=True, fresh=True)
        net._run_forward(x, y, ws)
        ctx.net, ctx.ws, ctx.shape = net, ws, (N, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        net = ctx.net
        N, H, W = ctx.shape
        dy = dy.contiguous()
        dflat = torch.empty_like(net._flat)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((N, net.in_nc, H, W), dtype=torch.float32, device=dy.device)
        net._run_backward(dy, dflat, ctx.ws, N, H, W, dx=dx)
        ctx.ws = None
        grads = [dflat[o:o + p.numel()].view_as(p) if need else None
                 for (o, p), need in zip(net._param_views(), ctx.needs_input_grad[2:])]
        return (dx, None, *grads)


class RESNET(nn.Module):
    """arch_unet.py:263 RESNET(in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False)."""

    def __init__(self, in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False):
        super().__init__()
        if blindspot:
            raise NotImplementedError("blind-spot RESNET (arch_unet.py:65-97) is out of scope")
        if out_nc != in_nc:
            raise ValueError("the HIP RESNET adds its input to its output: out_nc must equal in_nc "
                             "(torch would broadcast a one-channel side)")
        if n_feature != 48:
            raise ValueError("n_feature must be 48 (kernel tiles are instantiated for the "
                             "reference width)")
        self.in_nc, self.out_nc, self.n_feature = in_nc, out_nc, n_feature
        self.blindspot, self.zero_last = blindspot, zero_last
        self._cfg = _lib.cfg(in_nc, out_nc, n_feature)
        n = ctypes.c_size_t()
        _lib.check(_lib.lib().dn_resnet_param_count(ctypes.byref(self._cfg), ctypes.byref(n)),
                   "dn_resnet_param_count")
        flat = reference_init(in_nc, out_nc, n_feature, zero_last)
        assert flat.numel() == n.value, (flat.numel(), n.value)
        self._flat = flat
        self._layout = []  # (holder, attr, offset, shape)
        off = 0
        for name, wshape, blen, _ in layer_shapes(in_nc, out_nc, n_feature):
            holder = self
            for p in name.split("."):
                if not hasattr(holder, p) or not isinstance(getattr(holder, p), nn.Module):
                    setattr(holder, p, _Holder())
                holder = getattr(holder, p)
            wn = int(torch.Size(wshape).numel())
            holder.weight = nn.Parameter(flat[off:off + wn].view(wshape))
            self._layout.append((holder, "weight", off, wshape))
            off += wn
            holder.bias = nn.Parameter(flat[off:off + blen])
            self._layout.append((holder, "bias", off, (blen,)))
            off += blen
        self._ws_cache = {}

    @property
    def flat_params(self) -> torch.Tensor:
        """the flat fp32 parameter buffer every parameter is a view of"""
        return self._flat

    def _param_views(self):
        return [(off, getattr(h, a)) for (h, a, off, _) in self._layout]

    def param_range(self, name: str):
        """(begin, end) of layer `name`'s weight and bias in the flat buffer"""
        off = 0
        for n, wshape, blen, _ in layer_shapes(self.in_nc, self.out_nc, self.n_feature):
            cnt = int(torch.Size(wshape).numel()) + blen
            if n == name:
                return off, off + cnt
            off += cnt
        raise KeyError(name)

    def _apply(self, fn, recurse=True):  # keep the parameters views of ONE flat buffer
        new = fn(self._flat)
        if not isinstance(new, torch.Tensor) or new.dtype != torch.float32:
            raise ValueError("RESNET parameters are fp32 (the HIP path computes in fp32)")
        self._flat = new.contiguous()
        for (h, a, off, shape) in self._layout:
            p = getattr(h, a)
            p.data = self._flat[off:off + int(torch.Size(shape).numel())].view(shape)
            p.grad = None
        self._ws_cache = {}
        return self

    def _workspace(self, N, H, W, with_backward, fresh=False):
        key = (N, H, W, bool(with_backward), self._flat.device)
        if not fresh and key in self._ws_cache:
            return self._ws_cache[key]
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().dn_resnet_workspace_size(ctypes.byref(self._cfg), N, H, W,
                                                       int(with_backward), ctypes.byref(nbytes)),
                   "dn_resnet_workspace_size")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self._flat.device)
        if not fresh:
            self._ws_cache = {key: ws}
        return ws

    # arithmetic of the 3x3 convolutions (include/denoise_hip.h DN_PREC_*; bf16 is not built)
    _PRECISIONS = {"fp32": 0, "fp32_x6": 2}

    def set_precision(self, mode: str) -> "RESNET":
        """'fp32' (fp32 matrix cores) or 'fp32_x6' (exact three-piece bf16 split, six products,
        fp32 accumulation)"""
        if mode not in self._PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self._PRECISIONS)}")
        self.precision = mode
        return self

    def _prec(self) -> int:
        return self._PRECISIONS[getattr(self, "precision", "fp32")]

    def _run_forward(self, x, y, ws):
        N, _, H, W = x.shape
        _lib.call("dn_resnet_forward_prec", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(x), _lib.ptr(y), N, H, W, ws.data_ptr(), ws.numel(), self._prec(),
                  _lib.stream_of(x))

    def _run_forward_n2n(self, x, den, ws, rd_idx):
        """the N2N no-grad pass (N2NTrainer): the whole image, a superset of the rd pair pixels
        the loss reads (the pair-pixel fast path is built for the UNet)"""
        self._run_forward(x, den, ws)

    def _run_backward(self, dy, dflat, ws, N, H, W, dx=None):
        """dflat = dL/dparams (zeros over up5.deconv), and dx = dL/dx when given"""
        _lib.call("dn_resnet_backward_prec", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(dy), _lib.ptr(dflat), _lib.ptr(dx), N, H, W, ws.data_ptr(), ws.numel(),
                  self._prec(), _lib.stream_of(dy))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        if x.device.type != "cuda":
            raise RuntimeError("the HIP RESNET runs on a GPU: move the module and input to cuda")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != self.in_nc:
            raise ValueError(f"expected float32 [N,{self.in_nc},H,W], got {x.dtype} {tuple(x.shape)}")
        if self._flat.device != x.device:
            raise RuntimeError("module parameters and input are on different devices")
        N, _, H, W = x.shape
        if torch.is_grad_enabled() and (x.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            return _ResnetFunction.apply(x, self, *[p for _, p in self._param_views()])
        y = torch.empty((N, self.out_nc, H, W), dtype=torch.float32, device=x.device)
        self._run_forward(x, y, self._workspace(N, H, W, with_backward=False))
        return y
