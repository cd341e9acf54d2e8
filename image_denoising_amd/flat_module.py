"""What the networks and adapters share: parameters as views of ONE flat fp32 buffer (the layout
the C-ABI consumes), and for the three networks the common front of libdenoise_hip.so's
dn_<family>_* entry points.

`FlatParamModule` is the only place that knows how parameters live in the flat buffer: binding,
`flat_params`, re-pointing after `.to()` / `.cuda()`, and slicing a flat gradient for autograd.
`HipNet` adds what UNet, RESNET and ImprovedUNet have in common: workspace, precision, the
forward / backward calls, the input checks and the one autograd function.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib


class _Holder(nn.Module):
    """Parameter container so that state_dict keys read e.g. 'enc_conv0.weight'."""


class FlatParamModule(nn.Module):
    _display = "module"  # the class's name in messages

    def _bind_flat(self, flat: torch.Tensor, entries) -> None:
        """Make `flat` (CPU fp32) the parameter buffer: every `(dotted_name, shape)` of `entries`,
        in state_dict order, becomes an nn.Parameter viewing the next numel(shape) elements.
        Modules along a dotted path are created as `_Holder`s only where none exists yet."""
        self._flat = flat
        self._layout = []  # (module, attr, offset, shape)
        off = 0
        for name, shape in entries:
            *path, attr = name.split(".")
            mod = self
            for p in path:
                if not isinstance(getattr(mod, p, None), nn.Module):
                    setattr(mod, p, _Holder())
                mod = getattr(mod, p)
            shape = tuple(shape)
            cnt = math.prod(shape)
            setattr(mod, attr, nn.Parameter(flat[off:off + cnt].view(shape)))
            self._layout.append((mod, attr, off, shape))
            off += cnt
        assert off == flat.numel(), (off, flat.numel())

    @property
    def flat_params(self) -> torch.Tensor:
        """the flat fp32 parameter buffer every parameter is a view of"""
        return self._flat

    def _param_views(self):
        """[(offset, parameter)] in state_dict order"""
        return [(off, getattr(m, a)) for (m, a, off, _) in self._layout]

    def _params(self):
        return [getattr(m, a) for (m, a, _, _) in self._layout]

    def _grads_from_flat(self, dflat: torch.Tensor, needs):
        """per-parameter views of the flat gradient, None where autograd did not ask"""
        return [dflat[off:off + p.numel()].view_as(p) if need else None
                for (off, p), need in zip(self._param_views(), needs)]

    def _drop_scratch(self) -> None:
        """called after the parameters moved: forget scratch cached for the old device"""

    def _apply(self, fn, recurse=True):  # keep the parameters views of ONE flat buffer
        new = fn(self._flat)
        if not isinstance(new, torch.Tensor) or new.dtype != torch.float32:
            raise ValueError(f"{self._display} parameters are fp32 (the HIP path computes in fp32)")
        self._flat = new.contiguous()
        for (m, a, off, shape) in self._layout:
            p = getattr(m, a)
            p.data = self._flat[off:off + p.numel()].view(shape)
            p.grad = None
        self._drop_scratch()
        return self


class _HipNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net, *params):
        N, _, H, W = x.shape
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
        if ctx.needs_input_grad[0]:  # dL/dx from the same backward pass
            dx = torch.empty((N, net.in_nc, H, W), dtype=torch.float32, device=dy.device)
        net._run_backward(dy, dflat, ctx.ws, N, H, W, dx=dx)
        ctx.ws = None
        return (dx, None, *net._grads_from_flat(dflat, ctx.needs_input_grad[2:]))


class HipNet(FlatParamModule):
    """A network computed by the dn_<family>_* entry points.  A subclass sets the class
    attributes below and calls `_bind_net` once its flat init is drawn."""

    _family = ""         # C-ABI family: dn_<family>_forward_prec, ...
    _multiple = 1        # H and W must be multiples of this ...
    _multiple_why = ""   # ... because of this
    _has_dx = True       # the backward entry point takes a dL/dx argument
    _has_split_backward = False  # offers _run_backward_split / tail_begin (trainer.N2NTrainer)

    # arithmetic of the 3x3 convolutions (include/denoise_hip.h DN_PREC_*)
    _PRECISIONS = {"fp32": 0, "fp32_x6": 2}

    def __init__(self, in_nc: int, out_nc: int, n_feature: int):
        super().__init__()
        self.in_nc, self.out_nc, self.n_feature = in_nc, out_nc, n_feature
        self._cfg = _lib.cfg(in_nc, out_nc, n_feature)
        self._ws_cache = {}
        # the library's own check of the configuration, before any parameter is drawn: channel
        # counts or a width no kernel is built for are the caller's ValueError (DN_ERR_ARG)
        n = ctypes.c_size_t()
        what = f"dn_{self._family}_param_count"
        status = getattr(_lib.lib(), what)(ctypes.byref(self._cfg), ctypes.byref(n))
        if status == -1:
            raise ValueError(f"{self._display}(in_nc={in_nc}, out_nc={out_nc}, "
                             f"n_feature={n_feature}): {_lib.last_error()}")
        _lib.check(status, what)
        self._param_count = n.value

    def _bind_net(self, flat: torch.Tensor, entries) -> None:
        assert flat.numel() == self._param_count, (flat.numel(), self._param_count)
        self._bind_flat(flat, entries)

    def _drop_scratch(self) -> None:
        self._ws_cache = {}

    def param_range(self, name: str):
        """(begin, end) of layer `name`'s parameters (weight and bias) in the flat buffer"""
        mod = dict(self.named_modules()).get(name)
        spans = [(off, off + math.prod(shape)) for (m, _, off, shape) in self._layout if m is mod]
        if not spans:
            raise KeyError(name)
        return spans[0][0], spans[-1][1]

    def _workspace(self, N, H, W, with_backward, fresh=False):
        key = (N, H, W, bool(with_backward), self._flat.device)
        if not fresh and key in self._ws_cache:
            return self._ws_cache[key]
        nbytes = ctypes.c_size_t()
        what = f"dn_{self._family}_workspace_size"
        _lib.check(getattr(_lib.lib(), what)(ctypes.byref(self._cfg), N, H, W, int(with_backward),
                                             ctypes.byref(nbytes)), what)
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self._flat.device)
        if not fresh:
            self._ws_cache = {key: ws}
        return ws

    def set_precision(self, mode: str):
        """Arithmetic of the 3x3 convolutions in training and fp32 inference:
        'fp32'    fp32 operands on the fp32 matrix cores (v_mfma_f32_16x16x4_f32);
        'fp32_x6' fp32 operands split exactly into three bf16 pieces, the six piece products
                  of order <= 2 on the bf16 matrix cores, fp32 accumulation -- the rounding
                  error of an fp32 dot product at 2.67x the matrix-core peak.
        (ImprovedUNet: the 3x3 convolutions' forward and data gradient; its weight gradients and
        1x1 / noise-estimator convs stay fp32.)"""
        if mode not in self._PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self._PRECISIONS)}")
        self.precision = mode
        return self

    def _prec(self) -> int:
        return self._PRECISIONS[getattr(self, "precision", "fp32")]

    def _run_forward(self, x, y, ws):
        N, _, H, W = x.shape
        _lib.call(f"dn_{self._family}_forward_prec", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(x), _lib.ptr(y), N, H, W, ws.data_ptr(), ws.numel(), self._prec(),
                  _lib.stream_of(x))

    def _run_forward_inference(self, x, y, ws):
        """the no-grad forward (UNet: bf16 when set_inference_precision asks for it)"""
        self._run_forward(x, y, ws)

    def _run_forward_n2n(self, x, den, ws, rd_idx):
        """the N2N no-grad pass (N2NTrainer): the whole image, a superset of the rd pair pixels
        the loss reads (the pair-pixel fast path is built for the UNet's dec_conv1b / head)"""
        self._run_forward(x, den, ws)

    def _run_backward(self, dy, dflat, ws, N, H, W, dx=None):
        """dflat = dL/dparams (and dx = dL/dx when given) for dy = dL/dy"""
        if dx is not None and not self._has_dx:
            raise NotImplementedError("gradient w.r.t. the network input is not computed")
        dx_arg = (_lib.ptr(dx),) if self._has_dx else ()
        _lib.call(f"dn_{self._family}_backward_prec", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(dy), _lib.ptr(dflat), *dx_arg, N, H, W, ws.data_ptr(), ws.numel(),
                  self._prec(), _lib.stream_of(dy))

    def _check_input(self, x):
        if x.device.type != "cuda":
            raise RuntimeError(f"the HIP {self._display} runs on a GPU: move the module and input "
                               "to cuda")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != self.in_nc:
            raise ValueError(f"expected float32 [N,{self.in_nc},H,W], got {x.dtype} {tuple(x.shape)}")
        if self._flat.device != x.device:
            raise RuntimeError("module parameters and input are on different devices")

    def _check_size(self, H: int, W: int):
        if H % self._multiple or W % self._multiple:
            raise ValueError(f"H and W must be multiples of {self._multiple} ({self._multiple_why})")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        self._check_input(x)
        N, _, H, W = x.shape
        self._check_size(H, W)
        if torch.is_grad_enabled() and ((self._has_dx and x.requires_grad) or
                                        any(p.requires_grad for p in self.parameters())):
            # autograd: parameter gradients and/or dL/dx, as the reference module gives
            if x.requires_grad and not self._has_dx:
                raise NotImplementedError("gradient w.r.t. the network input is not computed")
            return _HipNetFunction.apply(x, self, *self._params())
        y = torch.empty((N, self.out_nc, H, W), dtype=torch.float32, device=x.device)
        self._run_forward_inference(x, y, self._workspace(N, H, W, with_backward=False))
        return y
