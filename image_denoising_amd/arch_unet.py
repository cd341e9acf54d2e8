"""Drop-in `UNet` for arch_unet.py:100-260, computed by libdenoise_hip.so on gfx950.

Same constructor signature, same `state_dict` keys/shapes (so reference checkpoints load with
`load_state_dict`), same `forward(x[N,C,H,W]) -> [N,out_nc,H,W]`.  Internally all parameters are
views into ONE flat fp32 buffer in state_dict order (the layout the C-ABI consumes), and the
forward/backward run through dn_unet_forward / dn_unet_backward (parameter gradients and, when the
input requires grad, dL/dx).  That machinery is flat_module.HipNet's, shared with RESNET and
ImprovedUNet; this file holds the UNet's own: layer table, init replay, bf16 inference,
prepacked weights, the N2N pair-pixel pass and the split backward.  The blind-spot variant
(arch_unet.py:65-97) is out of scope and raises.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.init as init

from . import _lib
from .flat_module import HipNet

# state_dict order of arch_unet.py:115-192
LAYER_NAMES = [
    "enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5", "enc_conv6",
    "up5.deconv", "dec_conv5a", "dec_conv5b", "up4.deconv", "dec_conv4a", "dec_conv4b",
    "up3.deconv", "dec_conv3a", "dec_conv3b", "up2.deconv", "dec_conv2a", "dec_conv2b",
    "up1.deconv", "dec_conv1a", "dec_conv1b", "nin_a", "nin_b", "nin_c",
]


def layer_shapes(in_nc: int, out_nc: int, nf: int):
    """[(name, weight_shape, bias_len, is_deconv)] in state_dict order (arch_unet.py:115-192)."""
    C, OC = in_nc, out_nc
    s = []
    conv = lambda name, co, ci, k: s.append((name, (co, ci, k, k), co, False))
    dec = lambda name, ci, co: s.append((name, (ci, co, 2, 2), co, True))
    conv("enc_conv0", nf, C, 3)
    for i in range(1, 7):
        conv(f"enc_conv{i}", nf, nf, 3)
    dec("up5.deconv", nf, nf)
    conv("dec_conv5a", 2 * nf, 2 * nf, 3)
    conv("dec_conv5b", 2 * nf, 2 * nf, 3)
    for lvl in (4, 3, 2):
        dec(f"up{lvl}.deconv", 2 * nf, 2 * nf)
        conv(f"dec_conv{lvl}a", 2 * nf, 3 * nf, 3)
        conv(f"dec_conv{lvl}b", 2 * nf, 2 * nf, 3)
    dec("up1.deconv", 2 * nf, 2 * nf)
    conv("dec_conv1a", 96, 2 * nf + C, 3)
    conv("dec_conv1b", 96, 96, 3)
    conv("nin_a", 96, 96, 1)
    conv("nin_b", 96, 96, 1)
    conv("nin_c", OC, 96, 1)
    return s


def param_count(in_nc: int, out_nc: int, nf: int) -> int:
    return sum(int(torch.Size(w).numel()) + b for _, w, b, _ in layer_shapes(in_nc, out_nc, nf))


def flat_entries(shapes):
    """layer_shapes() rows as the [(dotted parameter name, shape)] list the flat buffer is bound by"""
    return [e for name, wshape, blen, _ in shapes
            for e in ((name + ".weight", wshape), (name + ".bias", (blen,)))]


def _kaiming01(m: nn.Module) -> None:
    # arch_unet.py:24-48 initialize_weights(m, 0.1) for Conv2d / ConvTranspose2d
    init.kaiming_normal_(m.weight, a=0, mode="fan_in")
    m.weight.data *= 0.1
    if m.bias is not None:
        m.bias.data.zero_()


def reference_init(in_nc: int, out_nc: int, nf: int = 48, zero_last: bool = False) -> torch.Tensor:
    """Flat CPU fp32 parameters drawn exactly like arch_unet.UNet.__init__ does.

    The reference constructs torch modules (each consuming the global CPU RNG in its
    reset_parameters) and re-initialises them with kaiming_normal_; the construction /
    initialisation ORDER of arch_unet.py:115-192 is replayed here, so that
    `torch.manual_seed(s); UNet(...)` yields bit-identical weights to the reference.
    """
    C, OC = in_nc, out_nc
    mods = {}

    def conv(name, ci, co, k):
        mods[name] = nn.Conv2d(ci, co, k, 1, (k - 1) // 2)

    def up(name, ci, co):  # UpsampleCat.__init__ (arch_unet.py:52-58)
        mods[name] = nn.ConvTranspose2d(ci, co, 2, 2, 0, 0)
        _kaiming01(mods[name])

    with torch.no_grad():
        conv("enc_conv0", C, nf, 3)
        conv("enc_conv1", nf, nf, 3)
        _kaiming01(mods["enc_conv0"])
        _kaiming01(mods["enc_conv1"])
        for i in range(2, 7):
            conv(f"enc_conv{i}", nf, nf, 3)
            _kaiming01(mods[f"enc_conv{i}"])
        up("up5.deconv", nf, nf)
        conv("dec_conv5a", 2 * nf, 2 * nf, 3)
        conv("dec_conv5b", 2 * nf, 2 * nf, 3)
        _kaiming01(mods["dec_conv5a"])
        _kaiming01(mods["dec_conv5b"])
        for lvl in (4, 3, 2):
            up(f"up{lvl}.deconv", 2 * nf, 2 * nf)
            conv(f"dec_conv{lvl}a", 3 * nf, 2 * nf, 3)
            conv(f"dec_conv{lvl}b", 2 * nf, 2 * nf, 3)
            _kaiming01(mods[f"dec_conv{lvl}a"])
            _kaiming01(mods[f"dec_conv{lvl}b"])
        up("up1.deconv", 2 * nf, 2 * nf)
        conv("dec_conv1a", 2 * nf + C, 96, 3)
        _kaiming01(mods["dec_conv1a"])
        conv("dec_conv1b", 96, 96, 3)
        _kaiming01(mods["dec_conv1b"])
        conv("nin_a", 96, 96, 1)
        conv("nin_b", 96, 96, 1)
        _kaiming01(mods["nin_a"])
        _kaiming01(mods["nin_b"])
        conv("nin_c", 96, OC, 1)
        if not zero_last:
            _kaiming01(mods["nin_c"])
        parts = []
        for name in LAYER_NAMES:
            parts += [mods[name].weight.reshape(-1), mods[name].bias.reshape(-1)]
        return torch.cat(parts).float().contiguous()


class UNet(HipNet):
    """arch_unet.py:100 UNet(in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False)."""

    _family, _display = "unet", "UNet"
    _multiple, _multiple_why = 32, "arch_unet.py: 5 pooling levels"
    _has_split_backward = True

    def __init__(self, in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False):
        if blindspot:
            raise NotImplementedError("blind-spot UNet (arch_unet.py:65-97) is out of scope")
        super().__init__(in_nc, out_nc, n_feature)
        self.blindspot, self.zero_last = blindspot, zero_last
        self._bind_net(reference_init(in_nc, out_nc, n_feature, zero_last),
                       flat_entries(layer_shapes(in_nc, out_nc, n_feature)))

    def _infer_prec(self) -> int:
        """the precision code of a no-grad forward (bf16 for the configs[4] frozen base)"""
        return 1 if getattr(self, "inference_precision", "fp32") == "bf16" else self._prec()

    def _pack_weights(self, ws, N, H, W):
        """dn_unet_pack_weights: the forward's weight images for (N, H, W) into ws, once, for
        _run_forward_prepacked calls with these parameters (SURVEY §8b persistent packing)"""
        _lib.call("dn_unet_pack_weights", ctypes.byref(self._cfg), _lib.ptr(self._flat), N, H, W,
                  ws.data_ptr(), ws.numel(), self._infer_prec(), _lib.stream_of(self._flat))

    def _run_forward_prepacked(self, x, y, ws):
        """the no-grad forward on the images _pack_weights left in ws (no re-pack): bit-identical
        to _run_forward_inference while the parameters are unchanged"""
        N, _, H, W = x.shape
        _lib.call("dn_unet_forward_prepacked", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(x), _lib.ptr(y), N, H, W, ws.data_ptr(), ws.numel(), self._infer_prec(),
                  _lib.stream_of(x))

    def _run_forward_n2n(self, x, den, ws, rd_idx):
        """the N2N no-grad pass: den = UNet(x) at the pair pixels of rd_idx only
        (dn_unet_forward_n2n; training_script.md:141-144 reads nothing else)"""
        N, _, H, W = x.shape
        _lib.call("dn_unet_forward_n2n", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(x), _lib.ptr(den), _lib.ptr(rd_idx), N, H, W, ws.data_ptr(), ws.numel(),
                  self._prec(), _lib.stream_of(x))

    def set_inference_precision(self, dtype: str) -> "UNet":
        """'fp32' (default, the parity path) or 'bf16': no-grad forwards then multiply
        bf16-rounded operands on the bf16 matrix cores (fp32 accumulation and storage) —
        the mixed-precision frozen base of BASELINE configs[4].  Training is always fp32."""
        if dtype not in ("fp32", "bf16"):
            raise ValueError("inference precision must be 'fp32' or 'bf16'")
        self.inference_precision = dtype
        return self

    def _run_forward_inference(self, x, y, ws):
        if getattr(self, "inference_precision", "fp32") != "bf16":
            return self._run_forward(x, y, ws)
        N, _, H, W = x.shape
        _lib.call("dn_unet_forward_bf16", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(x), _lib.ptr(y), N, H, W, ws.data_ptr(), ws.numel(), _lib.stream_of(x))

    def _run_backward_split(self, dy, dflat, ws, N, H, W, tail_ready):
        """_run_backward that records tail_ready (a torch.cuda.Event) once dflat[tail_begin():]
        is final, while the encoder's gradients are still being computed
        (dn_unet_backward_split: the data-parallel step all-reduces that range early)"""
        _lib.call("dn_unet_backward_split", ctypes.byref(self._cfg), _lib.ptr(self._flat),
                  _lib.ptr(dy), _lib.ptr(dflat), None, N, H, W, ws.data_ptr(), ws.numel(),
                  self._prec(), _lib.stream_of(dy), ctypes.c_void_p(tail_ready.cuda_event), None)

    def tail_begin(self) -> int:
        """first flat-parameter index of the range (dec_conv5a .. nin_c, state_dict order) whose
        gradient the backward finishes before the encoder's"""
        t = ctypes.c_int64()
        _lib.call("dn_unet_backward_split", ctypes.byref(self._cfg), None, None, None, None, 1, 32,
                  32, None, 0, self._prec(), None, None, ctypes.byref(t))
        return int(t.value)
