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

import torch
import torch.nn as nn

from .arch_unet import _kaiming01, flat_entries
from .flat_module import HipNet

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


class RESNET(HipNet):
    """arch_unet.py:263 RESNET(in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False).
    Any H, W; the backward leaves zeros over up5.deconv's gradient; bf16 inference is not built."""

    _family, _display = "resnet", "RESNET"

    def __init__(self, in_nc=3, out_nc=3, n_feature=48, blindspot=False, zero_last=False):
        if blindspot:
            raise NotImplementedError("blind-spot RESNET (arch_unet.py:65-97) is out of scope")
        if out_nc != in_nc:
            raise ValueError("the HIP RESNET adds its input to its output: out_nc must equal in_nc "
                             "(torch would broadcast a one-channel side)")
        if n_feature != 48:
            raise ValueError("n_feature must be 48 (kernel tiles are instantiated for the "
                             "reference width)")
        super().__init__(in_nc, out_nc, n_feature)
        self.blindspot, self.zero_last = blindspot, zero_last
        self._bind_net(reference_init(in_nc, out_nc, n_feature, zero_last),
                       flat_entries(layer_shapes(in_nc, out_nc, n_feature)))
