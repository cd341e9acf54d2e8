"""Drop-in `ImprovedUNet` for arch_unet.py:421-531 (the model train.sh and evaluation.py
default to), computed by libdenoise_hip.so on gfx950 (dn_iunet_forward / dn_iunet_backward).

Same constructor, same `state_dict` keys and shapes (reference checkpoints load with
`load_state_dict`), same forward.  The module tree below only carries the parameters (drawn in
the reference's construction order, so `torch.manual_seed(s); ImprovedUNet(...)` matches the
reference bit for bit); every parameter is then re-pointed into ONE flat fp32 buffer, the layout
the C-ABI consumes.  Only the reference's defaults depth=4, noise=True and n_feature=48 are built.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .flat_module import HipNet

GROWTH = 32


def _gn(ch: int) -> nn.GroupNorm:  # norm2d('gn', ch, groups=32), arch_unet.py:7-15
    g = min(32, ch)
    while ch % g != 0 and g > 1:
        g -= 1
    return nn.GroupNorm(g, ch, affine=True)


class _RDB(nn.Module):  # parameter holder of arch_unet.py:436-444
    def __init__(self, ch):
        super().__init__()
        self.convs = nn.ModuleList()
        c = ch
        for _ in range(4):
            self.convs.append(nn.Conv2d(c, GROWTH, 3, 1, 1, bias=True))
            c += GROWTH
        self.lff = nn.Conv2d(c, ch, 1, 1, 0, bias=True)
        self.act = nn.LeakyReLU(0.2, True)


class _ResBlock(nn.Module):  # arch_unet.py:422-431
    def __init__(self, ch):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(ch, ch, 3, 1, 1, bias=False), _gn(ch),
                                   nn.LeakyReLU(0.2, True), nn.Conv2d(ch, ch, 3, 1, 1, bias=False),
                                   _gn(ch))


class _UpBlock(nn.Module):  # arch_unet.py:454-461
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv_ps = nn.Conv2d(in_ch, out_ch * 4, 3, 1, 1, bias=True)
        self.ps = nn.PixelShuffle(2)
        self.fuse = nn.Conv2d(out_ch * 3, out_ch, 3, 1, 1, bias=True)
        self.rdb = _RDB(out_ch)
        self.res = _ResBlock(out_ch)


class ImprovedUNet(HipNet):
    """arch_unet.py:475 ImprovedUNet(in_nc=3, out_nc=3, n_feature=48, depth=4, noise=True).
    dL/dx is not computed: an input that requires grad raises."""

    _family, _display = "iunet", "ImprovedUNet"
    _multiple, _multiple_why = 16, "ImprovedUNet: 4 pooling levels"
    _has_dx = False

    def __init__(self, in_nc=3, out_nc=3, n_feature=48, depth=4, noise=True):
        if depth != 4 or not noise or n_feature != 48:
            raise NotImplementedError("the HIP ImprovedUNet is built for depth=4, noise=True, "
                                      "n_feature=48 (the reference's defaults)")
        super().__init__(in_nc, out_nc, n_feature)
        self.noise = noise
        # construction order of arch_unet.py:476-516 (every Conv2d draws from the global RNG)
        nf = n_feature
        self.noise_estimator = nn.Sequential(nn.Conv2d(in_nc, nf, 3, 1, 1, bias=True),
                                             nn.LeakyReLU(0.2, True),
                                             nn.Conv2d(nf, 1, 3, 1, 1, bias=True), nn.Sigmoid())
        self.downs, self.pools = nn.ModuleList(), nn.ModuleList()
        for i in range(depth):
            inc = in_nc + 1 if i == 0 else nf // 2
            self.downs.append(nn.Sequential(nn.Conv2d(inc, nf, 3, 1, 1, bias=True),
                                            nn.LeakyReLU(0.2, True), _RDB(nf), _ResBlock(nf)))
            self.pools.append(nn.MaxPool2d(2))
            nf *= 2
        self.bottle = nn.Sequential(_RDB(nf // 2), _ResBlock(nf // 2))
        nf //= 2
        self.ups = nn.ModuleList()
        for _ in range(depth):
            self.ups.append(_UpBlock(nf, nf // 2))
            nf //= 2
        self.final = nn.Conv2d(n_feature // 2 + in_nc, out_nc, 3, 1, 1, bias=True)
        self.sigmoid = nn.Sigmoid()
        # one flat buffer in state_dict order; parameters become views of it
        named = list(self.named_parameters())
        self._bind_net(torch.cat([p.detach().reshape(-1) for _, p in named]).float().contiguous(),
                       [(name, p.shape) for name, p in named])
