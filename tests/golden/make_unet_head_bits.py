"""Records tests/golden/unet_head_bits.npz: the UNet forward at (1, 1, 32, 32) in fp32_x6, bit for
bit, from a library built BEFORE the nin heads gained their residual variants.

The committed file was recorded on an MI355X from commit d924ab2 ("ImprovedUNet executor: one
conv-site table, routes once, no dry run"), the parent of the change that added RESNET:

    git worktree add ../parent d924ab2
    (cd ../parent && DN_BUILD_TAG=parent python -m image_denoising_amd._build)
    DN_LIB_PATH=../parent/image_denoising_amd/libdenoise_hip_parent.so \
        python tests/golden/make_unet_head_bits.py tests/golden/unet_head_bits.npz

The network is the recipe of tests/test_gpu_resnet.py::test_unet_head_bits_unchanged: seed 0,
UNet(1, 1, 48), weights x10, x = rand(seed 17).  `y` comes from the forward-only plan
(k_nin_head_x6 without saves), `y_bwd_plan` from a with-backward workspace (with saves).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(out):
    import ctypes

    from image_denoising_amd import _lib

    # an older library lacks the symbols added since: bind what it has
    have = ctypes.CDLL(_lib.LIB_PATH)
    for k in [k for k in _lib.SIGNATURES if not hasattr(have, k)]:
        _lib.SIGNATURES.pop(k)
    from image_denoising_amd.arch_unet import UNet

    print("library:", _lib.LIB_PATH, _lib.lib().dn_version().decode())
    torch.manual_seed(0)
    net = UNet(1, 1, 48)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
    net = net.to("cuda").set_precision("fp32_x6")
    x = torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(17))
    with torch.no_grad():
        y = net(x.cuda()).cpu().numpy()
    ws = net._workspace(1, 32, 32, True, fresh=True)
    yb = torch.empty(1, 1, 32, 32, device="cuda")
    net._run_forward(x.cuda(), yb, ws)
    torch.cuda.synchronize()
    np.savez(out, x=x.numpy(), y=y, y_bwd_plan=yb.cpu().numpy())


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
