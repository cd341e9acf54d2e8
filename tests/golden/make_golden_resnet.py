"""Generates tests/golden/resnet_c1.npz .. resnet_c4.npz from the REFERENCE RESNET (build
container only; the GPU box never needs the reference).

Run:  python tests/golden/make_golden_resnet.py /path/to/reference [fixture names]

It imports the reference's arch_unet as a module (nothing is copied into this repository) and
records data only: inputs, outputs, the seed-0 initialisation's fingerprint and gradients.
The residual is small at init scale (y ~ x would hide errors), so every parameter is scaled by a
constant chosen such that max|y - x| >= 0.1 max|x|; the scale is stored.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
SCALE = 8.0
NSAMPLE = 8192


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def flat(net) -> np.ndarray:
    return torch.cat([v.reshape(-1) for v in net.state_dict().values()]).numpy().astype(np.float32)


def one(arch_unet, C, shape, seed, name):
    torch.manual_seed(0)
    net = arch_unet.RESNET(in_nc=C, out_nc=C, n_feature=48)
    keys = list(net.state_dict())
    init = flat(net)
    torch.manual_seed(0)
    sha_zero = sha(flat(arch_unet.RESNET(in_nc=C, out_nc=C, n_feature=48, zero_last=True)))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(SCALE)
        g = torch.Generator().manual_seed(seed + 100)
        for n_, p in net.named_parameters():  # non-zero biases: every bias gradient path is live
            if n_.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    params = flat(net)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed)).requires_grad_(True)
    y = net(x)
    loss = (y ** 2).mean()
    loss.backward()
    res = (y - x).detach().abs().max().item()
    assert res >= 0.1 * x.detach().abs().max().item(), res
    grads, norms = [], []
    for k, p in net.named_parameters():
        gk = torch.zeros_like(p) if p.grad is None else p.grad
        grads.append(gk.reshape(-1))
        norms.append(float(gk.double().norm()))
    gflat = torch.cat(grads).numpy()
    idx = np.sort(np.random.default_rng(seed).choice(gflat.size, NSAMPLE, replace=False))
    np.savez_compressed(
        os.path.join(OUT, name), x=x.detach().numpy(), y=y.detach().numpy(),
        loss=np.float64(loss.item()), dx=x.grad.numpy(), keys=np.array(keys),
        key_shapes=np.array([str(tuple(v.shape)) for v in net.state_dict().values()]),
        params_sha=sha(init), params_head=init[:64], params_sha_zero_last=sha_zero,
        scale=np.float32(SCALE), bias_seed=np.int64(seed + 100), params_scaled_sha=sha(params),
        grad_idx=idx.astype(np.int64), grad_sample=gflat[idx], grad_norms=np.array(norms),
        grad_max=np.array([float(gk.abs().max()) for gk in grads]), residual_max=np.float64(res))
    print(name, "max|y-x| =", res, "loss =", loss.item())


FIXTURES = {
    "resnet_c1.npz": (1, (2, 1, 24, 40), 11),
    "resnet_c3.npz": (3, (1, 3, 13, 22), 12),
    # the two channel counts between and above: enc_conv0 / dec_conv1a's K = 98 and 100
    "resnet_c2.npz": (2, (1, 2, 32, 32), 13),
    "resnet_c4.npz": (4, (1, 4, 32, 32), 14),
}


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import arch_unet

    for name in sys.argv[2:] or FIXTURES:  # (named fixtures only, or all of them)
        C, shape, seed = FIXTURES[name]
        one(arch_unet, C, shape, seed, name)


if __name__ == "__main__":
    main()
