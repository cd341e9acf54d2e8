"""Generates tests/golden/joint_c1.npz from the REFERENCE implementation (build container only).

Run:  python tests/golden/make_golden_joint.py [/path/to/reference]

What it executes from the reference (read from its source tree, nothing is copied into this
repo): adapter.DenoiserWithAdapter and arch_unet.UNet, imported as modules, and finetune.py's
gradient / gradient_loss, AST-extracted (finetune.py imports torchvision, absent here).

    model = DenoiserWithAdapter(UNet(1, 1, 48), freeze_base=False, use_no_grad_for_base=False)
    opt   = Adam(filter(requires_grad, model.parameters()), lr=1e-4)        (finetune.py:260-263)
    two steps of loss = L1 + 0.1 * gradient_loss at 2 x 1 x 32 x 32         (finetune.py:269-289)

Stored (data only): both batches, each step's three loss terms, of the first step all 449 adapter
gradients and per base layer the gradient's L2 norm and 16 samples at fixed indices, and the
parameters at the same indices (and the whole adapter) after each step.  The sampled indices of a
layer are drawn (seeded) among the elements whose first-step gradient is at least 1e-3 of the
layer's largest: Adam's first update is lr * g / (|g| + 1e-8), whose sign no arithmetic can
reproduce for a gradient that is rounding noise.
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
NS = 16  # samples per base layer


def extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in keep} == set(names)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy()


def main():
    sys.path.insert(0, REF)
    import adapter  # noqa: E402
    import arch_unet  # noqa: E402

    ft = extract(os.path.join(REF, "finetune.py"), ["gradient", "gradient_loss"],
                 {"torch": torch, "F": torch.nn.functional})
    torch.manual_seed(0)
    base = arch_unet.UNet(in_nc=1, out_nc=1, n_feature=48)
    torch.manual_seed(1)
    model = adapter.DenoiserWithAdapter(base, in_channels=1, hidden_channels=16,
                                        freeze_base=False, use_no_grad_for_base=False)
    base_pre = flat(model.base.parameters())
    g = torch.Generator().manual_seed(40)
    batches = []
    for _ in range(2):
        clean = torch.rand(2, 1, 32, 32, generator=g)
        batches.append((clean, clean + 0.1 * torch.randn(2, 1, 32, 32, generator=g)))
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4)
    fx = dict(base_sha=np.array(hashlib.sha256(base_pre.tobytes()).hexdigest()),
              adapter_pre=flat(model.adapter.parameters()))
    # layer = weight + bias, in state_dict order
    names = [k[:-len(".weight")] for k in model.base.state_dict() if k.endswith(".weight")]
    for s, (clean, noisy) in enumerate(batches, 1):
        opt.zero_grad()
        pred = model(noisy)
        l1 = torch.nn.functional.l1_loss(pred, clean)
        lg = ft["gradient_loss"](pred, clean)
        loss = l1 + 0.1 * lg
        loss.backward()
        fx[f"clean{s}"], fx[f"noisy{s}"] = clean.numpy(), noisy.numpy()
        fx[f"loss{s}"] = np.array([l1.item(), lg.item(), loss.item()], np.float32)
        if s == 1:
            fx["pred1"] = pred.detach().numpy()
            fx["adapter_grad"] = flat(p.grad for p in model.adapter.parameters())
            gb = flat(p.grad for p in model.base.parameters())
            idx, norms, off = [], [], 0
            mods = dict(model.base.named_modules())
            for li, name in enumerate(names):
                n = sum(p.numel() for p in mods[name].parameters())
                gl = gb[off:off + n]
                norms.append(np.linalg.norm(gl.astype(np.float64)))
                ok = np.flatnonzero(np.abs(gl) >= 1e-3 * np.abs(gl).max())
                pick = np.sort(np.random.default_rng(li).choice(ok, NS, replace=len(ok) < NS))
                idx.append(off + pick)
                off += n
            assert off == gb.size
            idx = np.stack(idx).astype(np.int64)  # [layers, NS] into the base's flat buffer
            fx.update(layer_names=np.array(names), base_idx=idx, base_grad_norms=np.array(norms),
                      base_grad_sample=gb[idx], base_grad_max=np.float64(np.abs(gb).max()))
        opt.step()
        fx[f"base_post{s}"] = flat(model.base.parameters())[fx["base_idx"]]
        fx[f"adapter_post{s}"] = flat(model.adapter.parameters())
    np.savez_compressed(os.path.join(OUT, "joint_c1.npz"), **fx)
    print("joint finetune fixture written to", OUT, os.path.getsize(os.path.join(OUT, "joint_c1.npz")))


if __name__ == "__main__":
    main()
