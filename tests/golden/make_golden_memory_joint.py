"""Generates tests/golden/memory_joint_c1.npz from the REFERENCE implementation (build container
only; run by hand, the GPU box never needs the reference).

Run:  python tests/golden/make_golden_memory_joint.py [/path/to/reference]

What it executes from the reference (read from its source tree at run time, nothing is copied
into this repository): arch_unet.UNet, imported as a module, and finetune_memory.py's
`HyperGatedResidualAdapter_FFT`, `HyperGatedResidualAdapter`, `DenoiserWithMemoryAdapter`,
`extract_patches`, `gradient` and `gradient_loss`, AST-extracted (the file imports torchvision and
tqdm, absent here).

(i)  The adapter's input gradient: per entry of DBASE_CASES (tests/memory_ref.ADAPTER_CASES
     inputs, seeded NON-zero parameters) the reference adapter's own d sum(out * dout) / d base_out
     in torch fp32 on the CPU.
(ii) The joint run, tests/memory_joint_ref.golden_setup's model and batches:

    model = DenoiserWithMemoryAdapter(UNet(1, 1, 48), 1, 16, noise bank, clean bank,
                                      freeze_base=False, use_no_grad_for_base=False)
    opt   = Adam(filter(requires_grad, model.parameters()), lr=1e-4)  (finetune_memory.py:1380-1383)
    two steps of loss = L1 + 0.1 * gradient_loss at 2 x 1 x 32 x 32  (finetune_memory.py:1409-1430)

Stored (data only), sized and sampled as joint_c1.npz: both batches, the selected bank index of
every sample and its fp64 gap to the runner-up, each step's three loss terms, of the first step
`pred`, every adapter gradient and per base layer the gradient's L2 norm and 16 samples at fixed
indices, and the parameters at the same indices (and the whole adapter) after each step.  The
sampled indices of a layer are drawn (seeded) among the elements whose first-step gradient is at
least 1e-3 of the layer's largest: Adam's first update is lr * g / (|g| + 1e-8), whose sign no
arithmetic can reproduce for a gradient that is rounding noise.
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import memory_joint_ref as J  # noqa: E402
import memory_ref as R  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
NS = 16  # samples per base layer


def extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in keep} == set(names)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy()


def main():
    sys.path.insert(0, REF)
    import arch_unet  # noqa: E402

    ns = extract(os.path.join(REF, "finetune_memory.py"),
                 ["HyperGatedResidualAdapter_FFT", "HyperGatedResidualAdapter",
                  "DenoiserWithMemoryAdapter", "extract_patches", "gradient", "gradient_loss"],
                 {"torch": torch, "nn": nn, "F": F, "np": np})
    fx = {}
    # (i) the adapter alone
    for name in J.DBASE_CASES:
        B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
        params, noisy, base, mem, dout = R.adapter_case(name)
        ad = (ns["HyperGatedResidualAdapter_FFT"](C, Hc, nb, clamp) if nb > 0
              else ns["HyperGatedResidualAdapter"](C, Hc, clamp))
        ad.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        b = torch.from_numpy(base).clone().requires_grad_(True)
        out = ad(torch.from_numpy(noisy), b, torch.from_numpy(mem))
        (out * torch.from_numpy(dout)).sum().backward()
        fx[name + "_dbase"] = b.grad.numpy().copy()
        fx[name + "_insum"] = np.array([v.astype(np.float64).sum() for v in (noisy, base, mem, dout)]
                                       + [R.flat_of(params).astype(np.float64).sum()])
        want, _ = J.adapter_input_grad(params, noisy, base, mem, dout, nb, clamp)
        e = (b.grad.double() - want).abs().max().item() / want.abs().max().item()
        print(f"{name}: reference fp32 dbase vs memory_ref fp64: {e:.2e}")
    # (ii) the joint run
    s = J.golden_setup()
    torch.manual_seed(0)
    base = arch_unet.UNet(in_nc=1, out_nc=1, n_feature=48)
    J.centre_state(base)
    P, st = s["patch"], s["stride"]
    nbank = torch.cat([ns["extract_patches"](im, P, st) for im in s["bank_noise"]])
    cbank = torch.cat([ns["extract_patches"](im, P, st) for im in s["bank_clean"]])
    model = ns["DenoiserWithMemoryAdapter"](base, 1, 16, nbank, cbank, freeze_base=False,
                                            use_no_grad_for_base=False)
    assert list(model.adapter.state_dict()) == R.KEYS
    model.adapter.load_state_dict(s["adapter"])
    base_pre = flat(model.base.parameters())
    opt = torch.optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4)
    fx.update(base_sha=np.array(hashlib.sha256(base_pre.tobytes()).hexdigest()),
              adapter_pre=flat(model.adapter.parameters()))
    names = [k[:-len(".weight")] for k in model.base.state_dict() if k.endswith(".weight")]
    for step, (clean, noisy) in enumerate(s["batches"], 1):
        opt.zero_grad()
        idx, best, second, scale = R.select(noisy.double(), nbank.double())
        mem = model._select_memory_patch(noisy)
        assert torch.equal(mem, cbank[idx]), "the reference's fp32 argmin differs from fp64"
        fx[f"idx{step}"] = idx.numpy()
        fx[f"gap{step}"] = ((second - best) / scale).numpy()
        assert fx[f"gap{step}"].min() >= R.GAP_SKIP
        pred = model(noisy)
        l1 = F.l1_loss(pred, clean)
        lg = ns["gradient_loss"](pred, clean)
        loss = l1 + 0.1 * lg
        loss.backward()
        fx[f"clean{step}"], fx[f"noisy{step}"] = clean.numpy(), noisy.numpy()
        fx[f"loss{step}"] = np.array([l1.item(), lg.item(), loss.item()], np.float32)
        if step == 1:
            fx["pred1"] = pred.detach().numpy()
            fx["adapter_grad"] = flat(p.grad for p in model.adapter.parameters())
            gb = flat(p.grad for p in model.base.parameters())
            sel, norms, off = [], [], 0
            mods = dict(model.base.named_modules())
            for li, name in enumerate(names):
                n = sum(p.numel() for p in mods[name].parameters())
                gl = gb[off:off + n]
                norms.append(np.linalg.norm(gl.astype(np.float64)))
                ok = np.flatnonzero(np.abs(gl) >= 1e-3 * np.abs(gl).max())
                pick = np.sort(np.random.default_rng(li).choice(ok, NS, replace=len(ok) < NS))
                sel.append(off + pick)
                off += n
            assert off == gb.size
            sel = np.stack(sel).astype(np.int64)  # [layers, NS] into the base's flat buffer
            fx.update(layer_names=np.array(names), base_idx=sel, base_grad_norms=np.array(norms),
                      base_grad_sample=gb[sel], base_grad_max=np.float64(np.abs(gb).max()))
            unclamped = ((pred > 0) & (pred < 1)).double().mean().item()
            print(f"step 1: loss {loss.item():.6f}, unclamped {unclamped:.3f}, "
                  f"max |g_base| {np.abs(gb).max():.3e}, max |g_adapter| "
                  f"{np.abs(fx['adapter_grad']).max():.3e}")
        opt.step()
        fx[f"base_post{step}"] = flat(model.base.parameters())[fx["base_idx"]]
        fx[f"adapter_post{step}"] = flat(model.adapter.parameters())
    path = os.path.join(OUT, "memory_joint_c1.npz")
    np.savez_compressed(path, **fx)
    print("memory joint fixture written to", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
