"""Generates tests/golden/memory_adapter.npz from the REFERENCE implementation (build container
only; run by hand, the GPU box never needs the reference).

Run:  python tests/golden/make_golden_memory.py /path/to/reference

What it executes from the reference (read from its source tree at run time, nothing is copied
into this repository): `extract_patches`, `HyperGatedResidualAdapter_FFT`,
`HyperGatedResidualAdapter`, `DenoiserWithMemoryAdapter._select_memory_patch` and
`denoise_full_image_patchwise` of finetune_memory.py, AST-extracted.

Recorded, data only (torch fp32 on the CPU):
  * per tests/memory_ref.ADAPTER_CASES entry: the inputs' fp64 checksums, the features, `out`, and
    the parameter gradients of the scalar loss sum(out * dout), with seeded random NON-zero
    parameters (the reference's zero init makes half the gradients vanish);
  * per selection case and B: the reference's selected indices for the random queries, and the
    smallest fp64 gap between best and runner-up relative to |q|^2 + |b|^2;
  * the bank order of a small case (extract_patches), and the blended image of each blend case.
It asserts in fp64 that no `pre` lies within 1e-5 of a clamp bound.
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import memory_ref as R  # noqa: E402


def extract(path: str, names: list, method_of: dict, ns: dict) -> dict:
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in keep} == set(names), names
    for cls, meth in method_of.items():
        c = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
        keep += [n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == meth]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ns = extract(os.path.join(sys.argv[1], "finetune_memory.py"),
                 ["extract_patches", "HyperGatedResidualAdapter_FFT", "HyperGatedResidualAdapter",
                  "denoise_full_image_patchwise"],
                 {"DenoiserWithMemoryAdapter": "_select_memory_patch"},
                 {"torch": torch, "nn": nn, "F": F, "np": np})
    fx = {}
    for name, (B, C, H, W, Hc, nb, clamp) in R.ADAPTER_CASES.items():
        params, noisy, base, mem, dout = R.adapter_case(name)
        if nb > 0:
            ad = ns["HyperGatedResidualAdapter_FFT"](C, Hc, nb, clamp)
        else:
            ad = ns["HyperGatedResidualAdapter"](C, Hc, clamp)
        assert list(ad.state_dict()) == R.KEYS
        ad.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        n, b, m = (torch.from_numpy(v) for v in (noisy, base, mem))
        out = ad(n, b, m)
        (out * torch.from_numpy(dout)).sum().backward()
        st = [s for t in (n, b, m) for s in ad._global_mean_std(t)]
        feat = torch.stack(st, 1)
        if nb > 0:
            feat = torch.cat([feat] + [ad._row_fft_features(t) for t in (n, b, m)], 1)
        f64, o64, pre64, g64 = R.run_case(name)
        assert (pre64.abs() > 1e-5).all() and ((pre64 - 1).abs() > 1e-5).all(), name
        lo, hi = (pre64 < 0).double().mean().item(), (pre64 > 1).double().mean().item()
        k = name + "_"
        fx[k + "insum"] = np.array([v.astype(np.float64).sum() for v in (noisy, base, mem, dout)]
                                   + [R.flat_of(params).astype(np.float64).sum()])
        fx[k + "feat"] = feat.detach().numpy()
        fx[k + "out"] = out.detach().numpy()
        grads = dict(ad.named_parameters())
        fx[k + "grad"] = np.concatenate([grads[key].grad.numpy().reshape(-1) for key in R.KEYS])
        e_out = (out.detach().double() - o64).abs().max().item() / o64.abs().max().item()
        e_feat = (feat.detach().double() - f64).abs().max().item() / f64.abs().max().item()
        print(f"{name}: clamped low {lo:.3f} high {hi:.3f}  fp32-vs-fp64 rel err: feat {e_feat:.2e} "
              f"out {e_out:.2e}")
        for key in R.KEYS:
            e = (grads[key].grad.double() - g64[key]).abs().max().item() / g64[key].abs().max().item()
            print(f"    d {key:22s} {e:.2e}  (max |g| {g64[key].abs().max().item():.3e})")
    # bank order and selection
    case = R.SELECT_CASES[2]
    P, s, H, W, n_img, C = case
    imgs = R.bank_images(case, 4242)
    fx["order_patches"] = np.concatenate(
        [ns["extract_patches"](torch.from_numpy(im), P, s).numpy() for im in imgs])
    for case in R.SELECT_CASES:
        P, s, H, W, n_img, C = case
        for B in R.SELECT_B:
            imgs = R.bank_images(case, R.select_seed(case, B))
            q = R.random_queries(case, B)
            bank = torch.cat([ns["extract_patches"](torch.from_numpy(im), P, s) for im in imgs])
            fake = types.SimpleNamespace(
                memory_noise_bank=bank,
                memory_clean_bank=torch.arange(bank.shape[0], dtype=torch.float32).reshape(-1, 1, 1, 1))
            got = ns["_select_memory_patch"](fake, torch.from_numpy(q)).reshape(-1).long().numpy()
            idx, best, second, scale = R.select(torch.from_numpy(q).double(), bank.double())
            gap = ((second - best) / scale).numpy()
            key = f"sel_{P}_{s}_{H}_{W}_{n_img}_{C}_B{B}_"
            fx[key + "idx"] = got
            fx[key + "idx64"] = idx.numpy()
            fx[key + "gap"] = gap
            skipped = int((gap < R.GAP_SKIP).sum())
            print(key, "ref idx", got, "fp64 idx", idx.numpy(), f"min gap {gap.min():.2e}",
                  "skipped", skipped)
            assert skipped * 64 <= B, key
            if C == 1 and P >= 16:
                assert skipped == 0, key
    # blend: the reference's function with a stub model
    for case in R.BLEND_CASES:
        H, W, P, ov = case
        img = R.blend_image(case)
        pred = ns["denoise_full_image_patchwise"](lambda x: x * 0.9 + 0.05, img, torch.device("cpu"),
                                                  P, ov)
        fx[f"blend_{H}_{W}_{P}_{ov}"] = pred
    path = os.path.join(OUT, "memory_adapter.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
