"""Generates tests/golden/l1fft.npz from the REFERENCE implementation (build container only; run
by hand, the GPU box never needs the reference).

Run:  python tests/golden/make_golden_l1fft.py /path/to/reference

What it executes from the reference (read from its source tree at run time, nothing is copied
into this repository): the class `L1FFT` of util.py, AST-extracted.

Recorded, data only, per shape of tests/l1fft_ref.GOLDEN_SHAPES, for the inputs
tests/l1fft_ref.inputs builds, converted to fp64:
  * the reference's loss for (alpha, beta) = (1, 0), (0, 1), (1, 0.7) with reduction='mean' and
    for (1, 0.7) with reduction='sum';
  * the autograd gradient w.r.t. pred of the (1, 0.7) reduction='mean' loss;
  * the inputs' fp64 sums (a test asserts them, so a drifted input generator is seen).
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import l1fft_ref as R  # noqa: E402

ALPHA, BETA = R.GOLDEN_ALPHA, R.GOLDEN_BETA


def extract_class(path: str, name: str, ns: dict):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(keep) == 1, name
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    cls = extract_class(os.path.join(sys.argv[1], "util.py"), "L1FFT", {"torch": torch, "nn": nn})
    fx = {}
    for shape in R.GOLDEN_SHAPES:
        pred, target = (x.double() for x in R.inputs(shape))
        k = "x".join(map(str, shape)) + "_"
        fx[k + "insum"] = np.array([pred.sum().item(), target.sum().item()])
        for tag, a, b, red in (("pix", 1.0, 0.0, "mean"), ("frq", 0.0, 1.0, "mean"),
                               ("mean", ALPHA, BETA, "mean"), ("sum", ALPHA, BETA, "sum")):
            p = pred.clone().requires_grad_(True)
            loss = cls(alpha=a, beta=b, reduction=red)(p, target)
            fx[k + tag] = np.float64(loss.item())
            if tag == "mean":
                loss.backward()
                fx[k + "dmean"] = p.grad.numpy()
            print(k + tag, loss.item())
    path = os.path.join(OUT, "l1fft.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
