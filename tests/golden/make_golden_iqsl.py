"""Generates tests/golden/iqsl.npz from the REFERENCE implementation (build container only; run
by hand, the GPU box never needs the reference).

Run:  python tests/golden/make_golden_iqsl.py /path/to/reference

What it executes from the reference (read from its source tree at run time, nothing is copied
into this repository): `gradient`, `gradient_loss`, `iqsl_loss` of finetune_iqsl.py and
`_to_gray_float01`, `_quantize_3class`, `compute_iq_iou` of evaluation_adapter_iqsl.py,
AST-extracted (both modules import torchvision, absent here).

Recorded, data only:
  * per (case, shape) of tests/iqsl_ref.PAIRS, for the inputs tests/iqsl_ref.case_inputs builds:
    loss4 = [l1, grad, iqsl, l1 + 0.1 grad + 0.1 iqsl] in torch fp32 on the CPU, the autograd
    dpred of that total (every element for the small shape, the elements `idx` for the others),
    max |dpred|, and the inputs' fp64 sums (a test asserts them, so a drifted input generator
    is seen);
  * IQ-IoU: small uint8 images, their thresholds, the reference's IoUs and the label counts.
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import iqsl_ref as R  # noqa: E402


def extract(path: str, names: list[str], ns: dict) -> dict:
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    missing = set(names) - {n.name for n in keep}
    assert not missing, missing
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def sample_idx(n: int, seed: int, count: int = 1024) -> np.ndarray:
    if n <= count:
        return np.arange(n, dtype=np.int64)
    return np.unique((R.uniform(count, seed) * n).astype(np.int64))


def palette_image(shape, levels, seed):
    u = R.uniform(int(np.prod(shape)), seed)
    return np.asarray(levels, np.uint8)[(u * len(levels)).astype(np.int64)].reshape(shape)


def iq_cases():
    """name -> (pred255 uint8, clean255 uint8, low_q, high_q); [H,W] or [H,W,3]"""
    lv = [12, 40, 77, 77, 130, 181, 181, 240]  # repeated levels: the quantiles land on a level
    out = {}
    for name, shape, seed in (("c1_7x9", (7, 9), 3), ("c3_7x9", (7, 9, 3), 4),
                              ("c1_64x80", (64, 80), 5), ("c3_64x80", (64, 80, 3), 6)):
        clean = palette_image(shape, lv, seed)
        if len(shape) == 3:  # gray levels repeat only if whole pixels do
            clean = np.repeat(palette_image(shape[:2], lv, seed)[:, :, None], 3, axis=2)
            clean[..., 1] = np.clip(clean[..., 1].astype(int) + 3, 0, 255)
            clean[..., 2] = np.clip(clean[..., 2].astype(int) - 2, 0, 255)
        noise = (R.uniform(clean.size, seed + 50).reshape(clean.shape) * 60 - 30).round()
        keep = R.uniform(clean.size, seed + 60).reshape(clean.shape) < 0.5  # half the pixels exact
        pred = np.where(keep, clean, np.clip(clean + noise, 0, 255)).astype(np.uint8)
        out[name] = (pred, clean, 0.25, 0.75)
    # two levels only: no pixel of either image is mid -> nan
    clean = palette_image((7, 9), [10, 200], 7)
    pred = np.where(R.uniform(63, 8).reshape(7, 9) < 0.8, clean, 210 - clean).astype(np.uint8)
    out["c1_7x9_nomid"] = (pred, clean, 0.25, 0.75)
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    ns = extract(os.path.join(ref, "finetune_iqsl.py"), ["gradient", "gradient_loss", "iqsl_loss"],
                 {"torch": torch, "F": F})
    ev = extract(os.path.join(ref, "evaluation_adapter_iqsl.py"),
                 ["_to_gray_float01", "_quantize_3class", "compute_iq_iou"], {"np": np})
    fx = {}
    for case, shape in R.PAIRS:
        tau, margin, cef = R.CASES[case]
        pred, target = R.case_inputs(case, shape)
        p = torch.from_numpy(pred).clone().requires_grad_(True)
        t = torch.from_numpy(target)
        l1 = F.l1_loss(p, t)
        lg = ns["gradient_loss"](p, t)
        iq = ns["iqsl_loss"](p, t, t1=R.T1, t2=R.T2, tau=tau, margin=margin, ce_factor=cef)
        loss = l1 + R.LAMBDA_GRAD * lg + R.LAMBDA_IQSL * iq
        loss.backward()
        d = p.grad.numpy().reshape(-1)
        idx = sample_idx(d.size, 100 + len(fx))
        k = f"{case}_{shape}_"
        fx[k + "loss4"] = np.array([l1.item(), lg.item(), iq.item(), loss.item()], np.float32)
        fx[k + "idx"] = idx
        fx[k + "dpred"] = d[idx]
        fx[k + "dmax"] = np.float32(np.abs(d).max())
        fx[k + "insum"] = np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()])
        print(k, fx[k + "loss4"], "max|dpred|", fx[k + "dmax"], "stored", idx.size)
    names = []
    for name, (pred, clean, lo, hi) in iq_cases().items():
        cf = clean.astype(np.float32)  # the reference reads its images as float32
        ious = ev["compute_iq_iou"](pred, cf, lo, hi)
        t1, t2 = np.quantile(ev["_to_gray_float01"](cf), [lo, hi])
        gp, gc = ev["_to_gray_float01"](pred), ev["_to_gray_float01"](cf)
        lp, lc = ev["_quantize_3class"](gp, t1, t2), ev["_quantize_3class"](gc, t1, t2)
        counts = np.array([((lp == c) & (lc == c)).sum() for c in range(3)]
                          + [((lp == c) | (lc == c)).sum() for c in range(3)], np.int64)
        for c in range(3):  # the counts are the reference's own ratios
            want = counts[c] / counts[3 + c] if counts[3 + c] else np.nan
            assert (np.isnan(want) and np.isnan(ious[c])) or want == ious[c], (name, c)
        if name != "c1_7x9_nomid":
            assert (gc == t1).any() and (gc == t2).any(), (name, t1, t2)
        else:
            assert np.isnan(ious[1])
        k = f"iq_{name}_"
        fx[k + "pred"], fx[k + "clean"] = pred, clean
        fx[k + "q"] = np.array([lo, hi])
        fx[k + "t"] = np.array([t1, t2], np.float64)
        fx[k + "ious"] = np.array(ious, np.float64)
        fx[k + "counts"] = counts
        names.append(name)
        print(k, "t", t1, t2, "ious", ious, "counts", counts)
    fx["iq_names"] = np.array(names)
    path = os.path.join(OUT, "iqsl.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
