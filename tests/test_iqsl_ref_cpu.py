"""tests/iqsl_ref.py (the fp64 restatement of the IQSL finetune loss the GPU tests compare the HIP
kernels with) against the reference program's fixture and against torch fp64 autograd of the same
formula, plus the input conditions every case must meet.  No GPU needed."""
import numpy as np
import pytest
import torch

import iqsl_ref as R

TOL = 1e-4  # the standing per-output tolerance against the reference program


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.fixture(scope="module")
def totals():
    cache = {}

    def get(case, shape):
        if (case, shape) not in cache:
            cache[(case, shape)] = R.case_total(case, shape)
        return cache[(case, shape)]

    return get


@pytest.mark.parametrize("case,shape", R.PAIRS)
def test_inputs_are_the_fixtures_and_meet_the_conditions(golden, case, shape):
    """the generator's inputs are the ones this file builds; every |z - c_k| >= 1e-4; no
    pred - target and no neighbour difference is exactly 0 except the placed tie"""
    g = golden("iqsl.npz")
    pred, target = R.case_inputs(case, shape)
    assert pred.shape == target.shape == R.SHAPES[shape] and pred.dtype == np.float32
    sums = np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()])
    assert np.array_equal(sums, g[f"{case}_{shape}_insum"])
    tau, margin, _ = R.CASES[case]
    a = R.scalars(R.T1, R.T2, tau, margin)
    for ck in a["c"]:
        assert np.abs(pred.astype(np.float64) - ck).min() >= 1e-4
    ties = np.flatnonzero(pred.reshape(-1) == target.reshape(-1))
    assert list(ties) == R.placed_ties(case)
    dx = (pred[..., 1:] - pred[..., :-1]) - (target[..., 1:] - target[..., :-1])
    dy = (pred[:, :, 1:] - pred[:, :, :-1]) - (target[:, :, 1:] - target[:, :, :-1])
    assert (dx != 0).all() and (dy != 0).all()
    y = target.reshape(-1)
    if case == "eq":
        assert (y == np.float32(R.T1)).any() and (y == np.float32(R.T2)).any()
        assert float(np.float32(R.T1)) != R.T1 and float(np.float32(R.T2)) != R.T2
    if case == "m05":
        assert all((y == np.float32(a[k])).any() for k in ("t1_lo", "t1_hi", "t2_lo", "t2_hi"))
    if case == "nobright":
        assert not (y >= np.float32(R.T2)).any() and (y <= np.float32(R.T1)).any()
    if case == "tauclamp":
        d = np.sort(np.abs(pred.reshape(-1, 1).astype(np.float64) - a["c"]), axis=1)
        assert (d[:, 1] - d[:, 0]).min() >= 1e-3 and a["tau"] == 1e-6


@pytest.mark.parametrize("case,shape", R.PAIRS)
def test_restatement_vs_reference_fixture(golden, totals, case, shape):
    g = golden("iqsl.npz")
    k = f"{case}_{shape}_"
    _, _, r = totals(case, shape)
    for i, name in enumerate(("l1", "grad", "iqsl", "loss")):
        want = float(g[k + "loss4"][i])
        print(name, r["loss4"][i], want)
        if want == 0.0:
            assert r["loss4"][i] == 0.0, name
        else:
            assert _rel(r["loss4"][i], want) < TOL, name
    got = r["dpred"].reshape(-1)[g[k + "idx"]]
    dmax = float(g[k + "dmax"])
    assert _rel(np.abs(r["dpred"]).max(), dmax) < TOL
    err = np.abs(got - g[k + "dpred"]).max()
    print("dpred err / max", err / dmax)
    assert err <= TOL * dmax


@pytest.mark.parametrize("case,shape", R.PAIRS)
def test_restatement_vs_torch_fp64_autograd(totals, case, shape):
    """the same formula written with torch ops in fp64 (z - c_k keeps its fp32 value through a
    detached correction) and differentiated by autograd: loss and gradient at 1e-10"""
    tau, margin, cef = R.CASES[case]
    pred, target = R.case_inputs(case, shape)
    a = R.scalars(R.T1, R.T2, tau, margin)
    z = torch.from_numpy(pred[:, 0].astype(np.float64)).requires_grad_(True)
    y = torch.from_numpy(target[:, 0])
    f = lambda k: torch.tensor(a[k], dtype=torch.float32)  # noqa: E731
    if a["use_margin"]:
        v = (y <= f("t1_lo")) | ((y >= f("t1_hi")) & (y <= f("t2_lo"))) | (y >= f("t2_hi"))
    else:
        v = torch.ones_like(y, dtype=torch.bool)
    v = v.double()
    m = torch.stack([y <= f("t1"), (y > f("t1")) & (y < f("t2")), y >= f("t2")]).double() * v
    c = torch.tensor(a["c"], dtype=torch.float64).view(3, 1, 1, 1)
    d32 = torch.from_numpy(np.stack([(pred[:, 0] - np.float32(ck)).astype(np.float64)
                                     for ck in a["c"]]))
    diff = z - c
    diff = diff + (d32 - diff).detach()
    q = torch.softmax(-diff.abs() / a["tau"], dim=0) * v
    inter, ps, ts = (q * m).sum(dim=(1, 2, 3)), q.sum(dim=(1, 2, 3)), m.sum(dim=(1, 2, 3))
    dice = (2.0 * inter + R.EPS) / (ps + ts + R.EPS)
    ce = -(m * torch.log(q + R.EPS)).sum() / (3.0 * v.sum() + R.EPS)
    loss = (1.0 - dice.mean()) + cef * ce
    loss.backward()
    r = R.iqsl(pred[:, 0], target[:, 0], R.T1, R.T2, tau, margin, cef)
    assert abs(r["loss"] - loss.item()) <= 1e-10 * max(abs(loss.item()), 1e-30) or \
        (loss.item() == 0.0 and r["loss"] == 0.0)
    gmax = float(z.grad.abs().max())
    err = float(np.abs(r["dz"] - z.grad.numpy()).max())
    print("loss", r["loss"], "grad max", gmax, "err", err)
    assert err <= 1e-10 * max(gmax, 1e-30) or (gmax == 0.0 and err == 0.0)
    if case == "inmargin":
        assert r["loss"] == 0.0 and not r["dz"].any() and r["sums"]["V"] == 0.0
    if case == "nobright":
        assert r["sums"]["T"][2] == 0.0 and r["sums"]["P"][2] > 0.0
    # the bounds the GPU test will use are far below the fixture tolerance
    _, _, tot = totals(case, shape)
    assert (tot["b_loss4"] <= 1e-5 * np.maximum(np.abs(tot["loss4"]), 1e-3)).all()


@pytest.mark.parametrize("name", ["c1_7x9", "c3_7x9", "c1_64x80", "c3_64x80", "c1_7x9_nomid"])
def test_iq_counts_restatement_vs_fixture(golden, name):
    g = golden("iqsl.npz")
    assert name in list(g["iq_names"])
    k = f"iq_{name}_"
    t1, t2 = g[k + "t"]
    counts = R.iq_counts(g[k + "pred"], g[k + "clean"], t1, t2)
    assert np.array_equal(counts, g[k + "counts"])
    gray = g[k + "clean"].astype(np.float32)
    gray = (gray.mean(axis=2) if gray.ndim == 3 else gray) / 255.0
    assert np.array_equal(np.quantile(gray, g[k + "q"]), g[k + "t"])
    if name == "c1_7x9_nomid":
        assert counts[4] == 0 and np.isnan(g[k + "ious"][1])
    else:
        assert (gray == t1).any() and (gray == t2).any()
