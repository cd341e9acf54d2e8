"""fp64 restatement of the IQSL finetune loss with its analytic gradient, a-priori
rounding bounds for an implementation that follows the kernels' arithmetic contract, and the
deterministic inputs of the test cases.

Shared by tests/test_iqsl_ref_cpu.py (this file against the reference program's fixture and against
torch fp64 autograd), tests/test_gpu_iqsl.py (the HIP kernels against this file) and
tests/golden/make_golden_iqsl.py (which feeds the same inputs to the reference program).

Arithmetic contract (include/denoise_hip.h, dn_finetune_iqsl_loss): the six comparison values
(t1, t2, t1 -+ margin, t2 -+ margin) and the three centres are formed in double and rounded once
to fp32; compares and z - c_k are fp32; everything after that is fp64; the L1 / gradient-L1 part
is dn_finetune_loss's (fp32 differences and coefficients, fp64 sums).  This file does exactly the
same up to the order of fp64 operations, so the bounds below hold only the roundings to fp32 of
the outputs, the fp32 coefficient arithmetic of the L1 part, and a term for fp64 noise.  With
u = 2^-24 and n64 = M 2^-52 (M fp64 additions, doubled for the exp / log / divisions):

  loss_l1   one fp32 rounding of an fp64 mean:                     u l1
  loss_grad two means rounded, one fp32 add:                       2 u lg
  loss_iqsl one rounding; L_dice = 1 - mean dice and the CE sum
            carry the fp64 noise at their own scale:               u |iqsl| + n64 (1 + cef |ce|)
  loss      fl(fl(l1 + lam lg) + fl(lam_iq iq)):                   b_l1 + lam b_lg + lam_iq b_iq
                                                                   + 4 u (l1 + lam lg + lam_iq |iq|)
  dpred     L1 part: up to five terms coefficient * sign; each coefficient fl(lam / fl(M')) is off
            by at most 2 u, four additions add u of a partial sum <= sum |term|: 6 u sum |term|.
            IQSL part h = fl(lam_iq g): u |h| + lam_iq n64 G, G = sum_k |a_k| p_k (|s_k| + |r|)
            the magnitude the cancelling sum g is formed from.  The final add: u (sum |term| + |h|).
The tests allow twice each bound because the bounds are first order (as tests/step_ops_ref.py).
Nothing here is fitted to a kernel's output.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EPS = 1e-6
T1, T2 = 75.0 / 255.0, 180.0 / 255.0  # not fp32 numbers: the rounding of the thresholds matters
LAMBDA_GRAD, LAMBDA_IQSL = 0.1, 0.1

SHAPES = {"small": (2, 1, 5, 7), "mid": (3, 1, 33, 65), "big": (5, 1, 240, 250)}
# name: (tau, margin, ce_factor)
CASES = {
    "m0": (0.1, 0.0, 0.5),          # margin = 0: every pixel valid
    "m05": (0.1, 0.05, 0.5),        # margin = 0.05, targets exactly on the four margin edges
    "eq": (0.1, 0.0, 0.5),          # targets exactly fp32(t1) and fp32(t2); one pred == target tie
    "nobright": (0.1, 0.0, 0.5),    # no target >= t2: T_2 = 0
    "inmargin": (0.1, 0.3, 0.5),    # every target inside a margin: V = 0, iqsl = 0, d iqsl = 0
    "tauclamp": (1e-7, 0.0, 0.5),   # tau below 1e-6 is clamped to 1e-6: the softmax saturates
}
# the (case, shape) pairs the fixture and the tests cover; big only where it adds a path: the
# second trip of both grid-stride loops (300000 > 262144 elements), with and without a margin
PAIRS = [(c, s) for s in ("small", "mid") for c in CASES] + [("m0", "big"), ("m05", "big")]


def f32(x) -> float:
    return float(np.float32(x))


def scalars(t1, t2, tau, margin):
    """the fp32-rounded comparison values and centres, as Python floats, and the clamped tau"""
    return dict(t1=f32(t1), t2=f32(t2), t1_lo=f32(t1 - margin), t1_hi=f32(t1 + margin),
                t2_lo=f32(t2 - margin), t2_hi=f32(t2 + margin),
                c=np.array([f32(t1 / 2.0), f32((t1 + t2) / 2.0), f32((t2 + 1.0) / 2.0)]),
                use_margin=margin > 0.0, tau=max(float(tau), 1e-6))


# ---------------------------------------------------------------------------------------------
# inputs: a counter-based generator (splitmix64 of the element index) so the arrays depend on
# nothing but this file
# ---------------------------------------------------------------------------------------------
def uniform(n: int, seed: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000000)) \
            * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def case_inputs(case: str, shape_name: str):
    """-> (pred, target) fp32 [N,1,H,W], built so that every |z - c_k| >= 1e-4 and (tauclamp) the
    two nearest centres' distances differ by >= 1e-3"""
    tau, margin, _ = CASES[case]
    shape = SHAPES[shape_name]
    n = int(np.prod(shape))
    seed = 1 + 16 * list(CASES).index(case) + list(SHAPES).index(shape_name)
    y = uniform(n, seed)
    if case == "nobright":
        y = y * 0.65
    y = y.astype(np.float32)
    z = (y + 0.3 * (uniform(n, seed + 8) - 0.5)).astype(np.float32)
    a = scalars(T1, T2, tau, margin)
    if case == "eq":
        y[1::11] = np.float32(T1)
        y[2::13] = np.float32(T2)
    if case == "m05":
        for i, k in enumerate(("t1_lo", "t1_hi", "t2_lo", "t2_hi")):
            y[3 + i::17] = np.float32(a[k])
    # keep z off the centres (|.| is not differentiable there) and, for the saturated softmax,
    # off the midpoints between centres
    c = a["c"]
    gap = 1e-3 if case == "tauclamp" else 0.0
    for _ in range(4):
        for k in range(3):
            near = np.abs(z - np.float32(c[k])) < 2e-4
            z[near] = np.float32(c[k] + 4e-4)
        if gap:
            for m in ((c[0] + c[1]) / 2.0, (c[1] + c[2]) / 2.0):
                near = np.abs(z.astype(np.float64) - m) < gap
                z[near] = np.float32(m + 2.0 * gap)
    if case == "eq":
        y[0] = z[0]  # sgn(0) = 0 in the L1 term, on purpose
    return z.reshape(shape), y.reshape(shape)


def placed_ties(case: str):
    """flat indices where a case sets pred == target on purpose"""
    return [0] if case == "eq" else []


# ---------------------------------------------------------------------------------------------
# IQSL in fp64
# ---------------------------------------------------------------------------------------------
def pixel_terms(z, y, a):
    """valid v, one-hot m [3,...] (already times v), p [3,...], s [3,...] from fp32 z, y"""
    z = np.asarray(z, np.float32)
    y = np.asarray(y, np.float32)
    g = lambda k: np.float32(a[k])  # noqa: E731
    if a["use_margin"]:
        v = (y <= g("t1_lo")) | ((y >= g("t1_hi")) & (y <= g("t2_lo"))) | (y >= g("t2_hi"))
    else:
        v = np.ones(y.shape, bool)
    m = np.stack([y <= g("t1"), (y > g("t1")) & (y < g("t2")), y >= g("t2")]).astype(np.float64)
    m = m * v
    diff = np.stack([(z - np.float32(ck)).astype(np.float64) for ck in a["c"]])  # fp32 subtract
    logit = -np.abs(diff) / a["tau"]
    e = np.exp(logit - logit.max(axis=0))
    p = e / e.sum(axis=0)
    s = -np.sign(diff) / a["tau"]
    return v.astype(np.float64), m, p, s, diff


def iqsl(z, y, t1, t2, tau=0.1, margin=0.0, ce_factor=0.5):
    """-> dict(loss, dz, ce, G): the loss, d loss / dz, the CE term and the gradient's magnitude
    sum G (see the module docstring)"""
    a = scalars(t1, t2, tau, margin)
    v, m, p, s, _ = pixel_terms(z, y, a)
    q = p * v
    ax = tuple(range(1, q.ndim))
    I, P, T = (q * m).sum(axis=ax), q.sum(axis=ax), m.sum(axis=ax)
    S, V = (m * np.log(q + EPS)).sum(), v.sum()
    D, Nk, VV = P + T + EPS, 2.0 * I + EPS, 3.0 * V + EPS
    ce = -S / VV
    loss = (1.0 - (Nk / D).mean()) + ce_factor * ce
    bc = (slice(None),) + (None,) * (q.ndim - 1)
    ak = -(1.0 / 3.0) * (2.0 * m / D[bc] - (Nk / D ** 2)[bc]) - ce_factor * m / ((q + EPS) * VV)
    r = (p * s).sum(axis=0)
    dz = v * (ak * p * (s - r)).sum(axis=0)
    G = v * (np.abs(ak) * p * (np.abs(s) + np.abs(r))).sum(axis=0)
    return dict(loss=float(loss), dz=dz, ce=float(ce), G=G, sums=dict(I=I, P=P, T=T, S=S, V=V))


def total(pred, target, lambda_grad, lambda_iqsl, t1, t2, tau=0.1, margin=0.0, ce_factor=0.5):
    """L1 + lambda_grad * gradient_loss + lambda_iqsl * iqsl of [N,1,H,W] fp32 inputs.  Returns
    loss4 = [l1, lg, iqsl, loss], dpred, dpred_l1 (the part without IQSL) and the doubled bounds
    b_loss4, b_dpred."""
    p32, t32 = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    N, C, H, W = p32.shape
    lam, lam_iq = f32(lambda_grad), f32(lambda_iqsl)
    M, Mx, My = float(N * C * H * W), float(N * C * H * (W - 1)), float(N * C * (H - 1) * W)
    # the differences in fp32, as dn_finetune_loss forms them
    d0 = (p32 - t32).astype(np.float64)
    dx = ((p32[..., 1:] - p32[..., :-1]) - (t32[..., 1:] - t32[..., :-1])).astype(np.float64)
    dy = ((p32[:, :, 1:] - p32[:, :, :-1]) - (t32[:, :, 1:] - t32[:, :, :-1])).astype(np.float64)
    l1 = np.abs(d0).sum() / M
    lg = np.abs(dx).sum() / Mx + np.abs(dy).sum() / My
    terms = np.zeros((5,) + p32.shape)
    terms[0] = np.sign(d0) / M
    terms[1][..., :-1] = -lam / Mx * np.sign(dx)
    terms[2][..., 1:] = lam / Mx * np.sign(dx)
    terms[3][:, :, :-1] = -lam / My * np.sign(dy)
    terms[4][:, :, 1:] = lam / My * np.sign(dy)
    g_l1, mag_l1 = terms.sum(0), np.abs(terms).sum(0)
    q = iqsl(p32[:, 0], t32[:, 0], t1, t2, tau, margin, ce_factor)
    iq, h = q["loss"], lam_iq * q["dz"][:, None]
    loss = l1 + lam * lg + lam_iq * iq
    n64 = M * 2.0 ** -52
    b_l1, b_lg = U * l1, 2.0 * U * lg
    b_iq = U * abs(iq) + n64 * (1.0 + abs(ce_factor * q["ce"]))
    b_loss = b_l1 + lam * b_lg + lam_iq * b_iq + 4.0 * U * (l1 + lam * lg + lam_iq * abs(iq))
    b_dpred = 6.0 * U * mag_l1 + U * np.abs(h) + lam_iq * n64 * q["G"][:, None] \
        + U * (mag_l1 + np.abs(h))
    return dict(loss4=np.array([l1, lg, iq, loss]), dpred=g_l1 + h, dpred_l1=g_l1, dpred_iqsl=h,
                b_loss4=2.0 * np.array([b_l1, b_lg, b_iq, b_loss]), b_dpred=2.0 * b_dpred)


def case_total(case: str, shape_name: str, lambda_iqsl: float = LAMBDA_IQSL):
    tau, margin, cef = CASES[case]
    pred, target = case_inputs(case, shape_name)
    return pred, target, total(pred, target, LAMBDA_GRAD, lambda_iqsl, T1, T2, tau, margin, cef)


# ---------------------------------------------------------------------------------------------
# IQ-IoU: label counts in numpy, as evaluation_adapter_iqsl.py forms them
# ---------------------------------------------------------------------------------------------
def iq_counts(pred255, clean255, t1, t2):
    """[H,W] or [H,W,C] images -> int64 [6]: intersections, then unions, of classes 0..2"""
    def labels(img):
        g = np.asarray(img).astype(np.float32)
        if g.ndim == 3:
            g = g.mean(axis=2)
        g = g / 255.0
        lab = np.zeros(g.shape, np.int32)
        lab[(g > t1) & (g < t2)] = 1
        lab[g >= t2] = 2
        return lab

    lp, lc = labels(pred255), labels(clean255)
    return np.array([((lp == k) & (lc == k)).sum() for k in range(3)]
                    + [((lp == k) | (lc == k)).sum() for k in range(3)], np.int64)
