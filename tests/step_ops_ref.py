"""fp64 references and a-priori rounding bounds for the training step's elementwise ops.

Shared by tests/test_gpu_step_ops.py (the HIP kernels against these) and
tests/test_step_ops_ref_cpu.py (these against the reference program's fixtures and against torch).
Every bound here is computed from the reference's own magnitudes with u = 2^-24, the unit
roundoff of fp32; nothing is fitted to a kernel's output.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import n2n_ref

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------
# N2N loss (training_script.md:141-153): loss1 = mean(diff^2), loss2 = lam mean((diff - ed)^2),
# diff = out - sub2, ed = den1 - den2 (the two sub-images of the no-grad output under the same rd).
#
# Rounding model of an fp32 implementation that forms diff, ed and q = diff - ed in fp32, sums the
# squares in fp64 and rounds each loss once to fp32 (first order in u, fp64 noise dropped):
#   diff~ = diff (1 + d1), ed~ = ed (1 + d2), |d| <= u, so
#   q~ = (diff~ - ed~)(1 + d3)  =>  |q~ - q| <= u (|diff| + |ed| + |q|)            =: q_err
#   loss1: each square moves by 2 |diff| u |diff|; the mean is rounded once to fp32:
#          (sum 2 |diff| u |diff|) / M + u loss1
#   loss2: each square moves by 2 |q| q_err; the mean is rounded once and multiplied by lam once:
#          lam (sum 2 |q| q_err) / M + 2 u loss2
#   loss : the fp32 sum of the two: b1 + b2 + u loss
#   dout = invM (2 diff) + lamM (2 q), invM = fl(1 / fl(M)), lamM = fl(lam / fl(M)): the first
#          product carries u from invM, u from diff~ and u of its own (3 u invM 2 |diff|); the second
#          u from lamM, q_err from q~ and u of its own (lamM 2 (q_err + 2 u |q|)); the final add
#          another u of the sum.  Both are below 4 u of their magnitude terms:
#          4 u (invM 2 |diff| + lamM 2 (|diff| + |ed| + |q|))
# The tests allow twice each bound because the bounds are first order.
# ---------------------------------------------------------------------------------------------
def n2n_loss_ref(out, sub2, den, rd, lam):
    """fp64 from the fp32 inputs.  Returns a dict: loss1, loss2, loss, dout and the bounds b_*
    (already doubled)."""
    out64 = np.asarray(out, dtype=np.float32).astype(np.float64)
    sub64 = np.asarray(sub2, dtype=np.float32).astype(np.float64)
    den64 = np.asarray(den, dtype=np.float32).astype(np.float64)
    lam = float(np.float32(lam))
    d1, d2 = n2n_ref.subimages_closed_form(den64, rd)
    diff = out64 - sub64
    ed = d1 - d2
    q = diff - ed
    M = float(diff.size)
    loss1 = float((diff * diff).sum() / M)
    loss2 = float(lam * (q * q).sum() / M)
    loss = loss1 + loss2
    a_diff, a_ed, a_q = np.abs(diff), np.abs(ed), np.abs(q)
    q_err = U * (a_diff + a_ed + a_q)
    b1 = float((2.0 * a_diff * U * a_diff).sum() / M + U * loss1)
    b2 = float(lam * (2.0 * a_q * q_err).sum() / M + 2.0 * U * loss2)
    b = b1 + b2 + U * loss
    invM, lamM = 1.0 / M, lam / M
    dout = invM * 2.0 * diff + lamM * 2.0 * q
    b_dout = 4.0 * U * (invM * 2.0 * a_diff + lamM * 2.0 * (a_diff + a_ed + a_q))
    return dict(loss1=loss1, loss2=loss2, loss=loss, dout=dout, b_loss1=2.0 * b1, b_loss2=2.0 * b2,
                b_loss=2.0 * b, b_dout=2.0 * b_dout)


# ---------------------------------------------------------------------------------------------
# Structure loss (util.py:56-70): alpha L1(pred, t) + beta (tv1 + tv2) / 2 + gamma L1(pred2, t),
# tv1 / tv2 the L1 of pred2's vertical / horizontal neighbour differences.
#
#   dpred  = fl(alpha / fl(M)) sign(pred - t): one coefficient times 0 or +-1, so it is exact and
#            the test compares bits (sign of a tie is 0, as torch.sign gives)
#   dpred2 = up to five terms coefficient * sign: gc s(p2 - t), -gtv1 s(down - p2),
#            +gtv1 s(p2 - up), -gtv2 s(right - p2), +gtv2 s(p2 - left).  Against the exact
#            coefficients each fp32 coefficient is off by u (M, M1, M2 < 2^24 are exact in fp32;
#            beta / 2 is exact) and each of the four additions adds u of a partial sum that is at
#            most sum |term|:  5 u sum |term|
#   parts  : fp64 sums (noise ~ M 2^-53, dropped) divided in fp64 and rounded once to fp32 = u;
#            the tests allow 2 u relative each
#   total  : alpha pix + beta (tv1 + tv2) / 2 + gamma cst within the same combination of the
#            parts' bounds
# ---------------------------------------------------------------------------------------------
def _sign(x):
    return np.sign(x)  # 0 at a tie


def structure_loss_ref(pred, pred2, target, alpha=1.0, beta=0.5, gamma=0.5):
    p = np.asarray(pred, dtype=np.float32).astype(np.float64)
    p2 = np.asarray(pred2, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    N, C, H, W = p.shape
    M, M1, M2 = float(N * C * H * W), float(N * C * (H - 1) * W), float(N * C * H * (W - 1))
    dv = p2[:, :, 1:, :] - p2[:, :, :-1, :]
    dh = p2[:, :, :, 1:] - p2[:, :, :, :-1]
    pix = float(np.abs(p - t).sum() / M)
    tv1 = float(np.abs(dv).sum() / M1)
    tv2 = float(np.abs(dh).sum() / M2)
    cst = float(np.abs(p2 - t).sum() / M)
    total = alpha * pix + beta * (tv1 + tv2) / 2.0 + gamma * cst
    parts = np.array([pix, tv1, tv2, cst, total])
    b_parts = 2.0 * U * parts[:4]
    b_total = alpha * b_parts[0] + beta * (b_parts[1] + b_parts[2]) / 2.0 + gamma * b_parts[3]
    # dpred: the fp32 coefficient, exactly
    ga = np.float32(np.float32(alpha) / np.float32(M))
    dpred = (ga * _sign(p - t).astype(np.float32)).astype(np.float32)
    gc, g1, g2 = gamma / M, (beta / 2.0) / M1, (beta / 2.0) / M2
    terms = np.zeros((5,) + p.shape)
    terms[0] = gc * _sign(p2 - t)
    terms[1][:, :, :-1, :] = -g1 * _sign(dv)
    terms[2][:, :, 1:, :] = g1 * _sign(dv)
    terms[3][:, :, :, :-1] = -g2 * _sign(dh)
    terms[4][:, :, :, 1:] = g2 * _sign(dh)
    dpred2 = terms.sum(0)
    b_dpred2 = 5.0 * U * np.abs(terms).sum(0)
    return dict(parts=parts, b_parts=np.append(b_parts, b_total), dpred=dpred, dpred2=dpred2,
                b_dpred2=b_dpred2)


# ---------------------------------------------------------------------------------------------
# batched L1: mean |a_p - b_p| per item.  math.fsum is exact up to the final rounding.
# ---------------------------------------------------------------------------------------------
def l1_batched_ref(a, b):
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    return np.array([math.fsum(np.abs(x - y).tolist()) / x.size for x, y in zip(a, b)])


# ---------------------------------------------------------------------------------------------
# max-pool 2x2 inputs with the edge values ATen's kernel is specified on
# ---------------------------------------------------------------------------------------------
def pool_edge_input(N, C, H, W, seed):
    """randn [N,C,H,W] whose first windows (row-major over n, c, y2, x2) carry, in turn: NaN in
    window slot 0, 1, 2, 3 (TL, TR, BL, BR); NaN in slots 1 and 2; NaN in all four; all -inf;
    -inf in three slots; all-equal values; exact zeros (one window all zero, one with zero as the
    maximum).  Cycled until the windows run out, so a one-window-per-channel shape gets the first
    kinds."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    nan, ninf = np.float32("nan"), np.float32("-inf")
    kinds = [
        (nan, None, None, None), (None, nan, None, None), (None, None, nan, None),
        (None, None, None, nan), (None, nan, nan, None), (nan, nan, nan, nan),
        (ninf, ninf, ninf, ninf), (ninf, ninf, None, ninf), (0.75, 0.75, 0.75, 0.75),
        (0.0, 0.0, 0.0, 0.0), (-1.0, 0.0, -0.5, 0.0), (0.0, -2.0, -3.0, -1.0),
    ]
    w = x.reshape(N, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(-1, 4).copy()
    for i in range(min(len(w), 2 * len(kinds))):
        for s, v in enumerate(kinds[i % len(kinds)]):
            if v is not None:
                w[i, s] = v
    return np.ascontiguousarray(
        w.reshape(N, C, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H, W))
