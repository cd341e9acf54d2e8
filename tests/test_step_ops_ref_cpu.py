"""Anchors of the references tests/test_gpu_step_ops.py compares the HIP kernels with.  No GPU.

* oracle.philox at the stream positions the GPU tests use (odd and > 2^32 bases, lam = 500, clean
  <= 0) against a scalar restatement in Python integers and an independent Poisson CDF;
* step_ops_ref's fp64 N2N / structure losses against the reference program's own fixtures
  (tests/golden/n2n_step.npz, structure_loss.npz), inside the bounds the GPU tests use;
* the max-pool edge input really holds the edge values it promises.
"""
import math

import numpy as np
import pytest

import step_ops_ref as R
from oracle import n2n_ref, philox


# ---- Philox, restated with Python integers (no numpy in the arithmetic) ---------------------
def _philox_int(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _block(seed, offset, blk):
    return _philox_int((blk & 0xFFFFFFFF, blk >> 32, offset & 0xFFFFFFFF, offset >> 32),
                       (seed & 0xFFFFFFFF, seed >> 32))


def _uniform53_int(seed, offset, q):
    o = _block(seed, offset, q >> 1)
    p = q & 1
    return ((o[2 * p] >> 5) * 67108864 + (o[2 * p + 1] >> 6) + 0.5) / 9007199254740992.0


def _normal_int(seed, offset, q):
    o = _block(seed, offset, q >> 2)
    p = (q >> 1) & 1
    u1 = ((o[2 * p] >> 8) + 1.0) / 16777216.0
    u2 = (o[2 * p + 1] >> 8) / 16777216.0
    r, th = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
    return r * math.sin(th) if q & 1 else r * math.cos(th)


BASES = [0, 1, 6, 7, 8, 2 ** 33 + 1, 2 ** 34 + 4, 2 ** 34 + 6]


@pytest.mark.parametrize("base", BASES)
def test_philox_streams_at_the_bases_the_gpu_tests_use(base):
    """the high counter word (blk >> 32) is non-zero from 2^33 (uniform53) / 2^34 (the others)"""
    q = np.arange(base, base + 13, dtype=np.uint64)
    u = philox.uniform53(5, 2 ** 32 + 9, q)
    z = philox.normal(5, 2 ** 32 + 9, q)
    c = philox.cell_u32(5, 2 ** 32 + 9, q)
    for i in range(13):
        assert u[i] == _uniform53_int(5, 2 ** 32 + 9, base + i)
        assert abs(z[i] - _normal_int(5, 2 ** 32 + 9, base + i)) <= 1e-15 * max(1.0, abs(z[i]))
        assert int(c[i]) == _block(5, 2 ** 32 + 9, (base + i) >> 2)[(base + i) & 3]
    assert np.array_equal(philox.rd_idx(5, 2 ** 32 + 9, 13, cell_base=base), (c & 7).astype(np.uint8))
    if base >= 2 ** 33:  # and the high word matters: the same low word alone draws other values
        assert not np.array_equal(u, philox.uniform53(5, 2 ** 32 + 9, q & np.uint64(0xFFFFFFFF)))


def _poisson_cdf(mu, k):
    """sum_{j<=k} exp(j ln mu - mu - lgamma(j + 1)), independent of the oracle's recurrence"""
    if k < 0:
        return 0.0
    return math.fsum(math.exp(j * math.log(mu) - mu - math.lgamma(j + 1)) for j in range(k + 1))


@pytest.mark.parametrize("lam", [500.0, 5.0])
@pytest.mark.parametrize("base", [1, 7, 2 ** 33 + 1])
def test_poisson_oracle_inverts_the_cdf(lam, base):
    """k = min{k : u <= F(k)} at mu up to the 500 cap (exp(-500) = 7e-218 is a normal fp64
    number, so the recurrence starts), clean = 0 and clean < 0 give 0, and a rank's slice of
    the stream is the stream's slice"""
    rng = np.random.default_rng(3)
    clean = rng.random(96).astype(np.float32)
    clean[:4] = [0.0, -0.25, 1.0, 1.0]
    out = philox.poisson_noise(clean, lam, seed=21, offset=3, elem_base=base)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    assert out[0] == 0.0 and out[1] == 0.0
    u = philox.uniform53(21, 3, np.arange(base, base + 96, dtype=np.uint64))
    for i in range(2, 96):
        mu = float(np.float32(lam) * clean[i])
        k = int(round(float(out[i]) * lam))
        assert np.float32(k) / np.float32(lam) == out[i]
        # u in (F(k-1), F(k)], up to the two CDFs' own rounding
        assert _poisson_cdf(mu, k) >= u[i] - 1e-12 and _poisson_cdf(mu, k - 1) <= u[i] + 1e-12, (i, mu, k)
    sl = philox.poisson_noise(clean[5:], lam, seed=21, offset=3, elem_base=base + 5)
    assert np.array_equal(sl, out[5:])


def test_poisson_oracle_per_image_lam():
    clean = np.random.default_rng(4).random((2, 1, 3, 5)).astype(np.float32)
    lam = np.array([30.0, 50.0], np.float32)
    both = philox.poisson_noise(clean, lam, seed=1, offset=2, elem_base=7)
    assert np.array_equal(both[0], philox.poisson_noise(clean[0], 30.0, 1, 2, elem_base=7))
    assert np.array_equal(both[1], philox.poisson_noise(clean[1], 50.0, 1, 2, elem_base=7 + 15))


# ---- the fp64 losses against the reference program's fixtures -----------------------------
def test_n2n_loss_ref_reproduces_the_reference_fixture(golden):
    """n2n_step.npz holds the reference's fp32 loss1 / loss2 / loss / dout.  An fp32 program is
    itself inside the rounding model of step_ops_ref, so the fp64 reference must reproduce it
    within the bounds the GPU test gives the kernel."""
    g = golden("n2n_step.npz")
    _, sub2 = n2n_ref.subimages_closed_form(g["noisy"], g["rd"])
    r = R.n2n_loss_ref(g["out"], sub2, g["den"], g["rd"], float(g["lam"]))
    for k in ("loss1", "loss2", "loss"):
        err = abs(float(g[k]) - r[k])
        print(k, "err", err, "bound", r["b_" + k])
        assert err <= r["b_" + k], k
    err = np.abs(g["dout"].astype(np.float64) - r["dout"])
    print("dout worst err/bound", float((err / r["b_dout"]).max()))
    assert (err <= r["b_dout"]).all()
    # and it is the same function as the fp32 torch restatement the older tests use
    t = n2n_ref.n2n_loss(g["out"], sub2, g["den"], g["rd"], float(g["lam"]))
    assert abs(t[0] - r["loss1"]) <= r["b_loss1"] and abs(t[1] - r["loss2"]) <= r["b_loss2"]


@pytest.mark.parametrize("lam", [0.0, 1.0, 2.0])
def test_n2n_loss_ref_against_torch_at_three_channels(lam):
    """C = 3 and all eight rd values: the n, c, i, j decomposition of the fp64 reference against
    autograd on the literal (unfold, mask, gather) restatement"""
    rng = np.random.default_rng(11)
    out = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    sub2 = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    den = rng.standard_normal((2, 3, 10, 14)).astype(np.float32)
    rd = (np.arange(70) % 8).astype(np.uint8)
    r = R.n2n_loss_ref(out, sub2, den, rd, lam)
    t = n2n_ref.n2n_loss(out, sub2, den, rd, lam)
    assert abs(t[0] - r["loss1"]) <= 1e-6 * r["loss1"]
    assert abs(t[1] - r["loss2"]) <= 1e-6 * r["loss2"] + (0.0 if lam else 1e-30)
    assert np.abs(t[3] - r["dout"]).max() <= 1e-6 * np.abs(r["dout"]).max()
    assert (r["b_dout"] > 0).all() and r["b_loss1"] < 1e-6 * r["loss1"]


def test_structure_loss_ref_reproduces_the_reference_fixture(golden):
    """structure_loss.npz: the reference's fp32 loss and both gradients.  M = 512 is a power of
    two, so its dpred is exact; its dpred2 is an fp32 sum of the same five terms."""
    g = golden("structure_loss.npz")
    r = R.structure_loss_ref(g["pred"], g["pred2"], g["target"])
    # the existing oracle test's own number for this fixture (test_oracle_structure_loss)
    assert abs(float(g["loss"]) - r["parts"][4]) < 1e-6
    assert np.array_equal(g["dpred"], r["dpred"])
    err = np.abs(g["dpred2"].astype(np.float64) - r["dpred2"])
    assert (err <= r["b_dpred2"]).all(), float((err / np.maximum(r["b_dpred2"], 1e-300)).max())
    _, dp, dp2, parts = n2n_ref.structure_loss(g["pred"], g["pred2"], g["target"])
    assert np.abs(np.array(parts) - r["parts"]).max() < 1e-6


def test_structure_loss_ref_ties_and_channels():
    """quantised inputs tie often; the sign of a tie is 0 as torch.sign gives, C = 3"""
    rng = np.random.default_rng(12)
    q = lambda: (rng.integers(-4, 5, (2, 3, 5, 7)) / 8.0).astype(np.float32)  # noqa: E731
    pred, pred2, tgt = q(), q(), q()
    assert (pred == tgt).any() and (pred2[:, :, 1:] == pred2[:, :, :-1]).any()
    r = R.structure_loss_ref(pred, pred2, tgt)
    _, dp, dp2, parts = n2n_ref.structure_loss(pred, pred2, tgt)
    assert (r["dpred"][pred == tgt] == 0).all()
    assert np.abs(dp - r["dpred"]).max() <= 2 * R.U * np.abs(r["dpred"]).max()
    assert (np.abs(dp2 - r["dpred2"]) <= r["b_dpred2"] + 1e-12).all()
    assert np.abs(np.array(parts) - r["parts"]).max() < 1e-6


def test_l1_batched_ref():
    rng = np.random.default_rng(13)
    a, b = rng.random((3, 1027)).astype(np.float32), rng.random((3, 1027)).astype(np.float32)
    ref = R.l1_batched_ref(a, b)
    assert np.allclose(ref, np.abs(a.astype(np.float64) - b).mean(1), rtol=1e-13, atol=0)


def test_pool_edge_input_holds_its_edges():
    import torch
    import torch.nn.functional as F

    x = R.pool_edge_input(2, 8, 6, 10, seed=5)
    w = x.reshape(2, 8, 3, 2, 5, 2).transpose(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    for s in range(4):
        assert np.isnan(w[s, s]) and np.isnan(w[s]).sum() == 1
    assert np.isnan(w[4]).sum() == 2 and np.isnan(w[5]).all()
    assert np.isneginf(w[6]).all() and np.isneginf(w[7]).sum() == 3
    assert (w[8] == 0.75).all() and (w[9] == 0).all() and w[10].max() == 0 and w[11].max() == 0
    y = F.max_pool2d(torch.from_numpy(x), 2).numpy().reshape(-1)
    assert np.isnan(y[:6]).all() and np.isneginf(y[6]) and np.isfinite(y[7]) and y[9] == 0
    small = R.pool_edge_input(1, 4, 2, 2, seed=6)
    assert np.isnan(small.reshape(4, 4)).sum(1).tolist() == [1, 1, 1, 1]
