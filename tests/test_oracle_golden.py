"""The CPU oracle pinned against fixtures produced by the reference itself
(tests/golden/make_golden.py).  No GPU needed."""
import numpy as np
import pytest
import torch

from oracle import n2n_ref, philox, unet_ref


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- Philox known-answer vectors (Random123 kat_vectors, philox4x32_10) -----------------
@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_kat(ctr, key, expect):
    out = philox.philox4x32_10(*[np.array([c], np.uint32) for c in ctr], *key)
    assert tuple(int(o[0]) for o in out) == expect


def test_philox_rd_is_uniform_and_indexed_globally():
    rd = philox.rd_idx(7, 3, 1 << 16)
    counts = np.bincount(rd, minlength=8)
    assert counts.min() > 0.9 * (1 << 13) and counts.max() < 1.1 * (1 << 13)
    # sharding invariance: a rank's slice equals the slice of the global stream
    assert np.array_equal(philox.rd_idx(7, 3, 1000, cell_base=5000), rd[5000:6000])
    z = philox.normal(1, 0, np.arange(1 << 16, dtype=np.uint64))
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02


# ---- sub-sampler --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_subsampler_literal_and_closed_form(golden, case):
    g = golden("subsampler.npz")
    img, rd = g[f"{case}_img"], g[f"{case}_rd"]
    m1, m2 = n2n_ref.masks_from_rd(rd)
    if case == "a":
        assert np.array_equal(m1, g["a_mask1"]) and np.array_equal(m2, g["a_mask2"])
    s1 = n2n_ref.generate_subimages(img, m1)
    s2 = n2n_ref.generate_subimages(img, m2)
    assert np.array_equal(s1, g[f"{case}_sub1"]) and np.array_equal(s2, g[f"{case}_sub2"])
    c1, c2 = n2n_ref.subimages_closed_form(img, rd)
    assert np.array_equal(c1, s1) and np.array_equal(c2, s2)


def test_masks_one_hot_and_distinct(golden):
    rd = golden("subsampler.npz")["b_rd"]
    m1, m2 = n2n_ref.masks_from_rd(rd)
    assert (m1.reshape(-1, 4).sum(1) == 1).all() and (m2.reshape(-1, 4).sum(1) == 1).all()
    assert not (m1 & m2).any()


# ---- U-Net init / forward / backward -------------------------------------------------------
# (in_nc, fixture): the reference's two usual channel counts (out_nc = in_nc), then in_nc 2 and 4,
# out_nc above 4 and in_nc != out_nc (make_golden.py unet_pairs_main: unet_c<in_nc>_<out_nc>.npz);
# out_nc is the fixture output's channel count
UNET_FIXTURES = [(1, "unet_c1.npz"), (3, "unet_c3.npz"), (2, "unet_c2_2.npz"),
                 (4, "unet_c4_16.npz"), (3, "unet_c3_1.npz")]


@pytest.mark.parametrize("C,name", UNET_FIXTURES)
def test_reference_init_matches(golden, C, name):
    import hashlib

    from image_denoising_amd.arch_unet import reference_init

    g = golden(name)
    torch.manual_seed(0)
    flat = reference_init(C, g["y"].shape[1], 48).numpy()
    assert hashlib.sha256(flat.tobytes()).hexdigest() == str(g["params_sha"])


@pytest.mark.parametrize("C,name", UNET_FIXTURES)
def test_oracle_unet_forward_backward(golden, C, name):
    from image_denoising_amd.arch_unet import reference_init

    g = golden(name)
    OC = g["y"].shape[1]
    assert name in ("unet_c1.npz", "unet_c3.npz") or name == f"unet_c{C}_{OC}.npz"
    torch.manual_seed(0)
    flat = reference_init(C, OC, 48)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    p = flat.clone().requires_grad_(True)
    y = unet_ref.forward(p, x, C, OC)
    assert y.shape == (x.shape[0], OC) + x.shape[2:]
    assert rel_err(y.detach().numpy(), g["y"]) < 1e-5
    (y ** 2).mean().backward()
    assert rel_err(x.grad.numpy(), g["dx"]) < 1e-4  # dL/dx of the reference module
    grad = p.grad.numpy()
    if "grad" in g:
        assert rel_err(grad, g["grad"]) < 1e-4
    else:
        assert rel_err(grad[g["grad_idx"]], g["grad_sample"]) < 1e-4
    # per-parameter norms
    norms, off = [], 0
    for _, ws, bl, _ in unet_ref.layer_table(C, OC):
        n = int(np.prod(ws))
        norms += [np.linalg.norm(grad[off:off + n]), np.linalg.norm(grad[off + n:off + n + bl])]
        off += n + bl
    assert rel_err(norms, g["grad_norms"]) < 1e-4


def test_oracle_n2n_step(golden):
    from image_denoising_amd.arch_unet import reference_init

    g = golden("n2n_step.npz")
    torch.manual_seed(0)
    flat = reference_init(1, 1, 48)
    r = unet_ref.n2n_step(flat, torch.from_numpy(g["noisy"]), g["rd"], float(g["lam"]))
    assert abs(r["loss1"] - float(g["loss1"])) <= 1e-5 * abs(float(g["loss1"]))
    assert abs(r["loss2"] - float(g["loss2"])) <= 1e-4 * abs(float(g["loss2"])) + 1e-12
    assert rel_err(r["dout"], g["dout"]) < 1e-4
    grad = r["grad"].numpy()
    assert rel_err(grad[g["grad_idx"]], g["grad_sample"]) < 1e-4
    post = r["params"].numpy()
    assert np.abs(post[g["post_idx"]] - g["post_sample"]).max() < 1e-6


def test_oracle_structure_loss(golden):
    g = golden("structure_loss.npz")
    loss, dp, dp2, _ = n2n_ref.structure_loss(g["pred"], g["pred2"], g["target"])
    assert abs(loss - float(g["loss"])) < 1e-6
    assert rel_err(dp, g["dpred"]) < 1e-6 and rel_err(dp2, g["dpred2"]) < 1e-6
