"""tests/memory_ref.py (the fp64 restatement of the memory-bank adapter path) against the reference
fixture tests/golden/memory_adapter.npz and torch's own autograd, and the host-side pieces of
image_denoising_amd.memory.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memory_ref as R

SMALL = [n for n in R.ADAPTER_CASES if n != "b4c1_128x128"]


@pytest.mark.parametrize("name", list(R.ADAPTER_CASES))
def test_restatement_matches_reference_fixture(name, golden):
    """fp32 restatement vs the reference's fp32 CPU results: features, out, every gradient"""
    fx = golden("memory_adapter.npz")
    feat, out, pre, grads = R.run_case(name, torch.float32)
    flat = torch.cat([grads[k].reshape(-1) for k in R.KEYS]).numpy()

    def rel(a, b):
        return np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()

    assert rel(feat.numpy(), fx[name + "_feat"]) < 1e-6
    assert rel(out.numpy(), fx[name + "_out"]) < 1e-6
    assert rel(flat, fx[name + "_grad"]) < 2e-5  # two fp32 summation orders of up to 65,536 terms


@pytest.mark.parametrize("name", SMALL)
def test_hand_backward_matches_torch_autograd_fp64(name):
    B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
    params, noisy, base, mem, dout = R.adapter_case(name)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params.items()}
    n, b, m, d = (torch.from_numpy(v).double() for v in (noisy, base, mem, dout))
    (R.forward(p, n, b, m, nb, clamp) * d).sum().backward()
    hand = R.backward({k: v.detach() for k, v in p.items()}, n, b, m, d, nb, clamp)
    for k in R.KEYS:
        assert (hand[k] - p[k].grad).abs().max() <= 1e-10 * max(1.0, p[k].grad.abs().max()), k


def test_bank_order_is_unfold_order(golden):
    from image_denoising_amd.memory import MemoryBank

    case = R.SELECT_CASES[2]
    P, s, H, W, n_img, C = case
    imgs = torch.from_numpy(R.bank_images(case, 4242))
    ref = R.bank_patches(imgs, P, s)
    unf = F.unfold(imgs, kernel_size=P, stride=s).transpose(1, 2).reshape(-1, C, P, P)
    assert torch.equal(ref, unf)
    assert np.array_equal(ref.numpy(), golden("memory_adapter.npz")["order_patches"])
    bank = MemoryBank(imgs, imgs + 1, P, s)
    assert len(bank) == ref.shape[0]
    assert torch.equal(bank.noise_patches(), ref) and torch.equal(bank.clean_patches(), ref + 1)
    ragged = MemoryBank(imgs, imgs, 4, 3)  # (9-4) % 3 != 0: trailing pixels unused
    assert torch.equal(ragged.noise_patches(), R.bank_patches(imgs, 4, 3))


def test_selection_restatement_matches_reference(golden):
    fx = golden("memory_adapter.npz")
    for case in R.SELECT_CASES[:3]:
        P, s, H, W, n_img, C = case
        for B in R.SELECT_B:
            imgs = torch.from_numpy(R.bank_images(case, R.select_seed(case, B))).double()
            q = torch.from_numpy(R.random_queries(case, B)).double()
            idx, best, second, scale = R.select(q, R.bank_patches(imgs, P, s))
            key = f"sel_{P}_{s}_{H}_{W}_{n_img}_{C}_B{B}_"
            assert np.array_equal(idx.numpy(), fx[key + "idx64"])
            keep = ((second - best) / scale).numpy() >= R.GAP_SKIP
            assert np.array_equal(idx.numpy()[keep], fx[key + "idx"][keep])  # the reference's fp32 pick


@pytest.mark.parametrize("case", R.ORIGIN_CASES)
def test_patch_origins(case):
    from image_denoising_amd.memory import patch_origins

    H, W, P, ov = case
    want = {(352, 352, 128, 64): ([0, 64, 128, 192, 224], [0, 64, 128, 192, 224]),
            (130, 200, 128, 64): ([0, 2], [0, 64, 72]),
            (128, 128, 128, 0): ([0], [0]),
            (45, 61, 24, 7): ([0, 17, 21], [0, 17, 34, 37])}[case]
    assert (patch_origins(H, P, ov), patch_origins(W, P, ov)) == want
    assert (R.origins(H, P, ov), R.origins(W, P, ov)) == want


@pytest.mark.parametrize("case", R.BLEND_CASES)
def test_blend_restatement_matches_reference(case, golden):
    H, W, P, ov = case
    t = R.blend_image(case) / np.float32(255.0)
    ys, xs = R.origins(H, P, ov), R.origins(W, P, ov)
    pred = np.stack([t[y:y + P, x:x + P] for y in ys for x in xs])[:, None] * np.float32(0.9) \
        + np.float32(0.05)
    got = R.hann_blend(pred, ys, xs, H, W)
    assert np.array_equal(got[0], golden("memory_adapter.npz")[f"blend_{H}_{W}_{P}_{ov}"][..., 0])


def test_init_order_and_state_dict_keys():
    """parameters drawn in the reference's construction order (torch's own modules, same seed),
    the last conv and both Linears zero; all ten are views of one flat buffer"""
    import torch.nn as nn

    from image_denoising_amd.memory import HyperGatedResidualAdapter, HyperGatedResidualAdapter_FFT

    torch.manual_seed(11)
    ad = HyperGatedResidualAdapter_FFT(1, 16, 3)
    torch.manual_seed(11)
    c1, c2 = nn.Conv2d(2, 16, 3, padding=1), nn.Conv2d(16, 16, 3, padding=1)
    sd = ad.state_dict()
    assert list(sd) == R.KEYS
    assert [tuple(v.shape) for v in sd.values()] == R.shapes_of(1, 16, 3)
    assert torch.equal(sd["local_net.0.weight"], c1.weight) and torch.equal(sd["local_net.2.bias"], c2.bias)
    for k in R.KEYS[4:]:
        assert not sd[k].any(), k
    assert sum(v.numel() for v in sd.values()) == ad.flat_params.numel()
    assert sd["hyper_mlp.2.bias"].data_ptr() == ad.flat_params[-2:].data_ptr()
    v4 = HyperGatedResidualAdapter(3, 8)
    assert tuple(v4.state_dict()["hyper_mlp.0.weight"].shape) == (8, 6)


def test_bank_rejects_mixed_sizes_and_bad_shapes(tmp_path):
    from PIL import Image

    from image_denoising_amd.memory import MemoryBank, build_memory_bank

    for k, hw in enumerate([(20, 24), (20, 24), (20, 28)]):
        a = (R.uniform(hw[0] * hw[1], k) * 255).reshape(hw).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / f"c{k}.png")
        Image.fromarray(255 - a).save(tmp_path / f"n{k}.png")
    c = [str(tmp_path / f"c{k}.png") for k in range(3)]
    n = [str(tmp_path / f"n{k}.png") for k in range(3)]
    bank = build_memory_bank(c[:2], n[:2], 8, 4, "cpu")
    assert len(bank) == 2 * 4 * 5 and bank.channels == 1
    a = np.array(Image.open(c[1]), dtype=np.float32) / 255.0
    assert np.array_equal(bank.clean_patches()[20 + 5 + 2, 0].numpy(), a[4:12, 8:16])
    with pytest.raises(ValueError):
        build_memory_bank(c, n, 8, 4, "cpu")
    with pytest.raises(ValueError):
        MemoryBank(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8), 9, 1)
