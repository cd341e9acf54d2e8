"""Host side of the device patch sampler (image_denoising_amd/data.py, dn_patch_sample): the
reference restatement tests/patch_ref.py against the reference loader's restatement
(finetune.DenoisePatchDataset), the epoch plan, the origin formula's range, and the C boundary's
rejections.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import patch_ref

SIZES = [(40, 56), (33, 47), (64, 64)]


def _write_pairs(root, channels):
    from PIL import Image

    rng = np.random.default_rng(5 + channels)
    for d in ("clean", "noise"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i, (h, w) in enumerate(SIZES):
        shape = (h, w) if channels == 1 else (h, w, channels)
        for d in ("clean", "noise"):
            Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(
                os.path.join(root, d, f"im{i}.png"))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("ps", [4, 13, 33])
def test_patch_ref_crops_equal_the_reference_dataset(tmp_path, channels, ps):
    """same (img, top, left) -> the bits of DenoisePatchDataset.__getitem__: seed np.random, draw
    the item, then replay the two randint draws"""
    from PIL import Image

    from image_denoising_amd.finetune import DenoisePatchDataset

    _write_pairs(str(tmp_path), channels)
    ppi = 3
    ds = DenoisePatchDataset(str(tmp_path), patch_size=ps, patches_per_image=ppi)
    clean = [np.array(Image.open(f), dtype=np.float32) for f in ds.clean]
    noise = [np.array(Image.open(f), dtype=np.float32) for f in ds.noise]
    for index in (0, 4, 8, 5):
        np.random.seed(100 + index)
        c, n = ds[index]
        np.random.seed(100 + index)
        m = index // ppi
        h, w = SIZES[m]
        top = np.random.randint(0, h - ps + 1)
        left = np.random.randint(0, w - ps + 1)
        assert c.dtype == torch.float32 and tuple(c.shape) == (channels, ps, ps)
        assert np.array_equal(c.numpy(), patch_ref.crop(clean[m], top, left, ps))
        assert np.array_equal(n.numpy(), patch_ref.crop(noise[m], top, left, ps))
        both = patch_ref.sample(noise, [m], [(top, left)], ps)
        assert np.array_equal(both[0], n.numpy())


def _flat(plan):
    return torch.cat([p[0] for p in plan]).tolist()


def test_epoch_plan_visits_every_image_patches_per_image_times():
    from image_denoising_amd.data import epoch_plan

    plan = epoch_plan(5, 16, 4, seed=3, epoch=1)
    assert len(plan) == 20 and all(p[0].numel() == 4 and p[0].dtype == torch.int32 for p in plan)
    assert [p[1] for p in plan] == list(range(0, 80, 4))
    assert np.bincount(_flat(plan), minlength=5).tolist() == [16] * 5
    # a short last batch is kept, as the reference's drop_last=False does, or dropped
    plan = epoch_plan(3, 5, 4, seed=3, epoch=1)
    assert [p[0].numel() for p in plan] == [4, 4, 4, 3] and plan[-1][1] == 12
    assert np.bincount(_flat(plan), minlength=3).tolist() == [5] * 3
    assert [p[0].numel() for p in epoch_plan(3, 5, 4, seed=3, epoch=1, drop_last=True)] == [4] * 3


def test_epoch_plan_is_a_function_of_seed_and_epoch():
    from image_denoising_amd.data import epoch_plan

    a = _flat(epoch_plan(5, 16, 4, seed=3, epoch=1))
    assert a == _flat(epoch_plan(5, 16, 4, seed=3, epoch=1))
    assert a != _flat(epoch_plan(5, 16, 4, seed=3, epoch=2))
    assert a != _flat(epoch_plan(5, 16, 4, seed=4, epoch=1))


@pytest.mark.parametrize("world", [2, 4])
def test_epoch_plan_shards_are_slices_of_the_single_process_plan(world):
    from image_denoising_amd.data import epoch_plan

    batch = 2
    whole = epoch_plan(5, 16, batch * world, seed=9, epoch=4)
    ranks = [epoch_plan(5, 16, batch, seed=9, epoch=4, world=world, rank=r) for r in range(world)]
    assert all(len(r) == len(whole) for r in ranks)
    for s, (img, base) in enumerate(whole):
        assert torch.equal(torch.cat([ranks[r][s][0] for r in range(world)]), img)
        assert [ranks[r][s][1] for r in range(world)] == [base + r * batch for r in range(world)]


def test_epoch_plan_ragged_last_batch_needs_drop_last_when_sharded():
    from image_denoising_amd.data import epoch_plan

    with pytest.raises(ValueError, match="drop_last"):
        epoch_plan(3, 5, 2, seed=0, epoch=1, world=2)  # 15 items, global batches of 4
    plan = epoch_plan(3, 5, 2, seed=0, epoch=1, world=2, rank=1, drop_last=True)
    assert [p[0].numel() for p in plan] == [2, 2, 2] and [p[1] for p in plan] == [2, 6, 10]
    with pytest.raises(ValueError):
        epoch_plan(3, 5, 2, seed=0, epoch=1, world=2, rank=2, drop_last=True)


def test_origin_formula_covers_its_range_and_nothing_else():
    """4096 ordinals, range 5 (h - ps + 1 = w - ps + 1 = 5): every origin in [0, 4], both ends
    occur (seed 7, offset 1: checked when this test was written); range 1 gives only 0"""
    idx = np.zeros(4096, dtype=np.int64)
    o = patch_ref.origins(7, 1, 0, idx, [(12, 12)], 8)
    assert o.shape == (4096, 2) and o.dtype == np.int32
    for k in (0, 1):
        assert o[:, k].min() == 0 and o[:, k].max() == 4
        assert np.bincount(o[:, k], minlength=5).min() > 4096 // 5 // 2  # roughly uniform
    assert not np.array_equal(o[:, 0], o[:, 1])
    assert not patch_ref.origins(7, 1, 0, idx, [(8, 8)], 8).any()
    # the key is the global ordinal: a later slice equals the slice of the whole
    assert np.array_equal(patch_ref.origins(7, 1, 100, idx[:50], [(12, 12)], 8), o[100:150])


def test_sampler_rejects_bad_image_sets_before_touching_a_device():
    from image_denoising_amd.data import DevicePatchSampler

    a, b = np.zeros((16, 16), np.float32), np.zeros((16, 20), np.float32)
    with pytest.raises(ValueError, match="differ"):
        DevicePatchSampler([a], [b], patch_size=8, patches_per_image=2)
    with pytest.raises(ValueError, match="channels"):
        DevicePatchSampler([a, np.zeros((16, 16, 3), np.float32)], patch_size=8, patches_per_image=2)
    with pytest.raises(ValueError, match="smaller than patch_size"):
        DevicePatchSampler([a, b], patch_size=17, patches_per_image=2)
    with pytest.raises(ValueError, match="same number"):
        DevicePatchSampler([a, a], [a], patch_size=8, patches_per_image=2)


# ---- the data header and its binding: what tests/test_host_abi.py and
# tests/test_capi_rejects_cpu.py pin for include/denoise_hip.h, here for denoise_hip_data.h -------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name):
    import re

    src = open(os.path.join(ROOT, "include", name)).read()
    return set(re.findall(r"\b(dn_[a-z0-9_]+)\s*\(", src))


def test_data_header_symbols_are_exported_and_bound():
    from image_denoising_amd import _build, _lib

    syms = _header_symbols("denoise_hip_data.h")
    assert syms == set(_lib.DATA_SIGNATURES) == {"dn_patch_sample"}
    assert not syms & _header_symbols("denoise_hip.h") and not syms & set(_lib.SIGNATURES)
    L = _lib.lib()
    for s in syms:
        fn = getattr(L, s)
        assert (fn.restype, list(fn.argtypes)) == (_lib.DATA_SIGNATURES[s][0],
                                                   list(_lib.DATA_SIGNATURES[s][1]))
    # the header is part of what dn_version()'s source hash covers
    assert "denoise_hip_data.h" in _build.API_HEADERS
    assert L.dn_version().decode().endswith("src=" + _build.source_hash())
    assert L.dn_abi_version() == _lib.ABI_VERSION == 5


def test_every_data_function_has_a_rejection_case():
    from image_denoising_amd import _lib

    # dn_patch_sample is the only one, and test_patch_sample_rejections is its table
    assert set(_lib.DATA_SIGNATURES) == {"dn_patch_sample"}


# ---- the C boundary, with host dummies: every call below returns before any launch -------------
_BUF = ctypes.create_string_buffer(1 << 12)
_A0 = (ctypes.addressof(_BUF) + 15) & ~15
ARG = -1


def _args(**kw):
    a = dict(clean_pool=_A0, noisy_pool=_A0 + 256, pool_elems=16, table=_A0 + 512, M=1, C=1,
             img_idx=_A0 + 768, N=1, ps=4, seed=0, offset=0, item_base=0, origins_in=None,
             clean_out=_A0 + 1024, noisy_out=_A0 + 2048, origins_out=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("kw,message", [
    (dict(clean_pool=None), "null argument"),
    (dict(table=None), "null argument"),
    (dict(img_idx=None), "null argument"),
    (dict(clean_out=None), "null argument"),
    (dict(noisy_out=None), "null argument"),  # required once there is a noisy pool
    (dict(N=-1), "need N >= 0 and M, C, ps >= 1"),
    (dict(M=0), "need N >= 0 and M, C, ps >= 1"),
    (dict(C=0), "need N >= 0 and M, C, ps >= 1"),
    (dict(ps=0), "need N >= 0 and M, C, ps >= 1"),
    (dict(pool_elems=0), "pool_elems >= 1 required"),
    (dict(clean_out=_A0 + 1028), "clean_out and noisy_out must be 16-byte aligned"),
], ids=lambda v: next(iter(v)) if isinstance(v, dict) else None)
def test_patch_sample_rejections(kw, message):
    from image_denoising_amd import _lib

    assert _lib.lib().dn_patch_sample(*_args(**kw)) == ARG
    assert _lib.last_error() == message


def test_patch_sample_empty_batch_is_ok():
    from image_denoising_amd import _lib

    # N == 0 launches nothing, whatever the pointers
    assert _lib.lib().dn_patch_sample(*_args(N=0)) == 0
    assert _lib.lib().dn_patch_sample(*_args(N=0, clean_pool=None, clean_out=None)) == 0
