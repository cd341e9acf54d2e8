"""Reference restatement of the paired patch loader (finetune.py:100-150) for the tests of
dn_patch_sample: plain numpy slicing by (image, top, left) and / 255 in fp32, with the crop
origins of the device sampler restated from oracle.philox (multiply-shift of one 32-bit word
per coordinate, keyed on the item's global ordinal)."""
import numpy as np

from oracle import philox


def chw(a) -> np.ndarray:
    """HW or HWC -> CHW float32 (transforms.ToTensor on a float32 array: no rescaling)"""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def crop(img, top: int, left: int, ps: int) -> np.ndarray:
    """img[top:top+ps, left:left+ps] of an HW / HWC image, as [C, ps, ps] float32 / 255"""
    a = np.asarray(img, dtype=np.float32)
    assert 0 <= top <= a.shape[0] - ps and 0 <= left <= a.shape[1] - ps
    return chw(a[top:top + ps, left:left + ps]) / np.float32(255.0)


def origins(seed: int, offset: int, item_base: int, img_idx, sizes, ps: int) -> np.ndarray:
    """int32 [N, 2] = (top, left) of items item_base .. item_base + N - 1:
    top = (u32(seed, offset, 2g) * (h - ps + 1)) >> 32, left the same with word 2g + 1 and w"""
    img_idx = np.asarray(img_idx, dtype=np.int64)
    g = np.arange(item_base, item_base + img_idx.size, dtype=np.uint64)
    h = np.array([sizes[m][0] for m in img_idx], dtype=np.uint64)
    w = np.array([sizes[m][1] for m in img_idx], dtype=np.uint64)
    u_top = philox.cell_u32(seed, offset, np.uint64(2) * g).astype(np.uint64)
    u_left = philox.cell_u32(seed, offset, np.uint64(2) * g + np.uint64(1)).astype(np.uint64)
    top = (u_top * (h - np.uint64(ps) + np.uint64(1))) >> np.uint64(32)
    left = (u_left * (w - np.uint64(ps) + np.uint64(1))) >> np.uint64(32)
    return np.stack([top, left], axis=1).astype(np.int32)


def sample(images, img_idx, org, ps: int) -> np.ndarray:
    """[N, C, ps, ps]: crop(images[img_idx[i]], *org[i]) for every item"""
    return np.stack([crop(images[m], int(t), int(l), ps)
                     for m, (t, l) in zip(np.asarray(img_idx).tolist(), np.asarray(org).tolist())])
