"""Device-resident paired patch sampler: the input side of the trainers.

The reference's loader (finetune.py:100-150 DenoisePatchDataset under a shuffled DataLoader,
restated as finetune.DenoisePatchDataset) decodes a whole image pair per item on the host, crops
one patch and ships fp32 batches over PCIe.  The B-domain set is five image pairs: here the pairs
are uploaded once, and a batch is one launch of dn_patch_sample (csrc/patch_sample.hip).

    plan      epoch_plan(): which image each item of the epoch crops, the reference's shuffle
              (a randperm of images x patches_per_image, // patches_per_image), host side, pure
    origins   in the kernel, Philox keyed on (seed, epoch, the item's position in the epoch), so
              a rank's shard is its slice of the single-process batch
    values    x / 255.0f, the bits of the reference's `tensor / 255.0`

Nothing here synchronises with the host; there is no host fallback.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import _lib

_U64 = (1 << 64) - 1


def _mix(seed: int, epoch: int) -> int:
    """(seed, epoch) -> one generator seed: the splitmix64 finaliser over both, kept to 32 bits
    (the CPU generator's mt19937 is seeded from the low 32 bits alone)"""
    z = ((int(seed) & _U64) * 0x9E3779B97F4A7C15 + (int(epoch) & _U64) * 0xD1B54A32D192ED03
         + 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return (z ^ (z >> 31)) & 0xFFFFFFFF


def epoch_plan(n_images: int, patches_per_image: int, batch: int, seed: int, epoch: int,
               world: int = 1, rank: int = 0, drop_last: bool = False):
    """The image index of every item of one epoch, as the reference's DataLoader(shuffle=True)
    over DenoisePatchDataset visits them: a torch.randperm of n_images * patches_per_image (CPU
    generator seeded by (seed, epoch)) // patches_per_image, so every image appears exactly
    patches_per_image times.  The permutation is cut into global batches of batch * world; the
    result is this rank's contiguous slice of each, a list of (img_idx int32 tensor, item_base),
    item_base being the position in the epoch of the slice's first item.  A short last batch is
    kept (drop_last=False, the reference's setting) or dropped; with world > 1 it cannot be kept,
    because the ranks' shards must be equal: ValueError."""
    if n_images < 1 or patches_per_image < 1 or batch < 1:
        raise ValueError("n_images, patches_per_image and batch must be >= 1")
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"need world >= 1 and 0 <= rank < world, got rank {rank} of {world}")
    g = torch.Generator()
    g.manual_seed(_mix(seed, epoch))
    total = n_images * patches_per_image
    img = (torch.randperm(total, generator=g) // patches_per_image).to(torch.int32)
    gb = batch * world
    full, ragged = divmod(total, gb)
    if ragged and world > 1 and not drop_last:
        raise ValueError(f"{total} items do not fill global batches of {gb}: with world > 1 the "
                         "ranks' shards must be equal, pass drop_last=True")
    plan = []
    for s in range(full):
        a = s * gb + rank * batch
        plan.append((img[a:a + batch].clone(), a))
    if ragged and not drop_last:  # world == 1
        plan.append((img[full * gb:].clone(), full * gb))
    return plan


def _chw(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError(f"an image must be HW or HWC, got shape {a.shape}")
    return np.ascontiguousarray(a.transpose(2, 0, 1))


class DevicePatchSampler:
    """Image pairs resident on the device, random paired crops from one launch per batch.

    clean, noisy: lists of HW or HWC arrays holding pixel values 0..255 (what
    np.array(Image.open(f), dtype=np.float32) gives); noisy=None is a clean-only set (N2NTrainer's
    input), for which no noisy tensor is produced.  Images may differ in size; a pair must share
    its shape, every image the channel count, and none may be smaller than patch_size
    (ValueError).  The pools and the offset table are uploaded once, here."""

    def __init__(self, clean, noisy=None, patch_size: int = 128, patches_per_image: int = 16,
                 seed: int = 0, device=None):
        clean = [_chw(a) for a in clean]
        if len(clean) == 0:
            raise ValueError("no images")
        if noisy is not None:
            noisy = [_chw(a) for a in noisy]
            if len(noisy) != len(clean):
                raise ValueError("clean and noisy must have the same number of images")
            for i, (c, n) in enumerate(zip(clean, noisy)):
                if c.shape != n.shape:
                    raise ValueError(f"pair {i}: clean {c.shape} and noisy {n.shape} differ")
        if patch_size < 1 or patches_per_image < 1:
            raise ValueError("patch_size and patches_per_image must be >= 1")
        C = clean[0].shape[0]
        for i, c in enumerate(clean):
            if c.shape[0] != C:
                raise ValueError(f"image {i} has {c.shape[0]} channels, image 0 has {C}")
            if c.shape[1] < patch_size or c.shape[2] < patch_size:
                raise ValueError(f"Image size ({c.shape[1]},{c.shape[2]}) smaller than "
                                 f"patch_size {patch_size}.")
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("the patch sampler runs on the GPU (HIP); no device visible")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.patch_size = int(patch_size)
        self.patches_per_image = int(patches_per_image)
        self.seed = int(seed) & _U64
        self.channels = C
        self.sizes = [(c.shape[1], c.shape[2]) for c in clean]
        table, off = [], 0
        for c in clean:
            table.append((off, c.shape[1], c.shape[2]))
            off += c.size
        self.pool_elems = off
        self._table = torch.tensor(table, dtype=torch.int64).to(self.device)
        self._clean = torch.from_numpy(np.concatenate([c.reshape(-1) for c in clean])).to(self.device)
        self._noisy = None
        if noisy is not None:
            self._noisy = torch.from_numpy(np.concatenate([n.reshape(-1) for n in noisy])).to(self.device)

    @classmethod
    def from_dir(cls, data_dir: str, patch_size: int, patches_per_image: int, seed: int = 0,
                 device=None, limit: int = 5):
        """data_dir/{clean,noise}/* paired by sorted name, the first `limit` pairs: the pairing
        and the [:5] of DenoisePatchDataset (finetune.py:108-112)"""
        from PIL import Image

        clean = sorted(glob.glob(os.path.join(data_dir, "clean", "*")))[:limit]
        noise = sorted(glob.glob(os.path.join(data_dir, "noise", "*")))[:limit]
        if len(clean) != len(noise) or len(clean) == 0:
            raise ValueError("clean and noise must have the same number of images and be non-empty.")
        return cls([np.array(Image.open(f), dtype=np.float32) for f in clean],
                   [np.array(Image.open(f), dtype=np.float32) for f in noise],
                   patch_size=patch_size, patches_per_image=patches_per_image, seed=seed,
                   device=device)

    def __len__(self) -> int:
        """items per epoch (DenoisePatchDataset.__len__)"""
        return len(self.sizes) * self.patches_per_image

    @property
    def paired(self) -> bool:
        return self._noisy is not None

    def _check_origins(self, img_idx, origins) -> torch.Tensor:
        if isinstance(img_idx, torch.Tensor) and img_idx.device.type != "cpu":
            raise ValueError("explicit origins are checked on the host: pass img_idx as host data")
        o = torch.as_tensor(np.asarray(origins), dtype=torch.int64)
        idx = torch.as_tensor(np.asarray(img_idx), dtype=torch.int64).reshape(-1)
        if o.shape != (idx.numel(), 2):
            raise ValueError(f"origins must be [N, 2] = (top, left), got {tuple(o.shape)}")
        ps = self.patch_size
        for i, (m, (top, left)) in enumerate(zip(idx.tolist(), o.tolist())):
            h, w = self.sizes[m]
            if not (0 <= top <= h - ps and 0 <= left <= w - ps):
                raise ValueError(f"item {i}: origin ({top}, {left}) outside image {m} "
                                 f"({h} x {w}) for patch_size {ps}")
        return o.to(torch.int32)

    def _index(self, img_idx) -> torch.Tensor:
        """device int32 [N]; host data is range-checked first, a device tensor is taken as it is
        (the kernel zeroes an item whose index is out of range)"""
        if isinstance(img_idx, torch.Tensor) and img_idx.device.type != "cpu":
            if img_idx.dtype != torch.int32 or img_idx.dim() != 1 or not img_idx.is_contiguous():
                raise ValueError("a device img_idx must be a contiguous int32 vector")
            if img_idx.device != self.device:
                raise ValueError(f"img_idx on {img_idx.device}, the pools on {self.device}")
            return img_idx
        idx = torch.as_tensor(np.asarray(img_idx), dtype=torch.int64).reshape(-1)
        if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < len(self.sizes)):
            raise ValueError(f"img_idx outside [0, {len(self.sizes)})")
        return idx.to(torch.int32).to(self.device)

    def _launch(self, idx, n, offset, item_base, origins_in, clean, noisy, origins_out):
        _lib.call("dn_patch_sample", _lib.ptr(self._clean), _lib.ptr(self._noisy), self.pool_elems,
                  self._table.data_ptr(), len(self.sizes), self.channels, idx.data_ptr(), n,
                  self.patch_size, self.seed, int(offset) & _U64, int(item_base) & _U64,
                  _lib.ptr(origins_in), _lib.ptr(clean), _lib.ptr(noisy), _lib.ptr(origins_out),
                  _lib.stream_of(clean))

    def sample(self, img_idx, epoch: int, item_base: int = 0, origins=None):
        """One batch: (clean, noisy, origins) as device tensors, [N, C, ps, ps] fp32 twice (noisy
        is None for a clean-only set) and int32 [N, 2] = the (top, left) used.  Item i crops image
        img_idx[i] at the Philox origin of (seed, offset = epoch, ordinal item_base + i), or at
        origins[i] when given (host data, checked here: ValueError outside the image)."""
        idx = self._index(img_idx)
        o_in = None
        if origins is not None:
            o_in = self._check_origins(img_idx, origins).to(self.device)
        n, ps = idx.numel(), self.patch_size
        f = dict(dtype=torch.float32, device=self.device)
        clean = torch.empty((n, self.channels, ps, ps), **f)
        noisy = torch.empty((n, self.channels, ps, ps), **f) if self.paired else None
        o_out = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        if n:
            self._launch(idx, n, epoch, item_base, o_in, clean, noisy, o_out)
        return clean, noisy, o_out

    def steps_per_epoch(self, batch: int, world: int = 1, drop_last: bool = False) -> int:
        full, ragged = divmod(len(self), batch * world)
        return full + (1 if ragged and not drop_last else 0)

    def batches(self, epoch: int, batch: int, world: int = 1, rank: int = 0,
                drop_last: bool = False):
        """The epoch's (clean, noisy) batches of this rank, in epoch_plan's order.  The plan is
        uploaded once; every step is one launch into the same two buffers, so a yielded batch is
        valid until the next one is asked for (a short last batch is a view of its first items).
        The Philox offset is the epoch, the ordinal the item's position in the epoch."""
        plan = epoch_plan(len(self.sizes), self.patches_per_image, batch, self.seed, epoch, world,
                          rank, drop_last)
        if not plan:
            return
        idx = torch.cat([p[0] for p in plan]).to(self.device)
        ps = self.patch_size
        f = dict(dtype=torch.float32, device=self.device)
        clean = torch.empty((batch, self.channels, ps, ps), **f)
        noisy = torch.empty((batch, self.channels, ps, ps), **f) if self.paired else None
        a = 0
        for img, item_base in plan:
            n = img.numel()
            self._launch(idx[a:a + n], n, epoch, item_base, None, clean, noisy, None)
            a += n
            yield clean[:n], (noisy[:n] if self.paired else None)
