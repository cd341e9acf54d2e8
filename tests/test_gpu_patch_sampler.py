"""dn_patch_sample (csrc/patch_sample.hip), data.DevicePatchSampler and the finetune command on
the device, against tests/patch_ref.py (numpy slicing, / 255 in fp32, Philox origins from
oracle.philox).  Every comparison is bit for bit.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

import patch_ref

pytestmark = pytest.mark.gpu
SIZES = [(40, 56), (33, 47), (64, 64)]  # mixed sizes, odd extents
ORDER7 = [2, 0, 1, 2, 2, 0, 1]  # repeats, not sorted
SEED = 11


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _images(C):
    rng = np.random.default_rng(40 + C)
    shape = (lambda h, w: (h, w)) if C == 1 else (lambda h, w: (h, w, C))
    clean = [rng.integers(0, 256, shape(h, w)).astype(np.float32) for h, w in SIZES]
    noisy = [rng.integers(0, 256, shape(h, w)).astype(np.float32) for h, w in SIZES]
    return clean, noisy


@pytest.fixture(scope="module")
def images():
    return {C: _images(C) for C in (1, 3)}


def _sampler(images, C, ps, paired=True, ppi=5):
    from image_denoising_amd import DevicePatchSampler

    clean, noisy = images[C]
    return DevicePatchSampler(clean, noisy if paired else None, patch_size=ps,
                              patches_per_image=ppi, seed=SEED)


def _same(t, ref):
    return torch.equal(t.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("ps", [4, 6, 13, 32])
def test_explicit_origins_equal_the_reference_crops(images, C, ps):
    clean, noisy = images[C]
    s = _sampler(images, C, ps)
    for idx in ([1], ORDER7):
        corners = {
            "first": [(0, 0) for m in idx],
            "last": [(SIZES[m][0] - ps, SIZES[m][1] - ps) for m in idx],
            "odd left": [((SIZES[m][0] - ps) // 2, (SIZES[m][1] - ps - 1) | 1) for m in idx],
        }
        for name, org in corners.items():
            assert all(o[1] <= SIZES[m][1] - ps for o, m in zip(org, idx))
            assert name != "odd left" or all(o[1] % 2 == 1 for o in org)
            c, n, o = s.sample(idx, epoch=1, item_base=0, origins=org)
            assert c.shape == n.shape == (len(idx), C, ps, ps) and c.dtype == torch.float32
            assert _same(o, np.asarray(org, dtype=np.int32)), name
            assert _same(c, patch_ref.sample(clean, idx, org, ps)), name
            assert _same(n, patch_ref.sample(noisy, idx, org, ps)), name


@pytest.mark.parametrize("C", [1, 3])
def test_patch_of_the_whole_image(images, C):
    from image_denoising_amd import DevicePatchSampler

    clean, noisy = images[C]
    s = DevicePatchSampler([clean[2]], [noisy[2]], patch_size=64, patches_per_image=2, seed=SEED)
    for org in (None, [(0, 0), (0, 0)]):
        c, n, o = s.sample([0, 0], epoch=3, item_base=7, origins=org)
        assert not o.any()  # range 1: the Philox origin is (0, 0) too
        for k in (0, 1):
            assert _same(c[k], patch_ref.chw(clean[2]) / np.float32(255.0))
            assert _same(n[k], patch_ref.chw(noisy[2]) / np.float32(255.0))


@pytest.mark.parametrize("C,ps", [(1, 13), (3, 32)])
def test_philox_origins_and_their_crops(images, C, ps):
    clean, noisy = images[C]
    s = _sampler(images, C, ps)
    seen = []
    for item_base in (0, 5):
        for offset in (1, 3):
            c, n, o = s.sample(ORDER7, epoch=offset, item_base=item_base)
            org = patch_ref.origins(SEED, offset, item_base, ORDER7, SIZES, ps)
            assert _same(o, org)
            assert _same(c, patch_ref.sample(clean, ORDER7, org, ps))
            assert _same(n, patch_ref.sample(noisy, ORDER7, org, ps))
            seen.append(org)
    assert not any(np.array_equal(seen[0], other) for other in seen[1:])


def test_a_shard_is_its_slice_of_the_whole_batch(images):
    s = _sampler(images, 1, 13)
    idx = ORDER7 + [0]
    c, n, o = s.sample(idx, epoch=2, item_base=0)
    for a in (0, 4):
        ca, na, oa = s.sample(idx[a:a + 4], epoch=2, item_base=a)
        assert torch.equal(ca, c[a:a + 4]) and torch.equal(na, n[a:a + 4])
        assert torch.equal(oa, o[a:a + 4])


def test_clean_only_pool(images):
    both = _sampler(images, 3, 6)
    alone = _sampler(images, 3, 6, paired=False)
    c, n, o = both.sample(ORDER7, epoch=1, item_base=3)
    c1, n1, o1 = alone.sample(ORDER7, epoch=1, item_base=3)
    assert n1 is None and n is not None
    assert torch.equal(c1, c) and torch.equal(o1, o)
    assert all(b[1] is None for b in alone.batches(1, 4))


def test_sample_rejects_bad_requests_on_the_host(images):
    s = _sampler(images, 1, 32)
    with pytest.raises(ValueError, match="outside image"):
        s.sample([1], epoch=1, origins=[(2, 0)])  # 33 rows: top <= 1
    with pytest.raises(ValueError, match="outside image"):
        s.sample([0], epoch=1, origins=[(0, -1)])
    with pytest.raises(ValueError, match="img_idx outside"):
        s.sample([3], epoch=1)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        s.sample([0, 1], epoch=1, origins=[(0, 0)])


def test_batches_follow_the_reference_loader_and_the_plan(images):
    from image_denoising_amd import epoch_plan

    ppi, batch, epoch = 5, 4, 2
    s = _sampler(images, 1, 13, ppi=ppi)
    ref = [len(b) for b in torch.utils.data.DataLoader(range(len(s)), batch_size=batch,
                                                       shuffle=True, drop_last=False)]
    plan = epoch_plan(len(SIZES), ppi, batch, SEED, epoch)
    got = []
    for (c, n), (img, item_base) in zip(s.batches(epoch, batch), plan):
        got.append(c.shape[0])
        cs, ns, _ = s.sample(img, epoch=epoch, item_base=item_base)
        assert torch.equal(c, cs) and torch.equal(n, ns)
    assert got == ref == [4, 4, 4, 3] and len(plan) == s.steps_per_epoch(batch) == 4
    # two ranks: each one's batches are its halves of the single-process batches
    whole = [c.clone() for c, _ in s.batches(epoch, batch, drop_last=True)]
    for rank in (0, 1):
        mine = [c.clone() for c, _ in s.batches(epoch, batch // 2, world=2, rank=rank,
                                                 drop_last=True)]
        assert len(mine) == len(whole) == 3
        for m, w in zip(mine, whole):
            assert torch.equal(m, w[2 * rank:2 * rank + 2])


def _finetune_setup(root):
    from PIL import Image

    from image_denoising_amd import UNet
    from image_denoising_amd.checkpoint import save_checkpoint

    rng = np.random.default_rng(3)
    data = os.path.join(root, "data")
    for d in ("clean", "noise"):
        os.makedirs(os.path.join(data, d))
    yy, xx = np.meshgrid(np.linspace(0, 1, 64), np.linspace(0, 1, 64), indexing="ij")
    for i in range(2):
        c = np.clip(128 + 90 * np.sin(5 * xx + 3 * yy + i), 0, 255).astype(np.uint8)
        n = np.clip(c.astype(int) + rng.integers(-25, 26, c.shape), 0, 255).astype(np.uint8)
        Image.fromarray(c).save(os.path.join(data, "clean", f"img{i}.png"))
        Image.fromarray(n).save(os.path.join(data, "noise", f"img{i}.png"))
    torch.manual_seed(0)
    ck = save_checkpoint(UNet(1, 1, 48), os.path.join(root, "base.pth"))
    return data, ck


def test_finetune_command_equals_the_hand_driven_loop(tmp_path):
    from image_denoising_amd import DenoiserWithAdapter, DevicePatchSampler, FinetuneTrainer, finetune
    from image_denoising_amd.checkpoint import load_adapter_checkpoint, read_state_dict

    data, ck = _finetune_setup(str(tmp_path))
    seed = 5
    res = finetune.main(["--data_dir", data, "--pretrained_ckpt", ck, "--arch", "UNet",
                         "--n_epoch", "2", "--patch_size", "32", "--patches_per_image", "4",
                         "--batchsize", "4", "--save_every", "1", "--seed", str(seed),
                         "--save_model_path", str(tmp_path / "out"), "--log_name", "ft",
                         "--num_workers", "2", "--gpu_devices", "0"])

    dev = torch.device("cuda", torch.cuda.current_device())
    sampler = DevicePatchSampler.from_dir(data, 32, 4, seed=seed)
    base = finetune.build_base_model("UNet", 1, 48)
    finetune.load_base_weights(base, ck)
    torch.manual_seed(seed)
    model = DenoiserWithAdapter(base, in_channels=1, hidden_channels=16).to(dev)
    tr = FinetuneTrainer(model, lr=1e-4, lambda_grad=0.1, distributed=False)
    losses = []
    for epoch in (1, 2):
        for clean, noisy in sampler.batches(epoch, 4):
            losses.append(tr.train_step(clean, noisy).clone())
    assert len(losses) == 4
    assert res["losses"] == torch.stack(losses).cpu().tolist()
    assert res["mean_l1"] == [float(np.mean([l[0] for l in res["losses"][a:a + 2]]))
                              for a in (0, 2)]

    out = str(tmp_path / "out" / "ft")
    assert res["checkpoints"] == [os.path.join(out, f"epoch_adapter_{e:03d}.pth") for e in (1, 2)]
    for path in res["checkpoints"]:
        assert os.path.exists(path) and read_state_dict(path)
    fresh = DenoiserWithAdapter(finetune.build_base_model("UNet", 1, 48), 1, 16)
    missing, unexpected = load_adapter_checkpoint(fresh, res["checkpoints"][-1])
    assert not missing and not unexpected
    assert torch.equal(fresh.adapter.flat_params.detach().cpu(),
                       model.adapter.flat_params.detach().cpu())
    first = DenoiserWithAdapter(finetune.build_base_model("UNet", 1, 48), 1, 16)
    load_adapter_checkpoint(first, res["checkpoints"][0])
    assert not torch.equal(first.adapter.flat_params, fresh.adapter.flat_params)
    # validation at both epochs: one PSNR per image, the first image's three PNGs
    assert sorted(res["psnr"]) == [1, 2] and all(len(v) == 2 for v in res["psnr"].values())
    assert all(0.0 < p <= 99.0 for v in res["psnr"].values() for p in v)
    vals = sorted(d for d in os.listdir(out) if d.startswith("val_"))
    assert len(vals) == 2
    assert sorted(os.listdir(os.path.join(out, vals[1]))) == [
        "img0_clean.png", "img0_denoised_ep002.png", "img0_noisy.png"]


def test_finetune_command_refuses_parallel(tmp_path, capsys):
    from image_denoising_amd import finetune

    with pytest.raises(SystemExit) as e:
        finetune.main(["--data_dir", str(tmp_path), "--pretrained_ckpt", "none.pth", "--parallel"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "torchrun" in err and "distributed=True" in err
