"""Memory-bank adapter path on the HIP kernels (csrc/memory.hip) vs tests/memory_ref.py in fp64 and
the reference fixture tests/golden/memory_adapter.npz.  Needs an MI355X.

Adapter tolerance, per quantity: 4 x the error of the reference's own torch-fp32 CPU result (the
fixture) against the fp64 restatement, relative to the quantity's max magnitude.  Measured fixture
errors (tests/golden/make_golden_memory.py): features 3.4e-8 .. 1.3e-7, out 3.9e-8 .. 6.8e-8,
conv weight gradients 1.1e-7 .. 2.6e-6 (largest at 4x1x128x128), conv bias gradients 2.6e-8 ..
1.1e-6, hyper-MLP gradients 5.1e-8 .. 3.7e-7.
"""
import numpy as np
import pytest
import torch

import memory_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- selection -----------------------------------------------------------------------------------
def _bank(case, seed):
    from image_denoising_amd.memory import MemoryBank

    P, s, H, W, n_img, C = case
    noise = torch.from_numpy(R.bank_images(case, seed))
    clean = torch.from_numpy(R.bank_images(case, seed + 1))
    return MemoryBank(noise.to(DEV), clean.to(DEV), P, s), noise


@pytest.mark.parametrize("B", R.SELECT_B)
@pytest.mark.parametrize("case", R.SELECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_select_planted_random_gather(case, B, golden):
    P, s, H, W, n_img, C = case
    bank, noise = _bank(case, R.select_seed(case, B))
    patches = R.bank_patches(noise, P, s)
    N = patches.shape[0]
    assert len(bank) == N
    # (a) perturbed bank windows: first / last window of the first / last image, then spread; sent
    # in batches of exactly B queries (the last one may be shorter)
    per = N // n_img
    plant = torch.tensor([0, per - 1, N - per, N - 1] + [(k * 7919) % N for k in range(1, B + 1)])
    g = torch.Generator().manual_seed(R.select_seed(case, B))
    q = patches[plant] + 0.05 * torch.randn(patches[plant].shape, generator=g)
    got = torch.cat([bank.select(qq.to(DEV)).cpu() for qq in torch.split(q, B)])
    assert torch.equal(R.select(q.double(), patches.double())[0], plant)  # planted = fp64 argmin
    assert torch.equal(got, plant), (got, plant)
    # (b) uniform-random queries vs the fp64 argmin; near-ties below GAP_SKIP are skipped
    q = torch.from_numpy(R.random_queries(case, B))
    idx, best, second, scale = R.select(q.double(), patches.double())
    keep = ((second - best) / scale >= R.GAP_SKIP)
    skipped = int((~keep).sum())
    assert skipped * 64 <= B
    if C == 1 and P >= 16:
        assert skipped == 0
    fx = golden("memory_adapter.npz")
    assert np.array_equal(fx[f"sel_{P}_{s}_{H}_{W}_{n_img}_{C}_B{B}_idx64"], idx.numpy())
    got = bank.select(q.to(DEV)).cpu()
    assert torch.equal(got[keep], idx[keep]), (got, idx)
    # from_patches: the same kernel over the materialised bank
    from image_denoising_amd.memory import MemoryBank

    mat = MemoryBank.from_patches(bank.noise_patches(), bank.clean_patches())
    assert torch.equal(mat.select(q.to(DEV)).cpu(), got)
    # gather: bit-equal to indexing the materialised clean bank
    sel = torch.cat([got, plant]).to(DEV)
    assert torch.equal(bank.gather_clean(sel), bank.clean_patches()[sel])
    assert torch.equal(bank.noise_patches().cpu(), patches)


def test_select_exact_tie_takes_lowest_index():
    from image_denoising_amd.memory import MemoryBank

    case = (16, 4, 40, 44, 2, 1)
    img = torch.from_numpy(R.bank_images((16, 4, 40, 44, 1, 1), 99))
    two = torch.cat([img, img]).to(DEV)
    bank = MemoryBank(two, two, 16, 4)
    per = len(bank) // 2
    pick = torch.tensor([0, 5, per - 1])
    q = bank.noise_patches()[pick.to(DEV) + per] + 0.01  # equally far from both copies
    assert torch.equal(bank.select(q).cpu(), pick)


# ---- adapter ---------------------------------------------------------------------------------------
def _module(name):
    from image_denoising_amd.memory import HyperGatedResidualAdapter, HyperGatedResidualAdapter_FFT

    B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
    params, noisy, base, mem, dout = R.adapter_case(name)
    ad = (HyperGatedResidualAdapter_FFT(C, Hc, nb, clamp) if nb > 0
          else HyperGatedResidualAdapter(C, Hc, clamp))
    assert list(ad.state_dict()) == R.KEYS
    ad.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    assert np.array_equal(ad.flat_params.numpy(), R.flat_of(params))
    return ad.to(DEV), [torch.from_numpy(v).to(DEV) for v in (noisy, base, mem, dout)]


@pytest.mark.parametrize("name", list(R.ADAPTER_CASES))
def test_adapter_forward_backward_vs_fp64(name, golden):
    fx = golden("memory_adapter.npz")
    B, C, H, W, Hc, nb, clamp = R.ADAPTER_CASES[name]
    params, noisy, base, mem, dout = R.adapter_case(name)
    want_sum = [v.astype(np.float64).sum() for v in (noisy, base, mem, dout)] \
        + [R.flat_of(params).astype(np.float64).sum()]
    assert np.array_equal(fx[name + "_insum"], np.array(want_sum))  # the generators have not drifted
    f64, o64, pre64, g64 = R.run_case(name)
    if clamp:
        assert (pre64 < 0).double().mean() > 0.01 and (pre64 > 1).double().mean() > 0.01
    ad, (n, b, m, d) = _module(name)
    feat = ad.features(n, b, m)
    out = ad(n, b, m)
    out.backward(d)
    grads = dict(ad.named_parameters())
    flat64 = torch.cat([g64[k].reshape(-1) for k in R.KEYS]).numpy()
    report, bad = [], []

    def check(what, got, want, ref32):
        tol = 4 * rel(ref32, want)
        err = rel(got, want)
        report.append(f"{name} {what}: err {err:.2e} tol {tol:.2e}")
        if not err <= tol:
            bad.append(report[-1])

    check("feat", feat.cpu().numpy(), f64.numpy(), fx[name + "_feat"])
    check("out", out.detach().cpu().numpy(), o64.numpy(), fx[name + "_out"])
    off = 0
    for k in R.KEYS:
        cnt = g64[k].numel()
        assert grads[k].grad is not None, k
        check("d " + k, grads[k].grad.cpu().numpy().reshape(-1), flat64[off:off + cnt],
              fx[name + "_grad"][off:off + cnt])
        off += cnt
    print("\n".join(report))
    assert not bad, bad
    # bit-identical repeated runs
    ad.zero_grad()
    out2 = ad(n, b, m)
    out2.backward(d)
    assert torch.equal(out2, out)
    for k in R.KEYS:
        assert torch.equal(dict(ad.named_parameters())[k].grad, grads[k].grad)


def test_features_of_rows_wider_than_the_lds_twiddle_table():
    """W = 1030 > 1024 (twiddles from the workspace, 516 bins in two passes), no power of two.
    The kernel works in fp64 and rounds once to fp32: 2^-24 relative; 2 x that is allowed."""
    from image_denoising_amd.memory import HyperGatedResidualAdapter_FFT

    ad = HyperGatedResidualAdapter_FFT(1, 16).to(DEV)
    x = [torch.from_numpy(R.uniform(2 * 3 * 1030, 900 + k).reshape(2, 1, 3, 1030).astype(np.float32))
         for k in range(3)]
    want = R.features(*(t.double() for t in x), 3).numpy()
    got = ad.features(*(t.to(DEV) for t in x)).cpu().numpy()
    assert np.abs(got - want).max() <= 2 * 2.0 ** -24 * np.abs(want).max()
    from image_denoising_amd._lib import DenoiseHipError
    from image_denoising_amd.memory import HyperGatedResidualAdapter

    with pytest.raises(DenoiseHipError):  # one element per sample: no unbiased std
        HyperGatedResidualAdapter(1, 16).to(DEV).features(
            *(t[:, :, :1, :1].contiguous().to(DEV) for t in x))


def test_zero_init_module_returns_clamped_base():
    from image_denoising_amd.memory import HyperGatedResidualAdapter_FFT

    torch.manual_seed(3)
    ad = HyperGatedResidualAdapter_FFT(1, 16).to(DEV)
    _, noisy, base, mem, _ = R.adapter_case("b3c1_17x23")
    n, b, m = (torch.from_numpy(v).to(DEV) for v in (noisy, base, mem))
    with torch.no_grad():
        assert torch.equal(ad(n, b, m), b.clamp(0, 1))
    with pytest.raises(NotImplementedError):
        ad(n, b.clone().requires_grad_(True), m)


# ---- the step ---------------------------------------------------------------------------------------
def _step_setup(seed=0):
    from image_denoising_amd.arch_unet import UNet
    from image_denoising_amd.memory import DenoiserWithMemoryAdapter, MemoryBank

    case = (32, 4, 48, 52, 2, 1)
    noise = torch.from_numpy(R.bank_images(case, 300))
    clean_imgs = (noise * 0.8 + 0.1)
    bank = MemoryBank(noise.to(DEV), clean_imgs.to(DEV), 32, 4)
    torch.manual_seed(seed)
    base = UNet(1, 1, 48)
    sd = base.state_dict()  # an untrained base near 0.5, so that few pixels sit in the clamp
    sd["nin_c.weight"] = sd["nin_c.weight"] * 0.05
    sd["nin_c.bias"] = torch.full_like(sd["nin_c.bias"], 0.5)
    base.load_state_dict(sd)
    model = DenoiserWithMemoryAdapter(base, 1, 16, bank).to(DEV)
    params, *_ = R.adapter_case("b3c1_17x23")  # non-zero adapter: every gradient is live
    model.adapter.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    clean = torch.from_numpy(R.uniform(4 * 32 * 32, 301).reshape(4, 1, 32, 32).astype(np.float32))
    noisy = (clean + 0.1 * torch.from_numpy(R.uniform(4 * 32 * 32, 302).reshape(4, 1, 32, 32)
                                            .astype(np.float32) - 0.05)).to(DEV)
    return model, clean.to(DEV), noisy


@pytest.mark.parametrize("lam_iq", [0.1, 0.0])
def test_step_equals_unfused_sequence_to_the_bit(lam_iq):
    """losses, gradient and updated parameters of one fused step == module forward, the loss
    call, autograd and FlatAdam, to the bit (the same kernels on the same inputs)"""
    from image_denoising_amd.finetune import finetune_iqsl_loss, finetune_loss
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer
    from image_denoising_amd.optim import FlatAdam

    model, clean, noisy = _step_setup()
    iq = dict(t1=0.3, t2=0.7)
    pred = model(noisy)
    if lam_iq > 0:
        loss, dpred = finetune_iqsl_loss(pred.detach(), clean, 0.1, lam_iq, **iq)
    else:
        loss, dpred = finetune_loss(pred.detach(), clean, 0.1)
    pred.backward(dpred)
    g_auto = torch.cat([p.grad.reshape(-1) for p in model.adapter._params()])
    assert len(model.adapter._params()) == 10 and bool((g_auto != 0).any())
    flat2 = model.adapter.flat_params.clone()
    FlatAdam(flat2, lr=1e-3).step(g_auto, grad_scale=1.0)
    tr = MemoryFinetuneTrainer(model, lr=1e-3, lambda_grad=0.1, lambda_iqsl=lam_iq,
                               iqsl=iq if lam_iq > 0 else None)
    got = tr.train_step(clean, noisy)
    assert got.numel() == (4 if lam_iq > 0 else 3)
    assert torch.equal(got, loss)
    assert torch.equal(tr.grad, g_auto)
    assert torch.equal(model.adapter.flat_params, flat2)


def test_ten_steps_lower_the_loss():
    from image_denoising_amd.finetune_memory import MemoryFinetuneTrainer

    model, clean, noisy = _step_setup()
    tr = MemoryFinetuneTrainer(model, lr=1e-3, lambda_grad=0.1, lambda_iqsl=0.1,
                               iqsl=dict(t1=0.3, t2=0.7))
    losses = torch.stack([tr.train_step(clean, noisy)[3] for _ in range(10)]).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


# ---- inference ---------------------------------------------------------------------------------------
class _Identity(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x


def _infer_model(P):
    from image_denoising_amd.memory import DenoiserWithMemoryAdapter, MemoryBank

    noise = torch.from_numpy(R.bank_images((P, 4, P + 9, P + 13, 2, 1), 400))
    bank = MemoryBank(noise.to(DEV), (noise * 0.8 + 0.1).to(DEV), P, 4)
    model = DenoiserWithMemoryAdapter(_Identity(), 1, 16, bank).to(DEV)
    params, *_ = R.adapter_case("b3c1_17x23")
    model.adapter.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return model


@pytest.mark.parametrize("case", R.BLEND_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patchwise_inference(case, golden):
    from image_denoising_amd import memory as M

    H, W, P, ov = case
    img = R.blend_image(case)
    ys, xs = M.patch_origins(H, P, ov), M.patch_origins(W, P, ov)
    # the blend alone, against the reference's own image (stub model x * 0.9 + 0.05) to the bit
    t = torch.from_numpy(img / np.float32(255.0))
    patches = torch.stack([t[y:y + P, x:x + P] for y in ys for x in xs])[:, None]
    stub = (patches * 0.9 + 0.05).to(DEV)
    got = M.hann_blend(stub, ys, xs, H, W).cpu().numpy()
    assert np.array_equal(got[0], golden("memory_adapter.npz")[f"blend_{H}_{W}_{P}_{ov}"][..., 0])
    assert rel(got, R.hann_blend(stub.cpu().numpy(), ys, xs, H, W, np.float64)) < 1e-6
    # the whole function: one batch == one patch at a time
    model = _infer_model(P)
    pred, pred255 = M.denoise_full_image_patchwise(model, img, P, ov, return_pred255=True)
    assert pred.shape == (H, W, 1) and pred.dtype == np.float32
    with torch.no_grad():
        one = torch.cat([model(p[None].to(DEV)) for p in patches])
        batch = model(patches.to(DEV))
    assert rel(batch.cpu().numpy(), one.cpu().numpy()) <= 4 * 6.8e-8  # the adapter's `out` bound
    want = R.hann_blend(batch.cpu().numpy(), ys, xs, H, W)
    assert np.array_equal(pred[..., 0], want[0])
    assert np.array_equal(pred255, np.clip(pred * 255.0 + 0.5, 0, 255).astype(np.uint8))


def test_cli_end_to_end(tmp_path):
    from PIL import Image

    from image_denoising_amd import checkpoint, evaluation, evaluation_memory
    from image_denoising_amd.arch_unet import UNet

    rng = np.random.RandomState(5)
    for sub in ("clean", "noise"):
        (tmp_path / "data" / sub).mkdir(parents=True)
    for k in range(4):
        c = rng.randint(0, 256, (64, 64)).astype(np.uint8)
        n = np.clip(c + rng.randint(-20, 21, (64, 64)), 0, 255).astype(np.uint8)
        Image.fromarray(c).save(tmp_path / "data" / "clean" / f"im{k}.png")
        Image.fromarray(n).save(tmp_path / "data" / "noise" / f"im{k}.png")
    torch.manual_seed(0)
    checkpoint.save_checkpoint(UNet(1, 1, 48), str(tmp_path / "base.pth"))
    model = _infer_model(32)
    checkpoint.save_adapter_checkpoint(model, str(tmp_path / "adapter.pth"))
    lines = []
    evaluation_memory.main(["--data_dir", str(tmp_path / "data"), "--save_dir", str(tmp_path / "out"),
                            "--base_ckpt", str(tmp_path / "base.pth"),
                            "--adapter_ckpt", str(tmp_path / "adapter.pth"), "--patch_size", "32",
                            "--overlap", "16", "--num_memory_images", "2", "--memory_stride", "4",
                            "--compute_iq_iou"], out=lines.append)
    psnr_lines = [ln for ln in lines if "PSNR" in ln and "im3" in ln]
    assert psnr_lines, lines
    saved = np.array(Image.open(tmp_path / "out" / "im3_denoised_mem.png"))
    clean = np.array(Image.open(tmp_path / "data" / "clean" / "im3.png"))
    want = evaluation.calculate_psnr(saved, clean)
    assert f"PSNR={want:.2f} dB" in psnr_lines[0] and "IoU(d/m/b)" in psnr_lines[0], psnr_lines[0]
    assert lines[-1] == "Inference with memory adapter model finished."


def test_adapter_checkpoint_roundtrip(tmp_path):
    from image_denoising_amd import checkpoint

    model = _infer_model(32)
    path = checkpoint.save_adapter_checkpoint(model, str(tmp_path / checkpoint.adapter_checkpoint_name(3)))
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert list(state) == R.KEYS
    torch.save({"module." + k: v for k, v in state.items()}, str(tmp_path / "dp.pth"))
    for p in (path, str(tmp_path / "dp.pth")):
        other = _infer_model(32)
        other.adapter.flat_params.zero_()
        missing, unexpected = checkpoint.load_adapter_checkpoint(other, p)
        assert not missing and not unexpected
        assert torch.equal(other.adapter.flat_params, model.adapter.flat_params)
    assert "bank" not in "".join(model.state_dict())
