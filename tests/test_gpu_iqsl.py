"""The IQSL finetune loss (csrc/adapter.hip: k_iqsl_sums, k_iqsl_finalize, k_iqsl_grad), the IQ-IoU
counts (csrc/eval.hip: k_iq_iou_part) and their Python surface.  Needs an MI355X.

Buffers handed to the C entry points are the guarded views of tests/test_gpu_step_ops.py (256
bytes of 0xA5 on each side that must survive; shift=1 moves a view one element off 16-byte
alignment).  Tolerances: 1e-4 against the reference program's fixture, the bounds
tests/iqsl_ref.py derives from the restatement's own magnitudes against the fp64 restatement, and
bit equality where the header promises it.

Routes: all three kernels run 1024 blocks x 256 threads with a grid-stride loop; the `big` shape
(300000 elements > 262144) takes the second trip of both loops.  With lambda_iqsl == 0 the
launcher skips k_iqsl_grad.
"""
import os

import numpy as np
import pytest
import torch

import iqsl_ref as R
from test_gpu_step_ops import ERR_ARG, Buf, L, S, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L().lib()


@pytest.fixture(scope="module")
def totals():
    cache = {}

    def get(case, shape, lam_iq=R.LAMBDA_IQSL):
        if (case, shape, lam_iq) not in cache:
            cache[(case, shape, lam_iq)] = R.case_total(case, shape, lam_iq)
        return cache[(case, shape, lam_iq)]

    return get


def _partials():
    return Buf((int(L().lib().dn_iqsl_partials_size()),), torch.uint8)


def _run(pred, target, case, lam_iq=R.LAMBDA_IQSL, shift=0, t1=R.T1, t2=R.T2):
    """dn_finetune_iqsl_loss on guarded views -> (dpred, loss4) numpy; guard bands checked"""
    tau, margin, cef = R.CASES[case]
    N, C, H, W = pred.shape
    bp, bt = Buf(pred.shape, shift=shift, init=pred), Buf(pred.shape, shift=shift, init=target)
    dp, loss4, part = Buf(pred.shape, shift=shift), Buf((4,), shift=shift), _partials()
    L().call("dn_finetune_iqsl_loss", bp.ptr, bt.ptr, N, C, H, W, R.LAMBDA_GRAD, lam_iq, t1, t2,
             tau, margin, cef, dp.ptr, loss4.ptr, part.ptr, S())
    torch.cuda.synchronize()
    for b, what in ((bp, "pred"), (bt, "target"), (dp, "dpred"), (loss4, "loss4"),
                    (part, "partials")):
        b.check(what)
    assert same_bits(bp.np(), pred) and same_bits(bt.np(), target), "an input was written"
    return dp.np(), loss4.np()


def _run_plain(pred, target):
    """dn_finetune_loss (the loss without IQSL) -> (dpred, loss3) numpy"""
    N, C, H, W = pred.shape
    bp, bt = Buf(pred.shape, init=pred), Buf(pred.shape, init=target)
    dp, loss3 = Buf(pred.shape), Buf((3,))
    part = Buf((int(L().lib().dn_loss_partials_size()),), torch.uint8)
    L().call("dn_finetune_loss", bp.ptr, bt.ptr, N, C, H, W, R.LAMBDA_GRAD, dp.ptr, loss3.ptr,
             part.ptr, S())
    torch.cuda.synchronize()
    return dp.np(), loss3.np()


@pytest.mark.parametrize("case,shape", R.PAIRS)
def test_loss_and_gradient_vs_fixture_and_fp64(golden, totals, case, shape):
    g = golden("iqsl.npz")
    k = f"{case}_{shape}_"
    pred, target, r = totals(case, shape)
    dpred, loss4 = _run(pred, target, case)
    # the reference program's fixture: 1e-4 relative, 1e-4 of max |dpred|
    for i, name in enumerate(("l1", "grad", "iqsl", "loss")):
        want = float(g[k + "loss4"][i])
        print(f"{name}: {loss4[i]!r} fixture {want!r} fp64 {r['loss4'][i]!r} "
              f"err {abs(loss4[i] - r['loss4'][i]):.3e} bound {r['b_loss4'][i]:.3e}")
    for i, name in enumerate(("l1", "grad", "iqsl", "loss")):
        want = float(g[k + "loss4"][i])
        assert abs(float(loss4[i]) - want) <= TOL * abs(want), name
        assert abs(float(loss4[i]) - r["loss4"][i]) <= r["b_loss4"][i], name
    dmax = float(g[k + "dmax"])
    err_fx = np.abs(dpred.reshape(-1)[g[k + "idx"]].astype(np.float64) - g[k + "dpred"]).max()
    err = np.abs(dpred.astype(np.float64) - r["dpred"])
    print(f"dpred: err vs fixture / max {err_fx / dmax:.3e}; worst err / bound vs fp64 "
          f"{float((err / r['b_dpred']).max()):.3f}")
    assert err_fx <= TOL * dmax
    assert (err <= r["b_dpred"]).all()
    if case == "inmargin":  # no valid pixel: iqsl is 0 and its gradient exactly 0
        d0, _ = _run_plain(pred, target)
        assert loss4[2] == 0.0 and same_bits(dpred, d0)
    if case == "tauclamp":  # saturated softmax: p is one-hot, so d iqsl is exactly 0 as well
        d0, _ = _run_plain(pred, target)
        assert same_bits(dpred, d0) and loss4[2] > 0.0


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_lambda_iqsl_zero_equals_finetune_loss_bits(totals, shape):
    """header: with lambda_iqsl == 0, dpred and loss4[0..1] carry dn_finetune_loss's bits"""
    pred, target, _ = totals("m05", shape)
    dpred, loss4 = _run(pred, target, "m05", lam_iq=0.0)
    d0, loss3 = _run_plain(pred, target)
    assert same_bits(dpred, d0)
    assert same_bits(loss4[:2], loss3[:2])
    r = R.case_total("m05", shape, 0.0)[2]
    assert abs(float(loss4[2]) - r["loss4"][2]) <= r["b_loss4"][2]  # iqsl is still reported
    assert abs(float(loss4[3]) - r["loss4"][3]) <= r["b_loss4"][3]


@pytest.mark.parametrize("case,shape", [("m05", "small"), ("m05", "mid"), ("m0", "big")])
def test_misaligned_views_and_second_call_equal_bits(totals, case, shape):
    pred, target, _ = totals(case, shape)
    d_a, l_a = _run(pred, target, case)
    d_b, l_b = _run(pred, target, case)
    assert same_bits(d_a, d_b) and same_bits(l_a, l_b), "two calls differ"
    d_c, l_c = _run(pred, target, case, shift=1)
    assert same_bits(d_a, d_c) and same_bits(l_a, l_c), "a view one float off alignment differs"


def test_iqsl_alone_autograd_surface(totals):
    """finetune.iqsl_loss: the scalar and its gradient through torch autograd, [B,1,H,W] and
    [B,H,W]; bound u |g| + n64 G (tests/iqsl_ref.py), doubled"""
    from image_denoising_amd.finetune import iqsl_loss

    pred, target, _ = totals("m05", "mid")
    tau, margin, cef = R.CASES["m05"]
    r = R.iqsl(pred[:, 0], target[:, 0], R.T1, R.T2, tau, margin, cef)
    n64 = pred.size * 2.0 ** -52
    for squeeze in (False, True):
        p = torch.from_numpy(pred[:, 0] if squeeze else pred).to(DEV).requires_grad_(True)
        t = torch.from_numpy(target[:, 0] if squeeze else target).to(DEV)
        loss = iqsl_loss(p, t, R.T1, R.T2, tau=tau, margin=margin, ce_factor=cef)
        (3.0 * loss).backward()
        assert loss.dim() == 0 and p.grad.shape == p.shape
        assert abs(loss.item() - r["loss"]) <= 2.0 * (R.U * abs(r["loss"]) + n64 * (1 + abs(cef * r["ce"])))
        got = p.grad.cpu().numpy().astype(np.float64).reshape(r["dz"].shape)
        bound = 2.0 * (2.0 * R.U * np.abs(3.0 * r["dz"]) + 3.0 * n64 * r["G"])
        assert (np.abs(got - 3.0 * r["dz"]) <= bound).all()
        assert np.abs(got).max() > 0


def test_errors_launch_nothing(totals):
    from image_denoising_amd.finetune import finetune_iqsl_loss, iqsl_loss

    pred, target, _ = totals("m0", "small")
    N, C, H, W = pred.shape
    bp, bt = Buf(pred.shape, init=pred), Buf(pred.shape, init=target)
    dp, loss4, part = Buf(pred.shape), Buf((4,)), _partials()

    def call(n, c, t1, t2):
        L().call("dn_finetune_iqsl_loss", bp.ptr, bt.ptr, n, c, H, W, 0.1, 0.1, t1, t2, 0.1, 0.0,
                 0.5, dp.ptr, loss4.ptr, part.ptr, S())

    with pytest.raises(L().DenoiseHipError, match=ERR_ARG + ".*C must be 1"):
        call(1, 2, R.T1, R.T2)  # the same 70 floats as [1,2,5,7]
    for t1, t2 in ((0.5, 0.5), (0.7, 0.3), (float("nan"), 0.7), (0.3, float("inf"))):
        with pytest.raises(L().DenoiseHipError, match=ERR_ARG):
            call(N, C, t1, t2)
    torch.cuda.synchronize()
    assert dp.untouched() and loss4.untouched() and part.untouched()
    p3 = torch.rand(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        finetune_iqsl_loss(p3, p3.clone(), t1=R.T1, t2=R.T2)
    with pytest.raises(ValueError):
        iqsl_loss(p3, p3.clone(), R.T1, R.T2)
    p1 = torch.rand(2, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        finetune_iqsl_loss(p1, p1.clone(), t1=0.7, t2=0.3)


# =============================================================================================
# IQ-IoU
# =============================================================================================
IQ_NAMES = ["c1_7x9", "c3_7x9", "c1_64x80", "c3_64x80", "c1_7x9_nomid"]


@pytest.mark.parametrize("name", IQ_NAMES)
def test_iq_iou_counts_equal_fixture(golden, name):
    from image_denoising_amd.evaluation import compute_iq_iou

    g = golden("iqsl.npz")
    k = f"iq_{name}_"
    pred, clean = g[k + "pred"], g[k + "clean"]
    chw = lambda a: a[None] if a.ndim == 2 else np.ascontiguousarray(a.transpose(2, 0, 1))  # noqa: E731
    C, H, W = chw(pred).shape
    bp, bc = Buf((C, H, W), torch.uint8, init=chw(pred)), Buf((C, H, W), torch.uint8, init=chw(clean))
    counts = Buf((6,), torch.int64)
    part = Buf((int(L().lib().dn_eval_partials_size()),), torch.uint8)
    t1, t2 = (float(v) for v in g[k + "t"])
    L().call("dn_iq_iou_u8", bp.ptr, bc.ptr, C, H, W, t1, t2, part.ptr, counts.ptr, S())
    torch.cuda.synchronize()
    for b, what in ((bp, "pred"), (bc, "clean"), (counts, "counts"), (part, "partials")):
        b.check(what)
    print(name, counts.np(), g[k + "counts"])
    assert np.array_equal(counts.np(), g[k + "counts"])
    # the Python surface: quantiles on the host, then the same counts; float32 clean images too
    for cl in (clean, clean.astype(np.float32)):
        ious = np.array(compute_iq_iou(pred, cl, *g[k + "q"]))
        assert np.array_equal(np.isnan(ious), np.isnan(g[k + "ious"]))
        assert np.array_equal(ious[~np.isnan(ious)], g[k + "ious"][~np.isnan(ious)])
    if name == "c1_7x9_nomid":
        assert np.isnan(ious[1])


def test_iq_iou_rejects_bad_arguments():
    b = Buf((1, 4, 4), torch.uint8, init=np.zeros((1, 4, 4), np.uint8))
    counts = Buf((6,), torch.int64)
    part = Buf((int(L().lib().dn_eval_partials_size()),), torch.uint8)
    for C, t1, t2 in ((0, 0.2, 0.8), (1, 0.8, 0.2), (1, float("nan"), 0.8)):
        with pytest.raises(L().DenoiseHipError, match=ERR_ARG):
            L().call("dn_iq_iou_u8", b.ptr, b.ptr, C, 4, 4, t1, t2, part.ptr, counts.ptr, S())
    torch.cuda.synchronize()
    assert counts.untouched()


# =============================================================================================
# Trainer and checkpoints
# =============================================================================================
def _model(seed=0):
    from image_denoising_amd.adapter import DenoiserWithAdapter
    from image_denoising_amd.arch_unet import UNet

    torch.manual_seed(seed)
    base = UNet(in_nc=1, out_nc=1, n_feature=48)
    torch.manual_seed(seed + 1)
    return DenoiserWithAdapter(base, in_channels=1, hidden_channels=16).to(DEV)


def test_trainer_two_steps_vs_fp64_restatement():
    """FinetuneTrainer(lambda_iqsl=0.1): two steps on 2x1x32x32 against oracle.adapter_ref's
    adapter (fp64) + tests/iqsl_ref.total + torch.optim.Adam, fed the HIP base's own output (the
    frozen base is not what this pins).  Losses at 1e-4; adapter parameters at
    test_finetune_step_vs_reference_fixture's bound, 1e-6 absolute."""
    from image_denoising_amd.finetune import FinetuneTrainer
    from oracle import adapter_ref

    model = _model()
    iq = dict(t1=R.T1, t2=R.T2, tau=0.1, margin=0.02, ce_factor=0.5)
    tr = FinetuneTrainer(model, lr=1e-4, lambda_grad=0.1, lambda_iqsl=0.1, iqsl=iq)
    n = 2 * 32 * 32
    clean = R.uniform(n, 77).astype(np.float32).reshape(2, 1, 32, 32)
    noisy = (clean + 0.2 * (R.uniform(n, 78).reshape(clean.shape) - 0.5)).astype(np.float32)
    cd, nd = torch.from_numpy(clean).to(DEV), torch.from_numpy(noisy).to(DEV)
    with torch.no_grad():
        base_out = model.base(nd).cpu().double()
    p = model.adapter.flat_params.detach().cpu().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-4)
    for step in range(2):
        loss4 = tr.train_step(cd, nd).cpu().numpy()
        pred = adapter_ref.adapter_forward(p, torch.from_numpy(noisy).double(), base_out)
        r = R.total(pred.detach().float().numpy(), clean, 0.1, 0.1, **iq)
        opt.zero_grad()
        pred.backward(torch.from_numpy(r["dpred"]))
        opt.step()
        print(step, loss4, r["loss4"])
        assert loss4.shape == (4,)
        assert (np.abs(loss4 - r["loss4"]) <= TOL * np.abs(r["loss4"])).all()
        assert r["loss4"][2] > 0.01
        err = np.abs(model.adapter.flat_params.cpu().numpy() - p.detach().numpy()).max()
        print("param err", err)
        assert err < 1e-6


def test_trainer_without_iqsl_is_the_plain_step():
    """lambda_iqsl = 0 (the default): loss3 and the parameters after a step carry the bits of a
    trainer built without the new arguments; lambda_iqsl > 0 without thresholds is an error"""
    from image_denoising_amd.finetune import FinetuneTrainer

    gen = torch.Generator().manual_seed(5)
    clean = torch.rand(2, 1, 32, 32, generator=gen).to(DEV)
    noisy = (clean.cpu() + 0.1 * torch.randn(2, 1, 32, 32, generator=gen)).to(DEV)
    out = []
    for kw in ({}, dict(lambda_iqsl=0.0, iqsl=None)):
        model = _model()
        tr = FinetuneTrainer(model, lr=1e-4, lambda_grad=0.1, **kw)
        loss3 = tr.train_step(clean, noisy)
        assert loss3.shape == (3,)
        out.append((loss3.cpu(), model.adapter.flat_params.cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    with pytest.raises(ValueError):
        FinetuneTrainer(_model(), lambda_iqsl=0.1)


def test_adapter_only_checkpoint_round_trip(tmp_path):
    """an adapter-only file saved under the reference's name loads through --base_ckpt /
    --adapter_ckpt: same parameters, same denoised image, and --compute_iq_iou reports what
    tests/iqsl_ref.iq_counts gives for the saved image"""
    from PIL import Image

    from image_denoising_amd import evaluation_adapter as EA
    from image_denoising_amd.checkpoint import (adapter_checkpoint_name, save_adapter_checkpoint,
                                                save_checkpoint)

    model = _model(3)
    with torch.no_grad():
        model.adapter.flat_params.mul_(1.5)
    assert adapter_checkpoint_name(7) == "epoch_adapter_only_007.pth"
    base_ckpt = save_checkpoint(model.base, str(tmp_path / "epoch_model_001.pth"), data_parallel=True)
    ad_ckpt = save_adapter_checkpoint(model, str(tmp_path / adapter_checkpoint_name(7)))
    state = torch.load(ad_ckpt, map_location="cpu", weights_only=True)
    assert list(state) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]
    m2 = EA.build_model("UNet", 1, 48, 16).to(DEV)
    EA.load_base_and_adapter(m2, base_ckpt, ad_ckpt)
    assert torch.equal(m2.adapter.flat_params, model.adapter.flat_params)
    assert torch.equal(m2.base.flat_params, model.base.flat_params)
    lv = np.array([12, 40, 77, 77, 130, 181, 181, 240], np.uint8)
    clean = lv[(R.uniform(32 * 32, 9) * 8).astype(np.int64)].reshape(32, 32)
    noisy = np.clip(clean + (R.uniform(32 * 32, 10).reshape(32, 32) * 40 - 20).round(), 0, 255).astype(np.uint8)
    for sub, img in (("clean", clean), ("noise", noisy)):
        os.makedirs(tmp_path / "data" / sub)
        Image.fromarray(img).save(str(tmp_path / "data" / sub / "a.png"))
    res = EA.main(["--data_dir", str(tmp_path / "data"), "--base_ckpt", base_ckpt, "--adapter_ckpt",
                   ad_ckpt, "--arch", "UNet", "--save_dir", str(tmp_path / "out"),
                   "--compute_iq_iou"])
    saved = np.array(Image.open(str(tmp_path / "out" / "a_denoised.png")))
    assert np.array_equal(saved, EA.denoise(model, noisy).cpu().numpy()[0])
    t1, t2 = np.quantile(clean.astype(np.float32) / 255.0, [0.25, 0.75])
    n = R.iq_counts(saved, clean, t1, t2)
    want = [n[k] / n[3 + k] if n[3 + k] else np.nan for k in range(3)]
    assert len(res["psnr"]) == 1 and len(res["iq_iou"]) == 1
    np.testing.assert_array_equal(np.array(res["iq_iou"][0]), np.array(want, np.float64))
    np.testing.assert_array_equal(np.array(res["avg_iq_iou"]), np.array(want, np.float64))
    with pytest.raises(SystemExit):
        EA.parse_args(["--data_dir", "x", "--base_ckpt", base_ckpt])
