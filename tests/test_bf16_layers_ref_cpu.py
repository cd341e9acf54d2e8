"""tests/bf16_layers_ref.py is itself right: the per-layer references chained equal the bf16-emulating
oracle, the windowed evaluation equals the full one, read_buffer addresses both storages, and the
comparator rejects each fault that the end-to-end bounds of test_gpu_bf16.py let through."""
import pytest
import torch
import torch.nn.functional as F

import bf16_layers_ref as R
from oracle import unet_ref


def _flat(C, OC, seed=0):
    """unit-gain random parameters: every level contributes O(1) to y"""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for _, ws, bl, kind in unet_ref.layer_table(C, OC):
        fan_in = (ws[0] if kind == "deconv" else ws[1] * ws[2] * ws[3])
        parts.append((torch.randn(ws, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).flatten())
        parts.append(torch.randn(bl, generator=g, dtype=torch.float64) * 0.1)
    return torch.cat(parts)


def _rand(*shape, seed=1):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------
# chained references == the oracle's bf16 emulation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(1, 32, 32), (3, 32, 64)])
def test_chain_equals_oracle(C, H, W):
    """The oracle rounds the operands of the same layers (every 3x3 after enc_conv0, the deconvs,
    nin_a / nin_b -- hence na) and nothing else; the plan's bf16 stores are invisible to it because
    their readers round.  So the chain reproduces it to fp64 rounding."""
    flat, x = _flat(C, C), _rand(1, C, H, W)
    y, _ = R.chain(flat, x, C, C)
    ref = unet_ref.forward(flat, x, C, C, bf16_3x3=True)
    assert float(ref.abs().max()) > 1e-2
    assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_bf16_stores_change_no_later_value():
    """rounding a0, d{l}a and d1b to bf16 where the plan stores them leaves their readers' results
    bit-identical (what fwd_routes' comment on bf16_store claims)"""
    P = R.params(_flat(1, 1), 1, 1)
    a = R.enc0(_rand(1, 1, 8, 8), *P["enc_conv0"])
    assert torch.equal(R.conv3(a, *P["enc_conv1"]), R.conv3(R.rb(a), *P["enc_conv1"]))
    d = _rand(1, 96, 4, 4) - 0.5
    prm = (*P["nin_a"], *P["nin_b"], *P["nin_c"])
    assert torch.equal(R.head(d, *prm), R.head(R.rb(d), *prm))


# ---------------------------------------------------------------------------------------------
# windowed == full
# ---------------------------------------------------------------------------------------------
def _grid(t, bits):
    """t on the grid of multiples of 2^-bits"""
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


def _layers():
    # Parameters on a 2^-10 grid and inputs on a 2^-6 grid (full_eval): every product and every sum
    # of a conv or deconv is then exact in fp64, so the bit-for-bit comparison below tests the
    # window geometry whatever order the BLAS under torch adds in.
    P = R.params(_grid(_flat(3, 5), 10), 3, 5)
    return {
        "enc0": (R.bind(R.enc0, *P["enc_conv0"]), 3, 1, 1),
        "conv3": (R.bind(R.conv3, *P["dec_conv2a"]), 144, 1, 1),
        "conv3_pool": (R.bind(R.conv3_pool, *P["enc_conv2"]), 48, 1, 2),
        "deconv": (R.bind(R.deconv, *P["up2.deconv"]), 96, 2, 1),
        "head": (R.bind(R.head, *P["nin_a"], *P["nin_b"], *P["nin_c"]), 96, 1, 1),
    }


@pytest.fixture(scope="module")
def full_eval():
    """every kind of layer on one 2 x cin x 24 x 40 input, evaluated in full once"""
    out = {}
    for name, (fn, cin, num, den) in _layers().items():
        xin = _grid(_rand(2, cin, 24, 40, seed=len(name)) - 0.3, 6)
        out[name] = (fn, xin, fn(xin))
    return out


@pytest.mark.parametrize("name", ["enc0", "conv3", "conv3_pool", "deconv", "head"])
def test_windowed_equals_full_bit_for_bit(full_eval, name):
    fn, xin, full = full_eval[name]
    OH, OW = full.shape[-2:]
    wins = {"top-left": (0, 5, 0, 7), "top-right": (0, 4, OW - 6, OW), "bottom-left": (OH - 5, OH, 0, 3),
            "bottom-right": (OH - 3, OH, OW - 5, OW), "interior": (3, OH - 4, 5, OW - 6),
            "odd interior": (5, 8, 7, 12), "whole": (0, OH, 0, OW)}
    for wname, (y0, y1, x0, x1) in wins.items():
        got = R.windowed(fn, xin, y0, y1, x0, x1)
        assert got.shape == full[:, :, y0:y1, x0:x1].shape, (name, wname)
        assert torch.equal(got, full[:, :, y0:y1, x0:x1]), (name, wname)


def test_windowed_reads_other_float_types():
    """the device's buffers arrive as fp32 / bf16 NHWC views; only the rectangle is converted"""
    fn, cin = _layers()["conv3"][:2]
    x16 = (_rand(1, 12, 10, cin) - 0.5).bfloat16()  # NHWC, bf16
    view = R.nchw(x16)
    assert torch.equal(R.windowed(fn, view, 2, 9, 1, 8), fn(view.double())[:, :, 2:9, 1:8])


# ---------------------------------------------------------------------------------------------
# read_buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_read_buffer_round_trip(bf16):
    """a buffer at a non-zero offset with a pixel stride (20) wider than the channels read (7 from
    channel 5), at level 1 of a 2 x 8 x 12 image, surrounded by 0xFF bytes"""
    N, H, W, level, stride, off, c0, c1 = 2, 8, 12, 1, 20, 192, 5, 12
    h, w = H >> level, W >> level
    vals = (torch.arange(N * h * w * stride, dtype=torch.float32) * 0.25 - 100.0).view(N, h, w, stride)
    ws = torch.full((4 * off + 4 * vals.numel() + 64,), 0xFF, dtype=torch.uint8)
    raw = (vals.bfloat16() if bf16 else vals).contiguous().view(-1).view(torch.uint8)
    ws[4 * off:4 * off + raw.numel()] = raw
    got = R.read_buffer(ws, (off, stride, level), N, H, W, bf16, c0, c1)
    want = (vals.bfloat16() if bf16 else vals)[..., c0:c1]
    assert got.shape == (N, h, w, c1 - c0) and got.dtype == want.dtype
    assert torch.equal(got, want)
    assert torch.equal(R.nchw(got)[1, 3, 2, 4], want[1, 2, 4, 3])
    # the whole stride, and nothing of the 0xFF bytes around the buffer
    assert bool(torch.isfinite(R.read_buffer(ws, (off, stride, level), N, H, W, bf16).float()).all())
    assert bool(torch.isnan(R.read_buffer(ws, (0, 4, 0), 1, 4, 12, bf16).float()).all())


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def test_ulp_bf16():
    v = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.75, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133,
                         2.0 ** -133], dtype=torch.float64)
    assert torch.equal(R.ulp_bf16(v), want)
    # the spacing of torch's bf16 around v
    for x in (1.0, 0.3, 517.0, 1e-3):
        b = torch.tensor(x).bfloat16()
        nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
        assert float(nxt.double() - b.double()) == float(R.ulp_bf16(b.double()))


@pytest.fixture(scope="module")
def conv_ref():
    """a dec_conv-like 3x3 output [1, 96, 20, 36] and the activated conv before its pool"""
    P = R.params(_flat(1, 1), 1, 1)
    xin = _rand(1, 96, 20, 36, seed=3) - 0.3
    return xin, P


def _fp32_noise(ref, seed=9):
    """the reference moved by what fp32 accumulation may move it: 1e-6 of max|ref|"""
    g = torch.Generator().manual_seed(seed)
    return ref + (torch.rand(ref.shape, generator=g, dtype=torch.float64) - 0.5) * 2e-6 * float(ref.abs().max())


def test_check_passes_what_the_kernels_may_do(conv_ref):
    xin, P = conv_ref
    ref = R.conv3(xin, *P["dec_conv1b"])
    assert R.check(_fp32_noise(ref).float(), ref, False).ok
    assert R.check(_fp32_noise(ref).float().bfloat16(), ref, True).ok  # RNE of the fp32 value
    assert not R.check(_fp32_noise(ref).float().bfloat16(), ref, False).ok  # ... is not an fp32 store
    bad = ref.clone()
    bad[0, 5, 7, 9] = float("nan")
    c = R.check(bad, ref, True)
    assert not c.ok and c.index == (0, 5, 7, 9)


def test_check_rejects_bf16_truncation(conv_ref):
    """(a) a store that truncates where it should round to nearest even"""
    xin, P = conv_ref
    ref = R.conv3(xin, *P["dec_conv1b"])
    trunc = (ref.float().view(torch.int32) & -65536).view(torch.float32)
    assert float((trunc.double() - ref).abs().max()) < 2 ** -7 * float(ref.abs().max())  # still a bf16 of it
    assert not R.check(trunc, ref, True).ok


def test_check_rejects_tile_seam(conv_ref):
    """(b) column 16 of a 3x3 output taken from column 15"""
    xin, P = conv_ref
    ref = R.conv3(xin, *P["dec_conv1b"])
    dev = ref.clone()
    dev[..., 16] = ref[..., 15]
    c = R.check(dev.float(), ref, False)
    assert not c.ok and c.index[3] == 16


def test_check_rejects_pool_missing_a_tap(conv_ref):
    """(c) a pool that takes three of its four taps in the last pooled column"""
    xin, P = conv_ref
    w, b = P["enc_conv2"]
    xin = xin[:, :48]
    ref = R.conv3_pool(xin, w, b)
    a = R.conv3(xin, w, b)
    dev = ref.clone()
    last = a[..., -2:]
    dev[..., -1] = torch.stack([last[:, :, 0::2, 0], last[:, :, 0::2, 1], last[:, :, 1::2, 0]]).amax(0)
    assert R.check(ref.float(), ref, False).ok
    c = R.check(dev.float(), ref, False)
    assert not c.ok and c.index[3] == ref.shape[3] - 1


def test_check_rejects_deconv_parity_swap(conv_ref):
    """(d) output parities (1,0) and (0,1) swapped in the last input row"""
    xin, P = conv_ref
    ref = R.deconv(xin, *P["up2.deconv"])
    dev = ref.clone()
    y = xin.shape[2] - 1
    dev[:, :, 2 * y + 1, 0::2] = ref[:, :, 2 * y, 1::2]
    dev[:, :, 2 * y, 1::2] = ref[:, :, 2 * y + 1, 0::2]
    assert R.check(ref.float(), ref, False).ok
    c = R.check(dev.float(), ref, False)
    assert not c.ok and c.index[2] in (2 * y, 2 * y + 1)


@pytest.mark.parametrize("OC", [1, 16])
def test_head_bound_rejects_unrounded_na(OC):
    """(e) k_nin_head_x6's B1 branch rounds na before nin_b (bf16_layers_ref.head's docstring); a head
    that does not is far above the floor of legitimate disagreement, an fp32-accumulated one is
    within it by construction"""
    P = R.params(_flat(1, OC), 1, OC)
    prm = (*P["nin_a"], *P["nin_b"], *P["nin_c"])
    d1b = R.rb(F.leaky_relu(torch.randn(1, 96, 32, 32, generator=torch.Generator().manual_seed(4),
                                        dtype=torch.float64), 0.2))
    ref, rel, floor = R.head_bound(d1b, prm)
    assert 0.0 < floor and rel <= 1e-3
    assert R.check(R.head(d1b, *prm, acc32=True).float(), ref, False, rel=rel).ok
    assert not R.check(R.head(d1b, *prm, round_na=False).float(), ref, False, rel=rel).ok
    # ... and so is a head with nin_b's bias left out
    wa, ba, wb, bb, wc, bc = prm
    assert not R.check(R.head(d1b, wa, ba, wb, torch.zeros_like(bb), wc, bc).float(), ref, False, rel=rel).ok
