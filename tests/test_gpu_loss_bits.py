"""Every loss and metric kernel on csrc/block_reduce.h reproduces its recorded bits.

tests/golden/loss_bits.json holds the fp32 / fp64 bits of every scalar and SHA-256 digests of every
gradient tensor, recorded by tests/golden/make_loss_bits.py (which lists the cases and why each
shape is there) with a library from before the kernels shared one reduction.  The other tests
bound these kernels against fp64 references, which a reordered sum would pass; the sums are
fixed-order, so the same kernels on the same inputs give the same bits.  A
mismatch fails and names the recording toolchain: IQSL's exp / log and SSIM's exp come from the
compiler's device math library, so another ROCm release may legitimately differ there.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "make_loss_bits", os.path.join(HERE, "golden", "make_loss_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(HERE, "golden", "loss_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _recorded_with():
    return (f"recorded from {GOLDEN['commit']} with {GOLDEN['dn_version']}, ROCm {GOLDEN['rocm']} "
            f"on {GOLDEN['device']}; this run: {rec.toolchain()}")


def test_fixture_holds_every_case():
    assert GOLDEN["commit"] and GOLDEN["dn_version"].startswith("denoise_hip") and GOLDEN["rocm"]
    assert sorted(GOLDEN["cases"]) == sorted(rec.KEYS)


@pytest.mark.parametrize("key", rec.KEYS)
def test_loss_bits_unchanged(key):
    got, want = rec.digests(key), GOLDEN["cases"][key]
    diff = {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want))
            if got.get(k) != want.get(k)}
    assert not diff, f"{key}: (got, recorded) {diff}; {_recorded_with()}"


@pytest.mark.parametrize("shape", list(rec.SHAPES))
@pytest.mark.parametrize("margin", list(rec.MARGINS))
def test_finetune_and_iqsl_share_one_pixel_body(shape, margin):
    """dn_finetune_iqsl_loss at lambda_iqsl = 0 against dn_finetune_loss on the same input and
    lambda_grad: dpred, loss_l1, loss_grad and the total carry the same bits"""
    iq = rec.finetune_iqsl(shape, margin, 0.0)
    ft = rec.finetune(shape, one_channel=True)
    assert rec.bits(iq["dpred"]) == rec.bits(ft["dpred"])
    assert rec.bits(iq["loss4"][:2]) == rec.bits(ft["loss3"][:2])
    assert rec.bits(iq["loss4"][3:]) == rec.bits(ft["loss3"][2:])
