"""The executors' host orchestration reproduces the recorded backward bit for bit.

tests/golden/backward_bits.json holds SHA-256 digests of y, dx and every layer's [W | b] range of
dparams, recorded by tests/golden/make_backward_bits.py with a library from before the UNet's and
the RESNET's shared pieces moved into csrc/exec_common.{h,cpp}.  Weight-gradient reductions are
fixed-order, so host code that launches the same kernels on the same arguments gives the same
bits; a digest that differs names the layer whose launch changed.
"""
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORDER = os.path.join(HERE, "golden", "make_backward_bits.py")

_spec = importlib.util.spec_from_file_location("make_backward_bits", RECORDER)
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(HERE, "golden", "backward_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _differing(got, want):
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_fixture_holds_every_case():
    assert GOLDEN["commit"] and GOLDEN["dn_version"].startswith("denoise_hip")
    assert sorted(GOLDEN["cases"]) == sorted(rec.KEYS)


@pytest.mark.parametrize("key", rec.KEYS)
def test_backward_bits_unchanged(key):
    assert _differing(rec.digests(key), GOLDEN["cases"][key]) == []


def test_backward_bits_unchanged_on_one_stream():
    """DN_BWD_STREAMS is read once per process: a fresh child runs the backward on one stream"""
    env = dict(os.environ, DN_BWD_STREAMS="0")
    p = subprocess.run([sys.executable, RECORDER, "--print", *rec.ONE_STREAM_KEYS], env=env,
                       cwd=ROOT, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for key in rec.ONE_STREAM_KEYS:
        assert _differing(got[key], GOLDEN["cases"][key]) == [], key
