"""Records tests/golden/backward_bits.json: SHA-256 digests of y, dx and every layer's [W | b] range
of dparams for one forward + backward of the UNet, the RESNET and the ImprovedUNet, bit for bit,
from a library built BEFORE the executors' shared pieces moved into csrc/exec_common.{h,cpp}.

The committed file was recorded on an MI355X from commit 83500ad ("Add the memory-bank adapter
finetune and patchwise inference on HIP"), the parent of that refactor:

    git worktree add ../parent 83500ad
    (cd ../parent && DN_BUILD_TAG=parent python -m image_denoising_amd._build)
    DN_LIB_PATH=../parent/image_denoising_amd/libdenoise_hip_parent.so \
        python tests/golden/make_backward_bits.py tests/golden/backward_bits.json 83500ad

Weight-gradient reductions are fixed-order, so a host refactor that leaves every launch argument
alone reproduces every bit.  Each case is the recipe of tests/test_gpu_ws_independence.py::_train
(forward on a with-backward workspace, dy = rand(seed 5) - 0.5, backward with dx) on a network
seeded with torch.manual_seed(0), weights x10, x = rand(seed 17); each is run twice and refused if
the two runs differ.  tests/test_gpu_backward_bits.py recomputes the digests with digests() below;

    python tests/golden/make_backward_bits.py --print KEY [KEY ...]

prints them as JSON (the test's DN_BWD_STREAMS=0 child process).
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# key = "net:shape:precision"; UNet (N, C, out_nc, H, W), RESNET and ImprovedUNet (N, C, H, W)
UNET = [(1, 1, 1, 32, 32),   # nin_c's weight gradient folded into nin_b's under fp32_x6
        (2, 3, 3, 32, 64),   # dy transpose, thin nin_c, dec_conv1a's thin slice with C = 3
        (1, 1, 8, 32, 32)]   # out_nc > 4: nin_c through wgrad(), the head's data gradients in fp32
RESNET = [(1, 1, 32, 48), (2, 3, 13, 22), (1, 1, 1, 5)]
KEYS = ([f"unet:{','.join(map(str, s))}:{p}" for s in UNET for p in ("fp32", "fp32_x6")] +
        [f"resnet:{','.join(map(str, s))}:{p}" for s in RESNET for p in ("fp32", "fp32_x6")] +
        ["iunet:1,1,32,32:fp32_x6"])
# the cases the test also runs in a DN_BWD_STREAMS=0 process (same digests: one stream or three)
ONE_STREAM_KEYS = ["unet:2,3,3,32,64:fp32_x6", "resnet:2,3,13,22:fp32_x6"]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(key):
    """{"y", "dx", "dparams/<layer>"...} (ImprovedUNet: {"y", "dparams"}) of case `key`"""
    kind, shape, prec = key.split(":")
    shape = tuple(int(v) for v in shape.split(","))
    torch.manual_seed(0)
    if kind == "unet":
        from image_denoising_amd import arch_unet as mod
        N, C, OC, H, W = shape
        net = mod.UNet(C, OC, 48)
    elif kind == "resnet":
        from image_denoising_amd import resnet as mod
        N, C, H, W = shape
        OC = C
        net = mod.RESNET(C, C, 48)
    else:
        from image_denoising_amd.improved_unet import ImprovedUNet
        N, C, H, W = shape
        OC = C
        net = ImprovedUNet(in_nc=C, out_nc=C, n_feature=48)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.mul_(10.0)
    net = net.to("cuda").set_precision(prec)
    x = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(17)).cuda()
    ws = net._workspace(N, H, W, with_backward=True, fresh=True)
    y = torch.zeros(N, OC, H, W, device="cuda")
    net._run_forward(x, y, ws)
    dy = torch.rand(y.shape, generator=torch.Generator().manual_seed(5)).cuda() - 0.5
    dflat, dx = torch.zeros_like(net.flat_params), torch.zeros_like(x)
    if kind == "iunet":
        net._run_backward(dy, dflat, ws, N, H, W)
        torch.cuda.synchronize()
        return {"y": _sha(y), "dparams": _sha(dflat)}
    net._run_backward(dy, dflat, ws, N, H, W, dx=dx)
    torch.cuda.synchronize()
    out = {"y": _sha(y), "dx": _sha(dx)}
    off = 0
    for name, wshape, blen, _ in mod.layer_shapes(C, OC, 48):  # layer_name / res_layer_name order
        n = int(torch.Size(wshape).numel()) + blen
        out["dparams/" + name] = _sha(dflat[off:off + n])
        off += n
    assert off == dflat.numel()
    return out


def main(out, commit):
    import ctypes

    from image_denoising_amd import _lib

    # an older library lacks the symbols added since: bind what it has
    have = ctypes.CDLL(_lib.LIB_PATH)
    for k in [k for k in _lib.SIGNATURES if not hasattr(have, k)]:
        _lib.SIGNATURES.pop(k)
    version = _lib.lib().dn_version().decode()
    print("library:", _lib.LIB_PATH, version)
    cases = {}
    for key in KEYS:
        a, b = digests(key), digests(key)
        if a != b:
            print("NOT bit-reproducible, left out:", key, [k for k in a if a[k] != b[k]])
            continue
        cases[key] = a
    with open(out, "w") as f:
        json.dump({"commit": commit, "dn_version": version, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(cases), "of", len(KEYS), "cases")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--print":
        print(json.dumps({k: digests(k) for k in sys.argv[2:]}))
    elif len(sys.argv) == 3:
        main(sys.argv[1], sys.argv[2])
    else:
        raise SystemExit(__doc__)
