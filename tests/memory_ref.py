"""Independent torch restatement (runnable in fp64 on the CPU) of the memory-bank adapter path:
bank order, nearest-patch selection, the hyper-gated residual adapter (v5 with row-FFT features,
v4 without) with a hand-written backward, the patch-origin lists and the Hann blend -- plus the
deterministic input generators the tests and tests/golden/make_golden_memory.py share.

Written from the description of the model, not from the reference's code:
  bank      patch n = img*ny*nx + iy*nx + ix, window at (iy*s, ix*s), ny = (H-P)//s + 1
  select    argmin_n sum (q - patch_n)^2, ties to the lowest n
  features  [mean, unbiased std] of noisy, base_out, mem_clean over C*H*W, then per tensor the
            row power spectrum |rfft along W|^2 averaged over the C*H rows, cut into nb bands of
            F//nb bins (the last takes the remainder), band mean -> log1p -> / (mean of bands + 1e-6)
  hyper     Linear -> ReLU -> Linear; gamma = sigmoid(h[:C]), beta = 0.1 tanh(h[C:])
  out       clamp(base_out + gamma * local_net(cat[noisy, base_out]) + beta, 0, 1)
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ["local_net.0.weight", "local_net.0.bias", "local_net.2.weight", "local_net.2.bias",
        "local_net.4.weight", "local_net.4.bias", "hyper_mlp.0.weight", "hyper_mlp.0.bias",
        "hyper_mlp.2.weight", "hyper_mlp.2.bias"]

# name -> (B, C, H, W, hidden, num_fft_bins, clamp_output)
ADAPTER_CASES = {
    "b1c1_8x8": (1, 1, 8, 8, 16, 3, True),
    "b3c1_17x23": (3, 1, 17, 23, 16, 3, True),
    "b2c3_16x20": (2, 3, 16, 20, 16, 3, True),
    "b4c1_128x128": (4, 1, 128, 128, 16, 3, True),
    "hid8": (3, 1, 17, 23, 8, 3, True),
    "v4": (3, 1, 17, 23, 16, 0, True),
    "noclamp": (3, 1, 17, 23, 16, 3, False),
}

# (P, s, H, W, n_img, C)
SELECT_CASES = [(16, 4, 40, 44, 2, 1), (24, 3, 45, 61, 3, 1), (5, 1, 9, 13, 2, 3),
                (128, 4, 160, 172, 2, 1), (128, 64, 128, 128, 3, 3)]
SELECT_B = (1, 4, 7)
GAP_SKIP = 8e-6   # a random query is skipped when its fp64 gap is below this * (|q|^2 + |b|^2)

ORIGIN_CASES = [(352, 352, 128, 64), (130, 200, 128, 64), (128, 128, 128, 0), (45, 61, 24, 7)]
BLEND_CASES = [(45, 61, 24, 7), (64, 64, 32, 16)]


def uniform(n: int, seed: int) -> np.ndarray:
    """n doubles in [0, 1) (MT19937: the same on every numpy)"""
    return np.random.RandomState(seed).random_sample(int(n))


def shapes_of(C: int, Hc: int, nb: int):
    NF = 6 + 3 * nb
    return [(Hc, 2 * C, 3, 3), (Hc,), (Hc, Hc, 3, 3), (Hc,), (C, Hc, 3, 3), (C,), (Hc, NF), (Hc,),
            (2 * C, Hc), (2 * C,)]


@functools.lru_cache(maxsize=None)
def adapter_case(name: str):
    """(params: dict key -> fp32 array, random NON-zero; noisy, base_out, mem_clean, dout) fp32.
    base_out is drawn from [-0.2, 1.2]; pixels whose fp64 `pre` would lie within 1e-4 of a clamp
    bound are moved by 2e-3 until none does (a pixel ON a bound has no defined gradient)."""
    B, C, H, W, Hc, nb, clamp = ADAPTER_CASES[name]
    seed = 1000 + 17 * list(ADAPTER_CASES).index(name)
    params = {}
    for k, (key, shp) in enumerate(zip(KEYS, shapes_of(C, Hc, nb))):
        fan = int(np.prod(shp[1:])) if len(shp) > 1 else 4
        a = 0.7 / np.sqrt(fan)
        params[key] = ((uniform(np.prod(shp), seed + k) * 2 - 1) * a).reshape(shp).astype(np.float32)
    n = B * C * H * W
    noisy = uniform(n, seed + 20).reshape(B, C, H, W).astype(np.float32)
    base = (uniform(n, seed + 21) * 1.4 - 0.2).reshape(B, C, H, W).astype(np.float32)
    mem = uniform(n, seed + 22).reshape(B, C, H, W).astype(np.float32)
    dout = (uniform(n, seed + 23) * 2 - 1).reshape(B, C, H, W).astype(np.float32)
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    for _ in range(20):
        pre = forward(p64, torch.from_numpy(noisy).double(), torch.from_numpy(base).double(),
                      torch.from_numpy(mem).double(), nb, clamp, keep=True)[1]["pre"].numpy()
        near = (np.abs(pre) < 1e-4) | (np.abs(pre - 1) < 1e-4)
        if not near.any():
            break
        base = np.where(near, base + np.float32(2e-3), base).astype(np.float32)
    else:
        raise AssertionError(name)
    return params, noisy, base, mem, dout


def flat_of(params: dict) -> np.ndarray:
    return np.concatenate([np.asarray(params[k]).reshape(-1) for k in KEYS])


# ---- bank ----------------------------------------------------------------------------------------
def bank_patches(imgs: torch.Tensor, P: int, s: int) -> torch.Tensor:
    """[n_img,C,H,W] -> [N,C,P,P] in bank order, by plain slicing"""
    n_img, C, H, W = imgs.shape
    ny, nx = (H - P) // s + 1, (W - P) // s + 1
    out = [imgs[i, :, iy * s:iy * s + P, ix * s:ix * s + P]
           for i in range(n_img) for iy in range(ny) for ix in range(nx)]
    return torch.stack(out)


def select(queries: torch.Tensor, patches: torch.Tensor):
    """(idx [B], best [B], runner-up [B], scale [B] = |q|^2 + |b|^2 of the best) in the tensors'
    dtype (use fp64); ties to the lowest n"""
    q = queries.reshape(queries.shape[0], 1, -1)
    b = patches.reshape(1, patches.shape[0], -1)
    d = torch.stack([((q[i] - b[0]) ** 2).sum(-1) for i in range(q.shape[0])])  # [B, N]
    idx = torch.tensor([int(torch.nonzero(r == r.min())[0]) for r in d])
    best = d.gather(1, idx[:, None])[:, 0]
    if d.shape[1] > 1:
        d2 = d.clone()
        d2.scatter_(1, idx[:, None], float("inf"))
        second = d2.min(1).values
    else:
        second = torch.full_like(best, float("inf"))
    scale = (q[:, 0] ** 2).sum(-1) + (b[0][idx] ** 2).sum(-1)
    return idx, best, second, scale


def bank_images(case, seed: int) -> np.ndarray:
    P, s, H, W, n_img, C = case
    return uniform(n_img * C * H * W, seed).reshape(n_img, C, H, W).astype(np.float32)


def select_seed(case, B: int) -> int:
    return 8000 + 31 * SELECT_CASES.index(tuple(case)) + B


def random_queries(case, B: int) -> np.ndarray:
    P, s, H, W, n_img, C = case
    return uniform(B * C * P * P, select_seed(case, B) + 7).reshape(B, C, P, P).astype(np.float32)


# ---- adapter ---------------------------------------------------------------------------------------
def fft_features(x: torch.Tensor, nb: int) -> torch.Tensor:
    B, C, H, W = x.shape
    spec = torch.fft.rfft(x.reshape(B, C * H, W), dim=-1)
    power = (spec.real ** 2 + spec.imag ** 2).mean(1)  # [B, F]
    Fq = power.shape[-1]
    assert Fq >= nb
    bs = Fq // nb
    bands = [power[:, k * bs:((k + 1) * bs if k < nb - 1 else Fq)].mean(-1) for k in range(nb)]
    f = torch.log1p(torch.stack(bands, 1))
    return f / (f.mean(1, keepdim=True) + 1e-6)


def features(noisy, base, mem, nb: int) -> torch.Tensor:
    st = []
    for t in (noisy, base, mem):
        v = t.reshape(t.shape[0], -1)
        st += [v.mean(1), v.std(1, unbiased=True)]
    f = [torch.stack(st, 1)]
    if nb > 0:
        f += [fft_features(t, nb) for t in (noisy, base, mem)]
    return torch.cat(f, 1)


def forward(p: dict, noisy, base, mem, nb: int, clamp: bool = True, keep: bool = False):
    """out (and, keep=True, everything the hand-written backward reads)"""
    C = noisy.shape[1]
    feat = features(noisy, base, mem, nb)
    z0 = feat @ p["hyper_mlp.0.weight"].t() + p["hyper_mlp.0.bias"]
    hh = z0.clamp_min(0)
    hy = hh @ p["hyper_mlp.2.weight"].t() + p["hyper_mlp.2.bias"]
    gamma = torch.sigmoid(hy[:, :C])[:, :, None, None]
    th = torch.tanh(hy[:, C:])
    beta = (0.1 * th)[:, :, None, None]
    x = torch.cat([noisy, base], 1)
    h1 = F.conv2d(x, p["local_net.0.weight"], p["local_net.0.bias"], padding=1).clamp_min(0)
    h2 = F.conv2d(h1, p["local_net.2.weight"], p["local_net.2.bias"], padding=1).clamp_min(0)
    r = F.conv2d(h2, p["local_net.4.weight"], p["local_net.4.bias"], padding=1)
    pre = base + (gamma * r + beta)
    out = pre.clamp(0, 1) if clamp else pre
    if keep:
        return out, dict(feat=feat, hh=hh, gamma=gamma, th=th, x=x, h1=h1, h2=h2, r=r, pre=pre)
    return out


def _wgrad(g, x):
    """dW[o,i,ky,kx] = sum g[n,o,y,x] * xpad[n,i,y+ky,x+kx] of a 3x3 pad-1 convolution"""
    H, W = g.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([torch.stack([torch.einsum("noyx,niyx->oi", g, xp[:, :, ky:ky + H, kx:kx + W])
                                     for kx in range(3)], -1) for ky in range(3)], -2)


def _dgrad(g, w):
    return F.conv2d(g, w.flip(2, 3).transpose(0, 1), padding=1)


def backward(p: dict, noisy, base, mem, dout, nb: int, clamp: bool = True) -> dict:
    """parameter gradients by hand (the features are constants)"""
    C = noisy.shape[1]
    _, k = forward(p, noisy, base, mem, nb, clamp, keep=True)
    dpre = dout * ((k["pre"] >= 0) & (k["pre"] <= 1)).to(dout.dtype) if clamp else dout
    dr = k["gamma"] * dpre
    dgamma = (k["r"] * dpre).sum((2, 3))
    dbeta = dpre.sum((2, 3))
    g = k["gamma"][:, :, 0, 0]
    dhy = torch.cat([dgamma * g * (1 - g), dbeta * 0.1 * (1 - k["th"] ** 2)], 1)
    G = {}
    G["hyper_mlp.2.weight"] = dhy.t() @ k["hh"]
    G["hyper_mlp.2.bias"] = dhy.sum(0)
    dz0 = (dhy @ p["hyper_mlp.2.weight"]) * (k["hh"] > 0).to(dout.dtype)
    G["hyper_mlp.0.weight"] = dz0.t() @ k["feat"]
    G["hyper_mlp.0.bias"] = dz0.sum(0)
    G["local_net.4.weight"] = _wgrad(dr, k["h2"])
    G["local_net.4.bias"] = dr.sum((0, 2, 3))
    g2 = _dgrad(dr, p["local_net.4.weight"]) * (k["h2"] > 0).to(dout.dtype)
    G["local_net.2.weight"] = _wgrad(g2, k["h1"])
    G["local_net.2.bias"] = g2.sum((0, 2, 3))
    g1 = _dgrad(g2, p["local_net.2.weight"]) * (k["h1"] > 0).to(dout.dtype)
    G["local_net.0.weight"] = _wgrad(g1, k["x"])
    G["local_net.0.bias"] = g1.sum((0, 2, 3))
    return G


def run_case(name: str, dtype=torch.float64):
    """(feat, out, pre, grads dict) of an ADAPTER_CASES entry in `dtype` on the CPU"""
    B, C, H, W, Hc, nb, clamp = ADAPTER_CASES[name]
    params, noisy, base, mem, dout = adapter_case(name)
    p = {k: torch.from_numpy(v).to(dtype) for k, v in params.items()}
    n, b, m, d = (torch.from_numpy(v).to(dtype) for v in (noisy, base, mem, dout))
    out, k = forward(p, n, b, m, nb, clamp, keep=True)
    return k["feat"], out, k["pre"], backward(p, n, b, m, d, nb, clamp)


# ---- patchwise inference -----------------------------------------------------------------------------
def origins(size: int, P: int, overlap: int) -> list:
    step = P - overlap
    o = list(range(0, size - P + 1, step))
    if o[-1] != size - P:
        o.append(size - P)
    return sorted(set(o))


def hann_blend(pred: np.ndarray, ys, xs, H: int, W: int, dtype=np.float32) -> np.ndarray:
    """pred [len(ys)*len(xs), C, P, P] -> [C,H,W]; patches added in the order iy, ix"""
    P = pred.shape[-1]
    h = torch.hann_window(P, periodic=False, dtype=torch.float32).numpy().astype(dtype)
    w = np.maximum(h[:, None] * h[None, :], dtype(1e-3))
    out = np.zeros((pred.shape[1], H, W), dtype)
    wt = np.zeros((1, H, W), dtype)
    k = 0
    for y in ys:
        for x in xs:
            out[:, y:y + P, x:x + P] += pred[k].astype(dtype) * w
            wt[:, y:y + P, x:x + P] += w
            k += 1
    return out / (wt + dtype(1e-8))


def blend_image(case) -> np.ndarray:
    """uint8-valued float32 (H,W) test image of a BLEND_CASES entry"""
    H, W, P, ov = case
    return np.floor(uniform(H * W, 7000 + H + W) * 256).reshape(H, W).astype(np.float32)
