"""The memory-conditioned adapter of the reference's finetune_memory.py /
evaluation_704_iqsl_memory.py, computed by libdenoise_hip.so on gfx950.

    base_out  = base(noisy)                       [no grad, or trained: freeze_base=False]
    idx       = argmin_n |noisy - noise patch n|^2            dn_memory_select
    mem_clean = clean patch idx                               dn_memory_gather
    out       = HyperGatedResidualAdapter_FFT(noisy, base_out, mem_clean)   dn_memadapter_forward

The bank is IMPLICIT: a `MemoryBank` keeps the few paired images the patches are windows of
(megabytes), never the unfolded `[N,C,P,P]` tensors (a gigabyte each at the reference's settings);
the selection kernel walks the windows in place.  Patch order is the reference's
(`extract_patches` = F.unfold, images concatenated in order).

With `DenoiserWithMemoryAdapter(freeze_base=False, use_no_grad_for_base=False)` the base trains
through the adapter: dn_memadapter_backward_input hands dL/dbase_out (direct + local + hyper
routes) to the base's own HIP backward.  The bank stays constant and the selection is an argmin:
no gradient flows to `noisy` or `mem_clean`.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_module import FlatParamModule


class MemoryBank:
    """n_img paired noisy / clean images `[n_img, C, H, W]` (fp32, one device) with patch_size P and
    stride s.  Patch n is the window at (img, iy, ix), n = img*ny*nx + iy*nx + ix,
    ny = (H-P)//s + 1, nx = (W-P)//s + 1; pixels past the last whole stride are unused, as
    F.unfold leaves them."""

    def __init__(self, noise_images: torch.Tensor, clean_images: torch.Tensor, patch_size: int,
                 stride: int):
        if noise_images.shape != clean_images.shape or noise_images.dim() != 4:
            raise ValueError("noise and clean images must share one [n_img,C,H,W] shape")
        if noise_images.device != clean_images.device:
            raise ValueError("noise and clean images must live on one device")
        n_img, C, H, W = noise_images.shape
        P, s = int(patch_size), int(stride)
        if C not in (1, 3) or n_img < 1 or P < 3 or s < 1 or H < P or W < P:
            raise ValueError("need C in {1, 3}, n_img >= 1, patch_size >= 3, stride >= 1 and "
                             "H, W >= patch_size")
        self.noise = noise_images.detach().to(torch.float32).contiguous()
        self.clean = clean_images.detach().to(torch.float32).contiguous()
        self.patch_size, self.stride = P, s
        self.ny, self.nx = (H - P) // s + 1, (W - P) // s + 1
        self._ws = None

    @classmethod
    def from_patches(cls, noise: torch.Tensor, clean: torch.Tensor) -> "MemoryBank":
        """Explicit `[N,C,P,P]` bank tensors (the reference's constructor arguments) as N images of
        P x P with one window each: the same kernel, not the fast case."""
        if noise.dim() != 4 or noise.shape[2] != noise.shape[3]:
            raise ValueError("expected [N,C,P,P] bank tensors")
        return cls(noise, clean, noise.shape[2], 1)

    def __len__(self) -> int:
        return self.noise.shape[0] * self.ny * self.nx

    @property
    def device(self):
        return self.noise.device

    @property
    def channels(self) -> int:
        return self.noise.shape[1]

    def to(self, device) -> "MemoryBank":
        return MemoryBank(self.noise.to(device), self.clean.to(device), self.patch_size, self.stride)

    def _geom(self):
        n_img, C, H, W = self.noise.shape
        return n_img, C, H, W, self.patch_size, self.stride

    def _patches(self, imgs: torch.Tensor) -> torch.Tensor:
        n_img, C, H, W = imgs.shape
        P, s = self.patch_size, self.stride
        w = imgs.unfold(2, P, s).unfold(3, P, s)  # [n_img, C, ny, nx, P, P]
        return w.permute(0, 2, 3, 1, 4, 5).reshape(-1, C, P, P).contiguous()

    def noise_patches(self) -> torch.Tensor:
        """the materialised `[N,C,P,P]` noisy bank: for tests and small banks only"""
        return self._patches(self.noise)

    def clean_patches(self) -> torch.Tensor:
        return self._patches(self.clean)

    def select(self, queries: torch.Tensor) -> torch.Tensor:
        """idx[B] (int64, on the device): the nearest noisy patch of every `[B,C,P,P]` query by
        squared L2 distance (fp32, formed directly), ties to the lowest index."""
        q = queries.detach().contiguous()
        n_img, C, H, W, P, s = self._geom()
        if q.dim() != 4 or tuple(q.shape[1:]) != (C, P, P) or q.dtype != torch.float32:
            raise ValueError(f"queries must be float32 [B,{C},{P},{P}]")
        if q.device != self.device or q.device.type != "cuda":
            raise RuntimeError("the bank and the queries must live on one GPU")
        B = q.shape[0]
        need = _lib.lib().dn_memory_select_ws_size(B, n_img, C, H, W, P, s)
        if self._ws is None or self._ws.numel() < need:
            self._ws = _lib.scratch(need, q.device)
        idx = torch.empty(B, dtype=torch.int64, device=q.device)
        _lib.call("dn_memory_select", _lib.ptr(q), _lib.ptr(self.noise), B, n_img, C, H, W, P, s,
                  idx.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream_of(q))
        return idx

    def gather_clean(self, idx: torch.Tensor) -> torch.Tensor:
        """`clean_patches()[idx]` without the bank: `[B,C,P,P]`"""
        n_img, C, H, W, P, s = self._geom()
        idx = idx.to(torch.int64).contiguous()
        out = torch.empty(idx.numel(), C, P, P, dtype=torch.float32, device=self.device)
        _lib.call("dn_memory_gather", _lib.ptr(self.clean), idx.data_ptr(), idx.numel(), n_img, C, H,
                  W, P, s, _lib.ptr(out), _lib.stream_of(out))
        return out


def build_memory_bank(clean_paths, noise_paths, patch_size: int, stride: int, device) -> MemoryBank:
    """finetune_memory.py build_memory_bank: PIL images / 255 (2-D, C = 1), paired in order, as a
    `MemoryBank`.  The images of one bank must share one H x W (the reference's torch.cat of patches
    tolerates mixed sizes; that case is out of scope here and raises)."""
    from PIL import Image

    if len(clean_paths) != len(noise_paths) or len(clean_paths) == 0:
        raise ValueError("clean_paths and noise_paths must be non-empty and of one length")
    clean, noise = [], []
    for cp, npth in zip(clean_paths, noise_paths):
        c = (np.array(Image.open(cp), dtype=np.float32) / 255.0).astype(np.float32)
        n = (np.array(Image.open(npth), dtype=np.float32) / 255.0).astype(np.float32)
        if c.ndim != 2 or c.shape != n.shape:
            raise ValueError(f"{cp}: the bank takes paired 2-D (grayscale) images")
        if clean and c.shape != clean[0].shape:
            raise ValueError(f"{cp}: images of one bank must share one size "
                             f"({c.shape} vs {clean[0].shape})")
        clean.append(c)
        noise.append(n)
    bank = MemoryBank(torch.from_numpy(np.stack(noise))[:, None].to(device),
                      torch.from_numpy(np.stack(clean))[:, None].to(device), patch_size, stride)
    print(f"[MemoryBank] #clean patches={len(bank)}, patch_size={patch_size}, stride={stride}")
    return bank


# ---- the adapters -----------------------------------------------------------------------------
def memadapter_reference_init(in_channels: int, hidden_channels: int, num_fft_bins: int) -> torch.Tensor:
    """Flat CPU parameters drawn in the reference's construction order (three Conv2d, two Linear,
    default inits), then the last conv and both Linears zeroed as it zeroes them."""
    C, Hc = in_channels, hidden_channels
    with torch.no_grad():
        c1 = nn.Conv2d(2 * C, Hc, kernel_size=3, padding=1, bias=True)
        c2 = nn.Conv2d(Hc, Hc, kernel_size=3, padding=1, bias=True)
        c3 = nn.Conv2d(Hc, C, kernel_size=3, padding=1, bias=True)
        l1 = nn.Linear(6 + 3 * num_fft_bins, Hc)
        l2 = nn.Linear(Hc, 2 * C)
        for m in (c3, l1, l2):
            m.weight.zero_()
            m.bias.zero_()
        return torch.cat([t.reshape(-1) for m in (c1, c2, c3, l1, l2)
                          for t in (m.weight, m.bias)]).float()


class _MemAdapterFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noisy, base_out, mem_clean, mod, *params):
        out = torch.empty_like(base_out)
        feat = mod._run_forward(noisy, base_out, mem_clean, out)
        ctx.mod = mod
        ctx.save_for_backward(noisy, base_out, feat)
        return out

    @staticmethod
    def backward(ctx, dout):
        noisy, base_out, feat = ctx.saved_tensors
        mod = ctx.mod
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            raise NotImplementedError("no gradient w.r.t. noisy or mem_clean is computed (the bank "
                                      "is constant and the selection is an argmin)")
        dout = dout.contiguous()
        need_params = any(ctx.needs_input_grad[4:])
        dflat = torch.empty_like(mod._flat) if need_params else None
        dbase = None
        if ctx.needs_input_grad[1]:  # one call: dbase and, when asked for, the parameter gradient
            dbase = torch.empty_like(base_out)
            mod._run_backward_input(noisy, base_out, feat, dout, dflat, dbase)
        elif need_params:
            mod._run_backward(noisy, base_out, feat, dout, dflat)
        pgrads = [None] * len(ctx.needs_input_grad[4:])
        if need_params:
            pgrads = mod._grads_from_flat(dflat, ctx.needs_input_grad[4:])
        return (None, dbase, None, None, *pgrads)


class HyperGatedResidualAdapter_FFT(FlatParamModule):
    """finetune_memory.py HyperGatedResidualAdapter_FFT (the "v5" adapter):
    out = clamp(base_out + gamma * local_net(cat[noisy, base_out]) + beta), (gamma, beta) from a
    small MLP of global statistics and row-FFT band features of noisy, base_out and mem_clean.
    Same state_dict keys (`local_net.{0,2,4}`, `hyper_mlp.{0,2}`); all parameters are views of one
    flat fp32 buffer."""

    _display = "adapter"

    def __init__(self, in_channels: int = 1, hidden_channels: int = 16, num_fft_bins: int = 3,
                 clamp_output: bool = True):
        super().__init__()
        n = ctypes.c_size_t()
        _lib.check(_lib.lib().dn_memadapter_param_count(in_channels, hidden_channels, num_fft_bins,
                                                        ctypes.byref(n)), "dn_memadapter_param_count")
        self.in_channels, self.hidden_channels = in_channels, hidden_channels
        self.num_fft_bins, self.clamp_output = num_fft_bins, clamp_output
        self.beta_scale = 0.1
        flat = memadapter_reference_init(in_channels, hidden_channels, num_fft_bins)
        assert flat.numel() == n.value
        C, Hc, NF = in_channels, hidden_channels, 6 + 3 * num_fft_bins
        layers = [("local_net.0", (Hc, 2 * C, 3, 3)), ("local_net.2", (Hc, Hc, 3, 3)),
                  ("local_net.4", (C, Hc, 3, 3)), ("hyper_mlp.0", (Hc, NF)),
                  ("hyper_mlp.2", (2 * C, Hc))]
        self._bind_flat(flat, [e for name, wshape in layers
                               for e in ((name + ".weight", wshape), (name + ".bias", wshape[:1]))])
        self._ws = None

    def _drop_scratch(self) -> None:
        self._ws = None

    def _check(self, noisy, base_out, mem_clean):
        if noisy.device.type != "cuda":
            raise RuntimeError("the HIP adapter runs on a GPU: move the module and inputs to cuda")
        if not (noisy.shape == base_out.shape == mem_clean.shape) or noisy.dim() != 4 \
                or noisy.shape[1] != self.in_channels:
            raise ValueError(f"expected noisy, base_out and mem_clean of one "
                             f"[N,{self.in_channels},H,W] shape")
        if any(t.dtype != torch.float32 for t in (noisy, base_out, mem_clean)):
            raise ValueError("adapter inputs must be float32")
        if self.num_fft_bins > 0 and noisy.shape[3] // 2 + 1 < self.num_fft_bins:
            raise ValueError("the row FFT has fewer bins than num_fft_bins")

    def _workspace(self, N, C, H, W, bwd, device):
        """bwd: 0 / False forward, 1 / True parameter gradient, 2 parameter and input gradient"""
        need = _lib.lib().dn_memadapter_ws_size(N, C, H, W, self.hidden_channels, self.num_fft_bins,
                                                int(bwd))
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = _lib.scratch(need, device)
        return self._ws

    def _run_forward(self, noisy, base_out, mem_clean, out) -> torch.Tensor:
        """writes out, returns the features `[N, 6 + 3 nb]` (what the backward reads)"""
        N, C, H, W = noisy.shape
        ws = self._workspace(N, C, H, W, False, noisy.device)
        feat = torch.empty(N, 6 + 3 * self.num_fft_bins, dtype=torch.float32, device=noisy.device)
        _lib.call("dn_memadapter_forward", _lib.ptr(self._flat), _lib.ptr(noisy), _lib.ptr(base_out),
                  _lib.ptr(mem_clean), _lib.ptr(out), _lib.ptr(feat), N, C, H, W,
                  self.hidden_channels, self.num_fft_bins, int(self.clamp_output), ws.data_ptr(),
                  ws.numel(), _lib.stream_of(noisy))
        return feat

    def _run_backward(self, noisy, base_out, feat, dout, dflat):
        N, C, H, W = noisy.shape
        ws = self._workspace(N, C, H, W, True, noisy.device)
        _lib.call("dn_memadapter_backward", _lib.ptr(self._flat), _lib.ptr(noisy),
                  _lib.ptr(base_out), _lib.ptr(feat), _lib.ptr(dout), _lib.ptr(dflat), N, C, H, W,
                  self.hidden_channels, self.num_fft_bins, int(self.clamp_output), ws.data_ptr(),
                  ws.numel(), _lib.stream_of(noisy))

    def _run_backward_input(self, noisy, base_out, feat, dout, dflat, dbase):
        """dbase = dL/dbase_out and, unless dflat is None, dflat = dL/dparams (the bits of
        _run_backward), in one call.  A constant base_out sample has std = 0 and no defined
        gradient, as in the reference."""
        N, C, H, W = noisy.shape
        ws = self._workspace(N, C, H, W, 2, noisy.device)
        _lib.call("dn_memadapter_backward_input", _lib.ptr(self._flat), _lib.ptr(noisy),
                  _lib.ptr(base_out), _lib.ptr(feat), _lib.ptr(dout), _lib.ptr(dflat),
                  _lib.ptr(dbase), N, C, H, W, self.hidden_channels, self.num_fft_bins,
                  int(self.clamp_output), ws.data_ptr(), ws.numel(), _lib.stream_of(noisy))

    def _feature_adjoint(self, base_out, dfeat) -> torch.Tensor:
        """the hyper route alone (for tests): the adjoint of base_out's features for the cotangent
        dfeat `[N, 2 + nb]` = (d mean, d std, d band features)"""
        base_out, dfeat = base_out.contiguous(), dfeat.contiguous()
        N, C, H, W = base_out.shape
        need = _lib.lib().dn_memadapter_ws_size(N, C, H, W, 8, self.num_fft_bins, 2)
        ws = _lib.scratch(need, base_out.device)
        out = torch.empty_like(base_out)
        _lib.call("dn_memadapter_feature_adjoint", _lib.ptr(base_out), _lib.ptr(dfeat),
                  _lib.ptr(out), N, C, H, W, self.num_fft_bins, ws.data_ptr(), ws.numel(),
                  _lib.stream_of(base_out))
        return out

    def features(self, noisy, base_out, mem_clean) -> torch.Tensor:
        """the hyper MLP's input `[N, 6 + 3 nb]` (for tests)"""
        noisy, base_out, mem_clean = noisy.contiguous(), base_out.contiguous(), mem_clean.contiguous()
        self._check(noisy, base_out, mem_clean)
        return self._run_forward(noisy, base_out, mem_clean, torch.empty_like(base_out))

    def forward(self, noisy, base_out, mem_clean) -> torch.Tensor:
        noisy, base_out, mem_clean = noisy.contiguous(), base_out.contiguous(), mem_clean.contiguous()
        self._check(noisy, base_out, mem_clean)
        if noisy.requires_grad or base_out.requires_grad or mem_clean.requires_grad:
            raise NotImplementedError("gradients w.r.t. the adapter inputs are not computed (the "
                                      "reference runs the base and the selection under no_grad)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._params()):
            return _MemAdapterFunction.apply(noisy, base_out, mem_clean, self, *self._params())
        out = torch.empty_like(base_out)
        self._run_forward(noisy, base_out, mem_clean, out)
        return out


class HyperGatedResidualAdapter(HyperGatedResidualAdapter_FFT):
    """finetune_memory.py HyperGatedResidualAdapter (v4): the same adapter with the six global
    statistics alone (no FFT features)."""

    def __init__(self, in_channels: int = 1, hidden_channels: int = 16, clamp_output: bool = True):
        super().__init__(in_channels, hidden_channels, 0, clamp_output)


class DenoiserWithMemoryAdapter(nn.Module):
    """finetune_memory.py DenoiserWithMemoryAdapter.  `memory_noise_bank` is a `MemoryBank` (then
    `memory_clean_bank` is omitted) or both are `[N,C,P,P]` tensors.  The bank is no parameter and
    no buffer: the reference's checkpoints hold `adapter.state_dict()` only.

    freeze_base=False, use_no_grad_for_base=False trains the base and the adapter together through
    one loss.backward() (finetune_memory.py:1201-1291): the base runs its ordinary autograd
    forward in `set_precision`'s training arithmetic, the selection stays under no_grad, and the
    adapter's autograd function returns dL/dbase_out.  The bf16 inference plan is forward-only
    and is not used on that path."""

    def __init__(self, base_model: nn.Module, in_channels: int, hidden_channels: int,
                 memory_noise_bank, memory_clean_bank=None, freeze_base: bool = True,
                 use_no_grad_for_base: bool = True):
        super().__init__()
        self.base = base_model
        self.in_channels = in_channels
        self.adapter = HyperGatedResidualAdapter_FFT(in_channels=in_channels,
                                                     hidden_channels=hidden_channels,
                                                     num_fft_bins=3, clamp_output=True)
        self.freeze_base = freeze_base
        self.use_no_grad_for_base = use_no_grad_for_base
        if freeze_base:
            for p in self.base.parameters():
                p.requires_grad = False
        if isinstance(memory_noise_bank, MemoryBank):
            if memory_clean_bank is not None:
                raise ValueError("a MemoryBank holds both sides: omit memory_clean_bank")
            self.bank = memory_noise_bank
        else:
            if memory_clean_bank is None:
                raise ValueError("memory_clean_bank is needed beside a noise bank tensor")
            self.bank = MemoryBank.from_patches(memory_noise_bank, memory_clean_bank)

    def _apply(self, fn, recurse=True):
        # .to(device) / .cuda() / .cpu() must move the bank with the module, but the bank is
        # neither parameter nor buffer: see where `fn` sends an empty fp32 tensor and follow it
        # there.  A dtype-changing `fn` never gets this far (the adapter's _apply refuses it).
        super()._apply(fn, recurse)
        probe = fn(torch.empty(0, dtype=torch.float32, device=self.bank.device))
        if probe.device != self.bank.device:
            self.bank = self.bank.to(probe.device)
        return self

    @torch.no_grad()
    def _select_index(self, noisy: torch.Tensor) -> torch.Tensor:
        return self.bank.select(noisy)

    @torch.no_grad()
    def _select_memory_patch(self, noisy: torch.Tensor) -> torch.Tensor:
        """the clean partner `[B,C,P,P]` of every input's nearest noisy bank patch"""
        return self.bank.gather_clean(self.bank.select(noisy))

    def forward(self, noisy: torch.Tensor) -> torch.Tensor:
        if self.use_no_grad_for_base:
            with torch.no_grad():
                base_out = self.base(noisy)
        else:
            base_out = self.base(noisy)
        mem_clean = self._select_memory_patch(noisy)
        if torch.is_grad_enabled() and base_out.requires_grad:
            # the base trains through the adapter.  The module's own forward refuses inputs that
            # require grad, so enter its autograd function directly
            ad = self.adapter
            noisy_c, base_c = noisy.contiguous(), base_out.contiguous()
            ad._check(noisy_c, base_c, mem_clean)
            if noisy.requires_grad:
                raise NotImplementedError("no gradient w.r.t. the noisy input is computed")
            return _MemAdapterFunction.apply(noisy_c, base_c, mem_clean, ad, *ad._params())
        return self.adapter(noisy, base_out.detach(), mem_clean)


# ---- patchwise whole-image inference ---------------------------------------------------------------
def patch_origins(size: int, patch_size: int, overlap: int) -> list:
    """the reference's origin list along one axis: steps of P - overlap, the last origin
    size - P appended, sorted and deduplicated"""
    if size < patch_size:
        raise ValueError(f"image side {size} smaller than patch_size {patch_size}")
    if not overlap < patch_size:
        raise ValueError("overlap must be smaller than patch_size")
    o = list(range(0, max(size - patch_size, 0) + 1, patch_size - overlap))
    if o[-1] != size - patch_size:
        o.append(size - patch_size)
    return sorted(set(int(v) for v in o))


def hann_blend(pred: torch.Tensor, ys, xs, H: int, W: int) -> torch.Tensor:
    """`[C,H,W]` = the Hann-weighted blend of `pred[len(ys)*len(xs), C, P, P]`, patch iy*len(xs)+ix
    at origin (ys[iy], xs[ix]): sum pred * w / (sum w + 1e-8), w = max(hann (x) hann, 1e-3)."""
    pred = pred.contiguous()
    K, C, P, _ = pred.shape
    if K != len(ys) * len(xs):
        raise ValueError("one patch per (y, x) origin pair expected")
    if min(ys) < 0 or min(xs) < 0 or max(ys) + P > H or max(xs) + P > W:
        raise ValueError("a patch origin lies outside the image")
    dev = pred.device
    hann = torch.hann_window(P, periodic=False, dtype=torch.float32).to(dev)  # the CPU's values
    ys_t = torch.tensor(list(ys), dtype=torch.int32, device=dev)
    xs_t = torch.tensor(list(xs), dtype=torch.int32, device=dev)
    out = torch.empty(C, H, W, dtype=torch.float32, device=dev)
    _lib.call("dn_hann_blend", _lib.ptr(pred), _lib.ptr(hann), ys_t.data_ptr(), xs_t.data_ptr(),
              len(ys), len(xs), C, H, W, P, _lib.ptr(out), _lib.stream_of(pred))
    return out


def quantize_pred255(pred: torch.Tensor) -> torch.Tensor:
    """uint8 clip(pred * 255 + 0.5, 0, 255), as the reference's caller forms pred255"""
    pred = pred.contiguous()
    out = torch.empty(pred.shape, dtype=torch.uint8, device=pred.device)
    _lib.call("dn_quantize_u8", _lib.ptr(pred), pred.numel(), 1, _lib.ptr(out), _lib.stream_of(pred))
    return out


@torch.no_grad()
def denoise_full_image_patchwise(model: nn.Module, noisy_np: np.ndarray, patch_size: int,
                                 overlap: int = 64, device=None, return_pred255: bool = False):
    """finetune_memory.py denoise_full_image_patchwise: `noisy_np` (H,W) or (H,W,1) in 0..255 ->
    (H,W,1) float32 in 0..1.  All patches of the image run as ONE batch (the adapter's statistics
    are per sample and the base networks are batch-independent).  return_pred255 adds the uint8
    image clip(pred*255 + 0.5, 0, 255)."""
    if noisy_np.ndim == 3 and noisy_np.shape[2] == 1:
        noisy_np = noisy_np[..., 0]
    if noisy_np.ndim != 2:
        raise ValueError("expected a (H,W) or (H,W,1) image")
    if device is None:
        device = next(model.parameters()).device
    img = torch.from_numpy(noisy_np.astype(np.float32) / 255.0).to(device)
    H, W = img.shape
    ps = int(patch_size)
    ys, xs = patch_origins(H, ps, overlap), patch_origins(W, ps, overlap)
    patches = img.unfold(0, ps, 1).unfold(1, ps, 1)[ys][:, xs]  # [ny, nx, ps, ps]
    patches = patches.reshape(-1, 1, ps, ps).contiguous()
    pred = model(patches).to(torch.float32)
    out = hann_blend(pred, ys, xs, H, W)  # [1,H,W]
    res = out.permute(1, 2, 0).cpu().numpy()
    if return_pred255:
        return res, quantize_pred255(out).permute(1, 2, 0).cpu().numpy()
    return res
