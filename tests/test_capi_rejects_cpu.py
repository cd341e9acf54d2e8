"""The C boundary's rejections: every call below is refused before any launch, and must return
the status and leave the dn_last_error text recorded here.

The expectations were recorded once from the library as it was before the boundary was split by
family (capi.cpp), so they pin "same status, same message, same order of checks" across that
refactor and any later one.  Pointers that have to be non-null to get past a null check are
16-byte-aligned host dummies; the module is skipped where a GPU is present, because a call that
a faulty boundary wrongly accepted would launch on them (without a GPU it only returns a HIP
error, and the comparison fails).

Not reachable with host-only arguments, so not pinned: every "<entry point>: <hipGetErrorString>"
text of hip_status(), the two side-stream messages of dn_prepare_streams, the executors' own
"HIP error in ..." texts, the "no ... kernel tile for layer ..." texts of the plan builders (no
accepted configuration lacks a tile), "ImprovedUNet: the parameter layout does not have kIConvs
convolutions", the route errors of wgrad_run(), and the exception barrier's two texts.
"""
import ctypes

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host-pointer rejections: run on a machine without a GPU", allow_module_level=True)

from image_denoising_amd import _lib  # noqa: E402

_BUF = ctypes.create_string_buffer(1 << 16)
_A0 = (ctypes.addressof(_BUF) + 15) & ~15


def A(k=0):
    """the k-th 16-byte-aligned host dummy (1 KiB apart)"""
    return _A0 + 1024 * k


U = _A0 + 4  # non-null, not 16-byte aligned
BIG = 1 << 30  # a claimed size no check finds too small
SZ = ctypes.byref(ctypes.c_size_t())
I64 = ctypes.byref(ctypes.c_int64())
I32 = ctypes.byref(ctypes.c_int())
STATS = ctypes.byref(_lib.DnGuardStats())
INF, NAN = float("inf"), float("nan")


def cfg(in_nc=1, out_nc=1, n_feature=48):
    return ctypes.byref(_lib.DnCfg(in_nc, out_nc, n_feature))


G = cfg()
ARG, WS = -1, -2  # DN_ERR_ARG, DN_ERR_WORKSPACE
NULL = "null argument"
SENTINEL = "ncells < 0"  # what dn_last_error holds before each call (see _call)

U_CFG = "in_nc must be in [1,4] and out_nc in [1,16]"
NF48 = "n_feature must be 48 (kernel tiles are instantiated for the reference width)"
U_SHAPE = "N >= 1 and H, W must be positive multiples of 32 (5 pooling levels)"
U_WS = "workspace smaller than dn_unet_workspace_size()"
U_WSB = "workspace smaller than dn_unet_workspace_size(with_backward=1)"
U_BPREC = "backward precision must be DN_PREC_FP32 or DN_PREC_FP32_X6"
R_PREC = "RESNET precision must be DN_PREC_FP32 or DN_PREC_FP32_X6"
I_PREC = "ImprovedUNet precision must be DN_PREC_FP32 or DN_PREC_FP32_X6"
I_SHAPE = "ImprovedUNet needs N >= 1 and H, W multiples of 16 (4 pooling levels)"
PACK = "pack scratch smaller than *_pack_size()"
CHAN = "unsupported channel count for this kernel build"
GUARD = "guard state must be non-null and 16-byte aligned"
GRADHW = "gradient_loss needs H, W >= 2"
TILE = "need C,H,W,patch >= 1 and 1 <= stride <= patch"
HID16 = "hidden_channels must be 16 (adapter.py default)"
GEOM = "need n_img >= 1, patch_size >= 3, stride >= 1 and H, W >= patch_size"
MA_SUP = "need in_channels 1 or 3, hidden_channels 8 or 16, 0 <= num_fft_bins <= 8"
GN_C = "GroupNorm: C must be a multiple of 4 and of G, at most 1024"
GN_V = "GroupNorm: views need 16-byte alignment and off + C <= stride"
X6DC = "shape outside the bf16x6 deconv kernel"

# (function, arguments, status or returned value, dn_last_error afterwards)
CASES = [
    # ---- library, profiler ------------------------------------------------------------------
    ("dn_profile_ops_read", (None, 0, None), ARG, SENTINEL),
    ("dn_profile_ops_read", (None, 4, I32), ARG, SENTINEL),
    # ---- UNet -------------------------------------------------------------------------------
    ("dn_unet_param_count", (None, SZ), ARG, NULL),
    ("dn_unet_param_count", (G, None), ARG, NULL),
    ("dn_unet_param_count", (cfg(9), SZ), ARG, U_CFG),
    ("dn_unet_param_count", (cfg(1, 17), SZ), ARG, U_CFG),
    ("dn_unet_param_count", (cfg(1, 1, 32), SZ), ARG, NF48),
    ("dn_unet_param_info", (G, 0, SZ, SZ, None), ARG, NULL),
    ("dn_unet_param_info", (cfg(0), 0, SZ, SZ, SZ), ARG, U_CFG),
    ("dn_unet_param_info", (G, -1, SZ, SZ, SZ), ARG, "layer index out of range"),
    ("dn_unet_param_info", (G, 25, SZ, SZ, SZ), ARG, "layer index out of range"),
    ("dn_unet_workspace_size", (G, 1, 32, 32, 0, None), ARG, NULL),
    ("dn_unet_workspace_size", (cfg(9), 1, 32, 32, 0, SZ), ARG, U_CFG),
    ("dn_unet_workspace_size", (G, 1, 33, 32, 1, SZ), ARG, U_SHAPE),
    ("dn_unet_workspace_size", (G, 0, 32, 32, 0, SZ), ARG, U_SHAPE),
    ("dn_unet_forward", (G, None, A(1), A(2), 1, 32, 32, A(3), BIG, None), ARG, NULL),
    ("dn_unet_forward", (G, A(), A(1), A(2), 1, 32, 48, A(3), BIG, None), ARG, U_SHAPE),
    ("dn_unet_forward", (G, A(), A(1), A(2), 1, 32, 32, A(3), 16, None), WS, U_WS),
    ("dn_unet_forward_prec", (None, None, None, None, 1, 32, 32, None, 0, 7, None), ARG,
     "unknown precision"),
    ("dn_unet_forward_prec", (G, A(), A(1), None, 1, 32, 32, A(3), BIG, 2, None), ARG, NULL),
    ("dn_unet_forward_prec", (G, A(), A(1), None, 1, 32, 32, A(3), BIG, 1, None), ARG, NULL),
    ("dn_unet_forward_prec", (cfg(5), A(), A(1), A(2), 1, 32, 32, A(3), BIG, 2, None), ARG, U_CFG),
    ("dn_unet_forward_prec", (G, A(), A(1), A(2), 1, 32, 32, A(3), 16, 2, None), WS, U_WS),
    ("dn_unet_forward_prec", (G, A(), A(1), A(2), 1, 32, 32, A(3), 16, 1, None), WS, U_WS),
    ("dn_unet_forward_prec", (G, A(), A(1), A(2), 1, 31, 32, A(3), BIG, 1, None), ARG, U_SHAPE),
    ("dn_unet_forward_bf16", (G, A(), None, A(2), 1, 32, 32, A(3), BIG, None), ARG, NULL),
    ("dn_unet_forward_bf16", (cfg(1, 1, 64), A(), A(1), A(2), 1, 32, 32, A(3), BIG, None), ARG, NF48),
    ("dn_unet_forward_bf16", (G, A(), A(1), A(2), 1, 32, 32, A(3), 16, None), WS, U_WS),
    ("dn_unet_forward_n2n", (None, None, None, None, None, 1, 32, 32, None, 0, 1, None), ARG,
     "precision must be DN_PREC_FP32 or DN_PREC_FP32_X6"),
    ("dn_unet_forward_n2n", (G, A(), A(1), A(2), None, 1, 32, 32, A(3), BIG, 2, None), ARG, NULL),
    ("dn_unet_forward_n2n", (G, A(), A(1), A(2), A(4), 1, 32, 40, A(3), BIG, 2, None), ARG, U_SHAPE),
    ("dn_unet_forward_n2n", (G, A(), A(1), A(2), A(4), 1, 32, 32, A(3), 16, 0, None), WS, U_WS),
    ("dn_unet_pack_weights", (G, None, 1, 32, 32, A(3), BIG, 7, None), ARG, NULL),
    ("dn_unet_pack_weights", (G, A(), 1, 32, 32, A(3), BIG, 7, None), ARG, "unknown precision"),
    ("dn_unet_pack_weights", (G, A(), 1, 32, 33, A(3), BIG, 2, None), ARG, U_SHAPE),
    ("dn_unet_pack_weights", (G, A(), 1, 32, 32, A(3), 16, 2, None), WS, U_WS),
    ("dn_unet_pack_weights", (G, A(), 1, 32, 32, A(3), 16, 1, None), WS, U_WS),
    ("dn_unet_forward_prepacked", (G, A(), None, A(2), 1, 32, 32, A(3), BIG, 7, None), ARG, NULL),
    ("dn_unet_forward_prepacked", (G, A(), A(1), A(2), 1, 32, 32, A(3), BIG, -1, None), ARG,
     "unknown precision"),
    ("dn_unet_forward_prepacked", (G, A(), A(1), A(2), 1, 32, 32, A(3), 16, 0, None), WS, U_WS),
    ("dn_unet_backward", (G, A(), A(1), None, None, 1, 32, 32, A(3), BIG, None), ARG, NULL),
    ("dn_unet_backward", (G, A(), A(1), A(2), None, 1, 32, 32, A(3), 16, None), WS, U_WSB),
    ("dn_unet_backward_prec", (None, None, None, None, None, 1, 32, 32, None, 0, 1, None), ARG,
     U_BPREC),
    ("dn_unet_backward_prec", (None, A(), A(1), A(2), None, 1, 32, 32, A(3), BIG, 2, None), ARG, NULL),
    ("dn_unet_backward_prec", (G, A(), A(1), A(2), None, 2, 32, 30, A(3), BIG, 2, None), ARG, U_SHAPE),
    ("dn_unet_backward_prec", (G, A(), A(1), A(2), A(4), 1, 32, 32, A(3), 16, 2, None), WS, U_WSB),
    ("dn_unet_backward_split", (None, None, None, None, None, 1, 32, 32, None, 0, 1, None, None, I64),
     ARG, U_BPREC),
    ("dn_unet_backward_split", (None, None, None, None, None, 1, 32, 32, None, 0, 2, None, None, I64),
     ARG, NULL),
    ("dn_unet_backward_split", (G, None, None, None, None, 1, 32, 31, None, 0, 2, None, None, I64),
     ARG, U_SHAPE),
    ("dn_unet_backward_split", (G, A(), None, None, None, 1, 32, 32, None, 0, 2, None, None, I64),
     ARG, NULL),
    ("dn_unet_backward_split", (G, None, None, None, None, 1, 32, 32, None, 0, 2, None, A(5), I64),
     ARG, NULL),
    ("dn_unet_backward_split", (G, A(), A(1), A(2), None, 1, 32, 32, A(3), 16, 0, None, None, None),
     WS, U_WSB),
    ("dn_unet_debug_buffers", (G, 1, 32, 32, 1, None, 0, I32), ARG, NULL),
    ("dn_unet_debug_buffers", (G, 1, 32, 32, 1, I64, 0, None), ARG, NULL),
    ("dn_unet_debug_buffers", (G, 1, 32, 34, 1, I64, 0, I32), ARG, U_SHAPE),
    # ---- RESNET -----------------------------------------------------------------------------
    ("dn_resnet_param_count", (None, SZ), ARG, NULL),
    ("dn_resnet_param_count", (cfg(5, 5), SZ), ARG, "in_nc must be in [1,4]"),
    ("dn_resnet_param_count", (cfg(1, 3), SZ), ARG,
     "RESNET adds its input to its output: out_nc must equal in_nc"),
    ("dn_resnet_param_count", (cfg(1, 1, 96), SZ), ARG, NF48),
    ("dn_resnet_param_info", (G, 0, None, SZ, SZ), ARG, NULL),
    ("dn_resnet_param_info", (cfg(1, 2), 0, SZ, SZ, SZ), ARG,
     "RESNET adds its input to its output: out_nc must equal in_nc"),
    ("dn_resnet_param_info", (G, 21, SZ, SZ, SZ), ARG, "layer index out of range"),
    ("dn_resnet_workspace_size", (None, 1, 8, 8, 0, SZ), ARG, NULL),
    ("dn_resnet_workspace_size", (G, 0, 8, 8, 0, SZ), ARG, "N >= 1 and H, W >= 1"),
    ("dn_resnet_workspace_size", (G, 1, 65536, 65536, 0, SZ), ARG,
     "N * H * W too large for the 32-bit pixel offsets of the strided views"),
    ("dn_resnet_forward_prec", (None, None, None, None, 1, 8, 8, None, 0, 1, None), ARG, R_PREC),
    ("dn_resnet_forward_prec", (G, A(), A(1), A(2), 1, 8, 8, None, 0, 2, None), ARG, NULL),
    ("dn_resnet_forward_prec", (G, A(), A(1), A(2), 1, 8, 0, A(3), BIG, 2, None), ARG,
     "N >= 1 and H, W >= 1"),
    ("dn_resnet_forward_prec", (G, A(), A(1), A(2), 1, 8, 8, A(3), 16, 0, None), WS,
     "workspace smaller than dn_resnet_workspace_size()"),
    ("dn_resnet_backward_prec", (None, None, None, None, None, 1, 8, 8, None, 0, 5, None), ARG, R_PREC),
    ("dn_resnet_backward_prec", (G, A(), None, A(2), None, 1, 8, 8, A(3), BIG, 0, None), ARG, NULL),
    ("dn_resnet_backward_prec", (cfg(2, 1), A(), A(1), A(2), None, 1, 8, 8, A(3), BIG, 0, None), ARG,
     "RESNET adds its input to its output: out_nc must equal in_nc"),
    ("dn_resnet_backward_prec", (G, A(), A(1), A(2), None, 1, 8, 8, A(3), 16, 2, None), WS,
     "workspace smaller than dn_resnet_workspace_size(with_backward=1)"),
    ("dn_resnet_debug_buffers", (None, 1, 8, 8, 0, I64, 0, I32), ARG, NULL),
    ("dn_resnet_debug_buffers", (G, -1, 8, 8, 0, I64, 0, I32), ARG, "N >= 1 and H, W >= 1"),
    # ---- ImprovedUNet -----------------------------------------------------------------------
    ("dn_iunet_param_count", (G, None), ARG, NULL),
    ("dn_iunet_param_count", (cfg(4), SZ), ARG, "ImprovedUNet: in_nc must be 1..3 and out_nc 1..4"),
    ("dn_iunet_param_count", (cfg(1, 1, 32), SZ), ARG,
     "ImprovedUNet: only n_feature=48 is built (train.py:30 default)"),
    ("dn_iunet_workspace_size", (G, 1, 16, 16, 1, None), ARG, NULL),
    ("dn_iunet_workspace_size", (G, 1, 24, 16, 1, SZ), ARG, I_SHAPE),
    ("dn_iunet_workspace_size", (cfg(1, 5), 1, 16, 16, 1, SZ), ARG,
     "ImprovedUNet: in_nc must be 1..3 and out_nc 1..4"),
    ("dn_iunet_forward", (G, A(), A(1), None, 1, 16, 16, A(3), BIG, None), ARG, NULL),
    ("dn_iunet_forward", (G, A(), A(1), A(2), 1, 16, 16, A(3), 16, None), WS,
     "workspace smaller than dn_iunet_workspace_size()"),
    ("dn_iunet_forward_prec", (None, None, None, None, 1, 16, 16, None, 0, 1, None), ARG, I_PREC),
    ("dn_iunet_forward_prec", (None, A(), A(1), A(2), 1, 16, 16, A(3), BIG, 2, None), ARG, NULL),
    ("dn_iunet_forward_prec", (G, A(), A(1), A(2), 0, 16, 16, A(3), BIG, 2, None), ARG, I_SHAPE),
    ("dn_iunet_forward_prec", (G, A(), A(1), A(2), 1, 16, 16, A(3), 16, 2, None), WS,
     "workspace smaller than dn_iunet_workspace_size()"),
    ("dn_iunet_backward", (G, A(), A(1), None, 1, 16, 16, A(3), BIG, None), ARG, NULL),
    ("dn_iunet_backward", (G, A(), A(1), A(2), 1, 16, 16, A(3), 16, None), WS,
     "workspace smaller than dn_iunet_workspace_size(with_backward=1)"),
    ("dn_iunet_backward_prec", (None, None, None, None, 1, 16, 16, None, 0, 1, None), ARG, I_PREC),
    ("dn_iunet_backward_prec", (G, A(), A(1), A(2), 1, 16, 16, None, BIG, 2, None), ARG, NULL),
    ("dn_iunet_backward_prec", (G, A(), A(1), A(2), 1, 16, 8, A(3), BIG, 2, None), ARG, I_SHAPE),
    ("dn_iunet_backward_prec", (G, A(), A(1), A(2), 1, 16, 16, A(3), 16, 2, None), WS,
     "workspace smaller than dn_iunet_workspace_size(with_backward=1)"),
    ("dn_iunet_debug_buffers", (G, 1, 16, 16, 0, I64, 0, None), ARG, NULL),
    ("dn_iunet_debug_buffers", (G, 1, 16, 17, 0, I64, 0, I32), ARG, I_SHAPE),
    # ---- sub-sampler, noise -----------------------------------------------------------------
    ("dn_n2n_subsample", (A(), 1, 1, 3, 2, None, 0, 0, 0, A(1), A(2), None, None), ARG,
     "H and W must be even"),
    ("dn_n2n_subsample", (A(), 1, 0, 2, 2, None, 0, 0, 0, A(1), A(2), None, None), ARG,
     "H and W must be even"),
    ("dn_n2n_subsample", (None, 1, 1, 2, 2, None, 0, 0, 0, A(1), A(2), None, None), ARG, NULL),
    ("dn_n2n_masks", (None, -1, None, None, None), ARG, "ncells < 0"),
    ("dn_n2n_masks", (A(), 4, None, A(2), None), ARG, NULL),
    ("dn_n2n_subimage_from_mask", (A(), 1, 1, 2, 5, A(1), A(2), None), ARG, "H and W must be even"),
    ("dn_n2n_subimage_from_mask", (A(), 1, 1, 2, 2, None, A(2), None), ARG, NULL),
    ("dn_add_gauss_noise", (A(), -1, 4, 0.1, None, 0, 0, 0, A(1), None), ARG, "negative size"),
    ("dn_add_gauss_noise", (A(), 1, 4, 0.1, None, 0, 0, 0, None, None), ARG, NULL),
    ("dn_add_poisson_noise", (A(), 1, -4, 1.0, None, 0, 0, 0, A(1), None), ARG, "negative size"),
    ("dn_add_poisson_noise", (A(), 1, 4, 0.0, None, 0, 0, 0, A(1), None), ARG,
     "lam must be in (0, 500]"),
    ("dn_add_poisson_noise", (A(), 1, 4, NAN, None, 0, 0, 0, A(1), None), ARG,
     "lam must be in (0, 500]"),
    ("dn_add_poisson_noise", (None, 1, 4, 1.0, None, 0, 0, 0, A(1), None), ARG, NULL),
    # ---- losses -----------------------------------------------------------------------------
    ("dn_n2n_loss", (A(), A(1), A(2), A(3), 1, 1, 2, 2, 1.0, A(4), A(5), None, None), ARG, NULL),
    ("dn_n2n_loss", (A(), A(1), A(2), A(3), 0, 1, 2, 2, 1.0, A(4), A(5), A(6), None), ARG,
     "empty loss input"),
    ("dn_structure_loss", (A(), A(1), None, 1, 1, 2, 2, 1.0, 1.0, 1.0, A(3), A(4), A(5), A(6), None),
     ARG, NULL),
    ("dn_structure_loss", (A(), A(1), A(2), 1, 1, 1, 2, 1.0, 1.0, 1.0, A(3), A(4), A(5), A(6), None),
     ARG, "Structure_loss needs H, W >= 2"),
    ("dn_l1fft_ws_size", (1, 1, 7, 8), 0, SENTINEL),
    ("dn_l1fft_loss", (None, None, 1, 1, 7, 8, 1.0, 1.0, 0, None, None, None, 0, None), ARG,
     "L1FFT needs N, C >= 1 and H, W = m * 2^k with m odd <= 31, k >= 3, at most 1024"),
    ("dn_l1fft_loss", (A(), A(1), 1, 1, 8, 8, 1.0, 1.0, 0, A(2), None, A(4), BIG, None), ARG, NULL),
    ("dn_l1fft_loss", (A(), A(1), 1, 1, 8, 8, 1.0, 1.0, 0, A(2), A(3), U, BIG, None), ARG,
     "workspace must be 16-byte aligned"),
    ("dn_l1fft_loss", (A(), A(1), 1, 1, 8, 8, 1.0, 1.0, 0, A(2), A(3), A(4), 16, None), WS,
     "workspace smaller than dn_l1fft_ws_size()"),
    ("dn_finetune_loss", (A(), None, 1, 1, 2, 2, 0.1, A(2), A(3), A(4), None), ARG, NULL),
    ("dn_finetune_loss", (A(), A(1), 1, 1, 2, 1, 0.1, A(2), A(3), A(4), None), ARG, GRADHW),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 2, 2, 0.1, 0.1, 0.3, 0.6, 1.0, 0.0, 1.0, A(2), None, A(4), None), ARG, NULL),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 3, 2, 2, 0.1, 0.1, 0.3, 0.6, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL assumes single-channel input: C must be 1"),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 1, 2, 0.1, 0.1, 0.3, 0.6, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG, GRADHW),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 2, 2, 0.1, 0.1, 0.3, INF, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL thresholds must be finite"),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 2, 2, 0.1, 0.1, 0.3, 0.6, NAN, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL tau, margin and ce_factor must be finite"),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 2, 2, 0.1, 0.1, 0.6, 0.6, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL needs t1 < t2 (as fp32 values too)"),
    ("dn_finetune_iqsl_loss",
     (A(), A(1), 1, 1, 2, 2, 0.1, 0.1, 0.5, 0.5 + 1e-12, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL needs t1 < t2 (as fp32 values too)"),
    ("dn_iqsl_loss", (A(), A(1), 1, 1, 2, 2, 0.3, 0.6, 1.0, 0.0, 1.0, None, A(3), A(4), None), ARG, NULL),
    ("dn_iqsl_loss", (A(), A(1), 1, 2, 2, 2, 0.3, 0.6, 1.0, 0.0, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL assumes single-channel input: C must be 1"),
    ("dn_iqsl_loss", (A(), A(1), 1, 1, 2, 2, 0.3, 0.6, 1.0, INF, 1.0, A(2), A(3), A(4), None), ARG,
     "IQSL tau, margin and ce_factor must be finite"),
    # ---- optimiser, guard -------------------------------------------------------------------
    ("dn_adam_step", (A(), A(1), A(2), A(3), -1, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None), ARG,
     "n >= 0 and step >= 1 required"),
    ("dn_adam_step", (A(), A(1), A(2), A(3), 4, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, None), ARG,
     "n >= 0 and step >= 1 required"),
    ("dn_adam_step", (A(), A(1), None, A(3), 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None), ARG, NULL),
    ("dn_guard_state_init", (None, 0, None), ARG, GUARD),
    ("dn_guard_state_init", (U, 0, None), ARG, GUARD),
    ("dn_guard_state_init", (A(), -1, None), ARG, "step >= 0 required"),
    ("dn_grad_norm", (A(), -1, 1.0, A(1), None, None), ARG, "n < 0"),
    ("dn_grad_norm", (None, 4, 1.0, A(1), None, None), ARG, NULL),
    ("dn_grad_norm", (A(), 4, 1.0, U, None, None), ARG, GUARD),
    ("dn_adam_step_guarded",
     (A(), A(1), A(2), A(3), -1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, 0.0, 0.0, 0.0, A(4), None), ARG,
     "n < 0"),
    ("dn_adam_step_guarded",
     (A(), A(1), A(2), None, 4, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, 0.0, 0.0, 0.0, A(4), None), ARG,
     NULL),
    ("dn_adam_step_guarded",
     (A(), A(1), A(2), A(3), 4, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, 0.0, 0.0, 0.0, None, None), ARG,
     GUARD),
    ("dn_guard_state_read", (U, STATS, None), ARG, "null argument or unaligned guard state"),
    ("dn_guard_state_read", (A(), None, None), ARG, "null argument or unaligned guard state"),
    ("dn_accumulate", (A(), A(1), -1, None), ARG, "n < 0"),
    ("dn_accumulate", (A(), None, 4, None), ARG, NULL),
    # ---- evaluation path --------------------------------------------------------------------
    ("dn_u8_to_unit", (A(), -1, A(1), None), ARG, "n < 0"),
    ("dn_u8_to_unit", (None, 4, A(1), None), ARG, NULL),
    ("dn_tile_count", (0, 4, 4), 0, SENTINEL),
    ("dn_tile_count", (8, 4, 0), 0, SENTINEL),
    ("dn_tile_extract", (A(), 1, 8, 8, 4, 4, None, None), ARG, NULL),
    ("dn_tile_extract", (A(), 1, 8, 8, 4, 5, A(1), None), ARG, TILE),
    ("dn_tile_blend", (A(), 1, 8, 8, 4, 4, A(1), None, None, None), ARG, NULL),
    ("dn_tile_blend", (A(), 0, 8, 8, 4, 4, A(1), A(2), None, None), ARG, TILE),
    ("dn_quantize_u8", (A(), -1, 0, A(1), None), ARG, "n < 0"),
    ("dn_quantize_u8", (A(), 4, 0, None, None), ARG, NULL),
    ("dn_psnr_u8", (A(), A(1), 0, A(2), A(3), None), ARG, "n >= 1 required"),
    ("dn_psnr_u8", (A(), A(1), 4, None, A(3), None), ARG, NULL),
    ("dn_ssim_u8", (None, None, 1, 10, 16, 0, None, None, None), ARG, "need C >= 1 and H, W > 10"),
    ("dn_ssim_u8", (A(), A(1), 1, 16, 16, 0, A(2), None, None), ARG, NULL),
    ("dn_l1_mean", (None, None, 0, None, None, None), ARG, "n >= 1 required"),
    ("dn_l1_mean", (A(), None, 4, A(2), A(3), None), ARG, NULL),
    ("dn_l1_mean_batched", (A(), A(1), -1, 4, A(2), None), ARG, "P >= 0 and n >= 1 required"),
    ("dn_l1_mean_batched", (A(), A(1), 1 << 31, 4, A(2), None), ARG, "P too large"),
    ("dn_l1_mean_batched", (A(), A(1), 2, 4, None, None), ARG, NULL),
    ("dn_iq_iou_u8", (A(), A(1), 1, 4, 4, 0.3, 0.6, A(2), None, None), ARG, NULL),
    ("dn_iq_iou_u8", (A(), A(1), 65537, 4, 4, 0.3, 0.6, A(2), I64, None), ARG,
     "need 1 <= C <= 65536 and H, W >= 1"),
    ("dn_iq_iou_u8", (A(), A(1), 1, 4, 4, 0.6, 0.3, A(2), I64, None), ARG,
     "need t1 <= t2, neither NaN"),
    ("dn_iq_iou_u8", (A(), A(1), 1, 4, 4, NAN, 0.3, A(2), I64, None), ARG,
     "need t1 <= t2, neither NaN"),
    ("dn_hann_blend", (A(), A(1), A(2), None, 1, 1, 1, 8, 8, 4, A(4), None), ARG, NULL),
    ("dn_hann_blend", (A(), A(1), A(2), A(3), 1, 1, 1, 8, 3, 4, A(4), None), ARG,
     "need ny, nx, C >= 1 and H, W >= patch_size >= 1"),
    # ---- op-level convolutions, deconvolutions, pooling ---------------------------------------
    ("dn_conv2d_pack_size", (48, 48, 5, 0), 0, SENTINEL),
    ("dn_deconv2x2_pack_size", (0, 48, 0), 0, SENTINEL),
    ("dn_conv2d_bf16_pack_size", (48, 0), 0, SENTINEL),
    ("dn_conv2d_x6_pack_size", (0, 48, 1), 0, SENTINEL),
    ("dn_conv2d_forward", (A(), 48, 1, 4, 4, 48, None, A(2), 48, 3, 1, A(3), 48, A(4), BIG, None),
     ARG, NULL),
    ("dn_conv2d_forward", (A(), 48, 1, 4, 4, 48, A(1), A(2), 48, 5, 1, A(3), 48, A(4), BIG, None),
     ARG, "ksize must be 1 or 3"),
    ("dn_conv2d_forward", (A(), 47, 1, 4, 4, 48, A(1), A(2), 48, 3, 1, A(3), 48, A(4), BIG, None),
     ARG, "bad shape"),
    ("dn_conv2d_forward", (A(), 48, 1, 4, 4, 48, A(1), A(2), 0, 3, 1, A(3), 48, A(4), BIG, None),
     ARG, CHAN),
    ("dn_conv2d_forward", (A(), 48, 1, 4, 4, 48, A(1), A(2), 48, 3, 1, A(3), 48, None, BIG, None),
     WS, PACK),
    ("dn_conv2d_forward", (A(), 48, 1, 4, 4, 48, A(1), A(2), 48, 3, 1, A(3), 48, A(4), 16, None),
     WS, PACK),
    ("dn_conv2d_forward_bf16", (A(), 48, 1, 4, 4, 48, A(1), None, 48, 1, A(3), 48, A(4), BIG, None),
     ARG, NULL),
    ("dn_conv2d_forward_bf16", (A(), 48, 1, 4, 4, 48, A(1), A(2), 46, 1, A(3), 48, A(4), BIG, None),
     ARG, "bad shape (Cout and y_stride must be multiples of 4)"),
    ("dn_conv2d_forward_bf16", (A(), 48, 1, 4, 4, 48, A(1), A(2), 0, 1, A(3), 48, A(4), BIG, None),
     ARG, CHAN),
    ("dn_conv2d_forward_bf16", (A(), 48, 1, 4, 4, 48, A(1), A(2), 48, 1, A(3), 48, A(4), 16, None),
     WS, PACK),
    ("dn_conv2d_forward_x6", (None, 48, 1, 4, 4, 48, A(1), A(2), 48, 1, A(3), 48, A(4), BIG, None),
     ARG, NULL),
    ("dn_conv2d_forward_x6", (A(), 48, 0, 4, 4, 48, A(1), A(2), 48, 1, A(3), 48, A(4), BIG, None),
     ARG, "bad shape"),
    ("dn_conv2d_forward_x6", (A(), 48, 1, 4, 4, 48, A(1), A(2), 200, 1, A(3), 200, A(4), BIG, None),
     ARG, "bf16x6 forward supports Cout <= 96"),
    ("dn_conv2d_forward_x6", (A(), 48, 1, 4, 4, 48, A(1), A(2), 48, 1, A(3), 48, A(4), 16, None),
     WS, PACK),
    ("dn_upconv3_forward_x6",
     (A(), 96, 1, 4, 4, A(1), 1, A(2), A(3), A(4), None, A(6), 96, A(7), BIG, None), ARG, NULL),
    ("dn_upconv3_forward_x6",
     (A(), 96, 1, 4, 4, A(1), 5, A(2), A(3), A(4), A(5), A(6), 96, A(7), BIG, None), ARG,
     "bad shape (1 <= C <= 4, strides >= 96 and multiples of 4)"),
    ("dn_upconv3_forward_x6",
     (A(), 96, 1, 4, 4, A(1), 1, A(2), A(3), A(4), A(5), A(6), 96, A(7), 16, None), WS, PACK),
    ("dn_conv2d_backward_data_x6",
     (A(), 1, 4, 4, 48, A(1), 48, None, 0, 0, None, 48, A(4), BIG, None), ARG, NULL),
    ("dn_conv2d_backward_data_x6",
     (A(), 1, 4, 4, 48, A(1), 48, None, 0, 0, A(3), 47, A(4), BIG, None), ARG, "bad shape"),
    ("dn_conv2d_backward_data_x6",
     (A(), 1, 4, 4, 48, A(1), 48, A(2), 48, 1, A(3), 48, A(4), BIG, None), ARG,
     "mask and accumulate are exclusive"),
    ("dn_conv2d_backward_data_x6",
     (A(), 1, 4, 4, 48, A(1), 0, None, 0, 0, A(3), 48, A(4), BIG, None), ARG,
     "bf16x6 data gradient: unsupported Cin"),
    ("dn_conv2d_backward_data_x6",
     (A(), 1, 4, 4, 48, A(1), 48, None, 0, 0, A(3), 48, A(4), 16, None), WS, PACK),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 4, 48, None, 48, 3, None, 0, 0, A(3), 48, A(4), BIG, None), ARG, NULL),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 4, 48, A(1), 48, 2, None, 0, 0, A(3), 48, A(4), BIG, None), ARG,
     "ksize must be 1 or 3"),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 0, 48, A(1), 48, 3, None, 0, 0, A(3), 48, A(4), BIG, None), ARG, "bad shape"),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 4, 48, A(1), 48, 3, A(2), 48, 1, A(3), 48, A(4), BIG, None), ARG,
     "mask and accumulate are exclusive"),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 4, 48, A(1), 0, 3, None, 0, 0, A(3), 48, A(4), BIG, None), ARG, CHAN),
    ("dn_conv2d_backward_data",
     (A(), 1, 4, 4, 48, A(1), 48, 3, None, 0, 0, A(3), 48, None, BIG, None), WS, PACK),
    ("dn_conv2d_backward_weight", (A(), A(1), 48, 1, 4, 4, 48, 48, 3, A(2), None, None), ARG, NULL),
    ("dn_conv2d_backward_weight", (A(), A(1), 48, 1, 4, 4, 48, 48, 4, A(2), A(3), None), ARG,
     "ksize must be 1 or 3"),
    ("dn_conv2d_backward_weight", (A(), A(1), 48, 1, 4, 4, 48, 20, 3, A(2), A(3), None), ARG,
     "unsupported Cout"),
    ("dn_conv2d_backward_weight", (A(), A(1), 100, 1, 4, 4, 100, 96, 1, A(2), A(3), None), ARG,
     "1x1 wgrad supports Cin <= 96"),
    ("dn_conv2d_backward_weight_x6", (A(), None, 48, 1, 4, 4, 48, 48, A(2), A(3), None), ARG, NULL),
    ("dn_conv2d_backward_weight_x6", (A(), A(1), 48, 1, 4, 4, 48, 64, A(2), A(3), None), ARG,
     "unsupported Cout"),
    ("dn_deconv2x2_forward", (A(), 1, 4, 4, 48, A(1), A(2), 48, None, 48, 0, A(4), BIG, None),
     ARG, NULL),
    ("dn_deconv2x2_forward", (A(), 1, 4, 4, 48, A(1), A(2), 48, A(3), 48, 4, A(4), BIG, None),
     ARG, "bad shape"),
    ("dn_deconv2x2_forward", (A(), 1, 4, 4, 48, A(1), A(2), 0, A(3), 48, 0, A(4), BIG, None),
     ARG, CHAN),
    ("dn_deconv2x2_forward", (A(), 1, 4, 4, 48, A(1), A(2), 48, A(3), 48, 0, A(4), 16, None),
     WS, PACK),
    ("dn_deconv2x2_forward_x6", (A(), 1, 4, 4, None, A(2), A(3), 96, 0, A(4), BIG, None), ARG, NULL),
    ("dn_deconv2x2_forward_x6", (A(), 1, 4, 4, A(1), A(2), A(3), 98, 0, A(4), BIG, None), ARG,
     "bad shape"),
    ("dn_deconv2x2_forward_x6", (A(), 1, 4, 4, A(1), A(2), A(3), 96, 0, A(4), 16, None), WS, PACK),
    ("dn_deconv2x2_forward_x6", (A(), 1, 1, 6000000, A(1), A(2), A(3), 96, 0, A(4), BIG, None), ARG,
     X6DC),
    ("dn_deconv2x2_backward_data_x6", (A(), 96, 1, 4, 4, A(1), None, None, A(4), BIG, None), ARG,
     NULL),
    ("dn_deconv2x2_backward_data_x6", (A(), 95, 1, 4, 4, A(1), None, A(3), A(4), BIG, None), ARG,
     "bad shape"),
    ("dn_deconv2x2_backward_data_x6", (A(), 96, 1, 4, 4, A(1), None, A(3), None, BIG, None), WS,
     PACK),
    ("dn_deconv2x2_backward_data_x6", (A(), 96, 1, 1, 3000000, A(1), None, A(3), A(4), BIG, None),
     ARG, X6DC),
    ("dn_deconv2x2_backward_data", (None, 48, 1, 4, 4, 48, A(1), 48, None, A(3), A(4), BIG, None),
     ARG, NULL),
    ("dn_deconv2x2_backward_data", (A(), 40, 1, 4, 4, 48, A(1), 48, None, A(3), A(4), BIG, None),
     ARG, "bad shape"),
    ("dn_deconv2x2_backward_data", (A(), 48, 1, 4, 4, 48, A(1), 0, None, A(3), A(4), BIG, None),
     ARG, CHAN),
    ("dn_deconv2x2_backward_data", (A(), 48, 1, 4, 4, 48, A(1), 48, None, A(3), A(4), 16, None),
     WS, PACK),
    ("dn_deconv2x2_backward_weight", (A(), 48, A(1), 1, 4, 4, 48, 48, None, A(3), None), ARG, NULL),
    ("dn_deconv2x2_backward_weight", (A(), 48, A(1), 1, 4, 4, 48, 8, A(2), A(3), None), ARG,
     "unsupported Cout"),
    ("dn_maxpool2x2_forward", (A(), 1, 4, 4, 48, None, 48, 0, None), ARG, NULL),
    ("dn_maxpool2x2_forward", (A(), 1, 4, 4, 46, A(1), 48, 0, None), ARG,
     "H, W even and C, y_stride, y_off multiples of 4 required"),
    ("dn_maxpool2x2_backward", (A(), 1, 4, 4, 48, None, 48, 0, 0, A(2), None), ARG, NULL),
    ("dn_maxpool2x2_backward", (A(), 1, 3, 4, 48, A(1), 48, 0, 0, A(2), None), ARG,
     "H, W even and C, dy_stride, dy_off multiples of 4 required"),
    # ---- ImprovedUNet building blocks ---------------------------------------------------------
    ("dn_groupnorm_scratch_size", (1, 4, 4, 6), 0, SENTINEL),
    ("dn_groupnorm_forward",
     (A(), 48, 0, None, 0, 0, A(1), 48, 0, 1, 4, 4, 48, 8, A(2), A(3), 1, None, A(5), BIG, None),
     ARG, NULL),
    ("dn_groupnorm_forward",
     (A(), 48, 0, None, 0, 0, A(1), 48, 0, 1, 4, 4, 48, 7, A(2), A(3), 1, A(4), A(5), BIG, None),
     ARG, GN_C),
    ("dn_groupnorm_forward",
     (U, 48, 0, None, 0, 0, A(1), 48, 0, 1, 4, 4, 48, 8, A(2), A(3), 1, A(4), A(5), BIG, None),
     ARG, GN_V),
    ("dn_groupnorm_forward",
     (None, 48, 0, None, 0, 0, A(1), 48, 0, 1, 4, 4, 48, 8, A(2), A(3), 1, A(4), A(5), BIG, None),
     ARG, GN_V),
    ("dn_groupnorm_forward",
     (A(), 48, 0, A(6), 48, 4, A(1), 48, 0, 1, 4, 4, 48, 8, A(2), A(3), 1, A(4), A(5), BIG, None),
     ARG, GN_V),
    ("dn_groupnorm_forward",
     (A(), 48, 0, None, 0, 0, A(1), 48, 0, 1, 4, 4, 48, 8, A(2), A(3), 1, A(4), A(5), 16, None),
     WS, "scratch smaller than dn_groupnorm_scratch_size()"),
    ("dn_groupnorm_backward",
     (A(), 48, 0, A(1), 48, 0, A(2), 48, 0, 1, 4, 4, 48, 8, None, A(4), A(5), A(6), A(7), BIG, None),
     ARG, NULL),
    ("dn_groupnorm_backward",
     (A(), 48, 0, A(1), 48, 0, A(2), 48, 0, 1, 4, 4, 2048, 8, A(3), A(4), A(5), A(6), A(7), BIG, None),
     ARG, GN_C),
    ("dn_groupnorm_backward",
     (A(), 48, 0, A(1), 48, 0, A(2), 48, 0, 1, 4, 4, 48, 8, A(3), A(4), A(5), A(6), U, BIG, None),
     ARG, GN_V),
    ("dn_groupnorm_backward",
     (A(), 48, 0, A(1), 48, 0, A(2), 48, 0, 1, 4, 4, 48, 8, A(3), A(4), A(5), A(6), A(7), 16, None),
     WS, "scratch smaller than dn_groupnorm_scratch_size()"),
    ("dn_conv2d_wgrad_blocked_slab_size", (0, 4, 4, 48, 48, 3), 0, SENTINEL),
    ("dn_conv2d_backward_weight_blocked",
     (A(), 48, 0, None, 48, 0, 1, 4, 4, 48, 48, 3, 1, 0, A(2), A(3), None), ARG, NULL),
    ("dn_conv2d_backward_weight_blocked",
     (A(), 48, 0, A(1), 48, 0, 1, 4, 4, 48, 48, 2, 1, 0, A(2), A(3), None), ARG,
     "ksize must be 1 or 3"),
    ("dn_conv2d_backward_weight_blocked",
     (A(), 48, 0, A(1), 48, 0, 1, 4, 4, 48, 48, 3, 1, 1, A(2), A(3), None), ARG,
     "precision must be DN_PREC_FP32 or DN_PREC_FP32_X6"),
    ("dn_conv2d_backward_weight_blocked",
     (A(), 48, -4, A(1), 48, 0, 1, 4, 4, 48, 48, 3, 1, 0, A(2), A(3), None), ARG, "bad shape"),
    ("dn_conv2d_backward_weight_blocked",
     (A(), 48, 0, U, 48, 0, 1, 4, 4, 48, 48, 3, 1, 0, A(2), A(3), None), ARG,
     "g, x and slab must be 16-byte aligned"),
    # ---- output adapter -----------------------------------------------------------------------
    ("dn_adapter_param_count", (1, 16, None), ARG, NULL),
    ("dn_adapter_param_count", (1, 8, SZ), ARG, HID16),
    ("dn_adapter_param_count", (2, 16, SZ), ARG, "in_channels must be 1 or 3"),
    ("dn_adapter_slab_size", (1, 1, 4, 4, 8), 0, SENTINEL),
    ("dn_adapter_forward", (A(), A(1), None, A(3), 1, 1, 4, 4, 16, None), ARG, NULL),
    ("dn_adapter_forward", (A(), A(1), A(2), A(3), 1, 1, 4, 4, 32, None), ARG, HID16),
    ("dn_adapter_forward", (A(), A(1), A(2), A(3), 1, 2, 4, 4, 16, None), ARG,
     "in_channels must be 1 or 3"),
    ("dn_adapter_forward", (A(), A(1), A(2), A(3), 0, 1, 4, 4, 16, None), ARG,
     "empty adapter input"),
    ("dn_adapter_backward", (A(), A(1), A(2), A(3), None, 1, 1, 4, 4, 16, A(5), BIG, None), ARG,
     NULL),
    ("dn_adapter_backward", (A(), A(1), A(2), A(3), A(4), 1, 1, 4, 0, 16, A(5), BIG, None), ARG,
     "empty adapter input"),
    ("dn_adapter_backward", (A(), A(1), A(2), A(3), A(4), 1, 1, 4, 4, 16, A(5), 16, None), WS,
     "slab smaller than dn_adapter_slab_size()"),
    ("dn_adapter_backward_input", (A(), A(1), A(2), A(3), None, None, 1, 1, 4, 4, 16, None), ARG,
     NULL),
    ("dn_adapter_backward_input", (A(), A(1), A(2), A(3), A(4), None, 1, 4, 4, 4, 16, None), ARG,
     "in_channels must be 1 or 3"),
    ("dn_adapter_backward_input", (A(), A(1), A(2), A(3), A(2), None, 1, 1, 4, 4, 16, None), ARG,
     "dbase / dnoisy must not alias noisy, base_out or dout"),
    ("dn_adapter_backward_input", (A(), A(1), A(2), A(3), A(4), A(3), 1, 1, 4, 4, 16, None), ARG,
     "dbase / dnoisy must not alias noisy, base_out or dout"),
    ("dn_adapter_backward_input", (A(), A(1), A(2), A(3), A(4), A(4), 1, 1, 4, 4, 16, None), ARG,
     "dbase and dnoisy must be distinct buffers"),
    # ---- memory bank, memory adapter ------------------------------------------------------------
    ("dn_memory_select_ws_size", (0, 1, 1, 8, 8, 3, 1), 0, SENTINEL),
    ("dn_memory_select_ws_size", (1, 1, 2, 8, 8, 3, 1), 0, "bank channels must be 1 or 3"),
    ("dn_memory_select", (A(), A(1), 1, 1, 1, 8, 8, 3, 1, None, A(3), BIG, None), ARG, NULL),
    ("dn_memory_select", (A(), A(1), 0, 1, 1, 8, 8, 3, 1, A(2), A(3), BIG, None), ARG,
     "need B >= 1"),
    ("dn_memory_select", (A(), A(1), 1, 1, 2, 8, 8, 3, 1, A(2), A(3), BIG, None), ARG,
     "bank channels must be 1 or 3"),
    ("dn_memory_select", (A(), A(1), 1, 1, 1, 8, 8, 2, 1, A(2), A(3), BIG, None), ARG, GEOM),
    ("dn_memory_select", (A(), A(1), 1, 1, 1, 8, 2, 3, 1, A(2), A(3), BIG, None), ARG, GEOM),
    ("dn_memory_select", (A(), A(1), 1, 1 << 30, 1, 8, 8, 3, 1, A(2), A(3), BIG, None), ARG,
     "bank too large (2^31 windows)"),
    ("dn_memory_select", (A(), A(1), 1, 1, 1, 8, 8, 3, 1, A(2), A(3), 16, None), WS,
     "workspace smaller than dn_memory_select_ws_size()"),
    ("dn_memory_gather", (A(), None, 1, 1, 1, 8, 8, 3, 1, A(2), None), ARG, NULL),
    ("dn_memory_gather", (A(), A(1), 0, 1, 1, 8, 8, 3, 1, A(2), None), ARG, "need B >= 1"),
    ("dn_memory_gather", (A(), A(1), 1, 0, 1, 8, 8, 3, 1, A(2), None), ARG, GEOM),
    ("dn_memadapter_param_count", (1, 8, 4, None), ARG, NULL),
    ("dn_memadapter_param_count", (1, 4, 4, SZ), ARG, MA_SUP),
    ("dn_memadapter_param_count", (1, 8, 9, SZ), ARG, MA_SUP),
    ("dn_memadapter_ws_size", (0, 1, 8, 8, 8, 4, 0), 0, SENTINEL),
    ("dn_memadapter_ws_size", (1, 2, 8, 8, 8, 4, 2), 0, SENTINEL),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), None, 1, 1, 8, 8, 8, 4, 0, A(6), BIG, None), ARG, NULL),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 2, 8, 8, 8, 4, 0, A(6), BIG, None), ARG, MA_SUP),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), A(5), 0, 1, 8, 8, 8, 4, 0, A(6), BIG, None), ARG,
     "empty adapter input"),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 1, 1, 8, 0, 0, A(6), BIG, None), ARG,
     "the unbiased std needs at least two elements per sample"),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 4, 4, 8, 8, 0, A(6), BIG, None), ARG,
     "row FFT has fewer bins than num_fft_bins"),
    ("dn_memadapter_forward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 8, 8, 8, 4, 0, A(6), 16, None), WS,
     "workspace smaller than dn_memadapter_ws_size()"),
    ("dn_memadapter_backward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 8, 8, 8, 4, 0, None, BIG, None), ARG, NULL),
    ("dn_memadapter_backward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 8, 8, 12, 4, 0, A(6), BIG, None), ARG, MA_SUP),
    ("dn_memadapter_backward",
     (A(), A(1), A(2), A(3), A(4), A(5), 1, 1, 8, 8, 8, 4, 0, A(6), 16, None), WS,
     "workspace smaller than dn_memadapter_ws_size()"),
    ("dn_memadapter_backward_input",
     (A(), A(1), A(2), A(3), A(4), None, None, 1, 1, 8, 8, 8, 4, 0, A(7), BIG, None), ARG, NULL),
    ("dn_memadapter_backward_input",
     (A(), A(1), A(2), A(3), A(4), None, A(6), 1, 1, 8, 8, 8, -1, 0, A(7), BIG, None), ARG, MA_SUP),
    ("dn_memadapter_backward_input",
     (A(), A(1), A(2), A(3), A(4), None, A(1), 1, 1, 8, 8, 8, 4, 0, A(7), BIG, None), ARG,
     "dbase must not alias an input or dparams"),
    ("dn_memadapter_backward_input",
     (A(), A(1), A(2), A(3), A(4), A(5), A(5) + 64, 1, 1, 8, 8, 8, 4, 0, A(7), BIG, None), ARG,
     "dbase must not alias an input or dparams"),
    ("dn_memadapter_backward_input",
     (A(), A(1), A(2), A(3), A(4), None, A(6), 1, 1, 8, 8, 8, 4, 0, A(7), 16, None), ARG,
     "workspace smaller than dn_memadapter_ws_size(with_backward = 2)"),
    ("dn_memadapter_feature_adjoint", (A(), None, A(2), 1, 1, 8, 8, 4, A(3), BIG, None), ARG, NULL),
    ("dn_memadapter_feature_adjoint", (A(), A(1), A(2), 1, 1, 8, 8, 9, A(3), BIG, None), ARG, MA_SUP),
    ("dn_memadapter_feature_adjoint", (A(), A(1), A() + 128, 1, 1, 8, 8, 4, A(3), BIG, None), ARG,
     "hyper must not alias base_out"),
    ("dn_memadapter_feature_adjoint", (A(), A(1), A(2), 1, 1, 8, 8, 4, A(3), 16, None), ARG,
     "workspace smaller than dn_memadapter_ws_size(hidden 8, with_backward = 2)"),
]

# exported functions with no case: they cannot fail (dn_version, dn_abi_version, dn_last_error,
# dn_profile_ops, the *_size queries without arguments, dn_conv2d_wgrad_slab_size and
# dn_deconv2x2_wgrad_slab_size, which answer for any shape) or must not be called with passing
# arguments here and check nothing (dn_prepare_streams)
NEVER_REJECT = {
    "dn_version", "dn_abi_version", "dn_last_error", "dn_profile_ops", "dn_prepare_streams",
    "dn_loss_partials_size", "dn_guard_state_size", "dn_eval_partials_size",
    "dn_iqsl_partials_size", "dn_upconv3_x6_pack_size", "dn_deconv2x2_x6_pack_size",
    "dn_conv2d_wgrad_slab_size", "dn_deconv2x2_wgrad_slab_size",
}


def _call(fn, args):
    """(returned value, dn_last_error afterwards); the message before the call is SENTINEL"""
    L = _lib.lib()
    assert L.dn_n2n_masks(None, -1, None, None, None) == ARG and _lib.last_error() == SENTINEL
    return getattr(L, fn)(*args), _lib.last_error()


@pytest.mark.parametrize("fn,args,status,message", CASES,
                         ids=[f"{i:03d}-{c[0]}" for i, c in enumerate(CASES)])
def test_rejected_as_recorded(fn, args, status, message):
    assert _call(fn, args) == (status, message)


def test_every_function_that_can_fail_has_a_case():
    covered = {c[0] for c in CASES}
    assert covered.isdisjoint(NEVER_REJECT)
    assert covered | NEVER_REJECT == set(_lib.SIGNATURES)


TAIL_BEGIN_1CH = 134448  # dprm's first float of dec_conv5a .. nin_c at cfg (1, 1, 48), as recorded


def test_backward_split_query_answers_without_buffers():
    """all of params, dy, dparams, ws and tail_ready null: DN_OK, tail_begin written, no message"""
    out = ctypes.c_int64(-1)
    args = (G, None, None, None, None, 1, 32, 32, None, 0, 2, None, None, ctypes.byref(out))
    assert _call("dn_unet_backward_split", args) == (0, SENTINEL)
    assert out.value == TAIL_BEGIN_1CH

