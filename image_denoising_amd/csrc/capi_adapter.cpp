// extern "C" boundary (include/denoise_hip.h): the output adapter (adapter.py:5-67,
// finetune.py:153-162) and the memory-bank adapter (finetune_memory.py,
// evaluation_704_iqsl_memory.py): bank selection and gather, the adapter's passes.
#include <string>

#include "capi_common.h"

using namespace dn;

namespace {

dn_status adapter_args(int N, int C, int H, int W, int hidden) {
  if (hidden != 16) return fail(DN_ERR_ARG, "hidden_channels must be 16 (adapter.py default)");
  if (C != 1 && C != 3) return fail(DN_ERR_ARG, "in_channels must be 1 or 3");
  if (N < 1 || H < 1 || W < 1) return fail(DN_ERR_ARG, "empty adapter input");
  return DN_OK;
}

dn_status mem_geom(int n_img, int C, int H, int W, int P, int stride, MemGeom& g) {
  if (C != 1 && C != 3) return fail(DN_ERR_ARG, "bank channels must be 1 or 3");
  if (n_img < 1 || P < 3 || stride < 1 || H < P || W < P)
    return fail(DN_ERR_ARG, "need n_img >= 1, patch_size >= 3, stride >= 1 and H, W >= patch_size");
  g.n_img = n_img; g.C = C; g.H = H; g.W = W; g.P = P; g.s = stride;
  g.ny = (H - P) / stride + 1;
  g.nx = (W - P) / stride + 1;
  g.N = (long)n_img * g.ny * g.nx;
  if (g.N >= (1L << 31) || (long)n_img * C * H * W >= (1L << 40))
    return fail(DN_ERR_ARG, "bank too large (2^31 windows)");
  return DN_OK;
}

dn_status memadapter_args(int N, int C, int H, int W, int hidden, int nb) {
  if (!memadapter_supported(C, hidden, nb))
    return fail(DN_ERR_ARG, "need in_channels 1 or 3, hidden_channels 8 or 16, 0 <= num_fft_bins <= 8");
  if (N < 1 || H < 1 || W < 1) return fail(DN_ERR_ARG, "empty adapter input");
  if ((long)C * H * W < 2)
    return fail(DN_ERR_ARG, "the unbiased std needs at least two elements per sample");
  if (nb > 0 && W / 2 + 1 < nb) return fail(DN_ERR_ARG, "row FFT has fewer bins than num_fft_bins");
  return DN_OK;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
bool ranges_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return q && a < b + qbytes && b < a + bytes;
}

}  // namespace

extern "C" {

// ---- output adapter -------------------------------------------------------------------
dn_status dn_adapter_param_count(int in_channels, int hidden_channels, size_t* count) {
  return guarded([&] {
    if (!count) return fail(DN_ERR_ARG, "null argument");
    if (hidden_channels != 16)
      return fail(DN_ERR_ARG, "hidden_channels must be 16 (adapter.py default)");
    const long n = adapter_param_count(in_channels);
    if (n < 0) return fail(DN_ERR_ARG, "in_channels must be 1 or 3");
    *count = (size_t)n;
    return DN_OK;
  });
}

size_t dn_adapter_slab_size(int N, int C, int H, int W, int hidden_channels) {
  return guarded_query([&]() -> size_t {
    if (hidden_channels != 16 || adapter_param_count(C) < 0 || N < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * (size_t)adapter_bwd_blocks(N, H, W) * (size_t)adapter_param_count(C);
  });
}

dn_status dn_adapter_forward(const float* params, const float* noisy, const float* base_out,
                             float* out, int N, int C, int H, int W, int hidden_channels,
                             void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !out) return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
    return hip_status(launch_adapter_fwd(params, noisy, base_out, N, C, H, W, out,
                                         (hipStream_t)stream),
                      "dn_adapter_forward");
  });
}

dn_status dn_adapter_backward(const float* params, const float* noisy, const float* base_out,
                              const float* dout, float* dparams, int N, int C, int H, int W,
                              int hidden_channels, void* slab, size_t slab_bytes, void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !dout || !dparams || !slab)
      return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
    if (slab_bytes < dn_adapter_slab_size(N, C, H, W, hidden_channels))
      return fail(DN_ERR_WORKSPACE, "slab smaller than dn_adapter_slab_size()");
    return hip_status(launch_adapter_bwd(params, noisy, base_out, dout, N, C, H, W, dparams,
                                         static_cast<float*>(slab), (hipStream_t)stream),
                      "dn_adapter_backward");
  });
}

dn_status dn_adapter_backward_input(const float* params, const float* noisy, const float* base_out,
                                    const float* dout, float* dbase, float* dnoisy, int N, int C,
                                    int H, int W, int hidden_channels, void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !dout || !dbase)
      return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
    // neighbouring tiles read the halo of every input: an output may overwrite none of them
    for (const float* in : {noisy, base_out, dout})
      if (dbase == in || dnoisy == in)
        return fail(DN_ERR_ARG, "dbase / dnoisy must not alias noisy, base_out or dout");
    if (dbase == dnoisy) return fail(DN_ERR_ARG, "dbase and dnoisy must be distinct buffers");
    return hip_status(launch_adapter_dinput(params, noisy, base_out, dout, N, C, H, W, dbase,
                                            dnoisy, (hipStream_t)stream),
                      "dn_adapter_backward_input");
  });
}

// ---- memory bank ------------------------------------------------------------------------
size_t dn_memory_select_ws_size(int B, int n_img, int C, int H, int W, int P, int stride) {
  return guarded_query([&]() -> size_t {
    MemGeom g;
    if (B < 1 || mem_geom(n_img, C, H, W, P, stride, g) != DN_OK) return 0;
    return mem_select_ws_bytes(g, B);
  });
}

dn_status dn_memory_select(const float* queries, const float* noise_images, int B, int n_img, int C,
                           int H, int W, int P, int stride, int64_t* idx, void* ws,
                           size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!queries || !noise_images || !idx || !ws) return fail(DN_ERR_ARG, "null argument");
    if (B < 1) return fail(DN_ERR_ARG, "need B >= 1");
    MemGeom g;
    if (dn_status st = mem_geom(n_img, C, H, W, P, stride, g)) return st;
    if (ws_bytes < mem_select_ws_bytes(g, B))
      return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memory_select_ws_size()");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const OpTimer timer(s, "mem_select", 2.0 * B * (double)g.N * C * P * P, 0, 0, P, P, B);
    return hip_status(launch_mem_select(queries, noise_images, g, B, idx, ws, s),
                      "dn_memory_select");
  });
}

dn_status dn_memory_gather(const float* clean_images, const int64_t* idx, int B, int n_img, int C,
                           int H, int W, int P, int stride, float* out, void* stream) {
  return guarded([&] {
    if (!clean_images || !idx || !out) return fail(DN_ERR_ARG, "null argument");
    if (B < 1) return fail(DN_ERR_ARG, "need B >= 1");
    MemGeom g;
    if (dn_status st = mem_geom(n_img, C, H, W, P, stride, g)) return st;
    return hip_status(launch_mem_gather(clean_images, g, idx, B, out, (hipStream_t)stream),
                      "dn_memory_gather");
  });
}

// ---- memory adapter ---------------------------------------------------------------------
dn_status dn_memadapter_param_count(int in_channels, int hidden_channels, int num_fft_bins,
                                    size_t* count) {
  return guarded([&] {
    if (!count) return fail(DN_ERR_ARG, "null argument");
    const long n = memadapter_param_count(in_channels, hidden_channels, num_fft_bins);
    if (n < 0) return memadapter_args(1, in_channels, 1, 64, hidden_channels, num_fft_bins);
    *count = (size_t)n;
    return DN_OK;
  });
}

size_t dn_memadapter_ws_size(int N, int C, int H, int W, int hidden_channels, int num_fft_bins,
                             int with_backward) {
  return guarded_query([&] {
    return memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins,
                               with_backward == 2 ? 2 : with_backward != 0);
  });
}

dn_status dn_memadapter_forward(const float* params, const float* noisy, const float* base_out,
                                const float* mem_clean, float* out, float* features, int N, int C,
                                int H, int W, int hidden_channels, int num_fft_bins,
                                int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !mem_clean || !out || !features || !ws)
      return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
    if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 0))
      return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memadapter_ws_size()");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const OpTimer timer(s, "memadapter_fwd", 0, 0, 0, H, W, N);
    return hip_status(launch_memadapter_fwd(params, noisy, base_out, mem_clean, out, features, N, C,
                                            H, W, hidden_channels, num_fft_bins, clamp_output != 0,
                                            ws, s),
                      "dn_memadapter_forward");
  });
}

dn_status dn_memadapter_backward(const float* params, const float* noisy, const float* base_out,
                                 const float* features, const float* dout, float* dparams, int N,
                                 int C, int H, int W, int hidden_channels, int num_fft_bins,
                                 int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !features || !dout || !dparams || !ws)
      return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
    if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 1))
      return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memadapter_ws_size()");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const OpTimer timer(s, "memadapter_bwd", 0, 0, 0, H, W, N);
    return hip_status(launch_memadapter_bwd(params, noisy, base_out, features, dout, dparams,
                                            nullptr, N, C, H, W, hidden_channels, num_fft_bins,
                                            clamp_output != 0, ws, s),
                      "dn_memadapter_backward");
  });
}

dn_status dn_memadapter_backward_input(const float* params, const float* noisy,
                                       const float* base_out, const float* features,
                                       const float* dout, float* dparams, float* dbase, int N, int C,
                                       int H, int W, int hidden_channels, int num_fft_bins,
                                       int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!params || !noisy || !base_out || !features || !dout || !dbase || !ws)
      return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
    const size_t px = sizeof(float) * (size_t)N * C * H * W;
    const size_t np =
        sizeof(float) * (size_t)memadapter_param_count(C, hidden_channels, num_fft_bins);
    const size_t nf = sizeof(float) * (size_t)N * (6 + 3 * num_fft_bins);
    if (ranges_overlap(dbase, px, params, np) || ranges_overlap(dbase, px, noisy, px) ||
        ranges_overlap(dbase, px, base_out, px) || ranges_overlap(dbase, px, features, nf) ||
        ranges_overlap(dbase, px, dout, px) || ranges_overlap(dbase, px, dparams, np))
      return fail(DN_ERR_ARG, "dbase must not alias an input or dparams");
    if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 2))
      return fail(DN_ERR_ARG, "workspace smaller than dn_memadapter_ws_size(with_backward = 2)");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const OpTimer timer(s, "memadapter_bwd_input", 0, 0, 0, H, W, N);
    return hip_status(launch_memadapter_bwd(params, noisy, base_out, features, dout, dparams, dbase,
                                            N, C, H, W, hidden_channels, num_fft_bins,
                                            clamp_output != 0, ws, s),
                      "dn_memadapter_backward_input");
  });
}

dn_status dn_memadapter_feature_adjoint(const float* base_out, const float* dfeat, float* hyper,
                                        int N, int C, int H, int W, int num_fft_bins, void* ws,
                                        size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!base_out || !dfeat || !hyper || !ws) return fail(DN_ERR_ARG, "null argument");
    if (dn_status st = memadapter_args(N, C, H, W, 8, num_fft_bins)) return st;
    if (ranges_overlap(hyper, sizeof(float) * (size_t)N * C * H * W, base_out,
                       sizeof(float) * (size_t)N * C * H * W))
      return fail(DN_ERR_ARG, "hyper must not alias base_out");
    if (ws_bytes < memadapter_ws_bytes(N, C, H, W, 8, num_fft_bins, 2))
      return fail(DN_ERR_ARG,
                  "workspace smaller than dn_memadapter_ws_size(hidden 8, with_backward = 2)");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const OpTimer timer(s, "memadapter_feat_adj", 0, 0, 0, H, W, N);
    return hip_status(launch_memadapter_feature_adjoint(base_out, dfeat, hyper, N, C, H, W,
                                                        num_fft_bins, ws, s),
                      "dn_memadapter_feature_adjoint");
  });
}

}  // extern "C"
