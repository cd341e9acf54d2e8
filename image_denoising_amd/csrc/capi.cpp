// extern "C" boundary of libdenoise_hip.so (declared in include/denoise_hip.h).
// Validates arguments, maps failures to dn_status + a thread-local message, never throws.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "iunet.h"
#include "resnet.h"
#include "unet.h"

using namespace dn;

namespace {

dn_status fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

dn_status hip_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return DN_OK;
  return fail(DN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The workspace's size decides a forward's plan: one sized with_backward=1 gets that plan (the
// forward saves what the backward reads); a smaller one, or !bwd_ok, gets the forward-only plan.
template <class P, class Build>
dn_status plan_for_workspace(Build build, const dn_unet_cfg& cfg, int N, int H, int W,
                             size_t ws_bytes, bool bwd_ok, const char* size_fn, P& p) {
  std::string err;
  if (!bwd_ok || !build(cfg, N, H, W, true, p, err) ||
      ws_bytes < (size_t)p.total_floats * sizeof(float))
    if (!build(cfg, N, H, W, false, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE, std::string("workspace smaller than ") + size_fn + "()");
  return DN_OK;
}

#define DN_GUARD_BEGIN try {
#define DN_GUARD_END                                              \
  }                                                               \
  catch (const std::exception& ex) { return fail(DN_ERR_ARG, ex.what()); } \
  catch (...) { return fail(DN_ERR_ARG, "unknown C++ exception"); }

}  // namespace

extern "C" {

#ifndef DN_SRC_HASH
#define DN_SRC_HASH "unknown"
#endif
// src= the sha256 prefix of the sources this library was compiled from (_build.source_hash)
const char* dn_version(void) { return "denoise_hip 0.5.0 gfx950 src=" DN_SRC_HASH; }

int dn_abi_version(void) { return DN_ABI_VERSION; }

int dn_last_error(char* buf, size_t len) {
  const std::string& s = g_last_error;
  if (buf && len) {
    size_t n = s.size() < len - 1 ? s.size() : len - 1;
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int)s.size();
}

dn_status dn_prepare_streams(void* stream) {
  DN_GUARD_BEGIN
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const StreamDeviceGuard device_guard(s);
  SideStream* ss = side_stream(s);
  if (!ss) return fail(DN_ERR_HIP, "creating the backward's side streams failed");
  // one marker on each (its first submission binds it to a hardware queue), ordered after the
  // caller's stream and joined back into it
  if (hipEventRecord(ss->fork, s) != hipSuccess ||
      hipStreamWaitEvent(ss->st, ss->fork, 0) != hipSuccess ||
      hipStreamWaitEvent(ss->rst, ss->fork, 0) != hipSuccess ||
      hipEventRecord(ss->join, ss->st) != hipSuccess ||
      hipEventRecord(ss->rjoin, ss->rst) != hipSuccess ||
      hipStreamWaitEvent(s, ss->join, 0) != hipSuccess ||
      hipStreamWaitEvent(s, ss->rjoin, 0) != hipSuccess)
    return fail(DN_ERR_HIP, "marker on the backward's side streams failed");
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_unet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  DN_GUARD_BEGIN
  if (!cfg || !count) return fail(DN_ERR_ARG, "null argument");
  ParamLayout P;
  std::string err;
  if (!build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
  *count = (size_t)P.total;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_unet_param_info(const dn_unet_cfg* cfg, int index, size_t* w_off, size_t* w_count,
                             size_t* b_count) {
  DN_GUARD_BEGIN
  if (!cfg || !w_off || !w_count || !b_count) return fail(DN_ERR_ARG, "null argument");
  ParamLayout P;
  std::string err;
  if (!build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
  if (index < 0 || index >= NL) return fail(DN_ERR_ARG, "layer index out of range");
  *w_off = (size_t)P.L[index].woff;
  *w_count = (size_t)P.L[index].wcount;
  *b_count = (size_t)P.L[index].cout;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_unet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                 size_t* bytes) {
  DN_GUARD_BEGIN
  if (!cfg || !bytes) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  *bytes = (size_t)p.total_floats * sizeof(float);
  return DN_OK;
  DN_GUARD_END
}

// the plan a UNet forward entry point runs on this workspace (bf16: the forward-only plan)
static dn_status forward_plan(const dn_unet_cfg* cfg, int N, int H, int W, size_t ws_bytes,
                              int precision, Plan& p) {
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6 && precision != DN_PREC_BF16)
    return fail(DN_ERR_ARG, "unknown precision");
  const bool bwd_ok = precision != DN_PREC_BF16;
  const dn_status st = plan_for_workspace(build_plan, *cfg, N, H, W, ws_bytes, bwd_ok,
                                          "dn_unet_workspace_size", p);
  if (st == DN_OK && !bwd_ok) p.with_bwd = false;
  return st;
}

dn_status dn_unet_forward(const dn_unet_cfg* cfg, const float* params, const float* x, float* y,
                          int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
  return dn_unet_forward_prec(cfg, params, x, y, N, H, W, ws, ws_bytes, DN_PREC_FP32, stream);
}

dn_status dn_unet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                               float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                               int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision == DN_PREC_BF16)
    return dn_unet_forward_bf16(cfg, params, x, y, N, H, W, ws, ws_bytes, stream);
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "unknown precision");
  if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  // (with-backward plan: dense concat strides; forward-only: strides padded to 128-B lines)
  if (dn_status st = forward_plan(cfg, N, H, W, ws_bytes, precision, p)) return st;
  return unet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision);
  DN_GUARD_END
}

dn_status dn_unet_pack_weights(const dn_unet_cfg* cfg, const float* params, int N, int H, int W,
                               void* ws, size_t ws_bytes, int precision, void* stream) {
  DN_GUARD_BEGIN
  if (!cfg || !params || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  const dn_status st = forward_plan(cfg, N, H, W, ws_bytes, precision, p);
  if (st != DN_OK) return st;
  return unet_forward(p, params, nullptr, nullptr, static_cast<float*>(ws), (hipStream_t)stream,
                      precision, nullptr, PACK_ONLY);
  DN_GUARD_END
}

dn_status dn_unet_forward_prepacked(const dn_unet_cfg* cfg, const float* params, const float* x,
                                    float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                    int precision, void* stream) {
  DN_GUARD_BEGIN
  if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  const dn_status st = forward_plan(cfg, N, H, W, ws_bytes, precision, p);
  if (st != DN_OK) return st;
  return unet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision,
                      nullptr, RUN_ONLY);
  DN_GUARD_END
}

dn_status dn_unet_forward_n2n(const dn_unet_cfg* cfg, const float* params, const float* x,
                              float* den, const uint8_t* rd_idx, int N, int H, int W, void* ws,
                              size_t ws_bytes, int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !x || !den || !rd_idx || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, false, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_unet_workspace_size()");
  p.with_bwd = false;  // no-grad pass: nothing is saved
  return unet_forward(p, params, x, den, static_cast<float*>(ws), (hipStream_t)stream, precision,
                      rd_idx);
  DN_GUARD_END
}

dn_status dn_unet_forward_bf16(const dn_unet_cfg* cfg, const float* params, const float* x,
                               float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                               void* stream) {
  DN_GUARD_BEGIN
  if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, false, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_unet_workspace_size()");
  p.with_bwd = false;  // inference only: nothing is saved for a backward
  return unet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream,
                      DN_PREC_BF16);
  DN_GUARD_END
}

dn_status dn_unet_backward(const dn_unet_cfg* cfg, const float* params, const float* dy,
                           float* dparams, float* dx, int N, int H, int W, void* ws,
                           size_t ws_bytes, void* stream) {
  return dn_unet_backward_prec(cfg, params, dy, dparams, dx, N, H, W, ws, ws_bytes, DN_PREC_FP32,
                               stream);
}

dn_status dn_unet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                float* dparams, float* dx, int N, int H, int W, void* ws,
                                size_t ws_bytes, int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "backward precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !dy || !dparams || !ws) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, true, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE,
                "workspace smaller than dn_unet_workspace_size(with_backward=1)");
  return unet_backward(p, params, dy, dparams, dx, static_cast<float*>(ws), (hipStream_t)stream,
                       precision);
  DN_GUARD_END
}

dn_status dn_unet_backward_split(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                 float* dparams, float* dx, int N, int H, int W, void* ws,
                                 size_t ws_bytes, int precision, void* stream, void* tail_ready,
                                 int64_t* tail_begin_out) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "backward precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, true, p, err)) return fail(DN_ERR_ARG, err);
  if (tail_begin_out) *tail_begin_out = tail_begin(p);
  if (!params || !dy || !dparams || !ws) {
    if (!params && !dy && !dparams && !ws && !tail_ready) return DN_OK;  // a tail_begin query
    return fail(DN_ERR_ARG, "null argument");
  }
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE,
                "workspace smaller than dn_unet_workspace_size(with_backward=1)");
  return unet_backward(p, params, dy, dparams, dx, static_cast<float*>(ws), (hipStream_t)stream,
                       precision, static_cast<hipEvent_t>(tail_ready));
  DN_GUARD_END
}

dn_status dn_unet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                int64_t* desc, int max_entries, int* n_entries) {
  DN_GUARD_BEGIN
  if (!cfg || !desc || !n_entries) return fail(DN_ERR_ARG, "null argument");
  Plan p;
  std::string err;
  if (!build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  int n = 0;
  auto add = [&](long off, int stride, int level) {
    if (n < max_entries) {
      desc[3 * n] = off;
      desc[3 * n + 1] = stride;
      desc[3 * n + 2] = level;
    }
    ++n;
  };
  const int nf = p.nf;
  add(p.c1, p.c1s, 0); add(p.a0, nf, 0); add(p.a1, nf, 0);
  for (int l = 1; l <= 4; ++l) add(p.c[l], p.cs[l], l);
  for (int l = 1; l <= 4; ++l) add(p.a[l], nf, l);
  add(p.p5, nf, 5); add(p.a6, nf, 5);
  for (int l = 1; l <= 4; ++l) add(p.da[l], 2 * nf, l);
  for (int l = 1; l <= 4; ++l) add(p.db[l], 2 * nf, l);
  add(p.d1a, 96, 0); add(p.d1b, 96, 0); add(p.na, 96, 0); add(p.nb, 96, 0);
  if (with_backward) {
    add(p.g_nb, 96, 0); add(p.g_na, 96, 0); add(p.g_d1b, 96, 0); add(p.g_d1a, 96, 0);
    add(p.g_c1, 2 * nf, 0);
    for (int l = 1; l <= 4; ++l) add(p.g_c[l], p.cs[l], l);
    for (int l = 1; l <= 4; ++l) add(p.g_da[l], 2 * nf, l);
    for (int l = 1; l <= 4; ++l) add(p.g_db[l], 2 * nf, l);
    for (int l = 1; l <= 4; ++l) add(p.g_a[l], nf, l);
    add(p.g_a6, nf, 5); add(p.g_p5, nf, 5); add(p.g_a0, nf, 0); add(p.g_a1, nf, 0);
  }
  *n_entries = n;
  return DN_OK;
  DN_GUARD_END
}

// ---- RESNET -------------------------------------------------------------------------
dn_status dn_resnet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  DN_GUARD_BEGIN
  if (!cfg || !count) return fail(DN_ERR_ARG, "null argument");
  ResParamLayout P;
  std::string err;
  if (!res_build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
  *count = (size_t)P.total;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_resnet_param_info(const dn_unet_cfg* cfg, int index, size_t* w_off, size_t* w_count,
                               size_t* b_count) {
  DN_GUARD_BEGIN
  if (!cfg || !w_off || !w_count || !b_count) return fail(DN_ERR_ARG, "null argument");
  ResParamLayout P;
  std::string err;
  if (!res_build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
  if (index < 0 || index >= R_NL) return fail(DN_ERR_ARG, "layer index out of range");
  *w_off = (size_t)P.L[index].woff;
  *w_count = (size_t)P.L[index].wcount;
  *b_count = (size_t)P.L[index].cout;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_resnet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                   size_t* bytes) {
  DN_GUARD_BEGIN
  if (!cfg || !bytes) return fail(DN_ERR_ARG, "null argument");
  ResPlan p;
  std::string err;
  if (!res_build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  *bytes = (size_t)p.total_floats * sizeof(float);
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_resnet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                                 float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                 int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "RESNET precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
  ResPlan p;
  if (dn_status st = plan_for_workspace(res_build_plan, *cfg, N, H, W, ws_bytes, true,
                                        "dn_resnet_workspace_size", p))
    return st;
  return resnet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision);
  DN_GUARD_END
}

dn_status dn_resnet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                  float* dparams, float* dx, int N, int H, int W, void* ws,
                                  size_t ws_bytes, int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "RESNET precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !dy || !dparams || !ws) return fail(DN_ERR_ARG, "null argument");
  ResPlan p;
  std::string err;
  if (!res_build_plan(*cfg, N, H, W, true, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE,
                "workspace smaller than dn_resnet_workspace_size(with_backward=1)");
  return resnet_backward(p, params, dy, dparams, dx, static_cast<float*>(ws), (hipStream_t)stream,
                         precision);
  DN_GUARD_END
}

/* order: c1 a0 c2 c3 c4 c5 a5 d2a d3a d4a d5a d1a d1b | na nb g_na g_d1b g_d1a g_c1 g_c2..g_c5
   g_d2a..g_d5a g_a1..g_a4 g_a5 g_a0 */
dn_status dn_resnet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                  int64_t* desc, int max_entries, int* n_entries) {
  DN_GUARD_BEGIN
  if (!cfg || !desc || !n_entries) return fail(DN_ERR_ARG, "null argument");
  ResPlan p;
  std::string err;
  if (!res_build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  int n = 0;
  auto add = [&](long off, int stride) {
    if (n < max_entries) {
      desc[3 * n] = off;
      desc[3 * n + 1] = stride;
      desc[3 * n + 2] = 0;
    }
    ++n;
  };
  const int nf = p.nf;
  add(p.c1, p.c1s); add(p.a0, nf);
  for (int k = 2; k <= 5; ++k) add(p.c[k], p.cs[k]);
  add(p.a5, nf);
  for (int k = 2; k <= 5; ++k) add(p.da[k], 2 * nf);
  add(p.d1a, 96); add(p.d1b, 96);
  if (with_backward) {
    add(p.na, 96); add(p.nb, 96);
    add(p.g_na, 96); add(p.g_d1b, 96); add(p.g_d1a, 96); add(p.g_c1, 2 * nf);
    for (int k = 2; k <= 5; ++k) add(p.g_c[k], p.cs[k]);
    for (int k = 2; k <= 5; ++k) add(p.g_da[k], 2 * nf);
    for (int j = 1; j <= 4; ++j) add(p.g_a[j], nf);
    add(p.g_a5, nf); add(p.g_a0, nf);
  }
  *n_entries = n;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_n2n_subsample(const float* img, int N, int C, int H, int W, const uint8_t* rd_idx_in,
                           uint64_t seed, uint64_t offset, uint64_t cell_base, float* sub1,
                           float* sub2, uint8_t* rd_idx_out, void* stream) {
  if (N < 0 || C < 1 || H < 0 || W < 0 || (H & 1) || (W & 1))
    return fail(DN_ERR_ARG, "H and W must be even");
  if ((long)N * H * W == 0) return DN_OK;
  if (!img || !sub1 || !sub2) return fail(DN_ERR_ARG, "null argument");
  const OpTimer timer((hipStream_t)stream, "subsample", 0, C, C, H, W, N);
  return hip_status(launch_subsample(img, N, C, H, W, rd_idx_in, seed, offset, cell_base, sub1,
                                     sub2, rd_idx_out, (hipStream_t)stream),
                    "dn_n2n_subsample");
}

dn_status dn_n2n_masks(const uint8_t* rd_idx, int64_t ncells, uint8_t* mask1, uint8_t* mask2,
                       void* stream) {
  if (ncells < 0) return fail(DN_ERR_ARG, "ncells < 0");
  if (ncells == 0) return DN_OK;
  if (!rd_idx || !mask1 || !mask2) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_masks(rd_idx, ncells, mask1, mask2, (hipStream_t)stream),
                    "dn_n2n_masks");
}

dn_status dn_n2n_subimage_from_mask(const float* img, int N, int C, int H, int W,
                                    const uint8_t* mask, float* sub, void* stream) {
  if (N < 0 || C < 1 || (H & 1) || (W & 1)) return fail(DN_ERR_ARG, "H and W must be even");
  if ((long)N * H * W == 0) return DN_OK;
  if (!img || !mask || !sub) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_subimage_from_mask(img, N, C, H, W, mask, sub, (hipStream_t)stream),
                    "dn_n2n_subimage_from_mask");
}

dn_status dn_add_gauss_noise(const float* clean, int N, int64_t per_image, float std_,
                             const float* std_per_image, uint64_t seed, uint64_t offset,
                             uint64_t elem_base, float* noisy, void* stream) {
  if (N < 0 || per_image < 0) return fail(DN_ERR_ARG, "negative size");
  if ((long)N * per_image == 0) return DN_OK;
  if (!clean || !noisy) return fail(DN_ERR_ARG, "null argument");
  const OpTimer timer((hipStream_t)stream, "noise", 0);
  return hip_status(launch_noise(clean, N, per_image, std_, std_per_image, seed, offset, elem_base,
                                 noisy, (hipStream_t)stream),
                    "dn_add_gauss_noise");
}

dn_status dn_add_poisson_noise(const float* clean, int N, int64_t per_image, float lam,
                               const float* lam_per_image, uint64_t seed, uint64_t offset,
                               uint64_t elem_base, float* noisy, void* stream) {
  if (N < 0 || per_image < 0) return fail(DN_ERR_ARG, "negative size");
  if (!lam_per_image && !(lam > 0.f && lam <= 500.f)) return fail(DN_ERR_ARG, "lam must be in (0, 500]");
  if ((long)N * per_image == 0) return DN_OK;
  if (!clean || !noisy) return fail(DN_ERR_ARG, "null argument");
  const OpTimer timer((hipStream_t)stream, "noise", 0);
  return hip_status(launch_poisson(clean, N, per_image, lam, lam_per_image, seed, offset, elem_base,
                                   noisy, (hipStream_t)stream),
                    "dn_add_poisson_noise");
}

size_t dn_loss_partials_size(void) { return loss_partials_bytes(); }

dn_status dn_n2n_loss(const float* out, const float* sub2, const float* den, const uint8_t* rd_idx,
                      int N, int C, int h, int w, float lambda, float* dout, float* loss3,
                      void* partial_ws, void* stream) {
  if (!out || !sub2 || !den || !rd_idx || !dout || !loss3 || !partial_ws)
    return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || C < 1 || h < 1 || w < 1) return fail(DN_ERR_ARG, "empty loss input");
  const OpTimer timer((hipStream_t)stream, "loss", 0);
  return hip_status(launch_n2n_loss(out, sub2, den, rd_idx, N, C, h, w, lambda, dout, loss3,
                                    partial_ws, (hipStream_t)stream),
                    "dn_n2n_loss");
}

dn_status dn_structure_loss(const float* pred, const float* pred2, const float* target, int N, int C,
                            int H, int W, float alpha, float beta, float gamma, float* dpred,
                            float* dpred2, float* loss5, void* partial_ws, void* stream) {
  if (!pred || !pred2 || !target || !dpred || !dpred2 || !loss5 || !partial_ws)
    return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || C < 1 || H < 2 || W < 2) return fail(DN_ERR_ARG, "Structure_loss needs H, W >= 2");
  const OpTimer timer((hipStream_t)stream, "loss", 0);
  return hip_status(launch_structure_loss(pred, pred2, target, N, C, H, W, alpha, beta, gamma,
                                          dpred, dpred2, loss5, partial_ws, (hipStream_t)stream),
                    "dn_structure_loss");
}

size_t dn_l1fft_ws_size(int N, int C, int H, int W) { return l1fft_ws_bytes(N, C, H, W); }

dn_status dn_l1fft_loss(const float* pred, const float* target, int N, int C, int H, int W,
                        float alpha, float beta, int reduction_sum, float* dpred, float* loss3,
                        void* ws, size_t ws_bytes, void* stream) {
  const size_t need = l1fft_ws_bytes(N, C, H, W);
  if (!need)
    return fail(DN_ERR_ARG, "L1FFT needs N, C >= 1 and H, W = m * 2^k with m odd <= 31, k >= 3, at most 1024");
  if (!pred || !target || !dpred || !loss3 || !ws) return fail(DN_ERR_ARG, "null argument");
  if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(DN_ERR_ARG, "workspace must be 16-byte aligned");
  if (ws_bytes < need) return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_l1fft_ws_size()");
  const OpTimer timer((hipStream_t)stream, "loss", 0);
  return hip_status(launch_l1fft_loss(pred, target, N, C, H, W, alpha, beta, reduction_sum != 0,
                                      dpred, loss3, ws, (hipStream_t)stream),
                    "dn_l1fft_loss");
}

// The double a caller wrote before the ABI narrowed it to fp32: the shortest decimal that rounds
// to x.  torch.optim.Adam keeps lr and the betas as Python doubles and forms 1 - beta, beta^step
// and lr / bc1 from those.  (double)0.999f is 0.99900001287..., and 1 - beta2 formed from it is
// 1.3e-5 (relative) away from torch's, and exp_avg_sq with it.
static double as_written(float x) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    std::snprintf(buf, sizeof buf, "%.*g", prec, (double)x);
    const double d = std::strtod(buf, nullptr);
    if ((float)d == x) return d;
  }
  return (double)x;
}

dn_status dn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, int64_t step,
                       float grad_scale, void* stream) {
  if (n < 0 || step < 1) return fail(DN_ERR_ARG, "n >= 0 and step >= 1 required");
  if (n == 0) return DN_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(DN_ERR_ARG, "null argument");
  // scalars exactly as torch/optim/adam.py _single_tensor_adam computes them (python floats)
  const double b1 = as_written(beta1), b2 = as_written(beta2);
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  const double step_size = as_written(lr) / bc1;
  const double bc2s = std::sqrt(bc2);
  const OpTimer timer((hipStream_t)stream, "adam", 0);
  return hip_status(launch_adam(param, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - b1), beta2,
                                (float)(1.0 - b2), (float)step_size, (float)bc2s, eps, grad_scale,
                                (hipStream_t)stream),
                    "dn_adam_step");
}

size_t dn_guard_state_size(void) { return guard_state_bytes(); }

static bool guard_state_ok(const void* state) {
  return state && (reinterpret_cast<uintptr_t>(state) & 15) == 0;
}

dn_status dn_guard_state_init(void* state, int64_t step, void* stream) {
  if (!guard_state_ok(state)) return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
  if (step < 0) return fail(DN_ERR_ARG, "step >= 0 required");
  return hip_status(launch_guard_init(state, step, (hipStream_t)stream), "dn_guard_state_init");
}

dn_status dn_grad_norm(const float* grad, int64_t n, float grad_scale, void* state,
                       double* norm_out, void* stream) {
  if (n < 0) return fail(DN_ERR_ARG, "n < 0");
  if (n == 0) return DN_OK;
  if (!grad) return fail(DN_ERR_ARG, "null argument");
  if (!guard_state_ok(state)) return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
  const OpTimer timer((hipStream_t)stream, "grad_norm", 0);
  return hip_status(launch_grad_norm(grad, n, grad_scale, state, norm_out, (hipStream_t)stream),
                    "dn_grad_norm");
}

dn_status dn_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                               int64_t n, float lr, float beta1, float beta2, float eps,
                               float grad_scale, const float* loss, float max_loss,
                               float max_norm_skip, float clip, void* state, void* stream) {
  if (n < 0) return fail(DN_ERR_ARG, "n < 0");
  if (n == 0) return DN_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(DN_ERR_ARG, "null argument");
  if (!guard_state_ok(state)) return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
  // the doubles torch forms from its Python floats, as dn_adam_step; the step-dependent scalars
  // are formed from them on the device, where the step count lives
  const double b1 = as_written(beta1), b2 = as_written(beta2);
  const auto on = [](float x) { return x > 0.f ? x : 0.f; };  // <= 0 and NaN: the guard is off
  const OpTimer timer((hipStream_t)stream, "adam_guarded", 0);
  return hip_status(launch_adam_guarded(param, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - b1),
                                        beta2, (float)(1.0 - b2), eps, grad_scale, as_written(lr),
                                        b1, b2, loss, on(max_loss), on(max_norm_skip), on(clip),
                                        state, (hipStream_t)stream),
                    "dn_adam_step_guarded");
}

dn_status dn_guard_state_read(const void* state, dn_guard_stats* out, void* stream) {
  if (!guard_state_ok(state) || !out) return fail(DN_ERR_ARG, "null argument or unaligned guard state");
  return hip_status(guard_state_read(state, out, (hipStream_t)stream), "dn_guard_state_read");
}

dn_status dn_accumulate(float* dst, const float* src, int64_t n, void* stream) {
  if (n < 0) return fail(DN_ERR_ARG, "n < 0");
  if (n == 0) return DN_OK;
  if (!dst || !src) return fail(DN_ERR_ARG, "null argument");
  const OpTimer timer((hipStream_t)stream, "accumulate", 0);
  return hip_status(launch_accumulate(dst, src, n, (hipStream_t)stream), "dn_accumulate");
}

// ---- evaluation path ----------------------------------------------------------------------
size_t dn_eval_partials_size(void) { return EVAL_PARTS * sizeof(double); }

dn_status dn_u8_to_unit(const uint8_t* x, int64_t n, float* y, void* stream) {
  if (n < 0) return fail(DN_ERR_ARG, "n < 0");
  if (n == 0) return DN_OK;
  if (!x || !y) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_u8_to_unit(x, n, y, (hipStream_t)stream), "dn_u8_to_unit");
}

int dn_tile_count(int extent, int patch, int stride) {
  if (extent < 1 || patch < 1 || stride < 1) return 0;
  return (extent + stride - 1) / stride;  // range(0, extent, stride)
}

static bool tile_args_ok(int C, int H, int W, int patch, int stride) {
  return C >= 1 && H >= 1 && W >= 1 && patch >= 1 && stride >= 1 && stride <= patch;
}

dn_status dn_tile_extract(const uint8_t* img, int C, int H, int W, int patch, int stride,
                          float* tiles, void* stream) {
  if (!img || !tiles) return fail(DN_ERR_ARG, "null argument");
  if (!tile_args_ok(C, H, W, patch, stride))
    return fail(DN_ERR_ARG, "need C,H,W,patch >= 1 and 1 <= stride <= patch");
  return hip_status(launch_tile_extract(img, C, H, W, patch, stride, dn_tile_count(H, patch, stride),
                                        dn_tile_count(W, patch, stride), tiles, (hipStream_t)stream),
                    "dn_tile_extract");
}

dn_status dn_tile_blend(const float* pred, int C, int H, int W, int patch, int stride,
                        const float* wmask, float* out, uint8_t* out_u8, void* stream) {
  if (!pred || !wmask || (!out && !out_u8)) return fail(DN_ERR_ARG, "null argument");
  if (!tile_args_ok(C, H, W, patch, stride))
    return fail(DN_ERR_ARG, "need C,H,W,patch >= 1 and 1 <= stride <= patch");
  return hip_status(launch_tile_blend(pred, C, H, W, patch, stride, dn_tile_count(H, patch, stride),
                                      dn_tile_count(W, patch, stride), wmask, out, out_u8,
                                      (hipStream_t)stream),
                    "dn_tile_blend");
}

dn_status dn_quantize_u8(const float* x, int64_t n, int plus_half, uint8_t* y, void* stream) {
  if (n < 0) return fail(DN_ERR_ARG, "n < 0");
  if (n == 0) return DN_OK;
  if (!x || !y) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_quantize_u8(x, n, plus_half, y, (hipStream_t)stream), "dn_quantize_u8");
}

dn_status dn_psnr_u8(const uint8_t* a, const uint8_t* b, int64_t n, void* part, double* psnr,
                     void* stream) {
  if (n < 1) return fail(DN_ERR_ARG, "n >= 1 required");
  if (!a || !b || !part || !psnr) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_psnr(a, b, n, static_cast<double*>(part), psnr, (hipStream_t)stream),
                    "dn_psnr_u8");
}

dn_status dn_ssim_u8(const uint8_t* a, const uint8_t* b, int C, int H, int W, int hwc, void* part,
                     double* ssim, void* stream) {
  if (C < 1 || H <= 10 || W <= 10) return fail(DN_ERR_ARG, "need C >= 1 and H, W > 10");
  if (!a || !b || !part || !ssim) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_ssim(a, b, C, H, W, hwc, static_cast<double*>(part), ssim,
                                (hipStream_t)stream),
                    "dn_ssim_u8");
}

dn_status dn_l1_mean(const float* a, const float* b, int64_t n, void* part, double* l1,
                     void* stream) {
  if (n < 1) return fail(DN_ERR_ARG, "n >= 1 required");
  if (!a || !b || !part || !l1) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_l1(a, b, n, static_cast<double*>(part), l1, (hipStream_t)stream),
                    "dn_l1_mean");
}

dn_status dn_l1_mean_batched(const float* a, const float* b, int64_t P, int64_t n, double* l1,
                             void* stream) {
  if (P < 0 || n < 1) return fail(DN_ERR_ARG, "P >= 0 and n >= 1 required");
  if (P == 0) return DN_OK;
  if (P > 0x7fffffffL) return fail(DN_ERR_ARG, "P too large");
  if (!a || !b || !l1) return fail(DN_ERR_ARG, "null argument");
  return hip_status(launch_l1_batched(a, b, P, n, l1, (hipStream_t)stream), "dn_l1_mean_batched");
}

// ---- op-level entry points ------------------------------------------------------------
size_t dn_conv2d_pack_size(int Cin, int Cout, int ksize, int backward_data) {
  if ((ksize != 1 && ksize != 3) || Cin < 1 || Cout < 1) return 0;
  const long n = backward_data ? conv_dgrad_pack_size(Cout, Cin, ksize)
                               : conv_fwd_pack_size(Cin, Cout, ksize);
  return n < 0 ? 0 : sizeof(float) * (size_t)n;
}

size_t dn_deconv2x2_pack_size(int Cin, int Cout, int backward_data) {
  if (Cin < 1 || Cout < 1) return 0;
  const long n = backward_data ? deconv_dgrad_pack_size(Cout, Cin) : deconv_fwd_pack_size(Cin, Cout);
  return n < 0 ? 0 : sizeof(float) * (size_t)n;
}

static dn_status need_pack(void* ws, size_t have, size_t need) {
  if (need == 0) return fail(DN_ERR_ARG, "unsupported channel count for this kernel build");
  if (!ws || have < need) return fail(DN_ERR_WORKSPACE, "pack scratch smaller than *_pack_size()");
  return DN_OK;
}

dn_status dn_conv2d_forward(const float* x, int x_stride, int N, int H, int W, int Cin,
                            const float* w, const float* b, int Cout, int ksize, int act, float* y,
                            int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
  if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || x_stride < Cin || y_stride < Cout)
    return fail(DN_ERR_ARG, "bad shape");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_pack_size(Cin, Cout, ksize, 0))) return st;
  hipStream_t s = (hipStream_t)stream;
  float* wp = static_cast<float*>(pack_ws);
  hipError_t e = pack_conv_fwd(w, Cin, Cout, ksize, wp, s);
  if (e == hipSuccess)
    e = conv_forward(View{const_cast<float*>(x), x_stride, 0}, N, H, W, Cin, wp, b, Cout, ksize,
                     act, View{y, y_stride, 0}, OUT_NHWC, s);
  return hip_status(e, "dn_conv2d_forward");
}

size_t dn_conv2d_bf16_pack_size(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  const long e = bf16_pack_elems(Cin, Cout);
  return e < 0 ? 0 : 2 * (size_t)e;
}

dn_status dn_conv2d_forward_bf16(const float* x, int x_stride, int N, int H, int W, int Cin,
                                 const float* w, const float* b, int Cout, int act, float* y,
                                 int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || x_stride < Cin || y_stride < Cout || (Cout & 3) ||
      (y_stride & 3))
    return fail(DN_ERR_ARG, "bad shape (Cout and y_stride must be multiples of 4)");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_bf16_pack_size(Cin, Cout))) return st;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = launch_pack_bf16(conv_fwd_view(w, Cin, 3), Cin, Cout, pack_ws, s);
  if (e == hipSuccess) {
    FwdArgs a = fwd_args(View{const_cast<float*>(x), x_stride, 0}, N, H, W, Cin, Cout,
                         View{y, y_stride, 0}, OUT_NHWC);
    a.wp = static_cast<const float*>(pack_ws); a.bias = b; a.epi = act ? EPI_BIAS_ACT : EPI_BIAS;
    e = launch_fwd_bf16(a, s);
  }
  return hip_status(e, "dn_conv2d_forward_bf16");
}

size_t dn_conv2d_x6_pack_size(int Cin, int Cout, int backward_data) {
  if (Cin < 1 || Cout < 1) return 0;
  const long e = backward_data ? x6_pack_elems(Cout, Cin, x6_dgrad_zc(Cin))
                               : x6_pack_elems(Cin, Cout, 0);
  return e < 0 ? 0 : 2 * (size_t)e;
}

dn_status dn_conv2d_forward_x6(const float* x, int x_stride, int N, int H, int W, int Cin,
                               const float* w, const float* b, int Cout, int act, float* y,
                               int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || x_stride < Cin || y_stride < Cout)
    return fail(DN_ERR_ARG, "bad shape");
  const size_t need = dn_conv2d_x6_pack_size(Cin, Cout, 0);
  if (need == 0) return fail(DN_ERR_ARG, "bf16x6 forward supports Cout <= 96");
  if (dn_status st = need_pack(pack_ws, pack_bytes, need)) return st;
  hipStream_t s = (hipStream_t)stream;
  // large grids with a partial last 32-channel chunk: the pipelined kernel's tail packing
  const int tail = x6_image_mode(N, H, W, Cin, Cout, 0,
                                 x_stride % 4 == 0 && Cin % 4 == 0 && y_stride % 4 == 0);
  hipError_t e = launch_pack_x6(conv_fwd_view(w, Cin, 3), Cin, Cout, 0, pack_ws, s, tail);
  if (e == hipSuccess) {
    FwdArgs a = fwd_args(View{const_cast<float*>(x), x_stride, 0}, N, H, W, Cin, Cout,
                         View{y, y_stride, 0}, OUT_NHWC);
    a.x6_tail = tail;
    a.wp = static_cast<const float*>(pack_ws); a.bias = b; a.epi = act ? EPI_BIAS_ACT : EPI_BIAS;
    // (dn_profile_ops: the record brackets the GEMM launch alone, so its label is the GEMM's)
    const OpTimer timer(s, "fwd3", 2.0 * Cin * Cout * 9 * N * H * W, Cin, Cout, H, W, N);
    e = launch_fwd_x6(a, s);
  }
  return hip_status(e, "dn_conv2d_forward_x6");
}

size_t dn_upconv3_x6_pack_size(void) { return (size_t)UPC_BYTES; }

dn_status dn_upconv3_forward_x6(const float* xlo, int xlo_stride, int N, int h, int w,
                                const float* img, int C, const float* w3, const float* b3,
                                const float* wd, const float* bd, float* y, int y_stride,
                                void* pack_ws, size_t pack_bytes, void* stream) {
  if (!xlo || !img || !w3 || !b3 || !wd || !bd || !y) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || h < 1 || w < 1 || C < 1 || C > 4 || xlo_stride < 96 || y_stride < 96 ||
      ((xlo_stride | y_stride) & 3))
    return fail(DN_ERR_ARG, "bad shape (1 <= C <= 4, strides >= 96 and multiples of 4)");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_upconv3_x6_pack_size())) return st;
  hipStream_t s = (hipStream_t)stream;
  PackBatch pb;
  pb.j[pb.n++] = pack_job_upconv_x6(w3, b3, wd, bd, C, pack_ws);
  hipError_t e = pack_flush(pb, s);
  if (e == hipSuccess) {
    FwdArgs a = fwd_args(View{const_cast<float*>(xlo), xlo_stride, 0}, h, w, N, 2 * h, 2 * w, 96 + C,
                         96, View{y, y_stride, 0}, OUT_NHWC);
    a.wp = static_cast<const float*>(pack_ws); a.in_t1 = img; a.epi = EPI_BIAS_ACT;
    const OpTimer timer(s, "fwd3", 2.0 * (96 + C) * 96 * 9 * N * 4 * h * w, 96 + C, 96, 2 * h, 2 * w, N);
    e = launch_upconv3_x6(a, s);
  }
  return hip_status(e, "dn_upconv3_forward_x6");
}

dn_status dn_conv2d_backward_data_x6(const float* dz, int N, int H, int W, int Cout,
                                     const float* w, int Cin, const float* mask, int mask_stride,
                                     int accumulate, float* dx, int dx_stride, void* pack_ws,
                                     size_t pack_bytes, void* stream) {
  if (!dz || !w || !dx) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || Cout < 1 || dx_stride < Cin) return fail(DN_ERR_ARG, "bad shape");
  if (mask && accumulate) return fail(DN_ERR_ARG, "mask and accumulate are exclusive");
  const size_t need = dn_conv2d_x6_pack_size(Cin, Cout, 1);
  if (need == 0) return fail(DN_ERR_ARG, "bf16x6 data gradient: unsupported Cin");
  if (dn_status st = need_pack(pack_ws, pack_bytes, need)) return st;
  hipStream_t s = (hipStream_t)stream;
  const int zc = x6_dgrad_zc(Cin);
  const int tail = x6_image_mode(N, H, W, Cout, Cin, zc,
                                 Cout % 4 == 0 && dx_stride % 4 == 0 && (!mask || mask_stride % 4 == 0));
  hipError_t e = launch_pack_x6(conv_dgrad_view(w, Cin, 3), Cout, Cin, zc, pack_ws, s, tail);
  if (e == hipSuccess) {
    FwdArgs a = fwd_args(View{const_cast<float*>(dz), Cout, 0}, N, H, W, Cout, Cin,
                         View{dx, dx_stride, 0}, OUT_NHWC);
    a.x6_tail = tail;
    a.zc = zc;
    a.wp = static_cast<const float*>(pack_ws);
    a.wp_z = x6_wp_z(Cout, Cin, zc);
    a.epi = mask ? EPI_MASK : (accumulate ? EPI_ACCUM : EPI_PLAIN);
    set_mask(a, View{const_cast<float*>(mask), mask_stride, 0});
    const OpTimer timer(s, "dgrad3", 2.0 * Cout * Cin * 9 * N * H * W, Cout, Cin, H, W, N);
    e = launch_fwd_x6(a, s);
  }
  return hip_status(e, "dn_conv2d_backward_data_x6");
}

dn_status dn_conv2d_backward_data(const float* dz, int N, int H, int W, int Cout, const float* w,
                                  int Cin, int ksize, const float* mask, int mask_stride,
                                  int accumulate, float* dx, int dx_stride, void* pack_ws,
                                  size_t pack_bytes, void* stream) {
  if (!dz || !w || !dx) return fail(DN_ERR_ARG, "null argument");
  if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
  if (N < 1 || H < 1 || W < 1 || Cout < 1 || dx_stride < Cin) return fail(DN_ERR_ARG, "bad shape");
  if (mask && accumulate) return fail(DN_ERR_ARG, "mask and accumulate are exclusive");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_pack_size(Cin, Cout, ksize, 1))) return st;
  const int epi = mask ? EPI_MASK : (accumulate ? EPI_ACCUM : EPI_PLAIN);
  hipStream_t s = (hipStream_t)stream;
  float* wp = static_cast<float*>(pack_ws);
  hipError_t e = pack_conv_dgrad(w, Cin, Cin, Cout, ksize, wp, s);
  if (e == hipSuccess)
    e = conv_dgrad(View{const_cast<float*>(dz), Cout, 0}, N, H, W, Cout, wp, Cin, ksize, epi,
                   View{const_cast<float*>(mask), mask_stride, 0}, View{dx, dx_stride, 0}, s);
  return hip_status(e, "dn_conv2d_backward_data");
}

size_t dn_conv2d_wgrad_slab_size(int N, int H, int W, int Cin, int Cout, int ksize) {
  const int mode = ksize == 3 ? W_C3 : W_C1;
  return sizeof(float) * (64 + (size_t)wgrad_size(mode, N, H, W, Cin, Cout, false).floats);
}

dn_status dn_conv2d_backward_weight(const float* dz, const float* x, int x_stride, int N, int H,
                                    int W, int Cin, int Cout, int ksize, float* dwb, void* slab,
                                    void* stream) {
  if (!dz || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
  if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
  const int mode = ksize == 3 ? W_C3 : W_C1;
  if (!wgrad_supported(mode, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
  if (mode == W_C1 && Cin > 96) return fail(DN_ERR_ARG, "1x1 wgrad supports Cin <= 96");
  return wgrad_run(wgrad_route(wgrad_shape(mode, N, H, W, Cin, Cout, Cout, 0, x_stride, 0)), dz, x,
                   dwb, static_cast<float*>(slab), nullptr, (hipStream_t)stream);
}

dn_status dn_conv2d_backward_weight_x6(const float* dz, const float* x, int x_stride, int N,
                                       int H, int W, int Cin, int Cout, float* dwb, void* slab,
                                       void* stream) {
  if (!dz || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
  if (!wgrad_supported(W_C3, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
  // (dn_profile_ops: wgrad_run() takes the "wgrad3" record itself)
  return wgrad_run(wgrad_route(wgrad_shape(W_C3, N, H, W, Cin, Cout, Cout, 0, x_stride, 0, true)),
                   dz, x, dwb, static_cast<float*>(slab), nullptr, (hipStream_t)stream);
}

dn_status dn_deconv2x2_forward(const float* x, int N, int H, int W, int Cin, const float* w,
                               const float* b, int Cout, float* y, int y_stride, int y_off,
                               void* pack_ws, size_t pack_bytes, void* stream) {
  if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || y_stride < y_off + Cout)
    return fail(DN_ERR_ARG, "bad shape");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_pack_size(Cin, Cout, 0))) return st;
  hipStream_t s = (hipStream_t)stream;
  float* wp = static_cast<float*>(pack_ws);
  hipError_t e = pack_deconv_fwd(w, Cin, Cout, wp, s);
  if (e == hipSuccess)
    e = deconv_forward(View{const_cast<float*>(x), Cin, 0}, N, H, W, Cin, wp, b, Cout,
                       View{y, y_stride, y_off}, s);
  return hip_status(e, "dn_deconv2x2_forward");
}

size_t dn_deconv2x2_x6_pack_size(void) { return 4 * sizeof(uint16_t) * (size_t)X6_HEAD_BF; }

dn_status dn_deconv2x2_forward_x6(const float* x, int N, int H, int W, const float* w,
                                  const float* b, float* y, int y_stride, int y_off, void* pack_ws,
                                  size_t pack_bytes, void* stream) {
  if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || y_stride < y_off + 96 || ((y_stride | y_off) & 3))
    return fail(DN_ERR_ARG, "bad shape");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_x6_pack_size())) return st;
  hipStream_t s = (hipStream_t)stream;
  FwdArgs a = fwd_args(View{const_cast<float*>(x), 96, 0}, N, H, W, 96, 96,
                       View{y, y_stride, y_off}, OUT_UP2);
  a.bias = b;
  if (!deconv_x6_ok(a)) return fail(DN_ERR_ARG, "shape outside the bf16x6 deconv kernel");
  hipError_t e = launch_pack_deconv_x6(w, pack_ws, s);
  if (e == hipSuccess) e = launch_deconv_x6(a, pack_ws, s);
  return hip_status(e, "dn_deconv2x2_forward_x6");
}

dn_status dn_deconv2x2_backward_data_x6(const float* dy, int dy_stride, int N, int H, int W,
                                        const float* w, const float* mask, float* dx,
                                        void* pack_ws, size_t pack_bytes, void* stream) {
  if (!dy || !w || !dx) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || dy_stride < 96 || (dy_stride & 3)) return fail(DN_ERR_ARG, "bad shape");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_x6_pack_size())) return st;
  hipStream_t s = (hipStream_t)stream;
  FwdArgs a = fwd_args(View{const_cast<float*>(dy), dy_stride, 0}, 2 * H, 2 * W, N, H, W, 96, 96,
                       View{dx, 96, 0}, OUT_NHWC);
  a.epi = mask ? EPI_MASK : EPI_PLAIN;
  set_mask(a, View{const_cast<float*>(mask), 96, 0});
  if (!deconv_dgrad_x6_ok(a)) return fail(DN_ERR_ARG, "shape outside the bf16x6 deconv kernel");
  PackBatch b;
  b.j[b.n++] = pack_job_deconv_dgrad_x6(w, pack_ws);
  hipError_t e = pack_flush(b, s);
  if (e == hipSuccess) e = launch_deconv_dgrad_x6(a, pack_ws, s);
  return hip_status(e, "dn_deconv2x2_backward_data_x6");
}

dn_status dn_deconv2x2_backward_data(const float* dy, int dy_stride, int N, int H, int W, int Cout,
                                     const float* w, int Cin, const float* mask, float* dx,
                                     void* pack_ws, size_t pack_bytes, void* stream) {
  if (!dy || !w || !dx) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || H < 1 || W < 1 || Cout < 1 || dy_stride < Cout) return fail(DN_ERR_ARG, "bad shape");
  if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_pack_size(Cin, Cout, 1))) return st;
  hipStream_t s = (hipStream_t)stream;
  float* wp = static_cast<float*>(pack_ws);
  hipError_t e = pack_deconv_dgrad(w, Cout, Cin, wp, s);
  if (e == hipSuccess)
    e = deconv_dgrad(View{const_cast<float*>(dy), dy_stride, 0}, N, H, W, Cout, wp, Cin,
                     View{const_cast<float*>(mask), Cin, 0}, mask ? EPI_MASK : EPI_PLAIN,
                     View{dx, Cin, 0}, s);
  return hip_status(e, "dn_deconv2x2_backward_data");
}

size_t dn_deconv2x2_wgrad_slab_size(int N, int H, int W, int Cin, int Cout) {
  return sizeof(float) * (64 + (size_t)wgrad_size(W_UP2, N, H, W, Cin, Cout, false).floats);
}

dn_status dn_deconv2x2_backward_weight(const float* dy, int dy_stride, const float* x, int N, int H,
                                       int W, int Cin, int Cout, float* dwb, void* slab,
                                       void* stream) {
  if (!dy || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
  if (!wgrad_supported(W_UP2, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
  return wgrad_run(wgrad_route(wgrad_shape(W_UP2, N, H, W, Cin, Cout, dy_stride, 0, Cin, 0)), dy, x,
                   dwb, static_cast<float*>(slab), nullptr, (hipStream_t)stream);
}

dn_status dn_maxpool2x2_forward(const float* x, int N, int H, int W, int C, float* y, int y_stride,
                                int y_off, void* stream) {
  if (!x || !y) return fail(DN_ERR_ARG, "null argument");
  if ((H & 1) || (W & 1) || (C & 3) || (y_stride & 3) || (y_off & 3))
    return fail(DN_ERR_ARG, "H, W even and C, y_stride, y_off multiples of 4 required");
  return hip_status(launch_pool_fwd(x, N, H, W, C, y, y_stride, y_off, (hipStream_t)stream),
                    "dn_maxpool2x2_forward");
}

dn_status dn_maxpool2x2_backward(const float* x, int N, int H, int W, int C, const float* dy,
                                 int dy_stride, int dy_off, int act, float* dx, void* stream) {
  if (!x || !dy || !dx) return fail(DN_ERR_ARG, "null argument");
  if ((H & 1) || (W & 1) || (C & 3) || (dy_stride & 3) || (dy_off & 3))
    return fail(DN_ERR_ARG, "H, W even and C, dy_stride, dy_off multiples of 4 required");
  return hip_status(launch_pool_bwd(x, N, H, W, C, dy, dy_stride, dy_off, act, dx,
                                    (hipStream_t)stream),
                    "dn_maxpool2x2_backward");
}

// ---- adapter finetune (adapter.py:5-67, finetune.py:153-162) ---------------------------------
dn_status dn_adapter_param_count(int in_channels, int hidden_channels, size_t* count) {
  if (!count) return fail(DN_ERR_ARG, "null argument");
  if (hidden_channels != 16) return fail(DN_ERR_ARG, "hidden_channels must be 16 (adapter.py default)");
  const long n = adapter_param_count(in_channels);
  if (n < 0) return fail(DN_ERR_ARG, "in_channels must be 1 or 3");
  *count = (size_t)n;
  return DN_OK;
}

static dn_status adapter_args(int N, int C, int H, int W, int hidden) {
  if (hidden != 16) return fail(DN_ERR_ARG, "hidden_channels must be 16 (adapter.py default)");
  if (C != 1 && C != 3) return fail(DN_ERR_ARG, "in_channels must be 1 or 3");
  if (N < 1 || H < 1 || W < 1) return fail(DN_ERR_ARG, "empty adapter input");
  return DN_OK;
}

size_t dn_adapter_slab_size(int N, int C, int H, int W, int hidden_channels) {
  if (hidden_channels != 16 || adapter_param_count(C) < 0 || N < 1 || H < 1 || W < 1) return 0;
  return sizeof(float) * (size_t)adapter_bwd_blocks(N, H, W) * (size_t)adapter_param_count(C);
}

dn_status dn_adapter_forward(const float* params, const float* noisy, const float* base_out,
                             float* out, int N, int C, int H, int W, int hidden_channels,
                             void* stream) {
  if (!params || !noisy || !base_out || !out) return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
  return hip_status(launch_adapter_fwd(params, noisy, base_out, N, C, H, W, out, (hipStream_t)stream),
                    "dn_adapter_forward");
}

dn_status dn_adapter_backward(const float* params, const float* noisy, const float* base_out,
                              const float* dout, float* dparams, int N, int C, int H, int W,
                              int hidden_channels, void* slab, size_t slab_bytes, void* stream) {
  if (!params || !noisy || !base_out || !dout || !dparams || !slab)
    return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
  if (slab_bytes < dn_adapter_slab_size(N, C, H, W, hidden_channels))
    return fail(DN_ERR_WORKSPACE, "slab smaller than dn_adapter_slab_size()");
  return hip_status(launch_adapter_bwd(params, noisy, base_out, dout, N, C, H, W, dparams,
                                       static_cast<float*>(slab), (hipStream_t)stream),
                    "dn_adapter_backward");
}

dn_status dn_adapter_backward_input(const float* params, const float* noisy, const float* base_out,
                                    const float* dout, float* dbase, float* dnoisy, int N, int C,
                                    int H, int W, int hidden_channels, void* stream) {
  if (!params || !noisy || !base_out || !dout || !dbase) return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = adapter_args(N, C, H, W, hidden_channels)) return st;
  // neighbouring tiles read the halo of every input: an output may overwrite none of them
  for (const float* in : {noisy, base_out, dout})
    if (dbase == in || dnoisy == in)
      return fail(DN_ERR_ARG, "dbase / dnoisy must not alias noisy, base_out or dout");
  if (dbase == dnoisy) return fail(DN_ERR_ARG, "dbase and dnoisy must be distinct buffers");
  return hip_status(launch_adapter_dinput(params, noisy, base_out, dout, N, C, H, W, dbase, dnoisy,
                                          (hipStream_t)stream),
                    "dn_adapter_backward_input");
}

dn_status dn_finetune_loss(const float* pred, const float* target, int N, int C, int H, int W,
                           float lambda_grad, float* dpred, float* loss3, void* partial_ws,
                           void* stream) {
  if (!pred || !target || !dpred || !loss3 || !partial_ws) return fail(DN_ERR_ARG, "null argument");
  if (N < 1 || C < 1 || H < 2 || W < 2) return fail(DN_ERR_ARG, "gradient_loss needs H, W >= 2");
  return hip_status(launch_ft_loss(pred, target, N, C, H, W, lambda_grad, dpred, loss3, partial_ws,
                                   (hipStream_t)stream),
                    "dn_finetune_loss");
}

// ---- IQSL finetune loss (finetune_iqsl.py:291-383) ---------------------------------------------
size_t dn_iqsl_partials_size(void) { return iqsl_partials_bytes(); }

// validates IQSL's scalars and forms what the kernels compare with: each value in double, rounded
// once to fp32 (torch rounds a Python float to the tensor's dtype before it compares)
static dn_status iqsl_scalars(int N, int C, int H, int W, double t1, double t2, double tau,
                              double margin, double ce_factor, IqslScalars& a) {
  if (C != 1) return fail(DN_ERR_ARG, "IQSL assumes single-channel input: C must be 1");
  if (N < 1 || H < 2 || W < 2) return fail(DN_ERR_ARG, "gradient_loss needs H, W >= 2");
  if (!std::isfinite(t1) || !std::isfinite(t2)) return fail(DN_ERR_ARG, "IQSL thresholds must be finite");
  if (!std::isfinite(tau) || !std::isfinite(margin) || !std::isfinite(ce_factor))
    return fail(DN_ERR_ARG, "IQSL tau, margin and ce_factor must be finite");
  if (!(t1 < t2) || !((float)t1 < (float)t2))
    return fail(DN_ERR_ARG, "IQSL needs t1 < t2 (as fp32 values too)");
  a.t1 = (float)t1;
  a.t2 = (float)t2;
  a.t1_lo = (float)(t1 - margin);
  a.t1_hi = (float)(t1 + margin);
  a.t2_lo = (float)(t2 - margin);
  a.t2_hi = (float)(t2 + margin);
  a.c[0] = (float)(t1 / 2.0);
  a.c[1] = (float)((t1 + t2) / 2.0);
  a.c[2] = (float)((t2 + 1.0) / 2.0);
  a.use_margin = margin > 0.0;
  a.tau = tau > 1e-6 ? tau : 1e-6;
  return DN_OK;
}

dn_status dn_finetune_iqsl_loss(const float* pred, const float* target, int N, int C, int H, int W,
                                float lambda_grad, float lambda_iqsl, double t1, double t2,
                                double tau, double margin, double ce_factor, float* dpred,
                                float* loss4, void* partial_ws, void* stream) {
  if (!pred || !target || !dpred || !loss4 || !partial_ws) return fail(DN_ERR_ARG, "null argument");
  IqslScalars a;
  if (dn_status st = iqsl_scalars(N, C, H, W, t1, t2, tau, margin, ce_factor, a)) return st;
  const OpTimer timer((hipStream_t)stream, "loss_iqsl", 0, 0, 0, H, W, N);
  return hip_status(launch_iqsl_loss(pred, target, N, C, H, W, lambda_grad, lambda_iqsl, a,
                                     ce_factor, true, dpred, loss4, partial_ws, (hipStream_t)stream),
                    "dn_finetune_iqsl_loss");
}

dn_status dn_iqsl_loss(const float* pred, const float* target, int N, int C, int H, int W,
                       double t1, double t2, double tau, double margin, double ce_factor,
                       float* dpred, float* loss1, void* partial_ws, void* stream) {
  if (!pred || !target || !dpred || !loss1 || !partial_ws) return fail(DN_ERR_ARG, "null argument");
  IqslScalars a;
  if (dn_status st = iqsl_scalars(N, C, H, W, t1, t2, tau, margin, ce_factor, a)) return st;
  return hip_status(launch_iqsl_loss(pred, target, N, C, H, W, 0.f, 1.f, a, ce_factor, false, dpred,
                                     loss1, partial_ws, (hipStream_t)stream),
                    "dn_iqsl_loss");
}

dn_status dn_iq_iou_u8(const uint8_t* pred, const uint8_t* clean, int C, int H, int W, double t1,
                       double t2, void* part, int64_t* counts6, void* stream) {
  if (!pred || !clean || !part || !counts6) return fail(DN_ERR_ARG, "null argument");
  if (C < 1 || C > 65536 || H < 1 || W < 1) return fail(DN_ERR_ARG, "need 1 <= C <= 65536 and H, W >= 1");
  if (std::isnan(t1) || std::isnan(t2) || t1 > t2) return fail(DN_ERR_ARG, "need t1 <= t2, neither NaN");
  return hip_status(launch_iq_iou(pred, clean, C, (long)H * W, t1, t2, part, counts6,
                                  (hipStream_t)stream),
                    "dn_iq_iou_u8");
}

// ---- ImprovedUNet (arch_unet.py:421-531) ------------------------------------------------------
dn_status dn_iunet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  DN_GUARD_BEGIN
  if (!cfg || !count) return fail(DN_ERR_ARG, "null argument");
  IParams P;
  std::string err;
  if (!iunet_build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
  *count = (size_t)P.total;
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_iunet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                  size_t* bytes) {
  DN_GUARD_BEGIN
  if (!cfg || !bytes) return fail(DN_ERR_ARG, "null argument");
  IPlan p;
  std::string err;
  if (!iunet_build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  *bytes = (size_t)p.total_floats * sizeof(float);
  return DN_OK;
  DN_GUARD_END
}

dn_status dn_iunet_forward(const dn_unet_cfg* cfg, const float* params, const float* x, float* y,
                           int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
  return dn_iunet_forward_prec(cfg, params, x, y, N, H, W, ws, ws_bytes, DN_PREC_FP32, stream);
}

dn_status dn_iunet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                                float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "ImprovedUNet precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
  IPlan p;
  // (the plan with the backward buffers has the same forward offsets)
  if (dn_status st = plan_for_workspace(iunet_build_plan, *cfg, N, H, W, ws_bytes, true,
                                        "dn_iunet_workspace_size", p))
    return st;
  return iunet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision);
  DN_GUARD_END
}

dn_status dn_iunet_backward(const dn_unet_cfg* cfg, const float* params, const float* dy,
                            float* dparams, int N, int H, int W, void* ws, size_t ws_bytes,
                            void* stream) {
  return dn_iunet_backward_prec(cfg, params, dy, dparams, N, H, W, ws, ws_bytes, DN_PREC_FP32,
                                stream);
}

dn_status dn_iunet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                 float* dparams, int N, int H, int W, void* ws, size_t ws_bytes,
                                 int precision, void* stream) {
  DN_GUARD_BEGIN
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "ImprovedUNet precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (!cfg || !params || !dy || !dparams || !ws) return fail(DN_ERR_ARG, "null argument");
  IPlan p;
  std::string err;
  if (!iunet_build_plan(*cfg, N, H, W, true, p, err)) return fail(DN_ERR_ARG, err);
  if (ws_bytes < (size_t)p.total_floats * sizeof(float))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_iunet_workspace_size(with_backward=1)");
  return iunet_backward(p, params, dy, dparams, static_cast<float*>(ws), (hipStream_t)stream,
                        precision);
  DN_GUARD_END
}

/* (offset_floats, channel_stride, level) of the main ImprovedUNet activations, in the order
   x0 h | per down level i: F r z1 a1 z2 | bottle: F r z1 a1 z2 | per up k: cc F r z1 a1 z2 | xb cf */
dn_status dn_iunet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                 int64_t* desc, int max_entries, int* n_entries) {
  DN_GUARD_BEGIN
  if (!cfg || !desc || !n_entries) return fail(DN_ERR_ARG, "null argument");
  IPlan p;
  std::string err;
  if (!iunet_build_plan(*cfg, N, H, W, with_backward != 0, p, err)) return fail(DN_ERR_ARG, err);
  int n = 0;
  auto add = [&](long off, int stride, int level) {
    if (n < max_entries) {
      desc[3 * n] = off;
      desc[3 * n + 1] = stride;
      desc[3 * n + 2] = level;
    }
    ++n;
  };
  auto blk = [&](const IBlockBufs& b, int ch, int l) {
    add(b.F, ch + 128, l); add(b.r, ch, l); add(b.z1, ch, l); add(b.a1, ch, l); add(b.z2, ch, l);
  };
  add(p.x0, 4, 0); add(p.h, 48, 0);
  for (int i = 0; i < 4; ++i) blk(p.dl[i], 48 << i, i);
  blk(p.bb, 384, 4);
  for (int k = 0; k < 4; ++k) {
    const int out = p.P.up[k].out;
    add(p.cc[k], 3 * out, 3 - k);
    blk(p.ul[k], out, 3 - k);
  }
  add(p.xb, 384, 4); add(p.cf, 28, 0);
  if (with_backward) {  // | per down level: dr dz2 dg1 dz1 | per up k: dcc | dpool
    for (int i = 0; i < 4; ++i) {
      const int ch = 48 << i;
      add(p.dl[i].dr, ch, i); add(p.dl[i].dz2, ch, i); add(p.dl[i].dg1, ch, i);
      add(p.dl[i].dz1, ch, i);
    }
    for (int k = 0; k < 4; ++k) add(p.dcc[k], 3 * p.P.up[k].out, 3 - k);
  }
  *n_entries = n;
  return DN_OK;
  DN_GUARD_END
}

// ---- ImprovedUNet building blocks as ops ---------------------------------------------------------
namespace {

// scratch of one GroupNorm call: [partials (doubles) | 3 coefficient arrays of N * C floats],
// each part rounded up to 64 floats
struct GnScratch {
  size_t part, coef, bytes;
  GnScratch(int N, int H, int W, int C) {
    part = ((size_t)gn_part_doubles(N, (long)H * W, C) * 2 + 63) / 64 * 64;  // in floats
    coef = ((size_t)N * C + 63) / 64 * 64;
    bytes = sizeof(float) * (part + 3 * coef);
  }
};

bool gn_shape_ok(int N, int H, int W, int C, int G) {
  return N >= 1 && H >= 1 && W >= 1 && C >= 4 && (C & 3) == 0 && C <= 1024 && G >= 1 && C % G == 0;
}

bool view_ok(const float* p, int stride, int off, int C) {
  return p && ((stride | off) & 3) == 0 && off >= 0 && off + C <= stride &&
         (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace

size_t dn_groupnorm_scratch_size(int N, int H, int W, int C) {
  if (!gn_shape_ok(N, H, W, C, 1)) return 0;
  return GnScratch(N, H, W, C).bytes;
}

dn_status dn_groupnorm_forward(const float* z, int z_stride, int z_off, const float* res,
                               int res_stride, int res_off, float* y, int y_stride, int y_off,
                               int N, int H, int W, int C, int G, const float* gamma,
                               const float* beta, int act, float* stats, void* scratch,
                               size_t scratch_bytes, void* stream) {
  DN_GUARD_BEGIN
  if (!gamma || !beta || !stats || !scratch) return fail(DN_ERR_ARG, "null argument");
  if (!gn_shape_ok(N, H, W, C, G))
    return fail(DN_ERR_ARG, "GroupNorm: C must be a multiple of 4 and of G, at most 1024");
  if (!view_ok(z, z_stride, z_off, C) || !view_ok(y, y_stride, y_off, C) ||
      (res && !view_ok(res, res_stride, res_off, C)) ||
      (reinterpret_cast<uintptr_t>(scratch) & 15))
    return fail(DN_ERR_ARG, "GroupNorm: views need 16-byte alignment and off + C <= stride");
  const GnScratch sc(N, H, W, C);
  if (scratch_bytes < sc.bytes)
    return fail(DN_ERR_WORKSPACE, "scratch smaller than dn_groupnorm_scratch_size()");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const StreamDeviceGuard device_guard(s);
  float* f = static_cast<float*>(scratch);
  const View zv{const_cast<float*>(z), z_stride, z_off};
  const View rv{const_cast<float*>(res), res_stride, res_off};
  const OpTimer timer(s, "gn", 0.0, 1, C, H, W, N);
  return gn_forward(zv, N, (long)H * W, C, G, gamma, beta, act, res ? &rv : nullptr,
                    View{y, y_stride, y_off}, stats, reinterpret_cast<double*>(f), f + sc.part,
                    f + sc.part + sc.coef, s);
  DN_GUARD_END
}

dn_status dn_groupnorm_backward(const float* dy, int dy_stride, int dy_off, const float* z,
                                int z_stride, int z_off, float* dz, int dz_stride, int dz_off,
                                int N, int H, int W, int C, int G, const float* gamma,
                                const float* stats, float* dgamma, float* dbeta, void* scratch,
                                size_t scratch_bytes, void* stream) {
  DN_GUARD_BEGIN
  if (!gamma || !stats || !dgamma || !dbeta || !scratch) return fail(DN_ERR_ARG, "null argument");
  if (!gn_shape_ok(N, H, W, C, G))
    return fail(DN_ERR_ARG, "GroupNorm: C must be a multiple of 4 and of G, at most 1024");
  if (!view_ok(dy, dy_stride, dy_off, C) || !view_ok(z, z_stride, z_off, C) ||
      !view_ok(dz, dz_stride, dz_off, C) || (reinterpret_cast<uintptr_t>(scratch) & 15))
    return fail(DN_ERR_ARG, "GroupNorm: views need 16-byte alignment and off + C <= stride");
  const GnScratch sc(N, H, W, C);
  if (scratch_bytes < sc.bytes)
    return fail(DN_ERR_WORKSPACE, "scratch smaller than dn_groupnorm_scratch_size()");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const StreamDeviceGuard device_guard(s);
  float* f = static_cast<float*>(scratch);
  const OpTimer timer(s, "gnbwd", 0.0, 1, C, H, W, N);
  return gn_backward(View{const_cast<float*>(dy), dy_stride, dy_off},
                     View{const_cast<float*>(z), z_stride, z_off}, N, (long)H * W, C, G, gamma,
                     stats, View{dz, dz_stride, dz_off}, dgamma, dbeta,
                     reinterpret_cast<double*>(f), f + sc.part, f + sc.part + sc.coef,
                     f + sc.part + 2 * sc.coef, s);
  DN_GUARD_END
}

size_t dn_conv2d_wgrad_blocked_slab_size(int N, int H, int W, int Cin, int Cout, int ksize) {
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3)) return 0;
  const int mode = ksize == 3 ? W_C3 : W_C1;
  return sizeof(float) * (64 + (size_t)wgrad_size(mode, N, H, W, Cin, Cout, true).floats);
}

dn_status dn_conv2d_backward_weight_blocked(const float* g, int g_stride, int g_off,
                                            const float* x, int x_stride, int x_off, int N, int H,
                                            int W, int Cin, int Cout, int ksize, int bias,
                                            int precision, float* dwb, void* slab, void* stream) {
  DN_GUARD_BEGIN
  if (!g || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
  if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
  if (precision != DN_PREC_FP32 && precision != DN_PREC_FP32_X6)
    return fail(DN_ERR_ARG, "precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || g_off < 0 || x_off < 0)
    return fail(DN_ERR_ARG, "bad shape");
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x) |
       reinterpret_cast<uintptr_t>(slab)) & 15)
    return fail(DN_ERR_ARG, "g, x and slab must be 16-byte aligned");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const StreamDeviceGuard device_guard(s);
  const int mode = ksize == 3 ? W_C3 : W_C1;
  WgradShape sh = wgrad_shape(mode, N, H, W, Cin, Cout, g_stride, g_off, x_stride, x_off,
                              precision == DN_PREC_FP32_X6);
  sh.blocked = true;
  sh.bias = bias != 0;
  return wgrad_run(wgrad_route(sh), g, x, dwb, static_cast<float*>(slab), nullptr, s);
  DN_GUARD_END
}

// ---- memory-bank adapter (finetune_memory.py, evaluation_704_iqsl_memory.py) --------------------
static dn_status mem_geom(int n_img, int C, int H, int W, int P, int stride, MemGeom& g) {
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

size_t dn_memory_select_ws_size(int B, int n_img, int C, int H, int W, int P, int stride) {
  MemGeom g;
  if (B < 1 || mem_geom(n_img, C, H, W, P, stride, g) != DN_OK) return 0;
  return mem_select_ws_bytes(g, B);
}

dn_status dn_memory_select(const float* queries, const float* noise_images, int B, int n_img, int C,
                           int H, int W, int P, int stride, int64_t* idx, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!queries || !noise_images || !idx || !ws) return fail(DN_ERR_ARG, "null argument");
  if (B < 1) return fail(DN_ERR_ARG, "need B >= 1");
  MemGeom g;
  if (dn_status st = mem_geom(n_img, C, H, W, P, stride, g)) return st;
  if (ws_bytes < mem_select_ws_bytes(g, B))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memory_select_ws_size()");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const OpTimer timer(s, "mem_select", 2.0 * B * (double)g.N * C * P * P, 0, 0, P, P, B);
  return hip_status(launch_mem_select(queries, noise_images, g, B, idx, ws, s), "dn_memory_select");
}

dn_status dn_memory_gather(const float* clean_images, const int64_t* idx, int B, int n_img, int C,
                           int H, int W, int P, int stride, float* out, void* stream) {
  if (!clean_images || !idx || !out) return fail(DN_ERR_ARG, "null argument");
  if (B < 1) return fail(DN_ERR_ARG, "need B >= 1");
  MemGeom g;
  if (dn_status st = mem_geom(n_img, C, H, W, P, stride, g)) return st;
  return hip_status(launch_mem_gather(clean_images, g, idx, B, out, (hipStream_t)stream),
                    "dn_memory_gather");
}

static dn_status memadapter_args(int N, int C, int H, int W, int hidden, int nb) {
  if (!memadapter_supported(C, hidden, nb))
    return fail(DN_ERR_ARG, "need in_channels 1 or 3, hidden_channels 8 or 16, 0 <= num_fft_bins <= 8");
  if (N < 1 || H < 1 || W < 1) return fail(DN_ERR_ARG, "empty adapter input");
  if ((long)C * H * W < 2)
    return fail(DN_ERR_ARG, "the unbiased std needs at least two elements per sample");
  if (nb > 0 && W / 2 + 1 < nb) return fail(DN_ERR_ARG, "row FFT has fewer bins than num_fft_bins");
  return DN_OK;
}

dn_status dn_memadapter_param_count(int in_channels, int hidden_channels, int num_fft_bins,
                                    size_t* count) {
  if (!count) return fail(DN_ERR_ARG, "null argument");
  const long n = memadapter_param_count(in_channels, hidden_channels, num_fft_bins);
  if (n < 0) return memadapter_args(1, in_channels, 1, 64, hidden_channels, num_fft_bins);
  *count = (size_t)n;
  return DN_OK;
}

size_t dn_memadapter_ws_size(int N, int C, int H, int W, int hidden_channels, int num_fft_bins,
                             int with_backward) {
  return memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins,
                             with_backward == 2 ? 2 : with_backward != 0);
}

dn_status dn_memadapter_forward(const float* params, const float* noisy, const float* base_out,
                                const float* mem_clean, float* out, float* features, int N, int C,
                                int H, int W, int hidden_channels, int num_fft_bins,
                                int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  if (!params || !noisy || !base_out || !mem_clean || !out || !features || !ws)
    return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
  if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 0))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memadapter_ws_size()");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const OpTimer timer(s, "memadapter_fwd", 0, 0, 0, H, W, N);
  return hip_status(launch_memadapter_fwd(params, noisy, base_out, mem_clean, out, features, N, C, H,
                                          W, hidden_channels, num_fft_bins, clamp_output != 0, ws, s),
                    "dn_memadapter_forward");
}

dn_status dn_memadapter_backward(const float* params, const float* noisy, const float* base_out,
                                 const float* features, const float* dout, float* dparams, int N,
                                 int C, int H, int W, int hidden_channels, int num_fft_bins,
                                 int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  if (!params || !noisy || !base_out || !features || !dout || !dparams || !ws)
    return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
  if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 1))
    return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_memadapter_ws_size()");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const OpTimer timer(s, "memadapter_bwd", 0, 0, 0, H, W, N);
  return hip_status(launch_memadapter_bwd(params, noisy, base_out, features, dout, dparams, nullptr,
                                          N, C, H, W, hidden_channels, num_fft_bins,
                                          clamp_output != 0, ws, s),
                    "dn_memadapter_backward");
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool ranges_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return q && a < b + qbytes && b < a + bytes;
}

dn_status dn_memadapter_backward_input(const float* params, const float* noisy,
                                       const float* base_out, const float* features,
                                       const float* dout, float* dparams, float* dbase, int N, int C,
                                       int H, int W, int hidden_channels, int num_fft_bins,
                                       int clamp_output, void* ws, size_t ws_bytes, void* stream) {
  if (!params || !noisy || !base_out || !features || !dout || !dbase || !ws)
    return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = memadapter_args(N, C, H, W, hidden_channels, num_fft_bins)) return st;
  const size_t px = sizeof(float) * (size_t)N * C * H * W;
  const size_t np = sizeof(float) * (size_t)memadapter_param_count(C, hidden_channels, num_fft_bins);
  const size_t nf = sizeof(float) * (size_t)N * (6 + 3 * num_fft_bins);
  if (ranges_overlap(dbase, px, params, np) || ranges_overlap(dbase, px, noisy, px) ||
      ranges_overlap(dbase, px, base_out, px) || ranges_overlap(dbase, px, features, nf) ||
      ranges_overlap(dbase, px, dout, px) || ranges_overlap(dbase, px, dparams, np))
    return fail(DN_ERR_ARG, "dbase must not alias an input or dparams");
  if (ws_bytes < memadapter_ws_bytes(N, C, H, W, hidden_channels, num_fft_bins, 2))
    return fail(DN_ERR_ARG, "workspace smaller than dn_memadapter_ws_size(with_backward = 2)");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const OpTimer timer(s, "memadapter_bwd_input", 0, 0, 0, H, W, N);
  return hip_status(launch_memadapter_bwd(params, noisy, base_out, features, dout, dparams, dbase, N,
                                          C, H, W, hidden_channels, num_fft_bins, clamp_output != 0,
                                          ws, s),
                    "dn_memadapter_backward_input");
}

dn_status dn_memadapter_feature_adjoint(const float* base_out, const float* dfeat, float* hyper,
                                        int N, int C, int H, int W, int num_fft_bins, void* ws,
                                        size_t ws_bytes, void* stream) {
  if (!base_out || !dfeat || !hyper || !ws) return fail(DN_ERR_ARG, "null argument");
  if (dn_status st = memadapter_args(N, C, H, W, 8, num_fft_bins)) return st;
  if (ranges_overlap(hyper, sizeof(float) * (size_t)N * C * H * W, base_out,
                     sizeof(float) * (size_t)N * C * H * W))
    return fail(DN_ERR_ARG, "hyper must not alias base_out");
  if (ws_bytes < memadapter_ws_bytes(N, C, H, W, 8, num_fft_bins, 2))
    return fail(DN_ERR_ARG, "workspace smaller than dn_memadapter_ws_size(hidden 8, with_backward = 2)");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const OpTimer timer(s, "memadapter_feat_adj", 0, 0, 0, H, W, N);
  return hip_status(launch_memadapter_feature_adjoint(base_out, dfeat, hyper, N, C, H, W,
                                                      num_fft_bins, ws, s),
                    "dn_memadapter_feature_adjoint");
}

dn_status dn_hann_blend(const float* pred, const float* hann, const int* ys, const int* xs, int ny,
                        int nx, int C, int H, int W, int P, float* out, void* stream) {
  if (!pred || !hann || !ys || !xs || !out) return fail(DN_ERR_ARG, "null argument");
  if (ny < 1 || nx < 1 || C < 1 || P < 1 || H < P || W < P)
    return fail(DN_ERR_ARG, "need ny, nx, C >= 1 and H, W >= patch_size >= 1");
  return hip_status(launch_hann_blend(pred, hann, ys, xs, ny, nx, C, H, W, P, out,
                                      (hipStream_t)stream), "dn_hann_blend");
}

}  // extern "C"
