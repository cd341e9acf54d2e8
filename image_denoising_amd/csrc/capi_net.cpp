// extern "C" boundary (include/denoise_hip.h): version and errors, the side streams, and the three
// networks.  UNet, RESNET and ImprovedUNet share one scaffold: a trait per family names its plan,
// builders, passes and messages, and the templates below are the entry points' bodies.
#include <cstring>
#include <string>

#include "capi_common.h"
#include "iunet.h"
#include "resnet.h"
#include "unet.h"

using namespace dn;

namespace {

bool fp32_or_x6(int precision) {
  return precision == DN_PREC_FP32 || precision == DN_PREC_FP32_X6;
}

struct UNetFamily {
  using params_t = ParamLayout;
  using plan_t = Plan;
  static constexpr int layers = NL;
  static constexpr auto build_params = dn::build_params;
  static constexpr auto build_plan = dn::build_plan;
  static constexpr auto debug_buffers = unet_debug_buffers;
  static constexpr const char* size_fn = "dn_unet_workspace_size";
  static constexpr const char* bad_forward_prec = "unknown precision";
  static constexpr const char* bad_backward_prec =
      "backward precision must be DN_PREC_FP32 or DN_PREC_FP32_X6";
  static bool forward_prec_ok(int prec) { return fp32_or_x6(prec) || prec == DN_PREC_BF16; }
  static dn_status forward(const Plan& p, const float* prm, const float* x, float* y, float* ws,
                           hipStream_t s, int prec) {
    return unet_forward(p, prm, x, y, ws, s, prec);
  }
  static dn_status backward(const Plan& p, const float* prm, const float* dy, float* dprm,
                            float* dx, float* ws, hipStream_t s, int prec) {
    return unet_backward(p, prm, dy, dprm, dx, ws, s, prec);
  }
};

struct ResnetFamily {
  using params_t = ResParamLayout;
  using plan_t = ResPlan;
  static constexpr int layers = R_NL;
  static constexpr auto build_params = res_build_params;
  static constexpr auto build_plan = res_build_plan;
  static constexpr auto debug_buffers = resnet_debug_buffers;
  static constexpr auto forward = resnet_forward;
  static constexpr auto backward = resnet_backward;
  static constexpr const char* size_fn = "dn_resnet_workspace_size";
  static constexpr const char* bad_forward_prec =
      "RESNET precision must be DN_PREC_FP32 or DN_PREC_FP32_X6";
  static constexpr const char* bad_backward_prec = bad_forward_prec;
  static bool forward_prec_ok(int prec) { return fp32_or_x6(prec); }
};

// (no layers: the family has no dn_iunet_param_info; no dx: its backward produces none)
struct IunetFamily {
  using params_t = IParams;
  using plan_t = IPlan;
  static constexpr auto build_params = iunet_build_params;
  static constexpr auto build_plan = iunet_build_plan;
  static constexpr auto debug_buffers = iunet_debug_buffers;
  static constexpr auto forward = iunet_forward;
  static constexpr const char* size_fn = "dn_iunet_workspace_size";
  static constexpr const char* bad_forward_prec =
      "ImprovedUNet precision must be DN_PREC_FP32 or DN_PREC_FP32_X6";
  static constexpr const char* bad_backward_prec = bad_forward_prec;
  static bool forward_prec_ok(int prec) { return fp32_or_x6(prec); }
  static dn_status backward(const IPlan& p, const float* prm, const float* dy, float* dprm,
                            float*, float* ws, hipStream_t s, int prec) {
    return iunet_backward(p, prm, dy, dprm, ws, s, prec);
  }
};

template <class F>
dn_status built_plan(const dn_unet_cfg& cfg, int N, int H, int W, bool bwd,
                     typename F::plan_t& p) {
  std::string err;
  return F::build_plan(cfg, N, H, W, bwd, p, err) ? DN_OK : fail(DN_ERR_ARG, err);
}

template <class F>
dn_status workspace_holds(const typename F::plan_t& p, size_t ws_bytes) {
  if (ws_bytes >= (size_t)p.total_floats * sizeof(float)) return DN_OK;
  return fail(DN_ERR_WORKSPACE, std::string("workspace smaller than ") + F::size_fn +
                                    (p.with_bwd ? "(with_backward=1)" : "()"));
}

// the plan an entry point runs, which the caller's workspace has to hold
template <class F>
dn_status plan_checked(const dn_unet_cfg& cfg, int N, int H, int W, bool bwd, size_t ws_bytes,
                       typename F::plan_t& p) {
  if (dn_status st = built_plan<F>(cfg, N, H, W, bwd, p)) return st;
  return workspace_holds<F>(p, ws_bytes);
}

// The plan a forward entry point runs.  The workspace's size decides it: one sized with_backward=1
// gets that plan (the forward saves what the backward reads); a smaller one, or a bf16 pass (which
// saves nothing for a backward), gets the forward-only plan.  (UNet's with-backward plan has dense
// concat strides, its forward-only plan strides padded to 128-B lines; ImprovedUNet's two plans
// have the same forward offsets.)
template <class F>
dn_status plan_for_workspace(const dn_unet_cfg& cfg, int N, int H, int W, size_t ws_bytes,
                             int precision, typename F::plan_t& p) {
  if (!F::forward_prec_ok(precision)) return fail(DN_ERR_ARG, F::bad_forward_prec);
  std::string err;
  if (precision != DN_PREC_BF16 && F::build_plan(cfg, N, H, W, true, p, err) &&
      ws_bytes >= (size_t)p.total_floats * sizeof(float))
    return DN_OK;
  return plan_checked<F>(cfg, N, H, W, false, ws_bytes, p);
}

template <class F>
dn_status param_count(const dn_unet_cfg* cfg, size_t* count) {
  return guarded([&] {
    if (!cfg || !count) return fail(DN_ERR_ARG, "null argument");
    typename F::params_t P;
    std::string err;
    if (!F::build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
    *count = (size_t)P.total;
    return DN_OK;
  });
}

template <class F>
dn_status param_info(const dn_unet_cfg* cfg, int index, size_t* w_off, size_t* w_count,
                     size_t* b_count) {
  return guarded([&] {
    if (!cfg || !w_off || !w_count || !b_count) return fail(DN_ERR_ARG, "null argument");
    typename F::params_t P;
    std::string err;
    if (!F::build_params(*cfg, P, err)) return fail(DN_ERR_ARG, err);
    if (index < 0 || index >= F::layers) return fail(DN_ERR_ARG, "layer index out of range");
    *w_off = (size_t)P.L[index].woff;
    *w_count = (size_t)P.L[index].wcount;
    *b_count = (size_t)P.L[index].cout;
    return DN_OK;
  });
}

template <class F>
dn_status workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                         size_t* bytes) {
  return guarded([&] {
    if (!cfg || !bytes) return fail(DN_ERR_ARG, "null argument");
    typename F::plan_t p;
    if (dn_status st = built_plan<F>(*cfg, N, H, W, with_backward != 0, p)) return st;
    *bytes = (size_t)p.total_floats * sizeof(float);
    return DN_OK;
  });
}

template <class F>
dn_status forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x, float* y, int N,
                       int H, int W, void* ws, size_t ws_bytes, int precision, void* stream) {
  return guarded([&] {
    if (!F::forward_prec_ok(precision)) return fail(DN_ERR_ARG, F::bad_forward_prec);
    if (!cfg || !params || !x || !y || !ws) return fail(DN_ERR_ARG, "null argument");
    typename F::plan_t p;
    if (dn_status st = plan_for_workspace<F>(*cfg, N, H, W, ws_bytes, precision, p)) return st;
    return F::forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision);
  });
}

// dx: nullable, and ignored by a family whose backward has none
template <class F>
dn_status backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                        float* dparams, float* dx, int N, int H, int W, void* ws, size_t ws_bytes,
                        int precision, void* stream) {
  return guarded([&] {
    if (!fp32_or_x6(precision)) return fail(DN_ERR_ARG, F::bad_backward_prec);
    if (!cfg || !params || !dy || !dparams || !ws) return fail(DN_ERR_ARG, "null argument");
    typename F::plan_t p;
    if (dn_status st = plan_checked<F>(*cfg, N, H, W, true, ws_bytes, p)) return st;
    return F::backward(p, params, dy, dparams, dx, static_cast<float*>(ws), (hipStream_t)stream,
                       precision);
  });
}

// desc gets the first max_entries (offset_floats, channel_stride, level) triples of the plan's
// list, n_entries the list's length
template <class F>
dn_status debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                        int64_t* desc, int max_entries, int* n_entries) {
  return guarded([&] {
    if (!cfg || !desc || !n_entries) return fail(DN_ERR_ARG, "null argument");
    typename F::plan_t p;
    if (dn_status st = built_plan<F>(*cfg, N, H, W, with_backward != 0, p)) return st;
    int n = 0;
    F::debug_buffers(p, [&](long off, int stride, int level) {
      if (n < max_entries) {
        desc[3 * n] = off;
        desc[3 * n + 1] = stride;
        desc[3 * n + 2] = level;
      }
      ++n;
    });
    *n_entries = n;
    return DN_OK;
  });
}

// dn_unet_pack_weights (PACK_ONLY; x, y unused) and dn_unet_forward_prepacked (RUN_ONLY)
dn_status unet_forward_packed(const dn_unet_cfg* cfg, const float* params, const float* x, float* y,
                              int N, int H, int W, void* ws, size_t ws_bytes, int precision,
                              void* stream, int pack) {
  return guarded([&] {
    if (!cfg || !params || !ws || (pack == RUN_ONLY && (!x || !y)))
      return fail(DN_ERR_ARG, "null argument");
    Plan p;
    if (dn_status st = plan_for_workspace<UNetFamily>(*cfg, N, H, W, ws_bytes, precision, p))
      return st;
    return unet_forward(p, params, x, y, static_cast<float*>(ws), (hipStream_t)stream, precision,
                        nullptr, pack);
  });
}

}  // namespace

extern "C" {

#ifndef DN_SRC_HASH
#define DN_SRC_HASH "unknown"
#endif
// src= the sha256 prefix of the sources this library was compiled from (_build.source_hash)
const char* dn_version(void) { return "denoise_hip 0.5.0 gfx950 src=" DN_SRC_HASH; }

int dn_abi_version(void) { return DN_ABI_VERSION; }

int dn_last_error(char* buf, size_t len) {
  return guarded_query([&] {
    const std::string& s = g_last_error;
    if (buf && len) {
      size_t n = s.size() < len - 1 ? s.size() : len - 1;
      std::memcpy(buf, s.data(), n);
      buf[n] = 0;
    }
    return (int)s.size();
  });
}

dn_status dn_prepare_streams(void* stream) {
  return guarded([&] {
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
  });
}

// ---- UNet -----------------------------------------------------------------------------
dn_status dn_unet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  return param_count<UNetFamily>(cfg, count);
}

dn_status dn_unet_param_info(const dn_unet_cfg* cfg, int index, size_t* w_off, size_t* w_count,
                             size_t* b_count) {
  return param_info<UNetFamily>(cfg, index, w_off, w_count, b_count);
}

dn_status dn_unet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                 size_t* bytes) {
  return workspace_size<UNetFamily>(cfg, N, H, W, with_backward, bytes);
}

dn_status dn_unet_forward(const dn_unet_cfg* cfg, const float* params, const float* x, float* y,
                          int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
  return forward_prec<UNetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, DN_PREC_FP32, stream);
}

dn_status dn_unet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                               float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                               int precision, void* stream) {
  return forward_prec<UNetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, precision, stream);
}

dn_status dn_unet_forward_bf16(const dn_unet_cfg* cfg, const float* params, const float* x,
                               float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                               void* stream) {
  return forward_prec<UNetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, DN_PREC_BF16, stream);
}

dn_status dn_unet_pack_weights(const dn_unet_cfg* cfg, const float* params, int N, int H, int W,
                               void* ws, size_t ws_bytes, int precision, void* stream) {
  return unet_forward_packed(cfg, params, nullptr, nullptr, N, H, W, ws, ws_bytes, precision,
                             stream, PACK_ONLY);
}

dn_status dn_unet_forward_prepacked(const dn_unet_cfg* cfg, const float* params, const float* x,
                                    float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                    int precision, void* stream) {
  return unet_forward_packed(cfg, params, x, y, N, H, W, ws, ws_bytes, precision, stream,
                             RUN_ONLY);
}

dn_status dn_unet_forward_n2n(const dn_unet_cfg* cfg, const float* params, const float* x,
                              float* den, const uint8_t* rd_idx, int N, int H, int W, void* ws,
                              size_t ws_bytes, int precision, void* stream) {
  return guarded([&] {
    if (!fp32_or_x6(precision))
      return fail(DN_ERR_ARG, "precision must be DN_PREC_FP32 or DN_PREC_FP32_X6");
    if (!cfg || !params || !x || !den || !rd_idx || !ws) return fail(DN_ERR_ARG, "null argument");
    Plan p;
    if (dn_status st = plan_checked<UNetFamily>(*cfg, N, H, W, false, ws_bytes, p)) return st;
    // (a no-grad pass: nothing is saved)
    return unet_forward(p, params, x, den, static_cast<float*>(ws), (hipStream_t)stream, precision,
                        rd_idx);
  });
}

dn_status dn_unet_backward(const dn_unet_cfg* cfg, const float* params, const float* dy,
                           float* dparams, float* dx, int N, int H, int W, void* ws,
                           size_t ws_bytes, void* stream) {
  return backward_prec<UNetFamily>(cfg, params, dy, dparams, dx, N, H, W, ws, ws_bytes,
                                   DN_PREC_FP32, stream);
}

dn_status dn_unet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                float* dparams, float* dx, int N, int H, int W, void* ws,
                                size_t ws_bytes, int precision, void* stream) {
  return backward_prec<UNetFamily>(cfg, params, dy, dparams, dx, N, H, W, ws, ws_bytes, precision,
                                   stream);
}

dn_status dn_unet_backward_split(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                 float* dparams, float* dx, int N, int H, int W, void* ws,
                                 size_t ws_bytes, int precision, void* stream, void* tail_ready,
                                 int64_t* tail_begin_out) {
  return guarded([&] {
    if (!fp32_or_x6(precision)) return fail(DN_ERR_ARG, UNetFamily::bad_backward_prec);
    if (!cfg) return fail(DN_ERR_ARG, "null argument");
    Plan p;
    if (dn_status st = built_plan<UNetFamily>(*cfg, N, H, W, true, p)) return st;
    if (tail_begin_out) *tail_begin_out = tail_begin(p);
    if (!params || !dy || !dparams || !ws) {
      if (!params && !dy && !dparams && !ws && !tail_ready) return DN_OK;  // a tail_begin query
      return fail(DN_ERR_ARG, "null argument");
    }
    if (dn_status st = workspace_holds<UNetFamily>(p, ws_bytes)) return st;
    return unet_backward(p, params, dy, dparams, dx, static_cast<float*>(ws), (hipStream_t)stream,
                         precision, static_cast<hipEvent_t>(tail_ready));
  });
}

dn_status dn_unet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                int64_t* desc, int max_entries, int* n_entries) {
  return debug_buffers<UNetFamily>(cfg, N, H, W, with_backward, desc, max_entries, n_entries);
}

// ---- RESNET -------------------------------------------------------------------------
dn_status dn_resnet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  return param_count<ResnetFamily>(cfg, count);
}

dn_status dn_resnet_param_info(const dn_unet_cfg* cfg, int index, size_t* w_off, size_t* w_count,
                               size_t* b_count) {
  return param_info<ResnetFamily>(cfg, index, w_off, w_count, b_count);
}

dn_status dn_resnet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                   size_t* bytes) {
  return workspace_size<ResnetFamily>(cfg, N, H, W, with_backward, bytes);
}

dn_status dn_resnet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                                 float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                 int precision, void* stream) {
  return forward_prec<ResnetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, precision, stream);
}

dn_status dn_resnet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                  float* dparams, float* dx, int N, int H, int W, void* ws,
                                  size_t ws_bytes, int precision, void* stream) {
  return backward_prec<ResnetFamily>(cfg, params, dy, dparams, dx, N, H, W, ws, ws_bytes,
                                     precision, stream);
}

dn_status dn_resnet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                  int64_t* desc, int max_entries, int* n_entries) {
  return debug_buffers<ResnetFamily>(cfg, N, H, W, with_backward, desc, max_entries, n_entries);
}

// ---- ImprovedUNet (arch_unet.py:421-531) ------------------------------------------------------
dn_status dn_iunet_param_count(const dn_unet_cfg* cfg, size_t* count) {
  return param_count<IunetFamily>(cfg, count);
}

dn_status dn_iunet_workspace_size(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                  size_t* bytes) {
  return workspace_size<IunetFamily>(cfg, N, H, W, with_backward, bytes);
}

dn_status dn_iunet_forward(const dn_unet_cfg* cfg, const float* params, const float* x, float* y,
                           int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
  return forward_prec<IunetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, DN_PREC_FP32, stream);
}

dn_status dn_iunet_forward_prec(const dn_unet_cfg* cfg, const float* params, const float* x,
                                float* y, int N, int H, int W, void* ws, size_t ws_bytes,
                                int precision, void* stream) {
  return forward_prec<IunetFamily>(cfg, params, x, y, N, H, W, ws, ws_bytes, precision, stream);
}

dn_status dn_iunet_backward(const dn_unet_cfg* cfg, const float* params, const float* dy,
                            float* dparams, int N, int H, int W, void* ws, size_t ws_bytes,
                            void* stream) {
  return backward_prec<IunetFamily>(cfg, params, dy, dparams, nullptr, N, H, W, ws, ws_bytes,
                                    DN_PREC_FP32, stream);
}

dn_status dn_iunet_backward_prec(const dn_unet_cfg* cfg, const float* params, const float* dy,
                                 float* dparams, int N, int H, int W, void* ws, size_t ws_bytes,
                                 int precision, void* stream) {
  return backward_prec<IunetFamily>(cfg, params, dy, dparams, nullptr, N, H, W, ws, ws_bytes,
                                    precision, stream);
}

dn_status dn_iunet_debug_buffers(const dn_unet_cfg* cfg, int N, int H, int W, int with_backward,
                                 int64_t* desc, int max_entries, int* n_entries) {
  return debug_buffers<IunetFamily>(cfg, N, H, W, with_backward, desc, max_entries, n_entries);
}

}  // extern "C"
