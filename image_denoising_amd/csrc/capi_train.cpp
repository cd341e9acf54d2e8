// extern "C" boundary (include/denoise_hip.h): the training step around the networks: the
// Neighbor2Neighbor sub-sampler, noise synthesis, the losses, Adam and its guarded step.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "capi_common.h"

using namespace dn;

namespace {

// The double a caller wrote before the ABI narrowed it to fp32: the shortest decimal that rounds
// to x.  torch.optim.Adam keeps lr and the betas as Python doubles and forms 1 - beta, beta^step
// and lr / bc1 from those.  (double)0.999f is 0.99900001287..., and 1 - beta2 formed from it is
// 1.3e-5 (relative) away from torch's, and exp_avg_sq with it.
double as_written(float x) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    std::snprintf(buf, sizeof buf, "%.*g", prec, (double)x);
    const double d = std::strtod(buf, nullptr);
    if ((float)d == x) return d;
  }
  return (double)x;
}

bool guard_state_ok(const void* state) {
  return state && (reinterpret_cast<uintptr_t>(state) & 15) == 0;
}

// validates IQSL's scalars and forms what the kernels compare with: each value in double, rounded
// once to fp32 (torch rounds a Python float to the tensor's dtype before it compares)
dn_status iqsl_scalars(int N, int C, int H, int W, double t1, double t2, double tau, double margin,
                       double ce_factor, IqslScalars& a) {
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

}  // namespace

extern "C" {

// ---- Neighbor2Neighbor sub-sampler, noise synthesis ---------------------------------------
dn_status dn_n2n_subsample(const float* img, int N, int C, int H, int W, const uint8_t* rd_idx_in,
                           uint64_t seed, uint64_t offset, uint64_t cell_base, float* sub1,
                           float* sub2, uint8_t* rd_idx_out, void* stream) {
  return guarded([&] {
    if (N < 0 || C < 1 || H < 0 || W < 0 || (H & 1) || (W & 1))
      return fail(DN_ERR_ARG, "H and W must be even");
    if ((long)N * H * W == 0) return DN_OK;
    if (!img || !sub1 || !sub2) return fail(DN_ERR_ARG, "null argument");
    const OpTimer timer((hipStream_t)stream, "subsample", 0, C, C, H, W, N);
    return hip_status(launch_subsample(img, N, C, H, W, rd_idx_in, seed, offset, cell_base, sub1,
                                       sub2, rd_idx_out, (hipStream_t)stream),
                      "dn_n2n_subsample");
  });
}

dn_status dn_n2n_masks(const uint8_t* rd_idx, int64_t ncells, uint8_t* mask1, uint8_t* mask2,
                       void* stream) {
  return guarded([&] {
    if (ncells < 0) return fail(DN_ERR_ARG, "ncells < 0");
    if (ncells == 0) return DN_OK;
    if (!rd_idx || !mask1 || !mask2) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_masks(rd_idx, ncells, mask1, mask2, (hipStream_t)stream),
                      "dn_n2n_masks");
  });
}

dn_status dn_n2n_subimage_from_mask(const float* img, int N, int C, int H, int W,
                                    const uint8_t* mask, float* sub, void* stream) {
  return guarded([&] {
    if (N < 0 || C < 1 || (H & 1) || (W & 1)) return fail(DN_ERR_ARG, "H and W must be even");
    if ((long)N * H * W == 0) return DN_OK;
    if (!img || !mask || !sub) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_subimage_from_mask(img, N, C, H, W, mask, sub, (hipStream_t)stream),
                      "dn_n2n_subimage_from_mask");
  });
}

dn_status dn_add_gauss_noise(const float* clean, int N, int64_t per_image, float std_,
                             const float* std_per_image, uint64_t seed, uint64_t offset,
                             uint64_t elem_base, float* noisy, void* stream) {
  return guarded([&] {
    if (N < 0 || per_image < 0) return fail(DN_ERR_ARG, "negative size");
    if ((long)N * per_image == 0) return DN_OK;
    if (!clean || !noisy) return fail(DN_ERR_ARG, "null argument");
    const OpTimer timer((hipStream_t)stream, "noise", 0);
    return hip_status(launch_noise(clean, N, per_image, std_, std_per_image, seed, offset,
                                   elem_base, noisy, (hipStream_t)stream),
                      "dn_add_gauss_noise");
  });
}

dn_status dn_add_poisson_noise(const float* clean, int N, int64_t per_image, float lam,
                               const float* lam_per_image, uint64_t seed, uint64_t offset,
                               uint64_t elem_base, float* noisy, void* stream) {
  return guarded([&] {
    if (N < 0 || per_image < 0) return fail(DN_ERR_ARG, "negative size");
    if (!lam_per_image && !(lam > 0.f && lam <= 500.f))
      return fail(DN_ERR_ARG, "lam must be in (0, 500]");
    if ((long)N * per_image == 0) return DN_OK;
    if (!clean || !noisy) return fail(DN_ERR_ARG, "null argument");
    const OpTimer timer((hipStream_t)stream, "noise", 0);
    return hip_status(launch_poisson(clean, N, per_image, lam, lam_per_image, seed, offset,
                                     elem_base, noisy, (hipStream_t)stream),
                      "dn_add_poisson_noise");
  });
}

// ---- losses ---------------------------------------------------------------------------
size_t dn_loss_partials_size(void) { return guarded_query([] { return loss_partials_bytes(); }); }

dn_status dn_n2n_loss(const float* out, const float* sub2, const float* den, const uint8_t* rd_idx,
                      int N, int C, int h, int w, float lambda, float* dout, float* loss3,
                      void* partial_ws, void* stream) {
  return guarded([&] {
    if (!out || !sub2 || !den || !rd_idx || !dout || !loss3 || !partial_ws)
      return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || C < 1 || h < 1 || w < 1) return fail(DN_ERR_ARG, "empty loss input");
    const OpTimer timer((hipStream_t)stream, "loss", 0);
    return hip_status(launch_n2n_loss(out, sub2, den, rd_idx, N, C, h, w, lambda, dout, loss3,
                                      partial_ws, (hipStream_t)stream),
                      "dn_n2n_loss");
  });
}

dn_status dn_structure_loss(const float* pred, const float* pred2, const float* target, int N, int C,
                            int H, int W, float alpha, float beta, float gamma, float* dpred,
                            float* dpred2, float* loss5, void* partial_ws, void* stream) {
  return guarded([&] {
    if (!pred || !pred2 || !target || !dpred || !dpred2 || !loss5 || !partial_ws)
      return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || C < 1 || H < 2 || W < 2) return fail(DN_ERR_ARG, "Structure_loss needs H, W >= 2");
    const OpTimer timer((hipStream_t)stream, "loss", 0);
    return hip_status(launch_structure_loss(pred, pred2, target, N, C, H, W, alpha, beta, gamma,
                                            dpred, dpred2, loss5, partial_ws, (hipStream_t)stream),
                      "dn_structure_loss");
  });
}

size_t dn_l1fft_ws_size(int N, int C, int H, int W) {
  return guarded_query([&] { return l1fft_ws_bytes(N, C, H, W); });
}

dn_status dn_l1fft_loss(const float* pred, const float* target, int N, int C, int H, int W,
                        float alpha, float beta, int reduction_sum, float* dpred, float* loss3,
                        void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    const size_t need = l1fft_ws_bytes(N, C, H, W);
    if (!need)
      return fail(DN_ERR_ARG, "L1FFT needs N, C >= 1 and H, W = m * 2^k with m odd <= 31, k >= 3, at most 1024");
    if (!pred || !target || !dpred || !loss3 || !ws) return fail(DN_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(ws) & 15)
      return fail(DN_ERR_ARG, "workspace must be 16-byte aligned");
    if (ws_bytes < need) return fail(DN_ERR_WORKSPACE, "workspace smaller than dn_l1fft_ws_size()");
    const OpTimer timer((hipStream_t)stream, "loss", 0);
    return hip_status(launch_l1fft_loss(pred, target, N, C, H, W, alpha, beta, reduction_sum != 0,
                                        dpred, loss3, ws, (hipStream_t)stream),
                      "dn_l1fft_loss");
  });
}

dn_status dn_finetune_loss(const float* pred, const float* target, int N, int C, int H, int W,
                           float lambda_grad, float* dpred, float* loss3, void* partial_ws,
                           void* stream) {
  return guarded([&] {
    if (!pred || !target || !dpred || !loss3 || !partial_ws)
      return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || C < 1 || H < 2 || W < 2) return fail(DN_ERR_ARG, "gradient_loss needs H, W >= 2");
    return hip_status(launch_ft_loss(pred, target, N, C, H, W, lambda_grad, dpred, loss3,
                                     partial_ws, (hipStream_t)stream),
                      "dn_finetune_loss");
  });
}

// ---- IQSL finetune loss (finetune_iqsl.py:291-383) ---------------------------------------------
size_t dn_iqsl_partials_size(void) { return guarded_query([] { return iqsl_partials_bytes(); }); }

dn_status dn_finetune_iqsl_loss(const float* pred, const float* target, int N, int C, int H, int W,
                                float lambda_grad, float lambda_iqsl, double t1, double t2,
                                double tau, double margin, double ce_factor, float* dpred,
                                float* loss4, void* partial_ws, void* stream) {
  return guarded([&] {
    if (!pred || !target || !dpred || !loss4 || !partial_ws)
      return fail(DN_ERR_ARG, "null argument");
    IqslScalars a;
    if (dn_status st = iqsl_scalars(N, C, H, W, t1, t2, tau, margin, ce_factor, a)) return st;
    const OpTimer timer((hipStream_t)stream, "loss_iqsl", 0, 0, 0, H, W, N);
    return hip_status(launch_iqsl_loss(pred, target, N, C, H, W, lambda_grad, lambda_iqsl, a,
                                       ce_factor, true, dpred, loss4, partial_ws,
                                       (hipStream_t)stream),
                      "dn_finetune_iqsl_loss");
  });
}

dn_status dn_iqsl_loss(const float* pred, const float* target, int N, int C, int H, int W,
                       double t1, double t2, double tau, double margin, double ce_factor,
                       float* dpred, float* loss1, void* partial_ws, void* stream) {
  return guarded([&] {
    if (!pred || !target || !dpred || !loss1 || !partial_ws)
      return fail(DN_ERR_ARG, "null argument");
    IqslScalars a;
    if (dn_status st = iqsl_scalars(N, C, H, W, t1, t2, tau, margin, ce_factor, a)) return st;
    return hip_status(launch_iqsl_loss(pred, target, N, C, H, W, 0.f, 1.f, a, ce_factor, false,
                                       dpred, loss1, partial_ws, (hipStream_t)stream),
                      "dn_iqsl_loss");
  });
}

// ---- optimiser ------------------------------------------------------------------------
dn_status dn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, int64_t step,
                       float grad_scale, void* stream) {
  return guarded([&] {
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
  });
}

size_t dn_guard_state_size(void) { return guarded_query([] { return guard_state_bytes(); }); }

dn_status dn_guard_state_init(void* state, int64_t step, void* stream) {
  return guarded([&] {
    if (!guard_state_ok(state))
      return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
    if (step < 0) return fail(DN_ERR_ARG, "step >= 0 required");
    return hip_status(launch_guard_init(state, step, (hipStream_t)stream), "dn_guard_state_init");
  });
}

dn_status dn_grad_norm(const float* grad, int64_t n, float grad_scale, void* state,
                       double* norm_out, void* stream) {
  return guarded([&] {
    if (n < 0) return fail(DN_ERR_ARG, "n < 0");
    if (n == 0) return DN_OK;
    if (!grad) return fail(DN_ERR_ARG, "null argument");
    if (!guard_state_ok(state))
      return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
    const OpTimer timer((hipStream_t)stream, "grad_norm", 0);
    return hip_status(launch_grad_norm(grad, n, grad_scale, state, norm_out, (hipStream_t)stream),
                      "dn_grad_norm");
  });
}

dn_status dn_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                               int64_t n, float lr, float beta1, float beta2, float eps,
                               float grad_scale, const float* loss, float max_loss,
                               float max_norm_skip, float clip, void* state, void* stream) {
  return guarded([&] {
    if (n < 0) return fail(DN_ERR_ARG, "n < 0");
    if (n == 0) return DN_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(DN_ERR_ARG, "null argument");
    if (!guard_state_ok(state))
      return fail(DN_ERR_ARG, "guard state must be non-null and 16-byte aligned");
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
  });
}

dn_status dn_guard_state_read(const void* state, dn_guard_stats* out, void* stream) {
  return guarded([&] {
    if (!guard_state_ok(state) || !out)
      return fail(DN_ERR_ARG, "null argument or unaligned guard state");
    return hip_status(guard_state_read(state, out, (hipStream_t)stream), "dn_guard_state_read");
  });
}

dn_status dn_accumulate(float* dst, const float* src, int64_t n, void* stream) {
  return guarded([&] {
    if (n < 0) return fail(DN_ERR_ARG, "n < 0");
    if (n == 0) return DN_OK;
    if (!dst || !src) return fail(DN_ERR_ARG, "null argument");
    const OpTimer timer((hipStream_t)stream, "accumulate", 0);
    return hip_status(launch_accumulate(dst, src, n, (hipStream_t)stream), "dn_accumulate");
  });
}

}  // extern "C"
