// extern "C" boundary (include/denoise_hip.h): the evaluation path (evaluation.py:23-114,
// evaluation_704.py:57-115, utils_eval.py:19-53): u8 conversion, tiling and blending, the metrics.
#include <cmath>
#include <string>

#include "capi_common.h"

using namespace dn;

namespace {

bool tile_args_ok(int C, int H, int W, int patch, int stride) {
  return C >= 1 && H >= 1 && W >= 1 && patch >= 1 && stride >= 1 && stride <= patch;
}

}  // namespace

extern "C" {

size_t dn_eval_partials_size(void) {
  return guarded_query([] { return EVAL_PARTS * sizeof(double); });
}

dn_status dn_u8_to_unit(const uint8_t* x, int64_t n, float* y, void* stream) {
  return guarded([&] {
    if (n < 0) return fail(DN_ERR_ARG, "n < 0");
    if (n == 0) return DN_OK;
    if (!x || !y) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_u8_to_unit(x, n, y, (hipStream_t)stream), "dn_u8_to_unit");
  });
}

int dn_tile_count(int extent, int patch, int stride) {
  return guarded_query([&] {
    if (extent < 1 || patch < 1 || stride < 1) return 0;
    return (extent + stride - 1) / stride;  // range(0, extent, stride)
  });
}

dn_status dn_tile_extract(const uint8_t* img, int C, int H, int W, int patch, int stride,
                          float* tiles, void* stream) {
  return guarded([&] {
    if (!img || !tiles) return fail(DN_ERR_ARG, "null argument");
    if (!tile_args_ok(C, H, W, patch, stride))
      return fail(DN_ERR_ARG, "need C,H,W,patch >= 1 and 1 <= stride <= patch");
    return hip_status(launch_tile_extract(img, C, H, W, patch, stride,
                                          dn_tile_count(H, patch, stride),
                                          dn_tile_count(W, patch, stride), tiles,
                                          (hipStream_t)stream),
                      "dn_tile_extract");
  });
}

dn_status dn_tile_blend(const float* pred, int C, int H, int W, int patch, int stride,
                        const float* wmask, float* out, uint8_t* out_u8, void* stream) {
  return guarded([&] {
    if (!pred || !wmask || (!out && !out_u8)) return fail(DN_ERR_ARG, "null argument");
    if (!tile_args_ok(C, H, W, patch, stride))
      return fail(DN_ERR_ARG, "need C,H,W,patch >= 1 and 1 <= stride <= patch");
    return hip_status(launch_tile_blend(pred, C, H, W, patch, stride,
                                        dn_tile_count(H, patch, stride),
                                        dn_tile_count(W, patch, stride), wmask, out, out_u8,
                                        (hipStream_t)stream),
                      "dn_tile_blend");
  });
}

dn_status dn_quantize_u8(const float* x, int64_t n, int plus_half, uint8_t* y, void* stream) {
  return guarded([&] {
    if (n < 0) return fail(DN_ERR_ARG, "n < 0");
    if (n == 0) return DN_OK;
    if (!x || !y) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_quantize_u8(x, n, plus_half, y, (hipStream_t)stream),
                      "dn_quantize_u8");
  });
}

dn_status dn_psnr_u8(const uint8_t* a, const uint8_t* b, int64_t n, void* part, double* psnr,
                     void* stream) {
  return guarded([&] {
    if (n < 1) return fail(DN_ERR_ARG, "n >= 1 required");
    if (!a || !b || !part || !psnr) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_psnr(a, b, n, static_cast<double*>(part), psnr, (hipStream_t)stream),
                      "dn_psnr_u8");
  });
}

dn_status dn_ssim_u8(const uint8_t* a, const uint8_t* b, int C, int H, int W, int hwc, void* part,
                     double* ssim, void* stream) {
  return guarded([&] {
    if (C < 1 || H <= 10 || W <= 10) return fail(DN_ERR_ARG, "need C >= 1 and H, W > 10");
    if (!a || !b || !part || !ssim) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_ssim(a, b, C, H, W, hwc, static_cast<double*>(part), ssim,
                                  (hipStream_t)stream),
                      "dn_ssim_u8");
  });
}

dn_status dn_l1_mean(const float* a, const float* b, int64_t n, void* part, double* l1,
                     void* stream) {
  return guarded([&] {
    if (n < 1) return fail(DN_ERR_ARG, "n >= 1 required");
    if (!a || !b || !part || !l1) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_l1(a, b, n, static_cast<double*>(part), l1, (hipStream_t)stream),
                      "dn_l1_mean");
  });
}

dn_status dn_l1_mean_batched(const float* a, const float* b, int64_t P, int64_t n, double* l1,
                             void* stream) {
  return guarded([&] {
    if (P < 0 || n < 1) return fail(DN_ERR_ARG, "P >= 0 and n >= 1 required");
    if (P == 0) return DN_OK;
    if (P > 0x7fffffffL) return fail(DN_ERR_ARG, "P too large");
    if (!a || !b || !l1) return fail(DN_ERR_ARG, "null argument");
    return hip_status(launch_l1_batched(a, b, P, n, l1, (hipStream_t)stream),
                      "dn_l1_mean_batched");
  });
}

dn_status dn_iq_iou_u8(const uint8_t* pred, const uint8_t* clean, int C, int H, int W, double t1,
                       double t2, void* part, int64_t* counts6, void* stream) {
  return guarded([&] {
    if (!pred || !clean || !part || !counts6) return fail(DN_ERR_ARG, "null argument");
    if (C < 1 || C > 65536 || H < 1 || W < 1)
      return fail(DN_ERR_ARG, "need 1 <= C <= 65536 and H, W >= 1");
    if (std::isnan(t1) || std::isnan(t2) || t1 > t2)
      return fail(DN_ERR_ARG, "need t1 <= t2, neither NaN");
    return hip_status(launch_iq_iou(pred, clean, C, (long)H * W, t1, t2, part, counts6,
                                    (hipStream_t)stream),
                      "dn_iq_iou_u8");
  });
}

dn_status dn_hann_blend(const float* pred, const float* hann, const int* ys, const int* xs, int ny,
                        int nx, int C, int H, int W, int P, float* out, void* stream) {
  return guarded([&] {
    if (!pred || !hann || !ys || !xs || !out) return fail(DN_ERR_ARG, "null argument");
    if (ny < 1 || nx < 1 || C < 1 || P < 1 || H < P || W < P)
      return fail(DN_ERR_ARG, "need ny, nx, C >= 1 and H, W >= patch_size >= 1");
    return hip_status(launch_hann_blend(pred, hann, ys, xs, ny, nx, C, H, W, P, out,
                                        (hipStream_t)stream),
                      "dn_hann_blend");
  });
}

}  // extern "C"
