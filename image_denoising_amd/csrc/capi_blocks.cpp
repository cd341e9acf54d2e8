// extern "C" boundary (include/denoise_hip.h): ImprovedUNet's building blocks as ops, the launch
// sequences its executor runs: GroupNorm and the blocked weight gradient.
#include <string>

#include "capi_common.h"
#include "iunet.h"

using namespace dn;

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

extern "C" {

size_t dn_groupnorm_scratch_size(int N, int H, int W, int C) {
  return guarded_query([&]() -> size_t {
    if (!gn_shape_ok(N, H, W, C, 1)) return 0;
    return GnScratch(N, H, W, C).bytes;
  });
}

dn_status dn_groupnorm_forward(const float* z, int z_stride, int z_off, const float* res,
                               int res_stride, int res_off, float* y, int y_stride, int y_off,
                               int N, int H, int W, int C, int G, const float* gamma,
                               const float* beta, int act, float* stats, void* scratch,
                               size_t scratch_bytes, void* stream) {
  return guarded([&] {
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
  });
}

dn_status dn_groupnorm_backward(const float* dy, int dy_stride, int dy_off, const float* z,
                                int z_stride, int z_off, float* dz, int dz_stride, int dz_off,
                                int N, int H, int W, int C, int G, const float* gamma,
                                const float* stats, float* dgamma, float* dbeta, void* scratch,
                                size_t scratch_bytes, void* stream) {
  return guarded([&] {
    if (!gamma || !stats || !dgamma || !dbeta || !scratch)
      return fail(DN_ERR_ARG, "null argument");
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
  });
}

size_t dn_conv2d_wgrad_blocked_slab_size(int N, int H, int W, int Cin, int Cout, int ksize) {
  return guarded_query([&]() -> size_t {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3)) return 0;
    const int mode = ksize == 3 ? W_C3 : W_C1;
    return sizeof(float) * (64 + (size_t)wgrad_size(mode, N, H, W, Cin, Cout, true).floats);
  });
}

dn_status dn_conv2d_backward_weight_blocked(const float* g, int g_stride, int g_off,
                                            const float* x, int x_stride, int x_off, int N, int H,
                                            int W, int Cin, int Cout, int ksize, int bias,
                                            int precision, float* dwb, void* slab, void* stream) {
  return guarded([&] {
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
  });
}

}  // extern "C"
