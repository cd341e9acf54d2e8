// extern "C" boundary (include/denoise_hip.h): the op-level entry points (NHWC) that the tests and
// the tiled-inference path use: convolutions, 2x2 deconvolutions and pooling on every kernel family.
#include <string>

#include "capi_common.h"

using namespace dn;

namespace {

dn_status need_pack(void* ws, size_t have, size_t need) {
  if (need == 0) return fail(DN_ERR_ARG, "unsupported channel count for this kernel build");
  if (!ws || have < need) return fail(DN_ERR_WORKSPACE, "pack scratch smaller than *_pack_size()");
  return DN_OK;
}

}  // namespace

extern "C" {

size_t dn_conv2d_pack_size(int Cin, int Cout, int ksize, int backward_data) {
  return guarded_query([&]() -> size_t {
    if ((ksize != 1 && ksize != 3) || Cin < 1 || Cout < 1) return 0;
    const long n = backward_data ? conv_dgrad_pack_size(Cout, Cin, ksize)
                                 : conv_fwd_pack_size(Cin, Cout, ksize);
    return n < 0 ? 0 : sizeof(float) * (size_t)n;
  });
}

size_t dn_deconv2x2_pack_size(int Cin, int Cout, int backward_data) {
  return guarded_query([&]() -> size_t {
    if (Cin < 1 || Cout < 1) return 0;
    const long n =
        backward_data ? deconv_dgrad_pack_size(Cout, Cin) : deconv_fwd_pack_size(Cin, Cout);
    return n < 0 ? 0 : sizeof(float) * (size_t)n;
  });
}

dn_status dn_conv2d_forward(const float* x, int x_stride, int N, int H, int W, int Cin,
                            const float* w, const float* b, int Cout, int ksize, int act, float* y,
                            int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
    if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || x_stride < Cin || y_stride < Cout)
      return fail(DN_ERR_ARG, "bad shape");
    if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_pack_size(Cin, Cout, ksize, 0)))
      return st;
    hipStream_t s = (hipStream_t)stream;
    float* wp = static_cast<float*>(pack_ws);
    hipError_t e = pack_conv_fwd(w, Cin, Cout, ksize, wp, s);
    if (e == hipSuccess) {
      // (dn_profile_ops: the record brackets the GEMM launch alone, so its label is the GEMM's)
      const OpTimer timer(s, ksize == 3 ? "fwd3" : "fwd1",
                          2.0 * Cin * Cout * ksize * ksize * N * H * W, Cin, Cout, H, W, N);
      e = conv_forward(View{const_cast<float*>(x), x_stride, 0}, N, H, W, Cin, wp, b, Cout, ksize,
                       act, View{y, y_stride, 0}, OUT_NHWC, s);
    }
    return hip_status(e, "dn_conv2d_forward");
  });
}

size_t dn_conv2d_bf16_pack_size(int Cin, int Cout) {
  return guarded_query([&]() -> size_t {
    if (Cin < 1 || Cout < 1) return 0;
    const long e = bf16_pack_elems(Cin, Cout);
    return e < 0 ? 0 : 2 * (size_t)e;
  });
}

dn_status dn_conv2d_forward_bf16(const float* x, int x_stride, int N, int H, int W, int Cin,
                                 const float* w, const float* b, int Cout, int act, float* y,
                                 int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || x_stride < Cin || y_stride < Cout || (Cout & 3) ||
        (y_stride & 3))
      return fail(DN_ERR_ARG, "bad shape (Cout and y_stride must be multiples of 4)");
    if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_bf16_pack_size(Cin, Cout)))
      return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = launch_pack_bf16(conv_fwd_view(w, Cin, 3), Cin, Cout, pack_ws, s);
    if (e == hipSuccess) {
      FwdArgs a = fwd_args(View{const_cast<float*>(x), x_stride, 0}, N, H, W, Cin, Cout,
                           View{y, y_stride, 0}, OUT_NHWC);
      a.wp = static_cast<const float*>(pack_ws); a.bias = b; a.epi = act ? EPI_BIAS_ACT : EPI_BIAS;
      const OpTimer timer(s, "fwd3", 2.0 * Cin * Cout * 9 * N * H * W, Cin, Cout, H, W, N);
      e = launch_fwd_bf16(a, s);
    }
    return hip_status(e, "dn_conv2d_forward_bf16");
  });
}

size_t dn_conv2d_x6_pack_size(int Cin, int Cout, int backward_data) {
  return guarded_query([&]() -> size_t {
    if (Cin < 1 || Cout < 1) return 0;
    const long e = backward_data ? x6_pack_elems(Cout, Cin, x6_dgrad_zc(Cin))
                                 : x6_pack_elems(Cin, Cout, 0);
    return e < 0 ? 0 : 2 * (size_t)e;
  });
}

dn_status dn_conv2d_forward_x6(const float* x, int x_stride, int N, int H, int W, int Cin,
                               const float* w, const float* b, int Cout, int act, float* y,
                               int y_stride, void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
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
  });
}

size_t dn_upconv3_x6_pack_size(void) { return guarded_query([] { return (size_t)UPC_BYTES; }); }

dn_status dn_upconv3_forward_x6(const float* xlo, int xlo_stride, int N, int h, int w,
                                const float* img, int C, const float* w3, const float* b3,
                                const float* wd, const float* bd, float* y, int y_stride,
                                void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
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
      FwdArgs a = fwd_args(View{const_cast<float*>(xlo), xlo_stride, 0}, h, w, N, 2 * h, 2 * w,
                           96 + C, 96, View{y, y_stride, 0}, OUT_NHWC);
      a.wp = static_cast<const float*>(pack_ws); a.in_t1 = img; a.epi = EPI_BIAS_ACT;
      const OpTimer timer(s, "fwd3", 2.0 * (96 + C) * 96 * 9 * N * 4 * h * w, 96 + C, 96, 2 * h,
                          2 * w, N);
      e = launch_upconv3_x6(a, s);
    }
    return hip_status(e, "dn_upconv3_forward_x6");
  });
}

dn_status dn_conv2d_backward_data_x6(const float* dz, int N, int H, int W, int Cout,
                                     const float* w, int Cin, const float* mask, int mask_stride,
                                     int accumulate, float* dx, int dx_stride, void* pack_ws,
                                     size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!dz || !w || !dx) return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || Cout < 1 || dx_stride < Cin)
      return fail(DN_ERR_ARG, "bad shape");
    if (mask && accumulate) return fail(DN_ERR_ARG, "mask and accumulate are exclusive");
    const size_t need = dn_conv2d_x6_pack_size(Cin, Cout, 1);
    if (need == 0) return fail(DN_ERR_ARG, "bf16x6 data gradient: unsupported Cin");
    if (dn_status st = need_pack(pack_ws, pack_bytes, need)) return st;
    hipStream_t s = (hipStream_t)stream;
    const int zc = x6_dgrad_zc(Cin);
    const int tail =
        x6_image_mode(N, H, W, Cout, Cin, zc,
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
  });
}

dn_status dn_conv2d_backward_data(const float* dz, int N, int H, int W, int Cout, const float* w,
                                  int Cin, int ksize, const float* mask, int mask_stride,
                                  int accumulate, float* dx, int dx_stride, void* pack_ws,
                                  size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!dz || !w || !dx) return fail(DN_ERR_ARG, "null argument");
    if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
    if (N < 1 || H < 1 || W < 1 || Cout < 1 || dx_stride < Cin)
      return fail(DN_ERR_ARG, "bad shape");
    if (mask && accumulate) return fail(DN_ERR_ARG, "mask and accumulate are exclusive");
    if (dn_status st = need_pack(pack_ws, pack_bytes, dn_conv2d_pack_size(Cin, Cout, ksize, 1)))
      return st;
    const int epi = mask ? EPI_MASK : (accumulate ? EPI_ACCUM : EPI_PLAIN);
    hipStream_t s = (hipStream_t)stream;
    float* wp = static_cast<float*>(pack_ws);
    hipError_t e = pack_conv_dgrad(w, Cin, Cin, Cout, ksize, wp, s);
    if (e == hipSuccess) {
      const OpTimer timer(s, ksize == 3 ? "dgrad3" : "dgrad1",
                          2.0 * Cout * Cin * ksize * ksize * N * H * W, Cout, Cin, H, W, N);
      e = conv_dgrad(View{const_cast<float*>(dz), Cout, 0}, N, H, W, Cout, wp, Cin, ksize, epi,
                     View{const_cast<float*>(mask), mask_stride, 0}, View{dx, dx_stride, 0}, s);
    }
    return hip_status(e, "dn_conv2d_backward_data");
  });
}

size_t dn_conv2d_wgrad_slab_size(int N, int H, int W, int Cin, int Cout, int ksize) {
  return guarded_query([&] {
    const int mode = ksize == 3 ? W_C3 : W_C1;
    return sizeof(float) * (64 + (size_t)wgrad_size(mode, N, H, W, Cin, Cout, false).floats);
  });
}

dn_status dn_conv2d_backward_weight(const float* dz, const float* x, int x_stride, int N, int H,
                                    int W, int Cin, int Cout, int ksize, float* dwb, void* slab,
                                    void* stream) {
  return guarded([&] {
    if (!dz || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
    if (ksize != 1 && ksize != 3) return fail(DN_ERR_ARG, "ksize must be 1 or 3");
    const int mode = ksize == 3 ? W_C3 : W_C1;
    if (!wgrad_supported(mode, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
    if (mode == W_C1 && Cin > 96) return fail(DN_ERR_ARG, "1x1 wgrad supports Cin <= 96");
    return wgrad_run(wgrad_route(wgrad_shape(mode, N, H, W, Cin, Cout, Cout, 0, x_stride, 0)), dz,
                     x, dwb, static_cast<float*>(slab), nullptr, (hipStream_t)stream);
  });
}

dn_status dn_conv2d_backward_weight_x6(const float* dz, const float* x, int x_stride, int N,
                                       int H, int W, int Cin, int Cout, float* dwb, void* slab,
                                       void* stream) {
  return guarded([&] {
    if (!dz || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
    if (!wgrad_supported(W_C3, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
    // (dn_profile_ops: wgrad_run() takes the "wgrad3" record itself)
    return wgrad_run(
        wgrad_route(wgrad_shape(W_C3, N, H, W, Cin, Cout, Cout, 0, x_stride, 0, true)), dz, x, dwb,
        static_cast<float*>(slab), nullptr, (hipStream_t)stream);
  });
}

dn_status dn_deconv2x2_forward(const float* x, int N, int H, int W, int Cin, const float* w,
                               const float* b, int Cout, float* y, int y_stride, int y_off,
                               void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!x || !w || !b || !y) return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || y_stride < y_off + Cout)
      return fail(DN_ERR_ARG, "bad shape");
    if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_pack_size(Cin, Cout, 0)))
      return st;
    hipStream_t s = (hipStream_t)stream;
    float* wp = static_cast<float*>(pack_ws);
    hipError_t e = pack_deconv_fwd(w, Cin, Cout, wp, s);
    if (e == hipSuccess) {
      const OpTimer timer(s, "deconv", 2.0 * N * H * W * Cin * Cout * 4, Cin, Cout, H, W, N);
      e = deconv_forward(View{const_cast<float*>(x), Cin, 0}, N, H, W, Cin, wp, b, Cout,
                         View{y, y_stride, y_off}, s);
    }
    return hip_status(e, "dn_deconv2x2_forward");
  });
}

size_t dn_deconv2x2_x6_pack_size(void) {
  return guarded_query([] { return 4 * sizeof(uint16_t) * (size_t)X6_HEAD_BF; });
}

dn_status dn_deconv2x2_forward_x6(const float* x, int N, int H, int W, const float* w,
                                  const float* b, float* y, int y_stride, int y_off, void* pack_ws,
                                  size_t pack_bytes, void* stream) {
  return guarded([&] {
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
  });
}

dn_status dn_deconv2x2_backward_data_x6(const float* dy, int dy_stride, int N, int H, int W,
                                        const float* w, const float* mask, float* dx,
                                        void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!dy || !w || !dx) return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || dy_stride < 96 || (dy_stride & 3))
      return fail(DN_ERR_ARG, "bad shape");
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
  });
}

dn_status dn_deconv2x2_backward_data(const float* dy, int dy_stride, int N, int H, int W, int Cout,
                                     const float* w, int Cin, const float* mask, float* dx,
                                     void* pack_ws, size_t pack_bytes, void* stream) {
  return guarded([&] {
    if (!dy || !w || !dx) return fail(DN_ERR_ARG, "null argument");
    if (N < 1 || H < 1 || W < 1 || Cout < 1 || dy_stride < Cout)
      return fail(DN_ERR_ARG, "bad shape");
    if (dn_status st = need_pack(pack_ws, pack_bytes, dn_deconv2x2_pack_size(Cin, Cout, 1)))
      return st;
    hipStream_t s = (hipStream_t)stream;
    float* wp = static_cast<float*>(pack_ws);
    hipError_t e = pack_deconv_dgrad(w, Cout, Cin, wp, s);
    if (e == hipSuccess) {
      const OpTimer timer(s, "deconv_dgrad", 2.0 * N * H * W * Cin * Cout * 4, Cout, Cin, H, W, N);
      e = deconv_dgrad(View{const_cast<float*>(dy), dy_stride, 0}, N, H, W, Cout, wp, Cin,
                       View{const_cast<float*>(mask), Cin, 0}, mask ? EPI_MASK : EPI_PLAIN,
                       View{dx, Cin, 0}, s);
    }
    return hip_status(e, "dn_deconv2x2_backward_data");
  });
}

size_t dn_deconv2x2_wgrad_slab_size(int N, int H, int W, int Cin, int Cout) {
  return guarded_query([&] {
    return sizeof(float) * (64 + (size_t)wgrad_size(W_UP2, N, H, W, Cin, Cout, false).floats);
  });
}

dn_status dn_deconv2x2_backward_weight(const float* dy, int dy_stride, const float* x, int N, int H,
                                       int W, int Cin, int Cout, float* dwb, void* slab,
                                       void* stream) {
  return guarded([&] {
    if (!dy || !x || !dwb || !slab) return fail(DN_ERR_ARG, "null argument");
    if (!wgrad_supported(W_UP2, Cout)) return fail(DN_ERR_ARG, "unsupported Cout");
    return wgrad_run(wgrad_route(wgrad_shape(W_UP2, N, H, W, Cin, Cout, dy_stride, 0, Cin, 0)), dy,
                     x, dwb, static_cast<float*>(slab), nullptr, (hipStream_t)stream);
  });
}

dn_status dn_maxpool2x2_forward(const float* x, int N, int H, int W, int C, float* y, int y_stride,
                                int y_off, void* stream) {
  return guarded([&] {
    if (!x || !y) return fail(DN_ERR_ARG, "null argument");
    if ((H & 1) || (W & 1) || (C & 3) || (y_stride & 3) || (y_off & 3))
      return fail(DN_ERR_ARG, "H, W even and C, y_stride, y_off multiples of 4 required");
    return hip_status(launch_pool_fwd(x, N, H, W, C, y, y_stride, y_off, (hipStream_t)stream),
                      "dn_maxpool2x2_forward");
  });
}

dn_status dn_maxpool2x2_backward(const float* x, int N, int H, int W, int C, const float* dy,
                                 int dy_stride, int dy_off, int act, float* dx, void* stream) {
  return guarded([&] {
    if (!x || !dy || !dx) return fail(DN_ERR_ARG, "null argument");
    if ((H & 1) || (W & 1) || (C & 3) || (dy_stride & 3) || (dy_off & 3))
      return fail(DN_ERR_ARG, "H, W even and C, dy_stride, dy_off multiples of 4 required");
    return hip_status(launch_pool_bwd(x, N, H, W, C, dy, dy_stride, dy_off, act, dx,
                                      (hipStream_t)stream),
                      "dn_maxpool2x2_backward");
  });
}

}  // extern "C"
