// RESNET orchestration (arch_unet.py:263-409): parameter layout (reference state_dict order),
// workspace plan and the forward / backward launch sequences, in the shape of unet.cpp: a plan,
// the kernel routes of a pass resolved once, one pack launch, then the run.  Every layer runs at
// the input resolution (any H, W >= 1); the concatenations are placements into strided slices.
#include "resnet.h"

#include <cstdlib>

namespace dn {

static const char* kResNames[R_NL] = {
    "enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5", "enc_conv6",
    "up5.deconv", "dec_conv5a", "dec_conv5b", "dec_conv4a", "dec_conv4b", "dec_conv3a",
    "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "nin_a", "nin_b",
    "nin_c"};

const char* res_layer_name(int i) { return (i >= 0 && i < R_NL) ? kResNames[i] : ""; }

bool res_build_params(const dn_unet_cfg& c, ResParamLayout& P, std::string& err) {
  const int C = c.in_nc, OC = c.out_nc, nf = c.n_feature;
  if (C < 1 || C > 4) {
    err = "in_nc must be in [1,4]";
    return false;
  }
  // (torch would broadcast a one-channel input or output over the other; not built)
  if (OC != C) {
    err = "RESNET adds its input to its output: out_nc must equal in_nc";
    return false;
  }
  if (nf != 48) {
    err = "n_feature must be 48 (kernel tiles are instantiated for the reference width)";
    return false;
  }
  auto conv = [&](int i, int cout, int cin, int k) { P.L[i] = {cout, cin, k, false, 0, 0}; };
  conv(R_ENC0, nf, C, 3);
  for (int i = R_ENC1; i <= R_ENC6; ++i) conv(i, nf, nf, 3);
  P.L[R_UP5] = {nf, nf, 2, true, 0, 0};
  conv(R_D5A, 2 * nf, 2 * nf, 3);
  conv(R_D5B, 2 * nf, 2 * nf, 3);
  for (int i = R_D4A; i <= R_D2A; i += 2) {
    conv(i, 2 * nf, 3 * nf, 3);
    conv(i + 1, 2 * nf, 2 * nf, 3);
  }
  conv(R_D1A, 96, 2 * nf + C, 3);
  conv(R_D1B, 96, 96, 3);
  conv(R_NINA, 96, 96, 1);
  conv(R_NINB, 96, 96, 1);
  conv(R_NINC, OC, 96, 1);
  long off = 0;
  for (int i = 0; i < R_NL; ++i) {
    Layer& L = P.L[i];
    L.wcount = (long)L.cout * L.cin * L.k * L.k;
    L.woff = off;
    off += L.wcount + L.cout;
  }
  P.total = off;
  return true;
}

// channels of the data gradient layer i's backward produces (dec_conv1a: only [d2b] of [d2b | x])
static int res_dgrad_nout(const ResPlan& p, int i) { return i == R_D1A ? 2 * p.nf : p.P.L[i].cin; }
// dec_conv{k}a / dec_conv{k}b of the concat level k = 2..5
static int res_da(int k) { return R_D5A + 2 * (5 - k); }

bool res_build_plan(const dn_unet_cfg& c, int N, int H, int W, bool bwd, ResPlan& p,
                    std::string& err) {
  if (N < 1 || H < 1 || W < 1) {
    err = "N >= 1 and H, W >= 1";
    return false;
  }
  if ((long)N * H * W >= (1L << 31) / 160) {
    err = "N * H * W too large for the 32-bit pixel offsets of the strided views";
    return false;
  }
  if (!res_build_params(c, p.P, err)) return false;
  p.N = N; p.H = H; p.W = W; p.C = c.in_nc; p.nf = c.n_feature;
  const int nf = p.nf;
  const long px = (long)N * H * W;
  long off = 0;
  auto alloc_f = [&](long n) {
    long o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  auto alloc = [&](int ch) { return alloc_f(px * ch); };
  p.c1k = 2 * nf + p.C;
  p.c1kp = (p.c1k + 3) / 4 * 4;
  p.c1s = p.c1kp;
  p.c1 = alloc(p.c1s);
  p.a0 = alloc(nf);
  p.a5 = alloc(nf);
  for (int k = 2; k <= 5; ++k) {
    p.cs[k] = (k == 5) ? 2 * nf : 3 * nf;
    p.c[k] = alloc(p.cs[k]);
    p.da[k] = alloc(2 * nf);
  }
  p.d1a = alloc(96);
  p.d1b = alloc(96);
  p.na = p.nb = -1;  // written only for a backward
  for (int i = 0; i < R_NL; ++i) {
    const Layer& L = p.P.L[i];
    p.packF[i] = p.packX[i] = -1;
    if (i == R_ENC0 || i == R_UP5 || i >= R_NINA) continue;  // direct kernel / unused / the head
    const long n = conv_fwd_pack_size(L.cin, L.cout, L.k);
    const long e = x6_pack_elems(L.cin, L.cout, 0);
    if (n < 0 || e < 0) {
      err = std::string("no forward kernel tile for layer ") + kResNames[i];
      return false;
    }
    p.packF[i] = alloc_f(n);
    p.packX[i] = alloc_f((e + 1) / 2);
  }
  p.packH = alloc_f(2 * HEAD_LW > X6_HEAD_BF ? 2 * HEAD_LW : X6_HEAD_BF);
  p.fwd_floats = off;
  if (bwd) {
    p.na = alloc(96);
    p.nb = alloc(96);
    p.g_nb = alloc(96);
    p.g_na = alloc(96);
    p.g_d1b = alloc(96);
    p.g_d1a = alloc(96);
    p.g_c1 = alloc(2 * nf);
    for (int k = 2; k <= 5; ++k) {
      p.g_c[k] = alloc(p.cs[k]);
      p.g_da[k] = alloc(2 * nf);
    }
    for (int j = 1; j <= 4; ++j) p.g_a[j] = alloc(nf);
    p.g_a5 = alloc(nf);
    p.g_a0 = alloc(nf);
    p.g_t = alloc(nf);
    p.xin = alloc(p.C);
    p.dyt = alloc(p.C);
    for (int i = 0; i < R_NL; ++i) {
      const Layer& L = p.P.L[i];
      p.packB[i] = p.packXB[i] = -1;
      if (i == R_ENC0 || i == R_UP5 || i >= R_NINA) continue;
      const int nout = res_dgrad_nout(p, i);
      const long n = conv_dgrad_pack_size(L.cout, nout, L.k);
      const long e = x6_pack_elems(L.cout, nout, x6_dgrad_zc(nout));
      if (n < 0 || e < 0) {
        err = std::string("no data-gradient kernel tile for layer ") + kResNames[i];
        return false;
      }
      p.packB[i] = alloc_f(n);
      p.packXB[i] = alloc_f((e + 1) / 2);
    }
    p.packHB = alloc_f(2 * HEAD_LW > X6_HEAD_BF ? 2 * HEAD_LW : X6_HEAD_BF);
    p.zeros = alloc_f(64);
    for (int i = 0; i < R_NL; ++i) {
      const Layer& L = p.P.L[i];
      p.splits[i] = 0;
      p.slab[i] = -1;
      if (i == R_UP5) continue;  // no gradient: its range of dparams is zeroed
      const int mode = L.k == 3 ? W_C3 : W_C1;
      const int sp = i == R_ENC0 ? enc0_wgrad_splits(N, H, W)
                     : i == R_NINC ? wgrad_thin_splits(px)
                                   : wgrad_splits(mode, N, H, W, i == R_D1A ? 2 * nf : L.cin, L.cout);
      p.splits[i] = sp;
      long need = (i == R_ENC0 || i == R_D1A || i == R_NINC)
                      ? (long)sp * (L.wcount + L.cout)
                      : wgrad_slab_floats(mode, N, H, W, L.cin, L.cout);
      if (i == R_NINC) {  // also the rows nin_b's k_wgrad1p<., GNB> writes nin_c's gradient into
        const long s1 = wgrad1_splits(W_C1, N, H, W);
        if (s1 * (L.wcount + L.cout) > need) need = s1 * (L.wcount + L.cout);
      }
      if (i == R_D1A) need += (long)enc0_wgrad_splits(N, H, W) * 96 * p.C * 9;  // input slice
      p.slab[i] = alloc_f(64 + need);
    }
  }
  p.total_floats = off;
  p.with_bwd = bwd;
  return true;
}

#define DN_TRY(x)                                                         \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      set_error(std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_)); \
      return DN_ERR_HIP;                                                  \
    }                                                                     \
  } while (0)

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
namespace {

enum ResKind { RK_F32, RK_X6 };  // conv on the fp32 kernel (packF / packB) | the bf16x6 kernels
struct ResRoute { int kind; long img; int tail; int zc; long wp_z; };
struct ResRoutes {
  ResRoute r[R_NL];  // enc_conv1 .. dec_conv1b
  bool head_x6;      // the nin head (forward) / its data gradients (backward) in bf16x6
};

ResRoutes res_fwd_routes(const ResPlan& p, int prec) {
  const bool x6 = prec == DN_PREC_FP32_X6;
  ResRoutes R{};
  for (int i = R_ENC1; i <= R_D1B; ++i) {
    if (i == R_UP5) continue;
    const Layer& L = p.P.L[i];
    ResRoute& r = R.r[i];
    if (x6 && p.packX[i] >= 0) {
      // dec_conv1a reads [d2b | x | zero pad]: the pad channels as reduction channels with zero
      // packed weights keep K % 4 == 0 (as the UNet's dec_conv1a)
      r.kind = RK_X6; r.img = p.packX[i];
      r.tail = x6_image_mode(p.N, p.H, p.W, i == R_D1A ? p.c1kp : L.cin, L.cout, 0, true);
    } else {
      r.kind = RK_F32; r.img = p.packF[i];
    }
  }
  R.head_x6 = x6 && p.C <= X6_HEAD_OCMAX;
  return R;
}

ResRoutes res_bwd_routes(const ResPlan& p, int prec) {
  const bool x6 = prec == DN_PREC_FP32_X6;
  ResRoutes B{};
  for (int i = R_ENC1; i <= R_D1B; ++i) {
    if (i == R_UP5) continue;
    const Layer& L = p.P.L[i];
    ResRoute& r = B.r[i];
    if (x6 && p.packXB[i] >= 0) {
      const int nout = res_dgrad_nout(p, i);
      r.kind = RK_X6; r.img = p.packXB[i];
      r.zc = x6_dgrad_zc(nout);
      r.wp_z = x6_wp_z(L.cout, nout, r.zc);
      r.tail = x6_image_mode(p.N, p.H, p.W, L.cout, nout, r.zc, true);
    } else {
      r.kind = RK_F32; r.img = p.packB[i];
    }
  }
  B.head_x6 = x6 && p.C <= X6_HEAD_BWD_OCMAX;
  return B;
}

dn_status res_pack_forward(const ResPlan& p, const ResRoutes& R, const float* prm, float* ws,
                           hipStream_t s) {
  PackBatch pb;
  auto add = [&](bool ok, const PackJob& j) { return ok ? pack_add(pb, j, s) : hipErrorInvalidValue; };
  for (int i = R_ENC1; i <= R_D1B; ++i) {
    if (i == R_UP5) continue;
    const Layer& L = p.P.L[i];
    const ResRoute& r = R.r[i];
    const float* w = prm + L.woff;
    PackJob j;
    if (r.kind == RK_X6)
      DN_TRY(add(pack_job_x6(conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 0, ws + r.img, r.tail, j), j));
    else
      DN_TRY(add(pack_job(G_C3, conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 1, ws + r.img, 0, 0, j), j));
  }
  const float* wa = prm + p.P.L[R_NINA].woff;
  const float* wb = prm + p.P.L[R_NINB].woff;
  if (R.head_x6)
    DN_TRY(add(true, pack_job_head_x6(wa, wb, ws + p.packH)));
  else
    DN_TRY(launch_pack_head(conv_fwd_view(wa, 96, 1), conv_fwd_view(wb, 96, 1), ws + p.packH, s, &pb));
  DN_TIMED(s, "pack", 0, 0, 0, 0, 0, 0, pack_flush(pb, s));
  return DN_OK;
}

dn_status res_run_forward(const ResPlan& p, const ResRoutes& R, const float* prm, const float* x,
                          float* y, float* ws, hipStream_t s) {
  const int N = p.N, H = p.H, W = p.W, nf = p.nf, C = p.C;
  auto Bs = [&](int i) { return prm + p.P.L[i].woff + p.P.L[i].wcount; };
  auto V = [&](long off, int stride, int coff = 0) { return View{ws + off, stride, coff}; };
  // 3x3 conv layer i (bias + LeakyReLU) on the kernel and image of its route
  auto conv = [&](int i, const View& in, const View& out) -> hipError_t {
    const Layer& L = p.P.L[i];
    const ResRoute& r = R.r[i];
    const OpTimer timer(s, "fwd3", 2.0 * N * H * W * L.cin * L.cout * 9, L.cin, L.cout, H, W, N);
    if (r.kind == RK_F32)
      return conv_forward(in, N, H, W, L.cin, ws + r.img, Bs(i), L.cout, 3, 1, out, OUT_NHWC, s);
    FwdArgs a = fwd_args(in, N, H, W, i == R_D1A ? p.c1kp : L.cin, L.cout, out, OUT_NHWC);
    a.wp = ws + r.img; a.bias = Bs(i); a.epi = EPI_BIAS_ACT;
    a.x6_tail = r.tail;
    return launch_fwd_x6(a, s);
  };
  // enc_conv0; x -> channels [2nf, c1kp) of c1 (zero padded), and the NCHW copy for the backward
  DN_TIMED(s, "enc0", 2.0 * N * H * W * C * nf * 9, C, nf, H, W, N,
           launch_enc0_fwd(x, N, C, H, W, prm + p.P.L[R_ENC0].woff, Bs(R_ENC0), ws + p.a0,
                           ws + p.c1, p.c1s, 2 * nf, p.c1kp, p.with_bwd ? ws + p.xin : nullptr, s));
  // a1..a4 into the skip slices of c2..c5, a5 on its own, a6 into c5[0:nf]
  const View skip[5] = {V(p.a0, nf), V(p.c[2], p.cs[2], 2 * nf), V(p.c[3], p.cs[3], 2 * nf),
                        V(p.c[4], p.cs[4], 2 * nf), V(p.c[5], p.cs[5], nf)};
  for (int j = 1; j <= 4; ++j) DN_TRY(conv(R_ENC0 + j, skip[j - 1], skip[j]));
  DN_TRY(conv(R_ENC5, skip[4], V(p.a5, nf)));
  DN_TRY(conv(R_ENC6, V(p.a5, nf), V(p.c[5], p.cs[5], 0)));
  // dec_conv{k}a on c_k, dec_conv{k}b into c_{k-1}[0:2nf] (k = 2: into c1)
  for (int k = 5; k >= 2; --k) {
    DN_TRY(conv(res_da(k), V(p.c[k], p.cs[k]), V(p.da[k], 2 * nf)));
    DN_TRY(conv(res_da(k) + 1, V(p.da[k], 2 * nf),
                k > 2 ? V(p.c[k - 1], p.cs[k - 1], 0) : V(p.c1, p.c1s, 0)));
  }
  DN_TRY(conv(R_D1A, V(p.c1, p.c1s), V(p.d1a, 96)));
  DN_TRY(conv(R_D1B, V(p.d1a, 96), V(p.d1b, 96)));
  // nin_a -> nin_b -> nin_c + x in one launch
  HeadArgs h{};
  h.wp = ws + p.packH;
  h.ba = Bs(R_NINA); h.bb = Bs(R_NINB);
  h.wc = prm + p.P.L[R_NINC].woff; h.bc = Bs(R_NINC); h.oc = C;
  h.y = y; h.res = x;
  if (p.with_bwd) { h.na = ws + p.na; h.nb = ws + p.nb; }
  const FwdArgs a = fwd_args(V(p.d1b, 96), N, H, W, 96, 96, View{nullptr, 0, 0}, OUT_NHWC);
  DN_TIMED(s, "head", 2.0 * N * H * W * 96 * (2 * 96 + C), 96, C, H, W, N,
           R.head_x6 ? launch_nin_head_x6(a, h, ws + p.packH, s) : launch_nin_head(a, h, s));
  return DN_OK;
}

}  // namespace

dn_status resnet_forward(const ResPlan& p, const float* prm, const float* x, float* y, float* ws,
                         hipStream_t s, int prec) {
  const StreamDeviceGuard device_guard(s);
  const ResRoutes R = res_fwd_routes(p, prec);
  const dn_status st = res_pack_forward(p, R, prm, ws, s);
  return st != DN_OK ? st : res_run_forward(p, R, prm, x, y, ws, s);
}

// ------------------------------------------------------------------------------------
// backward: the forward's autograd graph in reverse.  A data gradient masks with the layer's input
// (the producer's activation; a concat buffer masks both of its parts at once).  a1..a4 receive
// two gradients: the skip slice of dec_conv{5..2}a's data gradient, and enc_conv{j+1}'s, which is
// masked into g_t and summed with the slice into the compact g_a[j] (k_add_slice).  Weight
// gradients on the side stream, slab reductions on the reduction stream (DN_BWD_STREAMS=0: one
// stream), as the UNet backward.
// ------------------------------------------------------------------------------------
dn_status resnet_backward(const ResPlan& p, const float* prm, const float* dy, float* dprm,
                          float* dx, float* ws, hipStream_t s, int prec) {
  const StreamDeviceGuard device_guard(s);
  const bool x6 = prec == DN_PREC_FP32_X6;
  const int N = p.N, H = p.H, W = p.W, nf = p.nf, C = p.C, OC = p.C;
  const long px = (long)N * H * W;
  auto G = [&](int i) { return dprm + p.P.L[i].woff; };
  auto V = [&](long off, int stride, int coff = 0) { return View{ws + off, stride, coff}; };
  auto SL = [&](int i) { return ws + p.slab[i]; };
  const ResRoutes B = res_bwd_routes(p, prec);
  {  // every data-gradient image, the head's, the zero padding: one launch
    PackBatch pb;
    auto add = [&](bool ok, const PackJob& j) { return ok ? pack_add(pb, j, s) : hipErrorInvalidValue; };
    for (int i = R_ENC1; i <= R_D1B; ++i) {
      if (i == R_UP5) continue;
      const Layer& L = p.P.L[i];
      const ResRoute& r = B.r[i];
      const float* w = prm + L.woff;
      const int nout = res_dgrad_nout(p, i);
      PackJob j;
      if (r.kind == RK_X6)
        DN_TRY(add(pack_job_x6(conv_dgrad_view(w, L.cin, 3), L.cout, nout, r.zc, ws + r.img, r.tail, j), j));
      else
        DN_TRY(add(pack_job(G_C3, conv_dgrad_view(w, L.cin, 3), L.cout, nout, 1, ws + r.img, 0, 0, j), j));
    }
    if (B.head_x6)
      DN_TRY(add(true, pack_job_head_bwd_x6(prm + p.P.L[R_NINA].woff, prm + p.P.L[R_NINB].woff,
                                            ws + p.packHB)));
    else
      DN_TRY(launch_pack_head(conv_dgrad_view(prm + p.P.L[R_NINB].woff, 96, 1),
                              conv_dgrad_view(prm + p.P.L[R_NINA].woff, 96, 1), ws + p.packHB, s, &pb));
    DN_TRY(add(true, pack_job_zero(ws + p.zeros, 64)));
    DN_TIMED(s, "pack", 0, 0, 0, 0, 0, 0, pack_flush(pb, s));
  }
  RedBatch rb;
  const float* Z = ws + p.zeros;
  SideStream* side = bwd_two_streams() && !prof_on() ? side_stream(s) : nullptr;
  hipStream_t s2 = side ? side->st : s;
  auto fork = [&] { return side_fork(side, s); };
  auto flush_side = [&]() -> hipError_t {
    if (!side) return red_flush(rb, s);
    hipError_t e = hipEventRecord(side->rfork, s2);
    if (e == hipSuccess) e = hipStreamWaitEvent(side->rst, side->rfork, 0);
    if (e == hipSuccess) e = red_flush(rb, side->rst);
    return e;
  };
  // layer i: dz (its cout channels) -> dx = channels [0, res_dgrad_nout) of its input, * leaky'(mask)
  auto dgrad = [&](int i, const View& dz, const View& mask, const View& dxv) -> hipError_t {
    const Layer& L = p.P.L[i];
    const ResRoute& r = B.r[i];
    const int nout = res_dgrad_nout(p, i);
    const OpTimer timer(s, "dgrad3", 2.0 * N * H * W * L.cout * nout * 9, L.cout, nout, H, W, N);
    if (r.kind == RK_F32)
      return conv_dgrad(dz, N, H, W, L.cout, ws + r.img, nout, 3, EPI_MASK, mask, dxv, s);
    FwdArgs a = fwd_args(dz, N, H, W, L.cout, nout, dxv, OUT_NHWC);
    a.zc = r.zc;
    a.wp = ws + r.img; a.wp_z = r.wp_z;
    a.epi = EPI_MASK;
    set_mask(a, mask);
    a.x6_tail = r.tail;
    return launch_fwd_x6(a, s);
  };
  // layer i's weight gradient on the side stream, behind the main stream's work so far
  auto wg = [&](int i, const View& g, const View& xv) -> hipError_t {
    const Layer& L = p.P.L[i];
    hipError_t e = fork();
    if (e != hipSuccess) return e;
    return wgrad(L.k == 3 ? W_C3 : W_C1, g, xv, N, H, W, L.cout, L.cin, G(i), SL(i), p.splits[i], s2,
                 x6, Z, &rb);
  };

  // dy arrives NCHW; out_nc == 1: that is NHWC
  View dyv{const_cast<float*>(dy), OC, 0};
  if (OC > 1) {
    DN_TRY(launch_nchw_to_slice(dy, N, OC, H, W, ws + p.dyt, OC, 0, OC, s));
    dyv = V(p.dyt, OC);
  }
  const bool head_gnb = B.head_x6;  // g_nb recomputed by nin_b's weight gradient (k_wgrad1p)
  {
    HeadBwdArgs h{};
    h.wp = ws + p.packHB;
    h.wc = prm + p.P.L[R_NINC].woff; h.oc = OC;
    h.dy = dyv.p; h.dy_stride = dyv.stride;
    h.nb = ws + p.nb; h.na = ws + p.na; h.d1b = ws + p.d1b;
    h.g_nb = head_gnb ? nullptr : ws + p.g_nb;
    h.g_na = ws + p.g_na; h.g_d1b = ws + p.g_d1b;
    h.npx = px;
    DN_TIMED(s, "head_bwd", 2.0 * px * 96 * (2 * 96 + OC), OC, 96, H, W, N,
             B.head_x6 ? launch_head_bwd_x6(h, ws + p.packHB, s) : launch_head_bwd(h, s));
  }
  const bool fold_c = head_gnb && OC == 1;  // nin_c's weight gradient inside nin_b's
  if (!fold_c) {
    DN_TRY(fork());
    DN_TIMED(s2, "wgrad1", 2.0 * px * 96 * OC, 96, OC, H, W, N,
             launch_wgrad_thin(dyv.p, dyv.stride, OC, ws + p.nb, px, SL(R_NINC) + 64,
                               p.splits[R_NINC], G(R_NINC), s2, &rb));
  }
  DN_TRY(fork());
  const WgradHead hd{head_gnb ? OC : 0, dyv.p, dyv.stride, prm + p.P.L[R_NINC].woff,
                     fold_c ? SL(R_NINC) + 64 : nullptr, G(R_NINC)};
  DN_TRY(wgrad(W_C1, head_gnb ? V(p.nb, 96) : V(p.g_nb, 96), V(p.na, 96), N, H, W, 96, 96,
               G(R_NINB), SL(R_NINB), p.splits[R_NINB], s2, x6, Z, &rb, &hd));
  DN_TRY(wg(R_NINA, V(p.g_na, 96), V(p.d1b, 96)));
  DN_TRY(wg(R_D1B, V(p.g_d1b, 96), V(p.d1a, 96)));
  DN_TRY(dgrad(R_D1B, V(p.g_d1b, 96), V(p.d1a, 96), V(p.g_d1a, 96)));
  // dec_conv1a's weight gradient: the MFMA kernel over [d2b] and the thin kernel over the
  // network-input channels, each into its own slab rows (as the UNet's dec_conv1a)
  {
    const long n = (long)96 * p.c1k * 9 + 96;
    float* slab = SL(R_D1A) + 64;
    WgradArgs a{};
    a.g = ws + p.g_d1a; a.g_stride = 96; a.g_off = 0;
    a.x = ws + p.c1; a.x_stride = p.c1s; a.x_off = 0;
    a.N = N; a.KH = H; a.KW = W; a.Cout = 96; a.Cin = 2 * nf;
    a.zeros = Z; a.slab = slab; a.slab_stride = n;
    a.wlayout = 0; a.cin_total = p.c1k; a.ci_base = 0; a.bias = 1;
    const int sp = x6 ? wgrad_splits_x6(a, p.splits[R_D1A]) : p.splits[R_D1A];
    DN_TRY(fork());
    DN_TIMED(s2, "wgrad3", 2.0 * px * 96 * 2 * nf * 9, 2 * nf, 96, H, W, N,
             launch_wgrad(W_C3, a, sp, s2, x6));
    RedJob j = red_job(slab, n, sp, 96L * 2 * nf * 9, G(R_D1A));
    j.ig = j.og = 2 * nf * 9;
    j.is1 = j.os1 = p.c1k * 9;
    DN_TRY(red_add(&rb, j, s2));
    DN_TRY(red_add(&rb, red_job(slab + 96L * p.c1k * 9, n, sp, 96, G(R_D1A) + 96L * p.c1k * 9), s2));
    float* thin = slab + (long)p.splits[R_D1A] * n;
    const long nt = 96L * C * 9;
    const int st = enc0_wgrad_splits(N, H, W);
    DN_TIMED(s2, "wgrad3_thin", 2.0 * px * 96 * C * 9, C, 96, H, W, N,
             launch_wgrad_c3_thin(ws + p.g_d1a, 96, ws + p.xin, N, C, H, W, thin, nt, C, 0, 0, st, s2));
    DN_TRY(launch_reduce_scatter(thin, nt, st, nt, G(R_D1A), 9L * C, 9L * p.c1k, 9L * 2 * nf, s2, &rb));
  }
  // [d2b]'s gradient; the image channels of c1 carry no activation and get theirs in dgrad_input
  DN_TRY(dgrad(R_D1A, V(p.g_d1a, 96), V(p.c1, p.c1s, 0), V(p.g_c1, 2 * nf)));
  View g = V(p.g_c1, 2 * nf);  // pre-activation gradient of dec_conv{k}b's output
  for (int k = 2; k <= 5; ++k) {
    const int ia = res_da(k), ib = ia + 1;
    DN_TRY(wg(ib, g, V(p.da[k], 2 * nf)));
    DN_TRY(dgrad(ib, g, V(p.da[k], 2 * nf), V(p.g_da[k], 2 * nf)));
    DN_TRY(wg(ia, V(p.g_da[k], 2 * nf), V(p.c[k], p.cs[k])));
    // the concat buffer masks both parts: [dec_conv{k+1}b | a_{k-1}] ([a6 | a4] at k = 5)
    DN_TRY(dgrad(ia, V(p.g_da[k], 2 * nf), V(p.c[k], p.cs[k]), V(p.g_c[k], p.cs[k])));
    g = V(p.g_c[k], p.cs[k], 0);
  }
  if (side) DN_TIMED(side->rst, "reduce", 0, 0, 0, 0, 0, 0, flush_side());
  // enc_conv6 (input a5), then enc_conv5 .. enc_conv2 (input a_j = the skip slice of c_{j+1})
  DN_TRY(wg(R_ENC6, V(p.g_c[5], p.cs[5], 0), V(p.a5, nf)));
  DN_TRY(dgrad(R_ENC6, V(p.g_c[5], p.cs[5], 0), V(p.a5, nf), V(p.g_a5, nf)));
  View ge = V(p.g_a5, nf);  // pre-activation gradient of enc_conv{j+1}'s output
  for (int j = 4; j >= 1; --j) {
    const int i = R_ENC0 + j + 1, k = j + 1, so = (k == 5) ? nf : 2 * nf;
    const View aj = V(p.c[k], p.cs[k], so);
    DN_TRY(wg(i, ge, aj));
    DN_TRY(dgrad(i, ge, aj, V(p.g_t, nf)));
    DN_TIMED(s, "accumulate", 0, nf, nf, H, W, N,
             launch_add_slice(ws + p.g_c[k], p.cs[k], so, ws + p.g_t, nf, px, ws + p.g_a[j], s));
    ge = V(p.g_a[j], nf);
  }
  if (side) DN_TIMED(side->rst, "reduce", 0, 0, 0, 0, 0, 0, flush_side());
  // enc_conv1 (input a0), enc_conv0 (input x)
  DN_TRY(dgrad(R_ENC1, ge, V(p.a0, nf), V(p.g_a0, nf)));
  DN_TRY(fork());
  DN_TIMED(s2, "wgrad3_thin", 2.0 * px * nf * C * 9, C, nf, H, W, N,
           launch_enc0_wgrad(ws + p.g_a0, nf, ws + p.xin, N, C, H, W, SL(R_ENC0) + 64,
                             p.splits[R_ENC0], G(R_ENC0), s2, &rb));
  DN_TRY(wgrad(W_C3, ge, V(p.a0, nf), N, H, W, nf, nf, G(R_ENC1), SL(R_ENC1), p.splits[R_ENC1], s,
               x6, Z, &rb));
  // up5.deconv is never used: an exact zero gradient (dparams is overwritten, not accumulated)
  DN_TRY(hipMemsetAsync(G(R_UP5), 0, (p.P.L[R_UP5].wcount + p.P.L[R_UP5].cout) * sizeof(float), s));
  if (side) {
    DN_TRY(hipEventRecord(side->join, s2));
    DN_TRY(hipStreamWaitEvent(s, side->join, 0));
    DN_TRY(hipEventRecord(side->rjoin, side->rst));
    DN_TRY(hipStreamWaitEvent(s, side->rjoin, 0));
  }
  DN_TIMED(s, "reduce", 0, 0, 0, 0, 0, 0, red_flush(rb, s));
  // dL/dx = dy + enc_conv0^T g_a0 + (image-channel slice of dec_conv1a's data gradient)
  if (dx)
    DN_TIMED(s, "dgrad_input", 0, 0, 0, 0, 0, 0,
             launch_dgrad_input(ws + p.g_a0, prm + p.P.L[R_ENC0].woff, ws + p.g_d1a,
                                prm + p.P.L[R_D1A].woff, p.c1k, 2 * nf, N, C, H, W, dx, s, dy));
  return DN_OK;
}

}  // namespace dn
