// RESNET orchestration (arch_unet.py:263-409): parameter layout (reference state_dict order),
// workspace plan and the forward / backward launch sequences, in the shape of unet.cpp: a plan,
// the kernel routes of a pass resolved once, one pack launch, then the run.  Every layer runs at
// the input resolution (any H, W >= 1); the concatenations are placements into strided slices.
// The op helpers, the backward's streams and the tail shared with the UNet: exec_common.{h,cpp}.
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
      const int kind = i == R_ENC0 ? SLAB_ENC0 : i == R_D1A ? SLAB_D1A
                       : i == R_NINC ? SLAB_NINC_THIN : SLAB_CONV;  // (out_nc <= 4 always)
      const WgradSlab sl = plan_wgrad_slab(kind, mode, N, H, W, L, p.C);
      p.splits[i] = sl.splits;
      p.slab[i] = alloc_f(64 + sl.floats);
    }
  }
  p.total_floats = off;
  p.with_bwd = bwd;
  return true;
}

void resnet_debug_buffers(const ResPlan& p, const BufferVisitor& add_at) {
  const auto add = [&](long off, int stride) { add_at(off, stride, 0); };
  const int nf = p.nf;
  add(p.c1, p.c1s); add(p.a0, nf);
  for (int k = 2; k <= 5; ++k) add(p.c[k], p.cs[k]);
  add(p.a5, nf);
  for (int k = 2; k <= 5; ++k) add(p.da[k], 2 * nf);
  add(p.d1a, 96); add(p.d1b, 96);
  if (!p.with_bwd) return;
  add(p.na, 96); add(p.nb, 96);
  add(p.g_na, 96); add(p.g_d1b, 96); add(p.g_d1a, 96); add(p.g_c1, 2 * nf);
  for (int k = 2; k <= 5; ++k) add(p.g_c[k], p.cs[k]);
  for (int k = 2; k <= 5; ++k) add(p.g_da[k], 2 * nf);
  for (int j = 1; j <= 4; ++j) add(p.g_a[j], nf);
  add(p.g_a5, nf); add(p.g_a0, nf);
}

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
namespace {

struct ResRoutes {
  ConvRoute r[R_NL];  // enc_conv1 .. dec_conv1b: CV_F32 (packF / packB) | CV_X6 (packX / packXB)
  bool head_x6;      // the nin head (forward) / its data gradients (backward) in bf16x6
};

ResRoutes res_fwd_routes(const ResPlan& p, int prec) {
  const bool x6 = prec == DN_PREC_FP32_X6;
  ResRoutes R{};
  for (int i = R_ENC1; i <= R_D1B; ++i) {
    if (i == R_UP5) continue;
    const Layer& L = p.P.L[i];
    ConvRoute& r = R.r[i] = ConvRoute{CV_F32, p.packF[i]};
    if (x6 && p.packX[i] >= 0) {
      // dec_conv1a reads [d2b | x | zero pad]: the pad channels as reduction channels with zero
      // packed weights keep K % 4 == 0 (as the UNet's dec_conv1a)
      r.kind = CV_X6; r.img = p.packX[i];
      r.tail = x6_image_mode(p.N, p.H, p.W, i == R_D1A ? p.c1kp : L.cin, L.cout, 0, true);
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
    B.r[i] = dgrad_route(x6, p.packB[i], p.packXB[i], p.N, p.H, p.W, p.P.L[i], res_dgrad_nout(p, i));
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
    const ConvRoute& r = R.r[i];
    const float* w = prm + L.woff;
    PackJob j;
    if (r.kind == CV_X6)
      DN_TRY(add(pack_job_x6(conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 0, ws + r.img, r.tail, j), j));
    else
      DN_TRY(add(pack_job(G_C3, conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 1, ws + r.img, 0, 0, j), j));
  }
  DN_TRY(pack_head_fwd(pb, R.head_x6, prm + p.P.L[R_NINA].woff, prm + p.P.L[R_NINB].woff,
                       ws + p.packH, s));
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
    const ConvRoute& r = R.r[i];
    const OpTimer timer(s, "fwd3", 2.0 * N * H * W * L.cin * L.cout * 9, L.cin, L.cout, H, W, N);
    if (r.kind == CV_F32)
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
  HeadArgs h = head_args(prm, p.P.L[R_NINA], p.P.L[R_NINB], p.P.L[R_NINC], ws + p.packH, y);
  h.res = x;
  if (p.with_bwd) { h.na = ws + p.na; h.nb = ws + p.nb; }
  return head_forward(h, ws + p.d1b, N, H, W, R.head_x6, s);
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
    for (int i = R_ENC1; i <= R_D1B; ++i)
      if (i != R_UP5)
        DN_TRY(pack_dgrad(pb, B.r[i], prm + p.P.L[i].woff, p.P.L[i], res_dgrad_nout(p, i), ws, s));
    DN_TRY(pack_head_bwd(pb, B.head_x6, prm + p.P.L[R_NINA].woff, prm + p.P.L[R_NINB].woff,
                         ws + p.packHB, ws + p.zeros, s));
    DN_TIMED(s, "pack", 0, 0, 0, 0, 0, 0, pack_flush(pb, s));
  }
  BwdStreams bs(s);
  const float* Z = ws + p.zeros;
  auto dst = [&](int i) { return WgradDst{G(i), SL(i), p.splits[i]}; };
  const TailShape tail{N, H, W, x6, Z};
  // layer i: dz (its cout channels) -> dx = channels [0, res_dgrad_nout) of its input, * leaky'(mask)
  auto dgrad = [&](int i, const View& dz, const View& mask, const View& dxv) -> hipError_t {
    return run_dgrad(B.r[i], ws, dz, N, H, W, p.P.L[i], res_dgrad_nout(p, i), EPI_MASK, mask, dxv, s);
  };
  // layer i's weight gradient; side: on the side stream, behind the main stream's work so far
  auto wg = [&](int i, const View& g, const View& xv, bool side = true) -> dn_status {
    const Layer& L = p.P.L[i];
    if (side) DN_TRY(bs.fork());
    return wgrad_run(wgrad_route(L.k == 3 ? W_C3 : W_C1, g, xv, N, H, W, L.cout, L.cin, x6), g.p,
                     xv.p, G(i), SL(i), Z, side ? bs.s2 : s, &bs.rb);
  };

  // dy arrives NCHW; out_nc == 1: that is NHWC
  View dyv{const_cast<float*>(dy), OC, 0};
  if (OC > 1) {
    DN_TRY(launch_nchw_to_slice(dy, N, OC, H, W, ws + p.dyt, OC, 0, OC, s));
    dyv = V(p.dyt, OC);
  }
  {  // nin_c .. nin_a: data gradients in one kernel, then the three 1x1 weight gradients
    HeadBwdArgs h{};
    h.wp = ws + p.packHB;
    h.wc = prm + p.P.L[R_NINC].woff; h.oc = OC;
    h.dy = dyv.p; h.dy_stride = dyv.stride;
    h.nb = ws + p.nb; h.na = ws + p.na; h.d1b = ws + p.d1b;
    h.g_nb = ws + p.g_nb; h.g_na = ws + p.g_na; h.g_d1b = ws + p.g_d1b;
    h.npx = px;
    if (dn_status st = head_backward(bs, tail, h, B.head_x6, dst(R_NINA), dst(R_NINB), dst(R_NINC)))
      return st;
  }
  if (dn_status st_ = wg(R_D1B, V(p.g_d1b, 96), V(p.d1a, 96))) return st_;
  DN_TRY(dgrad(R_D1B, V(p.g_d1b, 96), V(p.d1a, 96), V(p.g_d1a, 96)));
  // dec_conv1a's weight gradient: [d2b]'s channels and the network input's (as the UNet's)
  if (dn_status st = d1a_wgrad(bs, tail, ws + p.g_d1a, V(p.c1, p.c1s), p.c1k, ws + p.xin, C, dst(R_D1A)))
    return st;
  // [d2b]'s gradient; the image channels of c1 carry no activation and get theirs in dgrad_input
  DN_TRY(dgrad(R_D1A, V(p.g_d1a, 96), V(p.c1, p.c1s, 0), V(p.g_c1, 2 * nf)));
  View g = V(p.g_c1, 2 * nf);  // pre-activation gradient of dec_conv{k}b's output
  for (int k = 2; k <= 5; ++k) {
    const int ia = res_da(k), ib = ia + 1;
    if (dn_status st_ = wg(ib, g, V(p.da[k], 2 * nf))) return st_;
    DN_TRY(dgrad(ib, g, V(p.da[k], 2 * nf), V(p.g_da[k], 2 * nf)));
    if (dn_status st_ = wg(ia, V(p.g_da[k], 2 * nf), V(p.c[k], p.cs[k]))) return st_;
    // the concat buffer masks both parts: [dec_conv{k+1}b | a_{k-1}] ([a6 | a4] at k = 5)
    DN_TRY(dgrad(ia, V(p.g_da[k], 2 * nf), V(p.c[k], p.cs[k]), V(p.g_c[k], p.cs[k])));
    g = V(p.g_c[k], p.cs[k], 0);
  }
  DN_TRY(bs.flush_reductions());
  // enc_conv6 (input a5), then enc_conv5 .. enc_conv2 (input a_j = the skip slice of c_{j+1})
  if (dn_status st_ = wg(R_ENC6, V(p.g_c[5], p.cs[5], 0), V(p.a5, nf))) return st_;
  DN_TRY(dgrad(R_ENC6, V(p.g_c[5], p.cs[5], 0), V(p.a5, nf), V(p.g_a5, nf)));
  View ge = V(p.g_a5, nf);  // pre-activation gradient of enc_conv{j+1}'s output
  for (int j = 4; j >= 1; --j) {
    const int i = R_ENC0 + j + 1, k = j + 1, so = (k == 5) ? nf : 2 * nf;
    const View aj = V(p.c[k], p.cs[k], so);
    if (dn_status st_ = wg(i, ge, aj)) return st_;
    DN_TRY(dgrad(i, ge, aj, V(p.g_t, nf)));
    DN_TIMED(s, "accumulate", 0, nf, nf, H, W, N,
             launch_add_slice(ws + p.g_c[k], p.cs[k], so, ws + p.g_t, nf, px, ws + p.g_a[j], s));
    ge = V(p.g_a[j], nf);
  }
  DN_TRY(bs.flush_reductions());
  // enc_conv1 (input a0), enc_conv0 (input x)
  DN_TRY(dgrad(R_ENC1, ge, V(p.a0, nf), V(p.g_a0, nf)));
  DN_TRY(bs.fork());
  DN_TIMED(bs.s2, "wgrad3_thin", 2.0 * px * nf * C * 9, C, nf, H, W, N,
           launch_enc0_wgrad(ws + p.g_a0, nf, ws + p.xin, N, C, H, W, SL(R_ENC0) + 64,
                             p.splits[R_ENC0], G(R_ENC0), bs.s2, &bs.rb));
  if (dn_status st_ = wg(R_ENC1, ge, V(p.a0, nf), false)) return st_;
  // up5.deconv is never used: an exact zero gradient (dparams is overwritten, not accumulated)
  DN_TRY(hipMemsetAsync(G(R_UP5), 0, (p.P.L[R_UP5].wcount + p.P.L[R_UP5].cout) * sizeof(float), s));
  DN_TRY(bs.join());
  DN_TIMED(s, "reduce", 0, 0, 0, 0, 0, 0, red_flush(bs.rb, s));
  // dL/dx = dy + enc_conv0^T g_a0 + (image-channel slice of dec_conv1a's data gradient)
  if (dx)
    DN_TIMED(s, "dgrad_input", 0, 0, 0, 0, 0, 0,
             launch_dgrad_input(ws + p.g_a0, prm + p.P.L[R_ENC0].woff, ws + p.g_d1a,
                                prm + p.P.L[R_D1A].woff, p.c1k, 2 * nf, N, C, H, W, dx, s, dy));
  return DN_OK;
}

}  // namespace dn
