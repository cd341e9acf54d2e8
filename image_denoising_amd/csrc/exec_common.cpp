// The executors' shared pieces (exec_common.h).
#include "exec_common.h"

#include <algorithm>
#include <cstdlib>
#include <map>

namespace dn {

thread_local std::string g_last_error;
void set_error(const std::string& s) { g_last_error = s; }

// ---- side streams ----
// One side stream (and its fork / join events) per host thread and device: keyed on the
// device of the caller's stream (not hipGetDevice(), which a caller need not have set to it) and
// created under a guard for that device; thread-local, so two host threads running backwards on
// one device never share the events between a record and its wait.  The owner destroys them when
// its thread exits (executors called from short-lived threads do not leak streams).
struct SideStreams {
  std::map<int, SideStream> per_device;
  ~SideStreams() {
    for (auto& kv : per_device) {
      SideStream& ss = kv.second;
      if (!ss.st) continue;
      // (HIP releases a stream / event with work still pending once that work completes)
      (void)hipEventDestroy(ss.fork);
      (void)hipEventDestroy(ss.join);
      (void)hipEventDestroy(ss.rfork);
      (void)hipEventDestroy(ss.rjoin);
      (void)hipStreamDestroy(ss.st);
      (void)hipStreamDestroy(ss.rst);
    }
  }
};

SideStream* side_stream(hipStream_t s) {
  thread_local SideStreams owner;
  std::map<int, SideStream>& per_device = owner.per_device;
  hipDevice_t dev = 0;
  if (hipStreamGetDevice(s, &dev) != hipSuccess) return nullptr;
  SideStream& ss = per_device[dev];
  if (!ss.st) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return nullptr;
    if (hipStreamCreateWithFlags(&ss.st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ss.join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&ss.rst, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ss.rfork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ss.rjoin, hipEventDisableTiming) != hipSuccess)
      ss = SideStream{};
    if (cur != dev) (void)hipSetDevice(cur);
    if (!ss.st) return nullptr;
  }
  return &ss;
}

bool bwd_two_streams() {
  static const bool on = !getenv("DN_BWD_STREAMS") || atoi(getenv("DN_BWD_STREAMS")) != 0;
  return on;
}

hipError_t side_fork(SideStream* side, hipStream_t s) {
  if (!side) return hipSuccess;
  hipError_t e = hipEventRecord(side->fork, s);
  return e != hipSuccess ? e : hipStreamWaitEvent(side->st, side->fork, 0);
}

BwdStreams::BwdStreams(hipStream_t stream)
    : side(bwd_two_streams() && !prof_on() ? side_stream(stream) : nullptr), s(stream),
      s2(side ? side->st : stream) {}

hipError_t BwdStreams::flush_reductions() {
  if (!side) return hipSuccess;
  const OpTimer timer(side->rst, "reduce", 0);
  hipError_t e = hipEventRecord(side->rfork, s2);
  if (e == hipSuccess) e = hipStreamWaitEvent(side->rst, side->rfork, 0);
  if (e == hipSuccess) e = red_flush(rb, side->rst);
  return e;
}

hipError_t BwdStreams::join(bool reductions) {
  if (!side) return hipSuccess;
  hipError_t e = hipEventRecord(side->join, s2);
  if (e == hipSuccess) e = hipStreamWaitEvent(s, side->join, 0);
  if (e != hipSuccess || !reductions) return e;
  e = hipEventRecord(side->rjoin, side->rst);
  return e != hipSuccess ? e : hipStreamWaitEvent(s, side->rjoin, 0);
}

// ---- op helpers ----
int x6_dgrad_zc(int nout) { return nout <= 96 ? 0 : 48; }

WView conv_fwd_view(const float* w, int K, int ksize) {
  return ksize == 3 ? WView{w, 0, 9, (long)K * 9, 1, 0, 9, 0} : WView{w, 0, 1, (long)K, 0, 0, 1, 0};
}
WView conv_dgrad_view(const float* w, int cin_total, int ksize) {  // flipped + transposed
  return ksize == 3 ? WView{w, 0, (long)cin_total * 9, 9, 1, 0, 9, 1}
                    : WView{w, 0, (long)cin_total, 1, 0, 0, 1, 0};
}
WView deconv_fwd_view(const float* w, int cout) { return WView{w, 0, (long)cout * 4, 4, 0, 1, 1, 0}; }
WView deconv_dgrad_view(const float* w, int cout) { return WView{w, 0, 4, (long)cout * 4, 1, 0, 4, 0}; }

long conv_fwd_pack_size(int K, int cout, int ksize) {
  return pack_floats(ksize == 3 ? G_C3 : G_C1, cout, K, 1);
}
long conv_dgrad_pack_size(int cout, int nout, int ksize) {
  return pack_floats(ksize == 3 ? G_C3 : G_C1, nout, cout, 1);
}
long deconv_fwd_pack_size(int cin, int cout) { return pack_floats(G_UP, cout, cin, 4); }
long deconv_dgrad_pack_size(int cout, int cin) { return pack_floats(G_DN2, cin, cout, 1); }

hipError_t pack_conv_fwd(const float* w, int K, int cout, int ksize, float* out, hipStream_t s) {
  return launch_pack(ksize == 3 ? G_C3 : G_C1, conv_fwd_view(w, K, ksize), K, cout, 1, out, s);
}
hipError_t pack_conv_dgrad(const float* w, int cin_total, int nout, int cout, int ksize, float* out,
                           hipStream_t s) {
  return launch_pack(ksize == 3 ? G_C3 : G_C1, conv_dgrad_view(w, cin_total, ksize), cout, nout, 1,
                     out, s);
}
hipError_t pack_deconv_fwd(const float* w, int cin, int cout, float* out, hipStream_t s) {
  return launch_pack(G_UP, deconv_fwd_view(w, cout), cin, cout, 4, out, s);
}
hipError_t pack_deconv_dgrad(const float* w, int cout, int cin, float* out, hipStream_t s) {
  return launch_pack(G_DN2, deconv_dgrad_view(w, cout), cout, cin, 1, out, s);
}

hipError_t conv_forward(const View& in, int N, int H, int W, int K, const float* wp,
                        const float* b, int cout, int ksize, int act, const View& out,
                        int out_layout, hipStream_t s) {
  FwdArgs a = fwd_args(in, N, H, W, K, cout, out, out_layout);
  a.wp = wp;
  a.bias = b; a.epi = act ? EPI_BIAS_ACT : EPI_BIAS;
  return launch_fwd(ksize == 3 ? G_C3 : G_C1, a, s);
}

// dx (channels [0, nout)) from dz [N,H,W,cout]; wp = pack_conv_dgrad(...)
hipError_t conv_dgrad(const View& dz, int N, int H, int W, int cout, const float* wp, int nout,
                      int ksize, int epi, const View& mask, const View& dx, hipStream_t s) {
  FwdArgs a = fwd_args(dz, N, H, W, cout, nout, dx, OUT_NHWC);
  a.wp = wp;
  a.epi = epi;
  set_mask(a, mask);
  return launch_fwd(ksize == 3 ? G_C3 : G_C1, a, s);
}

// ConvTranspose2d(cin, cout, 2, 2): x [N,h,w,cin] -> out at (2y+a, 2x+b); wp = pack_deconv_fwd
hipError_t deconv_forward(const View& x, int N, int h, int w, int cin, const float* wp,
                          const float* b, int cout, const View& out, hipStream_t s) {
  FwdArgs a = fwd_args(x, N, h, w, cin, cout, out, OUT_UP2);
  a.wp = wp; a.wp_z = pack_floats(G_UP, cout, cin, 1);
  a.bias = b; a.epi = EPI_BIAS;
  return launch_fwd(G_UP, a, s);
}

// dx [N,h,w,cin] = sum_{ab,co} dy[2y+a][2x+b][co] * W[ci][co][ab]  (* leaky'(mask));
// wp = pack_deconv_dgrad
hipError_t deconv_dgrad(const View& dy, int N, int h, int w, int cout, const float* wp, int cin,
                        const View& mask, int epi, const View& dx, hipStream_t s) {
  FwdArgs a = fwd_args(dy, 2 * h, 2 * w, N, h, w, cout, cin, dx, OUT_NHWC);
  a.wp = wp;
  a.epi = epi;
  set_mask(a, mask);
  return launch_fwd(G_DN2, a, s);
}

dn_status wgrad_run(const WgradRoute& r, const float* g, const float* x, float* dwb, float* slab,
                    const float* zeros, hipStream_t s, RedBatch* rb, const WgradHead* head) {
  const WgradShape& sh = r.sh;
  if (r.kernel == WK_NONE || (head ? head->gnb : 0) != sh.head_gnb) {
    set_error(r.err ? r.err : "weight-gradient route built for another head");
    return DN_ERR_ARG;
  }
  const int mode = sh.mode, taps = wgrad_taps(mode), sp = r.splits;
  WgradArgs a{};
  if (head) {
    a.head_gnb = head->gnb; a.hd_dy = head->dy; a.hd_dy_stride = head->dy_stride;
    a.hd_wc = head->wc; a.hd_slab_c = head->slab_c; a.hd_dwc = head->dwc;
  }
  a.g = g; a.g_stride = sh.g_stride; a.g_off = sh.g_off;
  a.x = x; a.x_stride = sh.x_stride; a.x_off = sh.x_off;
  a.N = sh.N; a.KH = sh.KH; a.KW = sh.KW; a.Cout = sh.Cout; a.Cin = sh.Cin;
  // slab scratch layout: [64 floats | par x splits rows of (W + b)]
  a.zeros = zeros ? zeros : slab;
  a.slab = slab + 64; a.slab_stride = r.row;
  a.wlayout = mode == W_UP2 ? 1 : 0;  // deconv weight (in, out, 2, 2)
  a.cin_total = sh.cin_total; a.ci_base = sh.ci_base; a.bias = sh.bias ? 1 : 0;
  if (r.zc) { a.zc = r.zc; a.cout_total = sh.Cout; }  // all output-channel blocks in ONE launch
  // (k_reduce_batch sets no label: the record keeps the GEMM kernel's)
  const OpTimer timer(s, mode == W_C3 ? "wgrad3" : (mode == W_UP2 ? "wgrad_up" : "wgrad1"),
                      2.0 * sh.N * sh.KH * sh.KW * sh.Cout * sh.Cin * taps, sh.Cin, sh.Cout, sh.KH,
                      sh.KW, sh.N);
  if (!zeros) DN_TRY(hipMemsetAsync(slab, 0, 64 * sizeof(float), s));
  switch (r.kernel) {
    case WK_WGRAD: DN_TRY(launch_wgrad(a, r, s)); break;
    case WK_WGRAD3: DN_TRY(launch_wgrad3(a, r, s)); break;
    case WK_WGRAD1: DN_TRY(launch_wgrad1(a, r, s)); break;
    case WK_WGRAD3S: DN_TRY(launch_wgrad3s(a, r, s)); break;
    case WK_WGRAD1P: DN_TRY(launch_wgrad1p(a, r, s)); break;
    default: DN_TRY(launch_wgrad3p(a, r, s)); break;  // WK_WGRAD3P, WK_WGRAD3Q
  }
  // the reductions into dwb (PyTorch layout, the bias after the weight)
  const long W = (long)sh.Cout * sh.Cin * taps, Wt = (long)sh.Cout * sh.cin_total * taps;
  if (r.par == 4) {
    // W[ci][co][a][b] in output order: element e = 4 (ci*Cout + co) + ab lives in parity ab's
    // block of sp rows
    RedJob j = red_job(a.slab, r.row, sp, W, dwb);
    j.ig = 4; j.is1 = 1; j.is2 = (int)(sp * r.row);
    DN_TRY(red_add(rb, j, s));
    DN_TRY(launch_reduce(a.slab + W / 4, r.row, 4 * sp, sh.Cout, dwb + W, s, rb));  // bias: all rows
    return DN_OK;
  }
  if (a.hd_slab_c) {  // nin_c's weight gradient formed by the same launch (k_wgrad1p GNB)
    const long rc = (long)a.head_gnb * 96 + a.head_gnb;
    DN_TRY(launch_reduce(a.hd_slab_c, rc, sp, rc, a.hd_dwc, s, rb));
  }
  if (sh.cin_total == sh.Cin) {
    DN_TRY(launch_reduce(a.slab, r.row, sp, r.row, dwb, s, rb));
    return DN_OK;
  }
  // an input-channel slice of a wider weight: W[co][ci_base + ci < Cin][t], then the bias
  RedJob j = red_job(a.slab + (long)sh.ci_base * taps, r.row, sp, W, dwb + (long)sh.ci_base * taps);
  j.ig = j.og = sh.Cin * taps;
  j.is1 = j.os1 = sh.cin_total * taps;
  DN_TRY(red_add(rb, j, s));  // (a full batch flushes on s, behind the weight gradients it reads)
  if (sh.bias) DN_TRY(red_add(rb, red_job(a.slab + Wt, r.row, sp, sh.Cout, dwb + Wt), s));
  return DN_OK;
}

// ---- the UNet's and the RESNET's common pieces ----
WgradSlab plan_wgrad_slab(int kind, int mode, int N, int KH, int KW, const Layer& L, int C) {
  const long row = L.wcount + L.cout;  // one split's (W + b)
  WgradSlab r;
  switch (kind) {
    case SLAB_ENC0:
      r.splits = enc0_wgrad_splits(N, KH, KW);
      r.floats = r.splits * row;
      break;
    case SLAB_D1A:  // the MFMA kernel's slice in rows of the whole weight; the thin kernel's rows hold [co][C][9]
      r.splits = wgrad_size(mode, N, KH, KW, L.cin - C, L.cout, false).rows;
      r.floats = r.splits * row + (long)enc0_wgrad_splits(N, KH, KW) * L.cout * C * 9;
      break;
    case SLAB_NINC_THIN: {  // ... or as many rows as nin_b's k_wgrad1p<., GNB> launch has splits
      WgradShape nb = wgrad_shape(W_C1, N, KH, KW, 96, 96, 96, 0, 96, 0, true);
      nb.head_gnb = 1;
      r.splits = wgrad_thin_splits((long)N * KH * KW);
      r.floats = std::max(r.splits, wgrad_route(nb).splits) * row;
      break;
    }
    default: {
      const WgradSize z = wgrad_size(mode, N, KH, KW, L.cin, L.cout, false);
      r.splits = z.rows;
      r.floats = z.floats;
      break;
    }
  }
  return r;
}

ConvRoute dgrad_route(bool x6, long img_f32, long img_x6, int N, int h, int w, const Layer& L,
                      int nout) {
  ConvRoute r{CV_F32, img_f32, 0, 0, 0};
  if (x6 && img_x6 >= 0) {
    r.kind = CV_X6; r.img = img_x6;
    r.zc = x6_dgrad_zc(nout);
    r.wp_z = x6_wp_z(L.cout, nout, r.zc);
    r.tail = x6_image_mode(N, h, w, L.cout, nout, r.zc, true);
  }
  return r;
}

hipError_t pack_dgrad(PackBatch& pb, const ConvRoute& r, const float* w, const Layer& L, int nout,
                      float* ws, hipStream_t s) {
  PackJob j;
  const bool ok =
      r.kind == CV_X6
          ? pack_job_x6(conv_dgrad_view(w, L.cin, 3), L.cout, nout, r.zc, ws + r.img, r.tail, j)
          : pack_job(L.k == 3 ? G_C3 : G_C1, conv_dgrad_view(w, L.cin, L.k), L.cout, nout, 1,
                     ws + r.img, 0, 0, j);
  return ok ? pack_add(pb, j, s) : hipErrorInvalidValue;
}

hipError_t run_dgrad(const ConvRoute& r, const float* ws, const View& dz, int N, int h, int w,
                     const Layer& L, int nout, int epi, const View& mask, const View& dx,
                     hipStream_t s) {
  const OpTimer timer(s, L.k == 3 ? "dgrad3" : "dgrad1", 2.0 * N * h * w * L.cout * nout * L.k * L.k,
                      L.cout, nout, h, w, N);
  if (r.kind == CV_F32)
    return conv_dgrad(dz, N, h, w, L.cout, ws + r.img, nout, L.k, epi, mask, dx, s);
  FwdArgs a = fwd_args(dz, N, h, w, L.cout, nout, dx, OUT_NHWC);
  a.zc = r.zc;
  a.wp = ws + r.img; a.wp_z = r.wp_z;
  a.epi = epi;
  set_mask(a, mask);
  a.x6_tail = r.tail;
  return launch_fwd_x6(a, s);
}

hipError_t pack_head_fwd(PackBatch& pb, bool x6, const float* wa, const float* wb, float* img,
                         hipStream_t s) {
  if (x6) return pack_add(pb, pack_job_head_x6(wa, wb, img), s);
  return launch_pack_head(conv_fwd_view(wa, 96, 1), conv_fwd_view(wb, 96, 1), img, s, &pb);
}

hipError_t pack_head_bwd(PackBatch& pb, bool x6, const float* wa, const float* wb, float* img,
                         float* zeros, hipStream_t s) {
  const hipError_t e =
      x6 ? pack_add(pb, pack_job_head_bwd_x6(wa, wb, img), s)
         : launch_pack_head(conv_dgrad_view(wb, 96, 1), conv_dgrad_view(wa, 96, 1), img, s, &pb);
  return e != hipSuccess ? e : pack_add(pb, pack_job_zero(zeros, 64), s);
}

HeadArgs head_args(const float* prm, const Layer& na, const Layer& nb, const Layer& nc,
                   const float* img, float* y) {
  HeadArgs h{};
  h.wp = img;
  h.ba = prm + na.woff + na.wcount; h.bb = prm + nb.woff + nb.wcount;
  h.wc = prm + nc.woff; h.bc = h.wc + nc.wcount; h.oc = nc.cout;
  h.y = y;
  return h;
}

dn_status head_forward(const HeadArgs& h, const float* d1b, int N, int H, int W, bool x6,
                       hipStream_t s) {
  const FwdArgs a = fwd_args(View{const_cast<float*>(d1b), 96, 0}, N, H, W, 96, 96,
                             View{nullptr, 0, 0}, OUT_NHWC);
  DN_TIMED(s, "head", 2.0 * N * H * W * 96 * (2 * 96 + h.oc), 96, h.oc, H, W, N,
           x6 ? launch_nin_head_x6(a, h, h.wp, s) : launch_nin_head(a, h, s));
  return DN_OK;
}

dn_status head_backward(BwdStreams& bs, const TailShape& t, HeadBwdArgs h, bool head_x6,
                        const WgradDst& nina, const WgradDst& ninb, const WgradDst& ninc) {
  const int N = t.N, H = t.H, W = t.W, OC = h.oc;
  const hipStream_t s2 = bs.s2;
  const float* g_nb = h.g_nb;
  // (head_x6: nin_b's weight gradient recomputes g_nb, nothing reads a stored one)
  if (head_x6) h.g_nb = nullptr;
  DN_TIMED(bs.s, "head_bwd", 2.0 * h.npx * 96 * (2 * 96 + OC), OC, 96, H, W, N,
           head_x6 ? launch_head_bwd_x6(h, h.wp, bs.s) : launch_head_bwd(h, bs.s));
  const bool fold_c = head_x6 && OC == 1;  // nin_c's weight gradient inside nin_b's (k_wgrad1p)
  if (!fold_c) {
    DN_TRY(bs.fork());
    if (OC <= 4) {
      DN_TIMED(s2, "wgrad1", 2.0 * h.npx * 96 * OC, 96, OC, H, W, N,
               launch_wgrad_thin(h.dy, h.dy_stride, OC, h.nb, h.npx, ninc.slab + 64, ninc.splits,
                                 ninc.dwb, s2, &bs.rb));
    } else {
      const WgradShape nc = wgrad_shape(W_C1, N, H, W, 96, OC, h.dy_stride, 0, 96, 0);
      if (dn_status st = wgrad_run(wgrad_route(nc), h.dy, h.nb, ninc.dwb, ninc.slab, t.zeros, s2,
                                   &bs.rb))
        return st;
    }
  }
  DN_TRY(bs.fork());
  const WgradHead hd{head_x6 ? OC : 0, h.dy, h.dy_stride, h.wc,
                     fold_c ? ninc.slab + 64 : nullptr, ninc.dwb};
  WgradShape nin = wgrad_shape(W_C1, N, H, W, 96, 96, 96, 0, 96, 0, t.x6);
  const WgradRoute r_a = wgrad_route(nin);
  nin.head_gnb = hd.gnb;
  if (dn_status st = wgrad_run(wgrad_route(nin), head_x6 ? h.nb : g_nb, h.na, ninb.dwb, ninb.slab,
                               t.zeros, s2, &bs.rb, &hd))
    return st;
  DN_TRY(bs.fork());
  return wgrad_run(r_a, h.g_na, h.d1b, nina.dwb, nina.slab, t.zeros, s2, &bs.rb);
}

dn_status d1a_wgrad(BwdStreams& bs, const TailShape& t, const float* g_d1a, const View& c1,
                    int c1k, const float* xin, int C, const WgradDst& d) {
  const int N = t.N, H = t.H, W = t.W, up = c1k - C;  // up: the channels ahead of the input's
  const hipStream_t s2 = bs.s2;
  const long n = (long)96 * c1k * 9 + 96;
  float* slab = d.slab + 64;
  WgradShape sh = wgrad_shape(W_C3, N, H, W, up, 96, 96, 0, c1.stride, c1.off, t.x6);
  sh.cin_total = c1k;  // rows of W[co][c1k][9]; the reduction takes this launch's columns
  DN_TRY(bs.fork());
  if (dn_status st = wgrad_run(wgrad_route(sh), g_d1a, c1.p, d.dwb, d.slab, t.zeros, s2, &bs.rb))
    return st;
  // input-channel slice: compact [co][C][9] rows after the MFMA kernel's, own split count,
  // scattered into W[co][up + ci][t]
  float* thin = slab + (long)d.splits * n;
  const long nt = 96L * C * 9;
  const int st = enc0_wgrad_splits(N, H, W);
  DN_TIMED(s2, "wgrad3_thin", 2.0 * N * H * W * 96 * C * 9, C, 96, H, W, N,
           launch_wgrad_c3_thin(g_d1a, 96, xin, N, C, H, W, thin, nt, C, 0, 0, st, s2));
  DN_TRY(launch_reduce_scatter(thin, nt, st, nt, d.dwb, 9L * C, 9L * c1k, 9L * up, s2, &bs.rb));
  return DN_OK;
}

}  // namespace dn
