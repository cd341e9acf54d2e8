// ImprovedUNet (arch_unet.py:421-531, noise=True, depth=4) forward and backward on the gfx950
// kernels: every 3x3 / 1x1 convolution with >= 16 channels on both sides runs on the fp32
// MFMA implicit-GEMM kernel (k_fwd, output-channel blocks over blockIdx.z; data gradients
// through the flipped weight view), thin ones (noise estimator, final conv, sigma-map
// gradient) on VALU kernels; GroupNorm, pooling and PixelShuffle are HBM-bound passes.
//
// Dataflow (NHWC fp32 in one workspace; "[a | b]" = one buffer, channel slices):
//   x0 = [x | sigma]            sigma = sigmoid(ne2(leaky(ne0(x))))          arch_unet.py:519-521
//   level i (C_i = 48 * 2^i, res H/2^i):
//     F_i = [leaky(conv_i(x_i)) | o0 | o1 | o2 | o3]   o_j = leaky(conv_j(F_i[:, :C_i+32j]))
//     r_i = F_i[:, :C_i] + lff(F_i)                      RDB, arch_unet.py:436-451
//     s_i = r_i + GN2(conv2(leaky(GN1(conv1(r_i)))))     ResBlock, arch_unet.py:422-433
//           written straight into the skip slice of up block 3-i's concat buffer
//     x_{i+1} = maxpool(s_i)                             arch_unet.py:524-526
//   bottle: ResBlock(RDB(x_4)) at H/16, 384 channels    arch_unet.py:507, 527
//   up k (in 384/2^k -> out 192/2^k):  cc_k = [PixelShuffle(conv_ps(x)) | s_{3-k}]
//     f = leaky(fuse(cc_k)), then ResBlock(RDB(f))      UpBlock, arch_unet.py:454-472
//   y = sigmoid(final([x_up3 | x]))                      arch_unet.py:530-531
#include <algorithm>

#include "exec_common.h"
#include "iunet.h"
#include "iunet_ops.h"

namespace dn {

namespace {

constexpr int GROWTH = 32;  // RDB growth (arch_unet.py:437)
constexpr float GN_EPS = 1e-5f;

int gn_groups(int ch) {  // norm2d('gn', ch, groups=32), arch_unet.py:12-15
  int g = std::min(32, ch);
  while (ch % g != 0 && g > 1) --g;
  return g;
}

// ---- routes: the kernel and the weight image of one conv launch -------------------------
// A pass resolves them once per conv site (iunet_fwd_routes / iunet_bwd_routes below); the pack
// loop writes exactly the image a route names and the launch reads it, neither decides anything.
struct IRoute {
  bool x6 = false;             // the bf16x6 kernels (else the fp32 MFMA kernel)
  int tail = 0, zc = 0;        // x6: image mode (x6_image_mode / x6_tail_mode), output-channel
  long wp_z = 0;               //   blocks over blockIdx.z and the bf16 elements of one
  int gather = G_C3, nt = 6, np = 96, nz = 1;  // fp32: tile width (np = 16 nt), z-blocks
  long img = 0;                //   floats of one z-block's packed image
  long floats = 0;             // the whole image (0: the site launches nothing in this pass)
  long off = 0;                // its offset in the arena
};

bool ggeom(int ksize, int K, int nout, IRoute& g) {
  g.gather = ksize == 3 ? G_C3 : G_C1;
  const int nts[3] = {6, 3, 2};
  // relative cost per output channel of the tile widths; with few reduction channels (K < 64:
  // at most 16 four-channel chunks) the 96-wide tile's fixed per-tile cost dominates
  const double eff[3] = {K < 64 ? 1.6 : 1.0, 1.3, 1.6};
  double best = 1e30;
  for (int i = 0; i < 3; ++i) {
    const int np = 16 * nts[i], nz = (nout + np - 1) / np;
    const double c = nz * np * eff[i];
    if (c < best) { best = c; g.nt = nts[i]; g.np = np; g.nz = nz; }
  }
  g.img = pack_floats(g.gather, g.np, K, 1);
  return g.img > 0;
}

// split-bf16 (DN_PREC_FP32_X6) 3x3 convs: the kernels tile 32, 48 or 96 output channels and
// 32 reduction channels (on large grids a partial last chunk of <= 16 channels costs 5 of 9
// stages, `tail`), so they take the convs that fill those tiles; small-grid K = 48 and the
// level conv (K = 4) stay on the fp32 kernels, where the padding would cost more than the
// faster matrix cores give (measured per shape)
bool x6_shape(int nout) { return nout == 32 || nout % 48 == 0; }
bool x6_takes(int K, int nout, int tail) {
  // 32-wide tiles with K < 80 were staging-bound on round 2's 8-row kernels (no gain for 32x48,
  // 32x56); the 16-row ones take K >= 48 at 0.33-0.37 of the x6 peak against the fp32 kernel's
  // 0.25-0.27 (48->32 @256^2: 1.05 -> 0.79 ms)
  if (nout == 32 && K < 80 && !(K % 4 == 0 && K >= 48)) return false;
  // 32-wide RDB growth convs with K >= 80 take a zero-padded last chunk when it cannot be
  // tail-packed (88, 120: 3 / 4 chunks, 9 / 7 % padding; on the fp32 kernel they ran at ~60 %
  // of the x6 rate of their 80- / 112-channel neighbours)
  if (nout == 32 && K % 4 == 0) return true;
  // likewise the data gradients of those convs (K = 32 = the growth, nout = 80..144 of the dense
  // concatenation: 48-channel output blocks, the last one partial) and the 24-channel top
  // level's 72 -> 24 (a 32-wide tile, 8 outputs idle): the fp32 kernel ran them at 0.19-0.22 of
  // the x6 ceiling
  if (K == 32 && nout >= 80 && nout % 8 == 0) return true;
  if (nout == 24 && K >= 72 && K % 4 == 0) return true;
  // round 6: the top level's 24 -> 24 (ResBlock) and 24 -> 32 (first growth conv) too, one
  // zero-padded chunk: fwd3 -0.25 ms/step against the fp32 kernel (profiles/r6_iunet_x624_ab.log)
  if (K == 24 && (nout == 24 || nout == 32)) return true;
  return x6_shape(nout) && (K % 32 == 0 || K >= 128 || tail) && (K > 32 || nout % 96 == 0);
}
// output-channel blocks of the wide layers: 96, or 48 where 96 would pad (144 = 3 x 48)
int x6_zc(int nout) { return nout <= 96 ? 0 : (nout % 96 == 0 ? 96 : 48); }

// The route of a k x k conv with K reduction channels and nout outputs over N x h x w pixels.
// The views count through their alignment only: x6 images tail-pack a partial last K chunk when
// the launch takes the pipelined kernel (aligned input), and x6_image_mode may add X6_W6 where
// the output / auxiliary views allow the Winograd kernel's float4 NHWC epilogue.
// false: no kernel has a weight image for this shape.
bool resolve_route(int prec, int ksize, int N, int h, int w, int K, int nout, const IView& in,
                   const IView& out, int layout, const IView& aux, IRoute& r) {
  r = IRoute{};
  if (prec == DN_PREC_FP32_X6 && ksize == 3) {
    const int zc = x6_zc(nout);
    const bool aligned = ((in.stride | in.off | K) & 3) == 0;
    const bool w6_ok = layout == OUT_NHWC && ((out.stride | out.off | nout) & 3) == 0 &&
                       (aux.o < 0 || ((aux.stride | aux.off) & 3) == 0);
    const int tail = w6_ok && aligned ? x6_image_mode(N, h, w, K, nout, zc, true)
                     : aligned && x6_pipelined(N, h, w, nout, zc) ? x6_tail_mode(K) : 0;
    if (x6_takes(K, nout, tail)) {
      const long elems = x6_pack_elems(K, nout, zc);  // bf16
      if (elems <= 0) return false;
      r.x6 = true; r.tail = tail; r.zc = zc;
      r.wp_z = x6_wp_z(K, nout, zc);
      r.floats = (elems + 1) / 2;
      return true;
    }
  }
  if (!ggeom(ksize, K, nout, r)) return false;
  r.floats = r.img * r.nz;
  return true;
}

// floats of a site's arena slot: the larger of the two precisions' images (for a 3x3 the bf16x6
// image of every shape x6_takes may route; -1 where those kernels have no tile)
long slot_floats(int ksize, int K, int nout) {
  IRoute g;
  long f = ggeom(ksize, K, nout, g) ? g.img * g.nz : -1;
  if (ksize == 3) f = std::max(f, (x6_pack_elems(K, nout, x6_zc(nout)) + 1) / 2);
  return (std::max(f, 0L) + 63) / 64 * 64;
}

// the launch of a resolved conv on its packed image wp
hipError_t run_conv(const IRoute& r, const float* wp, const View& in, int N, int h, int w, int K,
                    int nout, const float* bias, int epi, const View& out, int layout,
                    const View& aux, hipStream_t s) {
  FwdArgs a = fwd_args(in, N, h, w, K, nout, out, layout);
  a.wp = wp;
  a.bias = bias; a.epi = epi;
  set_mask(a, aux);
  if (r.x6) {
    a.x6_tail = r.tail;
    a.zc = r.zc; a.wp_z = r.wp_z;
    return launch_fwd_x6(a, s);
  }
  a.zc = r.np; a.wp_z = r.img;
  return launch_fwd_nt(r.gather, r.nt, a, s);
}

// ---- parameter layout (state_dict order of ImprovedUNet) ---------------------------------
struct Alloc {
  long off = 0;
  int convs = 0;
  IConv conv(int cout, int cin, int k, bool bias = true) {
    IConv c;
    c.cout = cout; c.cin = cin; c.k = k; c.idx = convs++;
    c.w = off; off += (long)cout * cin * k * k;
    if (bias) { c.b = off; off += cout; }
    return c;
  }
  IGN gn(int ch) {
    IGN n;
    n.C = ch; n.G = gn_groups(ch);
    n.g = off; off += ch;
    n.b = off; off += ch;
    return n;
  }
  IRdb rdb(int ch) {
    IRdb r;
    r.C = ch;
    for (int j = 0; j < 4; ++j) r.conv[j] = conv(GROWTH, ch + GROWTH * j, 3);
    r.lff = conv(ch, ch + 4 * GROWTH, 1);
    return r;
  }
  IRes res(int ch) {  // block = [conv(no bias), GN, LeakyReLU, conv(no bias), GN]
    IRes r;
    r.C = ch;
    r.c1 = conv(ch, ch, 3, false);
    r.n1 = gn(ch);
    r.c2 = conv(ch, ch, 3, false);
    r.n2 = gn(ch);
    return r;
  }
};

}  // namespace

// ---- GroupNorm and the blocked weight gradient: launch sequences shared with capi_blocks.cpp
long gn_part_doubles(int N, long P, int C) { return 2L * N * chan_sums_splits(N, P) * C; }

dn_status gn_forward(const View& z, int N, long P, int C, int G, const float* gamma,
                     const float* beta, int act, const View* res, const View& y, float* stats,
                     double* part, float* scale, float* shift, hipStream_t s) {
  const int S = chan_sums_splits(N, P);
  DN_TRY(launch_chan_sums(z, nullptr, N, P, C, S, part, s));
  DN_TRY(launch_gn_fwd_fin(part, S, N, C, G, P, GN_EPS, gamma, beta, stats, scale, shift, s));
  DN_TRY(launch_affine(z, nullptr, scale, nullptr, shift, act, res, y, N, P, C, s));
  return DN_OK;
}

dn_status gn_backward(const View& dy, const View& z, int N, long P, int C, int G,
                      const float* gamma, const float* stats, const View& dz, float* dgamma,
                      float* dbeta, double* part, float* ca, float* cb, float* cc, hipStream_t s) {
  const int S = chan_sums_splits(N, P);
  DN_TRY(launch_chan_sums(dy, &z, N, P, C, S, part, s));
  DN_TRY(launch_gn_bwd_fin(part, S, N, C, G, P, gamma, stats, ca, cb, cc, dgamma, dbeta, s));
  DN_TRY(launch_affine(dy, &z, ca, cb, cc, 0, nullptr, dz, N, P, C, s));
  return DN_OK;
}

bool iunet_build_params(const dn_unet_cfg& c, IParams& P, std::string& err) {
  if (c.in_nc < 1 || c.in_nc > 3 || c.out_nc < 1 || c.out_nc > 4) {
    err = "ImprovedUNet: in_nc must be 1..3 and out_nc 1..4";
    return false;
  }
  if (c.n_feature != 48) {
    err = "ImprovedUNet: only n_feature=48 is built (train.py:30 default)";
    return false;
  }
  P = IParams{};
  P.C = c.in_nc; P.OC = c.out_nc; P.nf = 48;
  Alloc A;
  P.ne0 = A.conv(48, P.C, 3);  // noise_estimator.0 (arch_unet.py:483)
  P.ne2 = A.conv(1, 48, 3);    // noise_estimator.2 (:485)
  int nf = 48;
  for (int i = 0; i < 4; ++i) {  // downs.i = [conv, LeakyReLU, RDB, ResBlock] (:499-503)
    const int inc = i == 0 ? P.C + 1 : nf / 2;
    P.down[i].conv = A.conv(nf, inc, 3);
    P.down[i].rdb = A.rdb(nf);
    P.down[i].res = A.res(nf);
    nf *= 2;
  }
  P.brdb = A.rdb(nf / 2);  // bottle (:507)
  P.bres = A.res(nf / 2);
  nf /= 2;
  for (int k = 0; k < 4; ++k) {  // ups.k = UpBlock(nf, nf/2) (:511-513, 454-461)
    IUp& u = P.up[k];
    u.in = nf; u.out = nf / 2;
    u.ps = A.conv(4 * u.out, u.in, 3);
    u.fuse = A.conv(u.out, 3 * u.out, 3);
    u.rdb = A.rdb(u.out);
    u.res = A.res(u.out);
    nf /= 2;
  }
  P.fin = A.conv(P.OC, 24 + P.C, 3);  // final (:515)
  P.total = A.off;
  if (A.convs != kIConvs) {
    err = "ImprovedUNet: the parameter layout does not have kIConvs convolutions";
    return false;
  }
  return true;
}

bool iunet_build_plan(const dn_unet_cfg& c, int N, int H, int W, bool bwd, IPlan& p,
                      std::string& err) {
  if (!iunet_build_params(c, p.P, err)) return false;
  if (N < 1 || H < 16 || W < 16 || (H % 16) || (W % 16)) {
    err = "ImprovedUNet needs N >= 1 and H, W multiples of 16 (4 pooling levels)";
    return false;
  }
  p.N = N; p.H = H; p.W = W; p.with_bwd = bwd;
  const IParams& P = p.P;
  long off = 0;
  auto px = [&](int l) { return (long)N * (H >> l) * (W >> l); };
  auto alloc = [&](int l, int ch) {
    long o = off;
    off += (px(l) * ch + 63) / 64 * 64;
    return o;
  };
  auto allocf = [&](long n) {
    long o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  auto block = [&](IBlockBufs& b, int l, int ch) {
    b.F = alloc(l, ch + 4 * GROWTH);
    b.r = alloc(l, ch);
    b.z1 = alloc(l, ch);
    b.a1 = alloc(l, ch);
    b.z2 = alloc(l, ch);
    b.st1 = allocf(2L * N * gn_groups(ch));
    b.st2 = allocf(2L * N * gn_groups(ch));
  };
  p.x0 = alloc(0, 4);
  p.h = alloc(0, 48);
  p.xin = alloc(0, P.C);
  p.yout = alloc(0, P.OC);
  p.sig = alloc(0, 1);
  for (int i = 0; i < 4; ++i) {
    block(p.dl[i], i, 48 << i);
    if (i > 0) p.pool[i] = alloc(i, 48 << (i - 1));
  }
  block(p.bb, 4, 384);
  for (int k = 0; k < 4; ++k) {
    const int out = P.up[k].out, l = 3 - k;
    p.cc[k] = alloc(l, 3 * out);
    block(p.ul[k], l, out);
    if (k < 3) p.xu[k] = alloc(l, out);
  }
  p.xb = alloc(4, 384);
  p.cf = alloc(0, 28);
  p.sc = allocf((long)N * 384);
  p.sh = allocf((long)N * 384);
  p.gpart = allocf(2L * 2 * std::max(2048L, (long)N) * 384);  // N*S splits x 384 ch x 2 doubles
  if (bwd) {
    auto gblock = [&](IBlockBufs& b, int l, int ch) {
      b.dF = alloc(l, ch + 4 * GROWTH);
      b.dr = alloc(l, ch);
      b.dz2 = alloc(l, ch);
      b.dg1 = alloc(l, ch);
      b.dz1 = alloc(l, ch);
      for (int j = 0; j < 4; ++j) b.dzj[j] = alloc(l, GROWTH);
      b.dzf = alloc(l, ch);
    };
    for (int i = 0; i < 4; ++i) gblock(p.dl[i], i, 48 << i);
    gblock(p.bb, 4, 384);
    for (int k = 0; k < 4; ++k) {
      const int out = P.up[k].out, l = 3 - k;
      p.dcc[k] = alloc(l, 3 * out);
      gblock(p.ul[k], l, out);
      if (k < 3) p.dxu[k] = alloc(l, out);
    }
    p.dxb = alloc(4, 384);
    p.dzfin = alloc(0, 4);
    for (int k = 0; k < 4; ++k)  // unshuffled PixelShuffle gradient of up block k (4 x out ch)
      p.dps[k] = alloc(4 - k, 4 * P.up[k].out);
    p.dpool = alloc(1, 48);     // largest pooled-input gradient: level 1 (48 ch at H/2)
    for (int i = 0; i < 4; ++i)  // level-conv pre-activation gradients
      p.dza[i] = alloc(i, 48 << i);
    p.dsg = alloc(0, 4);
    p.dh = alloc(0, 48);
    p.ca = allocf((long)N * 384);
    p.cb = allocf((long)N * 384);
    p.ccf = allocf((long)N * 384);
  }
  // ---- the conv sites: every convolution's place in the dataflow, stated once (after every
  // buffer they name is allocated; the arena and the slab, sized from them, follow) ----
  for (ISite& s : p.site) s = ISite{};
  auto V = [](long o, int stride, int ch = 0) { return IView{o, stride, ch}; };
  const IView none;
  auto input = [&](const IConv& L, int l, IView in) {
    ISite& s = p.site[L.idx];
    s.L = L; s.lvl = l; s.in = in;
  };
  auto fwd = [&](const IConv& L, int l, IView in, int epi, IView out, int layout = OUT_NHWC,
                 IView aux = IView{}) {
    input(L, l, in);
    ISite& s = p.site[L.idx];
    s.epi = epi; s.out = out; s.layout = layout; s.aux = aux;
  };
  // gradients from g = dL/d(conv output): the blocked weight gradient, and the data gradient of
  // the first nout input channels into dx (plans with a backward only: the views are its buffers)
  auto grad = [&](const IConv& L, IView g, int nout, int depi, IView daux, IView dx) {
    if (!bwd) return;
    ISite& s = p.site[L.idx];
    s.wmode = L.k == 3 ? W_C3 : W_C1;
    s.g = g; s.nout = nout; s.depi = depi; s.daux = daux; s.dx = dx;
  };
  // F[:, :C] holds the block input; the growth convs read prefixes of F and write their slice,
  // lff adds the input back (out = x + lff(F)) into b.r
  auto rdb = [&](const IRdb& R, const IBlockBufs& b, int l) {
    const int C = R.C, FS = C + 4 * GROWTH;
    const IView F = V(b.F, FS), dF = V(b.dF, FS);
    for (int j = 0; j < 4; ++j) {
      const int o = C + GROWTH * j;
      fwd(R.conv[j], l, F, EPI_BIAS_ACT, V(b.F, FS, o));
      grad(R.conv[j], V(b.dzj[j], GROWTH), o, EPI_ACCUM, none, dF);
    }
    fwd(R.lff, l, F, EPI_BIAS_ADD, V(b.r, C), OUT_NHWC, F);
    grad(R.lff, V(b.dr, C), FS, EPI_PLAIN, none, dF);
  };
  // r -> conv1 -> z1 -GN1, leaky-> a1 -> conv2 -> z2 -GN2-> (+ r); dout = the gradient of the
  // block's output: d r = conv1^T(dz1) + dout (the residual; EPI_BIAS_ADD with no bias)
  auto res = [&](const IRes& R, const IBlockBufs& b, int l, IView dout) {
    const int C = R.C;
    fwd(R.c1, l, V(b.r, C), EPI_PLAIN, V(b.z1, C));
    grad(R.c1, V(b.dz1, C), C, EPI_BIAS_ADD, dout, V(b.dr, C));
    fwd(R.c2, l, V(b.a1, C), EPI_PLAIN, V(b.z2, C));
    grad(R.c2, V(b.dz2, C), C, EPI_MASK, V(b.a1, C), V(b.dg1, C));
  };
  // ne0, ne2 and the final conv run their forward on the thin kernels (launched by the pass), ne0
  // and the level-0 conv (C + 1 < 16 input channels) their whole backward
  input(P.ne0, 0, none);
  input(P.ne2, 0, V(p.h, 48));
  grad(P.ne2, V(p.dsg, 4), 48, EPI_MASK, V(p.h, 48), V(p.dh, 48));
  for (int i = 0; i < 4; ++i) {
    const IConv& L = P.down[i].conv;
    const int out = P.up[3 - i].out;  // s_i lives in the skip slice of up block 3-i's concat
    fwd(L, i, i == 0 ? V(p.x0, 4) : V(p.pool[i], L.cin), EPI_BIAS_ACT,
        V(p.dl[i].F, L.cout + 4 * GROWTH));
    if (i > 0) grad(L, V(p.dza[i], L.cout), L.cin, EPI_PLAIN, none, V(p.dpool, L.cin));
    rdb(P.down[i].rdb, p.dl[i], i);
    res(P.down[i].res, p.dl[i], i, V(p.dcc[3 - i], 3 * out, out));
  }
  rdb(P.brdb, p.bb, 4);
  res(P.bres, p.bb, 4, V(p.dxb, 384));
  for (int k = 0; k < 4; ++k) {
    const IUp& u = P.up[k];
    const int l = 3 - k, out = u.out;
    // conv_ps reads the bottle output or the previous up block's, one level below its block
    fwd(u.ps, l + 1, k == 0 ? V(p.xb, 384) : V(p.xu[k - 1], u.in), EPI_BIAS, V(p.cc[k], 3 * out),
        OUT_PS);
    grad(u.ps, V(p.dps[k], 4 * out), u.in, EPI_PLAIN, none,
         k == 0 ? V(p.dxb, 384) : V(p.dxu[k - 1], u.in));
    fwd(u.fuse, l, V(p.cc[k], 3 * out), EPI_BIAS_ACT, V(p.ul[k].F, out + 4 * GROWTH));
    grad(u.fuse, V(p.ul[k].dzf, out), 3 * out, EPI_PLAIN, none, V(p.dcc[k], 3 * out));
    rdb(u.rdb, p.ul[k], l);
    // the last block's output gradient: the final conv's data gradient, in dh[:, :24] (dh's 48
    // channels are free until the noise estimator's backward)
    res(u.res, p.ul[k], l, k < 3 ? V(p.dxu[k], out) : V(p.dh, 24));
  }
  input(P.fin, 0, V(p.cf, 28));
  grad(P.fin, V(p.dzfin, 4), 24, EPI_PLAIN, none, V(p.dh, 24));  // x_up3's 24 of the concat
  // packed-weight arena: the forward's images, one slot per site that launches on the generic
  // kernels (the backward's data-gradient images reuse the region).  A pass packs the images its
  // routes name in a few batched launches first.
  long fsum = 0, bsum = 0, slab = 0;
  for (const ISite& s : p.site) {
    if (s.out.o >= 0) fsum += slot_floats(s.L.k, s.L.cin, s.L.cout);
    if (s.nout) bsum += slot_floats(s.L.k, s.L.cout, s.nout);
    if (s.wmode >= 0)
      slab = std::max(slab, wgrad_size(s.wmode, N, H >> s.lvl, W >> s.lvl, s.L.cin, s.L.cout, true).floats);
  }
  p.pack_floats = std::max(fsum, bsum);
  p.pack = allocf(p.pack_floats);
  if (bwd) {
    // weight-gradient slab: 64 zero floats + max over sites of splits x (W + b); the level-0
    // conv's thin kernel
    const int st = enc0_wgrad_splits(N, H, W);
    slab = std::max(slab, (long)st * (48L * (P.C + 1) * 9 + 48));
    p.slab = off;
    off += 64 + (slab + 63) / 64 * 64;
    p.slab_floats = slab;
  }
  p.total_floats = off;
  return true;
}

void iunet_debug_buffers(const IPlan& p, const BufferVisitor& add) {
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
  if (!p.with_bwd) return;
  for (int i = 0; i < 4; ++i) {
    const int ch = 48 << i;
    add(p.dl[i].dr, ch, i); add(p.dl[i].dz2, ch, i); add(p.dl[i].dg1, ch, i);
    add(p.dl[i].dz1, ch, i);
  }
  for (int k = 0; k < 4; ++k) add(p.dcc[k], 3 * p.P.up[k].out, 3 - k);
}

// ------------------------------------------------------------------------------------
// routes, packing and the launches of one conv site
// ------------------------------------------------------------------------------------
namespace {

struct IRoutes { IRoute r[kIConvs]; };

const View kNone{nullptr, 0, 0};

struct Ctx {
  const IPlan& p;
  const IRoutes& R;
  const float* prm;
  float* ws;
  hipStream_t s;
  int prec;
  BwdStreams* bs;  // backward: the weight gradients' stream and its fork (s2 == s on one stream)
  View V(long o, int stride, int off = 0) const { return View{ws + o, stride, off}; }
  View V(const IView& v) const { return v.o < 0 ? kNone : View{ws + v.o, v.stride, v.off}; }
  const ISite& site(const IConv& c) const { return p.site[c.idx]; }
  const float* image(const IConv& c) const { return ws + p.pack + R.r[c.idx].off; }
  const float* Wt(const IConv& c) const { return prm + c.w; }
  const float* Bs(const IConv& c) const { return c.b >= 0 ? prm + c.b : nullptr; }
};

// places r's image behind the pass's earlier ones in the arena
void place(IRoute& r, long& next) {
  r.off = next;
  next += (r.floats + 63) / 64 * 64;
}

// The forward route of every site that launches on the generic kernels, in the order the pass
// runs them (= state_dict order).  The arena holds them: every slot is at least its route's image.
dn_status iunet_fwd_routes(const IPlan& p, int prec, IRoutes& R) {
  long next = 0;
  for (int i = 0; i < kIConvs; ++i) {
    const ISite& s = p.site[i];
    if (s.out.o < 0) continue;
    if (!resolve_route(prec, s.L.k, p.N, p.H >> s.lvl, p.W >> s.lvl, s.L.cin, s.L.cout, s.in,
                       s.out, s.layout, s.aux, R.r[i])) {
      set_error("ImprovedUNet: no weight image for a forward conv");
      return DN_ERR_ARG;
    }
    place(R.r[i], next);
  }
  return DN_OK;
}

// ... and the data-gradient routes (reduction over the conv's outputs, the first nout input
// channels out), the backward's order: the forward's reversed
dn_status iunet_bwd_routes(const IPlan& p, int prec, IRoutes& R) {
  long next = 0;
  for (int i = kIConvs - 1; i >= 0; --i) {
    const ISite& s = p.site[i];
    if (!s.nout) continue;
    if (!resolve_route(prec, s.L.k, p.N, p.H >> s.lvl, p.W >> s.lvl, s.L.cout, s.nout, s.g, s.dx,
                       OUT_NHWC, s.daux, R.r[i])) {
      set_error("ImprovedUNet: no weight image for a data gradient");
      return DN_ERR_ARG;
    }
    place(R.r[i], next);
  }
  return DN_OK;
}

// packs the images the pass's routes name, in the pass's order (24 images per launch)
dn_status pack_images(const Ctx& c, bool bwd) {
  PackBatch pb;
  for (int n = 0; n < kIConvs; ++n) {
    const int i = bwd ? kIConvs - 1 - n : n;
    const IRoute& r = c.R.r[i];
    if (!r.floats) continue;
    const IConv& L = c.p.site[i].L;
    // forward image of the weight [cout][cin][k][k]: reduction K = cin, outputs = cout; data
    // gradient: reduction over cout, outputs = the first nout input channels
    const int K = bwd ? L.cout : L.cin, nout = bwd ? c.p.site[i].nout : L.cout;
    WView wv = bwd ? conv_dgrad_view(c.Wt(L), L.cin, L.k) : conv_fwd_view(c.Wt(L), L.cin, L.k);
    float* out = c.ws + c.p.pack + r.off;
    PackJob j;
    if (!r.x6) wv.sZ = (long)r.np * wv.sN;
    if (!(r.x6 ? pack_job_x6(wv, K, nout, r.zc, out, r.tail, j)
               : pack_job(r.gather, wv, K, r.np, r.nz, out, r.np, nout, j))) {
      set_error("ImprovedUNet: no weight image for a conv");
      return DN_ERR_ARG;
    }
    DN_TRY(pack_add(pb, j, c.s));
  }
  DN_TRY(pack_flush(pb, c.s));
  return DN_OK;
}

double conv_flops(int N, int h, int w, int cout, int cin, int k) {
  return 2.0 * N * h * w * (double)cout * cin * k * k;
}

dn_status conv_fwd(const Ctx& c, const IConv& L) {
  const ISite& s = c.site(L);
  const int N = c.p.N, h = c.p.H >> s.lvl, w = c.p.W >> s.lvl;
  const OpTimer timer(c.s, L.k == 3 ? "fwd3" : "fwd1", conv_flops(N, h, w, L.cout, L.cin, L.k),
                      L.cin, L.cout, h, w, N);
  DN_TRY(run_conv(c.R.r[L.idx], c.image(L), c.V(s.in), N, h, w, L.cin, L.cout, c.Bs(L), s.epi,
                  c.V(s.out), s.layout, c.V(s.aux), c.s));
  return DN_OK;
}

// dx (the site's first nout input channels) = conv^T(g) with its epilogue (daux = mask / residual)
dn_status dgrad_g(const Ctx& c, const IConv& L) {
  const ISite& s = c.site(L);
  const int N = c.p.N, h = c.p.H >> s.lvl, w = c.p.W >> s.lvl;
  const OpTimer timer(c.s, L.k == 3 ? "dgrad3" : "dgrad1", conv_flops(N, h, w, s.nout, L.cout, L.k),
                      L.cout, s.nout, h, w, N);
  DN_TRY(run_conv(c.R.r[L.idx], c.image(L), c.V(s.g), N, h, w, L.cout, s.nout, nullptr, s.depi,
                  c.V(s.dx), OUT_NHWC, c.V(s.daux), c.s));
  return DN_OK;
}

// dW (+ db) of a conv from g = dL/d(conv output) and its forward input; written into dprm
dn_status wgrad_g(const Ctx& c, float* dprm, const IConv& L) {
  const ISite& s = c.site(L);
  const int N = c.p.N, h = c.p.H >> s.lvl, w = c.p.W >> s.lvl;
  // on the side stream, behind the main stream's work so far (g is its latest output)
  const hipStream_t s2 = c.bs->s2;
  DN_TRY(c.bs->fork());
  const bool bias = L.b >= 0;
  if (bias && L.b != L.w + (long)L.cout * L.cin * wgrad_taps(s.wmode)) {
    set_error("ImprovedUNet: bias does not follow its weight");
    return DN_ERR_ARG;
  }
  // the blocked family (any Cout in output-channel blocks, views with a channel offset); the one
  // slab serves every layer in turn, so each reduction is launched behind its weight gradient
  const View g = c.V(s.g), x = c.V(s.in);
  WgradShape sh = wgrad_shape(s.wmode, N, h, w, L.cin, L.cout, g.stride, g.off, x.stride, x.off,
                              c.prec == DN_PREC_FP32_X6);
  sh.blocked = true;
  sh.bias = bias;
  return wgrad_run(wgrad_route(sh), g.p, x.p, dprm + L.w, c.ws + c.p.slab, nullptr, s2);
}

dn_status gn_fwd(const Ctx& c, const IGN& g, const View& z, int h, int w, float* stats, int act,
                 const View* res, const View& out) {
  const OpTimer timer(c.s, "gn", 0.0, 1, g.C, h, w, c.p.N);
  return gn_forward(z, c.p.N, (long)h * w, g.C, g.G, c.prm + g.g, c.prm + g.b, act, res, out, stats,
                    reinterpret_cast<double*>(c.ws + c.p.gpart), c.ws + c.p.sc, c.ws + c.p.sh,
                    c.s);
}

dn_status gn_bwd(const Ctx& c, float* dprm, const IGN& g, const View& dy, const View& z, int h,
                 int w, const float* stats, const View& dz) {
  const OpTimer timer(c.s, "gnbwd", 0.0, 1, g.C, h, w, c.p.N);
  return gn_backward(dy, z, c.p.N, (long)h * w, g.C, g.G, c.prm + g.g, stats, dz, dprm + g.g,
                     dprm + g.b, reinterpret_cast<double*>(c.ws + c.p.gpart), c.ws + c.p.ca,
                     c.ws + c.p.cb, c.ws + c.p.ccf, c.s);
}

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
// F[:, :C] holds the block input; writes the RDB output to b.r
dn_status rdb_fwd(const Ctx& c, const IRdb& R) {
  for (int j = 0; j < 4; ++j)
    if (dn_status st = conv_fwd(c, R.conv[j])) return st;
  return conv_fwd(c, R.lff);
}

// GN1 takes conv1's output to conv2's input, GN2 conv2's output (+ the block input) to `out`
dn_status res_fwd(const Ctx& c, const IRes& R, const IBlockBufs& b, int h, int w, const View& out) {
  const ISite &s1 = c.site(R.c1), &s2 = c.site(R.c2);
  const View r = c.V(s1.in);
  if (dn_status st = conv_fwd(c, R.c1)) return st;
  if (dn_status st = gn_fwd(c, R.n1, c.V(s1.out), h, w, c.ws + b.st1, 1, nullptr, c.V(s2.in)))
    return st;
  if (dn_status st = conv_fwd(c, R.c2)) return st;
  return gn_fwd(c, R.n2, c.V(s2.out), h, w, c.ws + b.st2, 0, &r, out);
}

WView thin_view(const float* w, int cin) {  // weight [o][cin][3][3] as W(o, k, t)
  WView v{};
  v.w = w; v.off = 0; v.sN = (long)cin * 9; v.sK = 9; v.sT = 1; v.taps = 9; v.flip = 0;
  return v;
}

dn_status forward_body(const Ctx& c, const float* x, float* y) {
  const IPlan& p = c.p;
  const float* prm = c.prm;
  float* ws = c.ws;
  const hipStream_t s = c.s;
  const IParams& P = p.P;
  const int N = p.N, H = p.H, W = p.W, C = P.C;
  // noise estimator: h = leaky(ne0(x)) (also writes x into x0[:, :C], zeros x0[:, C:4])
  DN_TRY(launch_enc0_fwd(x, N, C, H, W, prm + P.ne0.w, prm + P.ne0.b, ws + p.h, ws + p.x0, 4, 0, 4,
                         nullptr, s));
  DN_TRY(launch_conv3_thin(c.V(p.h, 48), N, H, W, 48, thin_view(prm + P.ne2.w, 48), prm + P.ne2.b,
                           TE_SIGMOID, kNone, c.V(p.x0, 4, C), 0, 1, s));
  if (p.with_bwd) {
    DN_TRY(hipMemcpyAsync(ws + p.xin, x, sizeof(float) * (size_t)N * C * H * W,
                          hipMemcpyDeviceToDevice, s));
    DN_TRY(launch_conv3_thin(c.V(p.h, 48), N, H, W, 48, thin_view(prm + P.ne2.w, 48),
                             prm + P.ne2.b, TE_SIGMOID, kNone, View{ws + p.sig, 0, 0}, 1, 1, s));
  }
  DN_TRY(launch_nchw_to_slice(x, N, C, H, W, ws + p.cf, 28, 24, 28, s));  // final concat input
  // encoder
  for (int i = 0; i < 4; ++i) {
    const ILevel& L = P.down[i];
    const int h = H >> i, w = W >> i, nf = L.conv.cout;
    if (dn_status st = conv_fwd(c, L.conv)) return st;
    if (dn_status st = rdb_fwd(c, L.rdb)) return st;
    const int k = 3 - i, out = P.up[k].out;  // skip slice of up block k's concat
    const View skip = c.V(p.cc[k], 3 * out, out);
    if (dn_status st = res_fwd(c, L.res, p.dl[i], h, w, skip)) return st;
    const View dst = i < 3 ? c.V(p.pool[i + 1], nf) : c.V(p.bb.F, 384 + 4 * GROWTH);
    DN_TRY(launch_vpool_fwd(skip, N, h, w, nf, dst, s));
  }
  // bottleneck
  if (dn_status st = rdb_fwd(c, P.brdb)) return st;
  if (dn_status st = res_fwd(c, P.bres, p.bb, H >> 4, W >> 4, c.V(p.xb, 384))) return st;
  // decoder
  for (int k = 0; k < 4; ++k) {
    const IUp& u = P.up[k];
    const int l = 3 - k, h = H >> l, w = W >> l;
    if (dn_status st = conv_fwd(c, u.ps)) return st;
    if (dn_status st = conv_fwd(c, u.fuse)) return st;
    if (dn_status st = rdb_fwd(c, u.rdb)) return st;
    const View o = k < 3 ? c.V(p.xu[k], u.out) : c.V(p.cf, 28);
    if (dn_status st = res_fwd(c, u.res, p.ul[k], h, w, o)) return st;
  }
  DN_TRY(launch_conv3_thin(c.V(p.cf, 28), N, H, W, 24 + C, thin_view(prm + P.fin.w, 24 + C),
                           prm + P.fin.b, TE_SIGMOID, kNone, View{y, 0, 0}, 1, P.OC, s));
  if (p.with_bwd)
    DN_TRY(hipMemcpyAsync(ws + p.yout, y, sizeof(float) * (size_t)N * P.OC * H * W,
                          hipMemcpyDeviceToDevice, s));
  return DN_OK;
}

}  // namespace

// Every pass: resolve the routes, pack the images they name, run on them.
dn_status iunet_forward(const IPlan& p, const float* prm, const float* x, float* y, float* ws,
                        hipStream_t s, int prec) {
  const StreamDeviceGuard device_guard(s);
  if (prec != DN_PREC_FP32 && prec != DN_PREC_FP32_X6) return DN_ERR_ARG;
  IRoutes R;
  if (dn_status st = iunet_fwd_routes(p, prec, R)) return st;
  const Ctx c{p, R, prm, ws, s, prec, nullptr};
  if (dn_status st = pack_images(c, false)) return st;
  return forward_body(c, x, y);
}

// ------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------
namespace {

// ResBlock backward: the block's output gradient (c1's residual view) -> b.dr (gradient of the
// block input r)
dn_status res_bwd(const Ctx& c, float* dprm, const IRes& R, const IBlockBufs& b, int h, int w) {
  const ISite &s1 = c.site(R.c1), &s2 = c.site(R.c2);
  if (dn_status st = gn_bwd(c, dprm, R.n2, c.V(s1.daux), c.V(s2.out), h, w, c.ws + b.st2, c.V(s2.g)))
    return st;
  if (dn_status st = wgrad_g(c, dprm, R.c2)) return st;
  if (dn_status st = dgrad_g(c, R.c2)) return st;
  if (dn_status st = gn_bwd(c, dprm, R.n1, c.V(s2.dx), c.V(s1.out), h, w, c.ws + b.st1, c.V(s1.g)))
    return st;
  if (dn_status st = wgrad_g(c, dprm, R.c1)) return st;
  return dgrad_g(c, R.c1);
}

// RDB backward: b.dr (gradient of the RDB output) -> b.dF[:, :C] (gradient of the block input)
dn_status rdb_bwd(const Ctx& c, float* dprm, const IRdb& R, const IBlockBufs& b, int h, int w) {
  const int C = R.C, FS = C + 4 * GROWTH;
  const long npx = (long)c.p.N * h * w;
  if (dn_status st = wgrad_g(c, dprm, R.lff)) return st;
  if (dn_status st = dgrad_g(c, R.lff)) return st;
  DN_TRY(launch_vadd(c.V(b.dF, FS), c.V(b.dr, C), npx, C, c.s));  // out = x + lff(...)
  for (int j = 3; j >= 0; --j) {
    const int o = C + GROWTH * j;
    DN_TRY(launch_vmask(c.V(b.dzj[j], GROWTH), c.V(b.dF, FS, o), c.V(b.F, FS, o), npx, GROWTH, c.s));
    if (dn_status st = wgrad_g(c, dprm, R.conv[j])) return st;
    if (dn_status st = dgrad_g(c, R.conv[j])) return st;
  }
  return DN_OK;
}

dn_status backward_body(const Ctx& c, const float* dy, float* dprm) {
  const IPlan& p = c.p;
  const float* prm = c.prm;
  float* ws = c.ws;
  const hipStream_t s = c.s;
  const hipStream_t s2 = c.bs->s2;
  const IParams& P = p.P;
  const int N = p.N, H = p.H, W = p.W, C = P.C, OC = P.OC;
  const long HW = (long)H * W;
  // final: dz = dy * y(1-y)  (stride-4 NHWC), then its weight / data gradients
  DN_TRY(launch_dsigmoid_nchw(ws + p.yout, dy, N, OC, HW, ws + p.dzfin, 4, s));
  if (dn_status st = wgrad_g(c, dprm, P.fin)) return st;
  // gradient of x_up3 = the first 24 channels of the final concat (the input slice needs none)
  DN_TRY(hipMemsetAsync(ws + p.dsg, 0, sizeof(float) * 4 * (size_t)N * HW, s));
  if (dn_status st = dgrad_g(c, P.fin)) return st;
  // decoder, last block first
  for (int k = 3; k >= 0; --k) {
    const IUp& u = P.up[k];
    const int l = 3 - k, h = H >> l, w = W >> l, out = u.out, FS = out + 4 * GROWTH;
    const IBlockBufs& b = p.ul[k];
    if (dn_status st = res_bwd(c, dprm, u.res, b, h, w)) return st;
    if (dn_status st = rdb_bwd(c, dprm, u.rdb, b, h, w)) return st;
    // f = leaky(fuse(cc)): dz = dF[:, :out] * leaky'(f)
    DN_TRY(launch_vmask(c.V(b.dzf, out), c.V(b.dF, FS), c.V(b.F, FS), (long)N * h * w, out, s));
    if (dn_status st = wgrad_g(c, dprm, u.fuse)) return st;
    if (dn_status st = dgrad_g(c, u.fuse)) return st;
    // PixelShuffle backward, then conv_ps (input: bottle output or the previous up block)
    DN_TRY(launch_unshuffle(c.V(p.dcc[k], 3 * out), N, h / 2, w / 2, out, ws + p.dps[k], s));
    if (dn_status st = wgrad_g(c, dprm, u.ps)) return st;
    if (dn_status st = dgrad_g(c, u.ps)) return st;
  }
  // bottleneck: its input is pool(s_3), living in bb.F[:, :384]
  if (dn_status st = res_bwd(c, dprm, P.bres, p.bb, H >> 4, W >> 4)) return st;
  if (dn_status st = rdb_bwd(c, dprm, P.brdb, p.bb, H >> 4, W >> 4)) return st;
  View dpooled = c.V(p.bb.dF, 384 + 4 * GROWTH);  // d x_4 (first 384 channels)
  // encoder, deepest level first
  for (int i = 3; i >= 0; --i) {
    const ILevel& L = P.down[i];
    const int h = H >> i, w = W >> i, nf = L.conv.cout, FS = nf + 4 * GROWTH;
    const IBlockBufs& b = p.dl[i];
    const int k = 3 - i, out = P.up[k].out;
    const View skip = c.V(p.cc[k], 3 * out, out), dskip = c.V(p.dcc[k], 3 * out, out);
    // d s_i = (skip gradient from the fuse conv) + maxpool backward of d x_{i+1}
    DN_TRY(launch_vpool_bwd_acc(skip, N, h, w, nf, dpooled, dskip, s));
    if (dn_status st = res_bwd(c, dprm, L.res, b, h, w)) return st;
    if (dn_status st = rdb_bwd(c, dprm, L.rdb, b, h, w)) return st;
    const View dza = c.V(p.dza[i], nf);
    DN_TRY(launch_vmask(dza, c.V(b.dF, FS), c.V(b.F, FS), (long)N * h * w, nf, s));
    if (i > 0) {
      if (dn_status st = wgrad_g(c, dprm, L.conv)) return st;
      if (dn_status st = dgrad_g(c, L.conv)) return st;
      dpooled = c.V(p.dpool, L.conv.cin);
    } else {
      // level-0 conv: input x0 = [x | sigma] with C+1 < 16 channels -> the thin wgrad kernel on
      // the NCHW input (channels [0, C)) and sigma map (channel C), into one slab
      float* slab = ws + p.slab;
      const long n = 48L * (C + 1) * 9 + 48;
      const int st = enc0_wgrad_splits(N, H, W);
      DN_TRY(c.bs->fork());
      DN_TRY(launch_wgrad_c3_thin(ws + p.dza[0], 48, ws + p.xin, N, C, H, W, slab, n, C + 1, 0, 1,
                                  st, s2));
      DN_TRY(launch_wgrad_c3_thin(ws + p.dza[0], 48, ws + p.sig, N, 1, H, W, slab, n, C + 1, C, 0,
                                  st, s2));
      DN_TRY(launch_reduce(slab, n, st, n, dprm + L.conv.w, s2));
      // d sigma (channel C of x0) through the sigmoid: flipped weight column ci = C
      WView fv{};
      fv.w = prm + L.conv.w; fv.off = (long)C * 9; fv.sN = 9; fv.sK = (long)(C + 1) * 9;
      fv.sT = 1; fv.taps = 9; fv.flip = 1;
      DN_TRY(launch_conv3_thin(dza, N, H, W, 48, fv, nullptr, TE_DSIG, c.V(p.x0, 4, C),
                               c.V(p.dsg, 4), 0, 1, s));
    }
  }
  // noise estimator: ne2 (48 -> 1) and ne0 (C -> 48)
  if (dn_status st = wgrad_g(c, dprm, P.ne2)) return st;
  if (dn_status st = dgrad_g(c, P.ne2)) return st;
  {
    float* slab = ws + p.slab;
    const long n = 48L * C * 9 + 48;
    const int st = enc0_wgrad_splits(N, H, W);
    DN_TRY(c.bs->fork());
    DN_TRY(launch_wgrad_c3_thin(ws + p.dh, 48, ws + p.xin, N, C, H, W, slab, n, C, 0, 1, st, s2));
    DN_TRY(launch_reduce(slab, n, st, n, dprm + P.ne0.w, s2));
  }
  // the caller's stream continues after every weight gradient (nothing ran on the reduction stream)
  DN_TRY(c.bs->join(/*reductions=*/false));
  return DN_OK;
}

}  // namespace

dn_status iunet_backward(const IPlan& p, const float* prm, const float* dy, float* dprm, float* ws,
                         hipStream_t s, int prec) {
  const StreamDeviceGuard device_guard(s);
  if (prec != DN_PREC_FP32 && prec != DN_PREC_FP32_X6) return DN_ERR_ARG;
  // The weight gradients (and their slab reductions) run on a side stream beside the
  // data-gradient chain (DN_BWD_STREAMS=0 or launch profiling: one stream).  Each is forked after
  // the launch that produced its output gradient; every buffer one reads (the forward's
  // activations, dz2 / dz1 / dr / dzf of a block, dzj[j], dps[k], dza[i], dzfin, dsg, dh once
  // written) is not rewritten later in the pass, and only they use the slab.  Joined at the end.
  BwdStreams bs(s);
  IRoutes R;
  if (dn_status st = iunet_bwd_routes(p, prec, R)) return st;
  const Ctx c{p, R, prm, ws, s, prec, &bs};
  if (dn_status st = pack_images(c, true)) return st;
  return backward_body(c, dy, dprm);
}

}  // namespace dn
