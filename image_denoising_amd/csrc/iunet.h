// Host-side plan and orchestration of ImprovedUNet (arch_unet.py:421-531) — internal.
#pragma once
#include <string>

#include "exec_common.h"

namespace dn {

// offsets (floats) of one layer's tensors in the flat parameter buffer
// (idx: the conv's position in state_dict order = its entry in IPlan::site)
struct IConv { long w = -1, b = -1; int cout = 0, cin = 0, k = 3, idx = -1; };
struct IGN { long g = -1, b = -1; int C = 0, G = 0; };
struct IRdb { IConv conv[4]; IConv lff; int C = 0; };
struct IRes { IConv c1, c2; IGN n1, n2; int C = 0; };
struct ILevel { IConv conv; IRdb rdb; IRes res; };
struct IUp { IConv ps, fuse; IRdb rdb; IRes res; int in = 0, out = 0; };

constexpr int kIConvs = 78;  // 2 (noise estimator) + 4 x 8 + 7 (bottle) + 4 x 9 + 1 (final)

struct IParams {
  int C = 1, OC = 1, nf = 48;
  IConv ne0, ne2;
  ILevel down[4];
  IRdb brdb;
  IRes bres;
  IUp up[4];
  IConv fin;
  long total = 0;
};

// activations of one RDB + ResBlock pair at one resolution
struct IBlockBufs {
  long F = 0;          // [x | o0..o3]  (C + 128 channels)
  long r = 0;          // RDB output (C)
  long z1 = 0, a1 = 0, z2 = 0;  // ResBlock conv1 out, leaky(GN1), conv2 out
  long st1 = 0, st2 = 0;        // GN stats (mean, rstd) per (n, group)
  // gradients
  // (dzj per growth conv, dzf = the up block's fuse-conv gradient: the weight gradients read
  // them on the side stream while the data-gradient chain goes on)
  long dF = 0, dr = 0, dz2 = 0, dg1 = 0, dz1 = 0, dzj[4] = {0, 0, 0, 0}, dzf = 0;
};

// a strided NHWC view of a workspace buffer: offset (floats; < 0: none), pixel stride, channel offset
struct IView { long o = -1; int stride = 0, off = 0; };

// Where one convolution sits in the dataflow: what its forward, data-gradient and weight-gradient
// launches read and write.  The passes look a conv's site up by IConv::idx; the weight gradient's
// x operand IS the forward input `in`.
struct ISite {
  IConv L;
  int lvl = 0;             // runs at (H >> lvl) x (W >> lvl); conv_ps: one level below its block
  IView in;                // forward input
  IView out, aux;          // forward on the generic kernels (out.o < 0: a thin kernel, launched
  int epi = 0, layout = 0; //   by the pass itself); aux = EPI_BIAS_ADD's residual
  int wmode = -1;          // weight gradient W_C3 / W_C1 on the blocked kernels (-1: thin, as above)
  IView g;                 // dL/d(conv output): read by the weight and the data gradient
  int nout = 0, depi = 0;  // data gradient of the first nout input channels (0: none) into dx;
  IView daux, dx;          //   daux = EPI_MASK's saved activation / EPI_BIAS_ADD's residual
};

struct IPlan {
  IParams P;
  ISite site[kIConvs];
  int N = 0, H = 0, W = 0;
  bool with_bwd = false;
  long x0 = 0, h = 0;                 // [x, sigma, 0] (stride 4); noise-estimator hidden (48)
  long xin = 0, yout = 0, sig = 0;    // NCHW copies of the input / output, sigma map (NCHW)
  IBlockBufs dl[4], bb, ul[4];        // down levels, bottle, up blocks
  long pool[4] = {0, 0, 0, 0};        // pooled input of down level i (i >= 1)
  long cc[4] = {0, 0, 0, 0};          // up-block concat [u | skip]  (3*out)
  long xb = 0;                        // bottle output (384)
  long xu[3] = {0, 0, 0};             // up-block outputs 0..2
  long cf = 0;                        // final concat [x_up3 (24) | x (C) | 0]  stride 28
  long sc = 0, sh = 0;                // GN scale / shift scratch [N * 384]
  long gpart = 0;                     // GN partial sums (doubles)
  long pack = 0, pack_floats = 0;     // packed-weight arena (a pass's weight images, one per site)
  // gradients
  long dzfin = 0, dcc[4] = {0, 0, 0, 0}, dps[4] = {0, 0, 0, 0}, dxu[3] = {0, 0, 0}, dxb = 0, dpool = 0;
  long dza[4] = {0, 0, 0, 0}, dsg = 0, dh = 0, ca = 0, cb = 0, ccf = 0;
  long slab = 0, slab_floats = 0;
  long total_floats = 0;
};

// ---- launch sequences the executor shares with the op-level entry points (capi_blocks.cpp) -
// GroupNorm(G groups of C channels, eps 1e-5) over N x P pixels of NHWC views.  part holds
// gn_part_doubles(N, P, C) doubles, every coefficient array N * C floats (16-byte aligned).
// Forward: stats [N][G] (mean, rstd) saved, y = [res +] [leaky](z * scale + shift).
long gn_part_doubles(int N, long P, int C);
dn_status gn_forward(const View& z, int N, long P, int C, int G, const float* gamma,
                     const float* beta, int act, const View* res, const View& y, float* stats,
                     double* part, float* scale, float* shift, hipStream_t s);
// Backward of the normalisation alone (dy = the gradient of z * scale + shift): dz, and dgamma /
// dbeta [C] overwritten.
dn_status gn_backward(const View& dy, const View& z, int N, long P, int C, int G,
                      const float* gamma, const float* stats, const View& dz, float* dgamma,
                      float* dbeta, double* part, float* ca, float* cb, float* cc, hipStream_t s);
bool iunet_build_params(const dn_unet_cfg& c, IParams& P, std::string& err);
bool iunet_build_plan(const dn_unet_cfg& c, int N, int H, int W, bool bwd, IPlan& p,
                      std::string& err);
// dn_iunet_debug_buffers' list: the main activations, in the order
//   x0 h | per down level i: F r z1 a1 z2 | bottle: F r z1 a1 z2 | per up k: cc F r z1 a1 z2 | xb cf
//   | with a backward: per down level: dr dz2 dg1 dz1 | per up k: dcc
void iunet_debug_buffers(const IPlan& p, const BufferVisitor& add);
// prec: DN_PREC_FP32, or DN_PREC_FP32_X6 (the 3x3 convs' forward and data gradient as split
// bf16 products, conv_x6.hip)
dn_status iunet_forward(const IPlan& p, const float* prm, const float* x, float* y, float* ws,
                        hipStream_t s, int prec = DN_PREC_FP32);
dn_status iunet_backward(const IPlan& p, const float* prm, const float* dy, float* dprm,
                         float* ws, hipStream_t s, int prec = DN_PREC_FP32);

}  // namespace dn
