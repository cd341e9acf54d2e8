// The weight-gradient route (wgrad_route.cpp): which kernel, grid and slab one weight-gradient
// launch gets, decided once from what is known before a pointer exists.  The launchers
// (conv.hip, conv_x6.hip, wgrad_x6p.hip) and wgrad_run (exec_common.cpp) only read it; the plans
// and the C ABI's size functions size their slabs from wgrad_size.  Host arithmetic only.
#pragma once

namespace dn {

enum WgradKernel {
  WK_NONE = 0,  // no kernel for this shape / these views (WgradRoute::err says why)
  WK_WGRAD,     // fp32 k_wgrad<mode, ...> (conv.hip): any view
  WK_WGRAD3,    // fp32 k_wgrad3 (conv.hip): 3x3, asynchronous staging
  WK_WGRAD1,    // fp32 k_wgrad1 (conv.hip): 1x1 / deconv parities
  WK_WGRAD3S,   // bf16x6 k_wgrad3s (conv_x6.hip)
  WK_WGRAD3P,   // bf16x6 k_wgrad3p (wgrad_x6p.hip)
  WK_WGRAD3Q,   // bf16x6 k_wgrad3q (wgrad_x6p.hip): 48 -> 48 on rows >= 128 wide
  WK_WGRAD1P,   // bf16x6 k_wgrad1p (wgrad_x6p.hip): 96 -> 96 1x1 / deconv parities
};

// One launch before its pointers: dW (+ db) of a conv (W_C3 / W_C1) or deconv (W_UP2) over
// N x KH x KW pixels from the NHWC views g (Cout channels) and x (Cin channels).
struct WgradShape {
  int mode, N, KH, KW, Cin, Cout;
  int g_stride, g_off, x_stride, x_off;
  int cin_total, ci_base;  // the weight tensor's Cin and this launch's first input channel
  bool bias;               // slab rows end with the bias gradient
  bool blocked;  // any Cout in output-channel blocks over blockIdx.z (ImprovedUNet), not the fixed 96 / 48 / 16
  bool x6;       // bf16x6 arithmetic where a kernel for it fits
  int head_gnb;  // > 0: nin_b's launch with the gradient operand recomputed (WgradArgs::head_gnb)
};
// the usual launch: the weight spans exactly the view's Cin channels, with a bias, fixed family
WgradShape wgrad_shape(int mode, int N, int KH, int KW, int Cin, int Cout, int g_stride, int g_off,
                       int x_stride, int x_off, bool x6 = false);

struct WgradRoute {
  WgradShape sh;
  int kernel;      // WgradKernel
  int co_fr;       // output channels per workgroup / 16: the kernels' CO_FR (MF x NW for k_wgrad)
  int zc, nz;      // output-channel block over blockIdx.z (0: the whole layer) and their count
  int cib;         // input channels per workgroup
  int swl;         // 3x3 kernels: log2 of the stage's row segment (5: 32 px x 1 row .. 2: 4 px x 8 rows)
  int par;         // parity blocks of slab rows (deconv on k_wgrad1 / k_wgrad1p: 4), else 1
  int splits;      // pixel splits launched = slab rows per parity
  long row;        // floats of one slab row
  long floats;     // par x splits x row: the slab behind its 64 leading floats
  const char* err; // kernel == WK_NONE: the reason
};

int wgrad_taps(int mode);
// the fixed family's k_wgrad instantiations: 96 / 48 outputs (3x3, deconv), 96 / <= 16 (1x1)
bool wgrad_supported(int mode, int cout);
// Split count: `slots` resident workgroups (768 = 3 per CU on 256 CUs for the fp32 kernels, 512 = 2
// per CU for the bf16x6 ones) hold ONE round of splits x wgs workgroups (floor: a straggler
// round would double the time), a slab of at most 256 MB (row floats per split), at least two
// pixel units per split; group8 (the deconv's four parity blocks): whole groups of 8, at least 8.
int wgrad_split_policy(int slots, long wgs, long units, long row, bool group8);
// the only place that decides a launch; splits / row / floats are filled even where kernel ==
// WK_NONE for want of a k_wgrad instantiation (the size functions answer for any shape)
WgradRoute wgrad_route(const WgradShape& sh);
// When the views are not known yet: the slab that every route of this shape fits in (aligned
// or unaligned views, fp32 or bf16x6, bias or none): the most rows (par x splits) and floats.
struct WgradSize { int rows; long floats; };
WgradSize wgrad_size(int mode, int N, int KH, int KW, int Cin, int Cout, bool blocked);

}  // namespace dn
