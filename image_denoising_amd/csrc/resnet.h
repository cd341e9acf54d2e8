// Host-side RESNET plan and orchestration (internal): arch_unet.py:263-409, the UNet's layers
// without pooling or upsampling (every layer at the input resolution) and the network input added
// to nin_c's output.  Shares the UNet's kernels, views and helpers (exec_common.h).
#pragma once
#include <string>

#include "exec_common.h"

namespace dn {

// state_dict order (arch_unet.py:279-346): no up4 .. up1; up5.deconv is constructed, never used
enum ResLayerIdx {
  R_ENC0, R_ENC1, R_ENC2, R_ENC3, R_ENC4, R_ENC5, R_ENC6,
  R_UP5, R_D5A, R_D5B, R_D4A, R_D4B, R_D3A, R_D3B, R_D2A, R_D2B, R_D1A, R_D1B,
  R_NINA, R_NINB, R_NINC, R_NL
};

struct ResParamLayout {
  Layer L[R_NL];
  long total;
};

// Workspace plan (offsets in floats).  The concatenations are placements: a producer writes its
// slice of the consumer's concat buffer and the next encoder conv reads that strided slice.
//   c[5] = [a6 | a4] (96)   c[4] = [d5b | a3] (144)   c[3] = [d4b | a2]   c[2] = [d3b | a1]
//   c1 = [d2b | x | zero pad] (c1s = 96 + C rounded up to 4)
struct ResPlan {
  ResParamLayout P;
  int N, H, W, C, nf;
  bool with_bwd;
  int c1s, c1k, c1kp;
  long c1, a0, a5;
  long c[6]; int cs[6];          // concat buffers 2..5: pixel stride = channels
  long da[6];                    // dec_conv{k}a outputs, k = 2..5
  long d1a, d1b;
  long na, nb;                   // saved for the backward (-1 in forward-only plans)
  long packF[R_NL];              // fp32 forward images
  long packX[R_NL];              // bf16x6 forward images of the 3x3 layers (-1: none)
  long packH;                    // the head's nin_a | nin_b images (fp32 | bf16x6)
  long fwd_floats;
  // gradients
  long g_nb, g_na, g_d1b, g_d1a, g_c1;
  long g_c[6], g_da[6];
  long g_a[5];                   // summed gradient of a1..a4 (skip slice + enc_conv{j+1}'s)
  long g_a5, g_a0, g_t;          // g_t: enc_conv{j+1}'s masked data gradient before the sum
  long xin, dyt;                 // NCHW copy of x; NHWC transpose of dy (out_nc > 1)
  long packB[R_NL], packXB[R_NL], packHB;
  long zeros;
  long slab[R_NL];
  int splits[R_NL];
  long total_floats;
};

const char* res_layer_name(int i);
bool res_build_params(const dn_unet_cfg& c, ResParamLayout& P, std::string& err);
bool res_build_plan(const dn_unet_cfg& c, int N, int H, int W, bool bwd, ResPlan& p,
                    std::string& err);
// dn_resnet_debug_buffers' list (every level 0), in order: c1 a0 c2 c3 c4 c5 a5 d2a d3a d4a d5a d1a
// d1b | with a backward: na nb g_na g_d1b g_d1a g_c1 g_c2..g_c5 g_d2a..g_d5a g_a1..g_a4 g_a5 g_a0
void resnet_debug_buffers(const ResPlan& p, const BufferVisitor& add);
// prec: DN_PREC_FP32 or DN_PREC_FP32_X6
dn_status resnet_forward(const ResPlan& p, const float* prm, const float* x, float* y, float* ws,
                         hipStream_t s, int prec);
// dx (nullable): dL/dx, NCHW; dprm is overwritten (the up5.deconv range with zeros)
dn_status resnet_backward(const ResPlan& p, const float* prm, const float* dy, float* dprm,
                          float* dx, float* ws, hipStream_t s, int prec);

}  // namespace dn
