// U-Net orchestration for the N2N training path: parameter layout (reference state_dict
// order), workspace plan (NHWC activation arena, gradient buffers, weight-gradient slabs),
// and the forward / backward launch sequences.  Mirrors arch_unet.py:100-260 (UNet) and
// the autograd graph that `loss.backward()` replays for it.  The op helpers, the backward's
// streams and the dec_conv1a .. nin_c tail shared with resnet.cpp live in exec_common.{h,cpp}.
#include "unet.h"

#include <cstdlib>

namespace dn {

// ------------------------------------------------------------------------------------
// parameters: arch_unet.py:115-192 registration order (== state_dict order)
// ------------------------------------------------------------------------------------
static const char* kNames[NL] = {
    "enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5", "enc_conv6",
    "up5.deconv", "dec_conv5a", "dec_conv5b", "up4.deconv", "dec_conv4a", "dec_conv4b",
    "up3.deconv", "dec_conv3a", "dec_conv3b", "up2.deconv", "dec_conv2a", "dec_conv2b",
    "up1.deconv", "dec_conv1a", "dec_conv1b", "nin_a", "nin_b", "nin_c"};

const char* layer_name(int i) { return (i >= 0 && i < NL) ? kNames[i] : ""; }

bool build_params(const dn_unet_cfg& c, ParamLayout& P, std::string& err) {
  const int C = c.in_nc, OC = c.out_nc, nf = c.n_feature;
  if (C < 1 || C > 4 || OC < 1 || OC > 16) {
    err = "in_nc must be in [1,4] and out_nc in [1,16]";
    return false;
  }
  if (nf != 48) {
    err = "n_feature must be 48 (kernel tiles are instantiated for the reference width)";
    return false;
  }
  auto conv = [&](int i, int cout, int cin, int k) { P.L[i] = {cout, cin, k, false, 0, 0}; };
  auto dec = [&](int i, int cin, int cout) { P.L[i] = {cout, cin, 2, true, 0, 0}; };
  conv(ENC0, nf, C, 3);
  for (int i = ENC1; i <= ENC6; ++i) conv(i, nf, nf, 3);
  dec(UP5, nf, nf);
  conv(D5A, 2 * nf, 2 * nf, 3);
  conv(D5B, 2 * nf, 2 * nf, 3);
  dec(UP4, 2 * nf, 2 * nf);
  conv(D4A, 2 * nf, 3 * nf, 3);
  conv(D4B, 2 * nf, 2 * nf, 3);
  dec(UP3, 2 * nf, 2 * nf);
  conv(D3A, 2 * nf, 3 * nf, 3);
  conv(D3B, 2 * nf, 2 * nf, 3);
  dec(UP2, 2 * nf, 2 * nf);
  conv(D2A, 2 * nf, 3 * nf, 3);
  conv(D2B, 2 * nf, 2 * nf, 3);
  dec(UP1, 2 * nf, 2 * nf);
  conv(D1A, 96, 2 * nf + C, 3);  // arch_unet.py:177 (hard-wired 96)
  conv(D1B, 96, 96, 3);
  conv(NINA, 96, 96, 1);
  conv(NINB, 96, 96, 1);
  conv(NINC, OC, 96, 1);
  long off = 0;
  for (int i = 0; i < NL; ++i) {
    Layer& L = P.L[i];
    L.wcount = (long)L.cout * L.cin * L.k * L.k;
    L.woff = off;
    off += L.wcount + L.cout;
  }
  P.total = off;
  return true;
}

// ------------------------------------------------------------------------------------
// workspace plan (offsets in floats, 256-byte aligned)
// ------------------------------------------------------------------------------------
int dgrad_nout(const Plan& p, int i);

bool build_plan(const dn_unet_cfg& c, int N, int H, int W, bool bwd, Plan& p, std::string& err) {
  if (N < 1 || H < 32 || W < 32 || (H % 32) || (W % 32)) {
    err = "N >= 1 and H, W must be positive multiples of 32 (5 pooling levels)";
    return false;
  }
  if (!build_params(c, p.P, err)) return false;
  p.N = N; p.H = H; p.W = W;
  p.C = c.in_nc; p.OC = c.out_nc; p.nf = c.n_feature;
  const int nf = p.nf;
  long off = 0;
  auto px = [&](int lvl) { return (long)N * (H >> lvl) * (W >> lvl); };
  auto alloc = [&](int lvl, int ch) {
    long o = off;
    off += (px(lvl) * ch + 63) / 64 * 64;
    return o;
  };
  p.c1k = 2 * nf + p.C;             // [up1 | x] channels
  p.c1kp = (p.c1k + 3) / 4 * 4;     // ... padded to float4 (pad channels kept at zero)
  // pixel stride of forward-only plans (the N2N target pass, the frozen finetune base, eval): a
  // multiple of 32 channels (128 B), so the deconv's 384-B pixel writes and dec_conv1a's 128-B
  // chunk reads stay line-aligned (stride 100: 400-B pixels, every 64-B piece split over two
  // lines; the 256^2 deconv measured 0.88 ms at stride 100, 0.64 at 96); channels [c1kp, c1s)
  // are never written or read.  Plans with a backward keep the float4 stride (measured faster
  // there).  DN_C1S_ALIGN=4 / 32 forces either.
  static const int c1s_env = getenv("DN_C1S_ALIGN") ? atoi(getenv("DN_C1S_ALIGN")) : 0;
  const int c1s_align = c1s_env > 0 ? c1s_env : (bwd ? 4 : 32);
  p.c1s = (p.c1k + c1s_align - 1) / c1s_align * c1s_align;
  p.c1 = alloc(0, p.c1s);
  p.a0 = alloc(0, nf);
  p.a1 = alloc(0, nf);
  for (int l = 1; l <= 4; ++l) {  // c2..c5 concat buffers (c5 is [u5 | p4] = 2nf)
    p.ck[l] = (l == 4) ? 2 * nf : 3 * nf;
    // forward-only plans: pixel stride a multiple of 32 channels like c1 (144 -> 160: 640-B
    // pixels, the deconv / pool writes and the 128-B chunk reads line-aligned)
    const int a = c1s_env > 0 ? c1s_env : (bwd ? 1 : 32);
    p.cs[l] = (p.ck[l] + a - 1) / a * a;
    p.c[l] = alloc(l, p.cs[l]);
  }
  for (int l = 1; l <= 4; ++l) p.a[l] = alloc(l, nf);  // a2..a5 live at levels 1..4
  p.p5 = alloc(5, nf);
  p.a6 = alloc(5, nf);
  for (int l = 1; l <= 4; ++l) {
    p.da[l] = alloc(l, 2 * nf);
    p.db[l] = alloc(l, 2 * nf);
  }
  p.d1a = alloc(0, 96);
  p.d1b = alloc(0, 96);
  p.na = alloc(0, 96);
  p.nb = alloc(0, 96);
  // packed forward weights (rebuilt by every dn_unet_forward from the flat parameters)
  auto alloc_f = [&](long n) {
    long o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  for (int i = 0; i < NL; ++i) {
    const Layer& L = p.P.L[i];
    const long n = L.deconv ? deconv_fwd_pack_size(L.cin, L.cout)
                            : conv_fwd_pack_size(L.cin, L.cout, L.k);
    if (n < 0) {
      err = std::string("no forward kernel tile for layer ") + kNames[i];
      return false;
    }
    p.packF[i] = alloc_f(n);
  }
  p.packH = alloc_f(2 * HEAD_LW > X6_HEAD_BF ? 2 * HEAD_LW : X6_HEAD_BF);  // fp32 | bf16x6 head images
  for (int i = 0; i < NL; ++i) {  // 4 x X6_HEAD_BF bf16 per 96-channel deconv
    const Layer& L = p.P.L[i];
    p.packUX[i] = (L.deconv && L.cin == 96 && L.cout == 96) ? alloc_f(2 * X6_HEAD_BF) : -1;
  }
  for (int i = 0; i < NL; ++i) {  // bf16 images (2 bytes each) of the 3x3 layers
    const Layer& L = p.P.L[i];
    p.packBF[i] = -1;
    if (i == ENC0 || i == NINC) continue;  // 3x3 layers, deconvs, nin_a / nin_b
    const long e = L.deconv ? 4 * bf16_pack_elems(L.cin, L.cout, 1) : bf16_pack_elems(L.cin, L.cout, L.k);
    if (e < 0) {
      err = std::string("no bf16 forward tile for layer ") + kNames[i];
      return false;
    }
    p.packBF[i] = alloc_f((e + 1) / 2);
  }
  for (int i = 0; i < NL; ++i) {  // bf16x6 (split fp32) images of the 3x3 layers
    const Layer& L = p.P.L[i];
    p.packX[i] = -1;
    if (i == ENC0 || L.deconv || L.k != 3) continue;
    const long e = x6_pack_elems(L.cin, L.cout, 0);
    if (e < 0) {
      err = std::string("no bf16x6 forward tile for layer ") + kNames[i];
      return false;
    }
    p.packX[i] = alloc_f((e + 1) / 2);
  }
  p.packXV = p.w6s_list = p.w6s_cnt = p.packUC = -1;
  if (!bwd) {
    p.packUC = alloc_f((UPC_BYTES + 3) / 4);
    p.packXV = alloc_f((x6_pack_elems(96, 96, 0) + 1) / 2);
    p.w6s_list = alloc_f(2L * N * (H / 2) * (W / 2));
    p.w6s_cnt = alloc_f(2L * N);
  }
  p.fwd_floats = off;
  if (bwd) {
    p.g_nb = alloc(0, 96);
    p.g_na = alloc(0, 96);
    p.g_d1b = alloc(0, 96);
    p.g_d1a = alloc(0, 96);
    p.g_c1 = alloc(0, 2 * nf);
    for (int l = 1; l <= 4; ++l) {
      p.g_c[l] = alloc(l, p.cs[l]);
      p.g_da[l] = alloc(l, 2 * nf);
      p.g_db[l] = alloc(l, 2 * nf);
      p.g_a[l] = alloc(l, nf);
    }
    p.g_a6 = alloc(5, nf);
    p.g_p5 = alloc(5, nf);
    p.g_a0 = alloc(0, nf);
    p.g_a1 = alloc(0, nf);
    p.xin = alloc(0, p.C);
    for (int i = 0; i < NL; ++i) {  // packed data-gradient weights
      const Layer& L = p.P.L[i];
      long n = 0;
      if (i == ENC0) n = 0;  // the network input needs no gradient
      else if (L.deconv) n = deconv_dgrad_pack_size(L.cout, L.cin);
      else n = conv_dgrad_pack_size(L.cout, dgrad_nout(p, i), L.k);
      if (n < 0) {
        err = std::string("no data-gradient kernel tile for layer ") + kNames[i];
        return false;
      }
      p.packB[i] = alloc_f(n);
    }
    p.packHB = alloc_f(2 * HEAD_LW > X6_HEAD_BF ? 2 * HEAD_LW : X6_HEAD_BF);  // fp32 | bf16x6 (Wb^T | Wa^T)
    for (int i = 0; i < NL; ++i)  // 4 x X6_HEAD_BF bf16 per 96-channel deconv
      p.packUXB[i] = p.packUX[i] >= 0 ? alloc_f(2 * X6_HEAD_BF) : -1;
    for (int i = 0; i < NL; ++i) {  // bf16x6 data-gradient images of the 3x3 layers
      const Layer& L = p.P.L[i];
      p.packXB[i] = -1;
      if (i == ENC0 || L.deconv || L.k != 3) continue;
      const int nout = dgrad_nout(p, i);
      const long e = x6_pack_elems(L.cout, nout, x6_dgrad_zc(nout));
      if (e < 0) {
        err = std::string("no bf16x6 data-gradient tile for layer ") + kNames[i];
        return false;
      }
      p.packXB[i] = alloc_f((e + 1) / 2);
    }
    // weight-gradient slabs, one per layer (the backward queues every layer's reduction and
    // launches them together at its end): splits * (W + b) after 64 floats
    p.zeros = alloc_f(64);
    p.slab_floats = 0;
    for (int i = 0; i < NL; ++i) {
      const Layer& L = p.P.L[i];
      int lvl = layer_level(i);
      int KH = H >> lvl, KW = W >> lvl;
      int mode = L.deconv ? W_UP2 : (L.k == 3 ? W_C3 : W_C1);
      if (L.deconv) { KH = H >> (lvl + 1); KW = W >> (lvl + 1); }
      // (nin_c above 4 outputs goes through wgrad_run() like any 1x1 layer)
      const int kind = i == ENC0 ? SLAB_ENC0 : i == D1A ? SLAB_D1A
                       : (i == NINC && p.OC <= 4) ? SLAB_NINC_THIN : SLAB_CONV;
      const WgradSlab sl = plan_wgrad_slab(kind, mode, N, KH, KW, L, p.C);
      p.splits[i] = sl.splits;
      p.slab[i] = alloc_f(64 + sl.floats);
      p.slab_floats += 64 + sl.floats;
    }
  }
  p.total_floats = off;
  p.with_bwd = bwd;
  return true;
}

void unet_debug_buffers(const Plan& p, const BufferVisitor& add) {
  const int nf = p.nf;
  add(p.c1, p.c1s, 0); add(p.a0, nf, 0); add(p.a1, nf, 0);
  for (int l = 1; l <= 4; ++l) add(p.c[l], p.cs[l], l);
  for (int l = 1; l <= 4; ++l) add(p.a[l], nf, l);
  add(p.p5, nf, 5); add(p.a6, nf, 5);
  for (int l = 1; l <= 4; ++l) add(p.da[l], 2 * nf, l);
  for (int l = 1; l <= 4; ++l) add(p.db[l], 2 * nf, l);
  add(p.d1a, 96, 0); add(p.d1b, 96, 0); add(p.na, 96, 0); add(p.nb, 96, 0);
  if (!p.with_bwd) return;
  add(p.g_nb, 96, 0); add(p.g_na, 96, 0); add(p.g_d1b, 96, 0); add(p.g_d1a, 96, 0);
  add(p.g_c1, 2 * nf, 0);
  for (int l = 1; l <= 4; ++l) add(p.g_c[l], p.cs[l], l);
  for (int l = 1; l <= 4; ++l) add(p.g_da[l], 2 * nf, l);
  for (int l = 1; l <= 4; ++l) add(p.g_db[l], 2 * nf, l);
  for (int l = 1; l <= 4; ++l) add(p.g_a[l], nf, l);
  add(p.g_a6, nf, 5); add(p.g_p5, nf, 5); add(p.g_a0, nf, 0); add(p.g_a1, nf, 0);
}

// channels of the data gradient a layer's backward must produce
int dgrad_nout(const Plan& p, int i) {
  if (i == D1A) return 2 * p.nf;  // only the up1 part of [up1 | x]
  return p.P.L[i].cin;
}

// output level of every layer (deconvs: level of their OUTPUT)
int layer_level(int i) {
  switch (i) {
    case ENC0: case ENC1: return 0;
    case ENC2: return 1;
    case ENC3: return 2;
    case ENC4: return 3;
    case ENC5: return 4;
    case ENC6: return 5;
    case UP5: case D5A: case D5B: return 4;
    case UP4: case D4A: case D4B: return 3;
    case UP3: case D3A: case D3B: return 2;
    case UP2: case D2A: case D2B: return 1;
    default: return 0;  // UP1, D1A, D1B, NIN*
  }
}

// ------------------------------------------------------------------------------------
// forward: arch_unet.py:194-260 (non-blind-spot branch)
// ------------------------------------------------------------------------------------
// A pass decides once, in fwd_routes(), which kernel every layer takes and which weight image in
// the workspace that kernel reads; pack_forward() writes exactly those images and run_forward()
// launches on them, each by a switch on the route's kind.
namespace {

enum FwdKind {
  F_F32,        // conv on the fp32 kernel (3x3 or 1x1; Plan::packF)
  F_X6,         // 3x3 conv on the bf16x6 kernels: split fp32 operands on the bf16 matrix cores
  F_BF16,       // conv on the bf16 kernel: bf16 operands, fp32 accumulation / bias / activation
  F_UP_F32,     // ConvTranspose2d(2,2) on the fp32 kernel
  F_UP_X6,      // ... on the persistent bf16x6 kernel (k_deconv_x6; `plain`: plain bf16 products)
  F_UP_BF16,    // ... as a bf16 1x1 launch per output parity
  F_FUSED_UP1,  // up1 and dec_conv1a: ONE composed image and launch (k_upconv3_x6)
  F_HEAD,       // nin_a .. nin_c inside the head launch, on the head's image
};
struct FwdRoute {
  int kind;
  long img;    // workspace offset (floats) of the layer's weight image
  int tail;    // F_X6: x6_image_mode (tail packing of the last K chunk | X6_W6) | X6_T1
  bool plain;  // F_UP_X6 in the bf16 base
  bool in_bf16, out_bf16;  // F_BF16: the input / output activation stored as bf16
  bool pool;   // enc_conv1..5: the 2x2 max-pool fused into the conv's epilogue
};
enum HeadKind {
  H_F32,       // dec_conv1b + nin_a + nin_b + nin_c in one fp32 kernel (launch_head)
  H_NIN,       // bf16x6 dec_conv1b, then the fp32 nin head (out_nc above X6_HEAD_OCMAX)
  H_NIN_X6,    // bf16x6 dec_conv1b (or the pair-pixel pass), then k_nin_head_x6
  H_NIN_BF16,  // bf16 dec_conv1b, then k_nin_head_x6 in plain bf16 products
  H_BF16_3,    // bf16 dec_conv1b, nin_a and nin_b as bf16 1x1 launches, nin_c on the fp32 kernel
};
struct FwdRoutes {
  FwdRoute r[NL];  // ENC1 .. NINC
  int head;
  long head_img;   // the head's nin_a | nin_b images (not H_BF16_3)
  bool up1_fuse;
  bool sel;        // dec_conv1b and the head on the N2N pair pixels only
  bool w6_sel;     // ... dec_conv1b on k_c3w6s: cell lists and the tap-transposed image img_xv
  long img_xv;
  bool enc0_c1;    // enc_conv0 copies x into its slice of the up1 concat buffer
  bool enc0_bf16;  // enc_conv0's output stored as bf16
  int pool_only;   // a conv with a fused pool stores only the pooled output
};

FwdRoutes fwd_routes(const Plan& p, int prec, bool pair_pass) {
  const bool bf16 = prec == DN_PREC_BF16, x6 = prec == DN_PREC_FP32_X6;
  // the encoder's 2x2 max-pools fused into the convs' epilogues (DN_POOL_FUSE=0: separate
  // k_pool_fwd launches, A/B)
  static const bool pool_fuse = !getenv("DN_POOL_FUSE") || atoi(getenv("DN_POOL_FUSE")) != 0;
  // DN_UP1_FUSE=0: up1 and dec_conv1a as two launches (A/B)
  static const bool up1_fuse_env = !getenv("DN_UP1_FUSE") || atoi(getenv("DN_UP1_FUSE")) != 0;
  FwdRoutes R{};
  // bf16 base (forward-only plans): bf16 storage of the activations that only a bf16 conv reads
  // (enc_conv0 -> enc_conv1, dec_conv{l}a -> dec_conv{l}b).  The consumer rounds its staged
  // operands to bf16 anyway, so the result is bit-identical and those tensors move half the bytes
  const bool bf16_store = bf16 && !p.with_bwd;
  for (int i = ENC1; i <= NINC; ++i) {
    const Layer& L = p.P.L[i];
    FwdRoute& r = R.r[i];
    if (L.deconv) {
      // the 96-channel deconvs on the persistent bf16x6 kernel, also in the bf16 base (one pass
      // over the input instead of a bf16 1x1 launch per output parity)
      if ((x6 || bf16) && p.packUX[i] >= 0) { r.kind = F_UP_X6; r.img = p.packUX[i]; r.plain = bf16; }
      else if (bf16 && p.packBF[i] >= 0) { r.kind = F_UP_BF16; r.img = p.packBF[i]; }
      else { r.kind = F_UP_F32; r.img = p.packF[i]; }
    } else if (x6 && p.packX[i] >= 0) {
      r.kind = F_X6; r.img = p.packX[i];
      // the pipelined kernel takes a partial last K chunk (dec_conv1a's x channels, the
      // 48-channel encoder's second chunk) packed over fewer stages; | X6_W6: the Winograd kernel
      // on the 96- and 48-output layers from one round of 8 x 16 tiles.  dec_conv1a reads
      // [up1 | x | zero pad] (c1kp = c1k rounded to 4): taking the zero pad channel as a reduction
      // channel (its packed weights are zero) keeps K % 4 == 0 (pipelined)
      const int l = layer_level(i);
      r.tail = x6_image_mode(p.N, p.H >> l, p.W >> l, i == D1A ? p.c1kp : L.cin, L.cout, 0, true);
      // dec_conv1a at C = 1 on the Winograd kernel: the image channel alone in the last chunk
      if (i == D1A && (r.tail & X6_W6) && (r.tail & 7) == 1 && L.cin % 32 == 1 && L.cout == 96)
        r.tail |= X6_T1;
    } else if (bf16 && p.packBF[i] >= 0) {
      r.kind = F_BF16; r.img = p.packBF[i];
      r.in_bf16 = bf16_store && (i == ENC1 || i == D1B || i == D2B || i == D3B || i == D4B || i == D5B);
      r.out_bf16 = bf16_store && (i == D1A || i == D2A || i == D3A || i == D4A || i == D5A);
    } else {
      r.kind = F_F32; r.img = p.packF[i];
    }
    r.pool = pool_fuse && i >= ENC1 && i <= ENC5 && (r.kind == F_X6 || r.kind == F_BF16);
  }
  R.enc0_bf16 = bf16_store;  // only enc_conv1 reads enc_conv0's output in a forward-only plan
  // forward-only plans: an encoder conv whose pool is fused stores only the pooled output (its
  // full-resolution activation is read by nothing but that pool; the backward's pool routing
  // reads it in plans with a backward)
  R.pool_only = !p.with_bwd ? 1 : 0;
  // Forward-only bf16x6 plans from the grid size k_c3w6 takes dec_conv1a at: up1 and dec_conv1a
  // as ONE launch (k_upconv3_x6: the deconv composed into the conv's 96 up1 channels, 2x2 taps
  // per output parity over d2b; nothing else reads up1 without a backward)
  const int d1a_tail = R.r[D1A].tail;
  R.up1_fuse = up1_fuse_env && x6 && !p.with_bwd && p.packUC >= 0 && p.nf == 48 && p.C <= 4 &&
               (d1a_tail & X6_W6);
  if (R.up1_fuse) {
    R.r[UP1] = FwdRoute{F_FUSED_UP1, p.packUC};
    R.r[D1A] = FwdRoute{F_FUSED_UP1, p.packUC};
  }
  // dec_conv1a reading x itself (X6_T1, the fused launch): the concat slice is never read -- 16
  // scattered bytes per 512-B pixel cost the enc_conv0 launch 0.19 ms/step; c1's channels
  // [2nf, c1s) then hold stale data, which the debug-buffer contract in denoise_hip.h states
  R.enc0_c1 = !(x6 && ((d1a_tail & X6_T1) || R.up1_fuse));
  // the head.  bf16 base (inference only): the fused head kernel in plain bf16 products instead
  // of nin_a / nin_b as two bf16 1x1 launches + an fp32 nin_c (two 96-channel round trips through
  // HBM saved); it reads d1b as bf16
  if (bf16) R.head = !p.with_bwd && p.OC <= X6_HEAD_OCMAX ? H_NIN_BF16 : H_BF16_3;
  else if (x6) R.head = p.OC <= X6_HEAD_OCMAX ? H_NIN_X6 : H_NIN;
  else R.head = H_F32;
  R.head_img = p.packH;
  if (R.head != H_BF16_3)
    for (int i = NINA; i <= NINC; ++i) R.r[i] = FwdRoute{F_HEAD, p.packH};
  if (R.head == H_NIN_BF16) R.r[D1B].out_bf16 = true;
  // the N2N no-grad pass: the bf16x6 nin head at the pair pixels; its dec_conv1b on the Winograd
  // kernel k_c3w6s wherever the full forward's dec_conv1b has a Winograd image, the direct
  // k_c3x6s below one round of tiles
  R.sel = x6 && pair_pass && !p.with_bwd && p.OC <= X6_HEAD_OCMAX;
  R.w6_sel = R.sel && p.packXV >= 0 && (R.r[D1B].tail & X6_W6);
  R.img_xv = p.packXV;
  return R;
}

// every weight image of the pass (fp32, bf16x6 and bf16 alike) in one pack launch
dn_status pack_forward(const Plan& p, const FwdRoutes& R, const float* prm, float* ws,
                       hipStream_t s) {
  auto Bs = [&](int i) { return prm + p.P.L[i].woff + p.P.L[i].wcount; };
  PackBatch pb;
  auto add = [&](bool ok, const PackJob& j) { return ok ? pack_add(pb, j, s) : hipErrorInvalidValue; };
  for (int i = ENC1; i <= NINC; ++i) {
    const Layer& L = p.P.L[i];
    const FwdRoute& r = R.r[i];
    const float* w = prm + L.woff;
    PackJob j;
    switch (r.kind) {
      case F_FUSED_UP1:  // one composed image for the pair
        if (i == D1A)
          DN_TRY(add(true, pack_job_upconv_x6(w, Bs(D1A), prm + p.P.L[UP1].woff, Bs(UP1), p.C,
                                              ws + r.img)));
        break;
      case F_UP_X6:
        DN_TRY(add(true, pack_job_deconv_x6(w, ws + r.img)));
        break;
      case F_UP_BF16: {  // ConvTranspose2d [cin][cout][2][2]: a 1x1 image per parity
        const long img = bf16_pack_elems(L.cin, L.cout, 1);
        for (int ab = 0; ab < 4; ++ab) {
          WView v{};
          v.w = w; v.off = ab; v.sK = (long)L.cout * 4; v.sN = 4; v.taps = 1;
          DN_TRY(add(pack_job_bf16(v, L.cin, L.cout, 1,
                                   reinterpret_cast<unsigned short*>(ws + r.img) + ab * img, j), j));
        }
        break;
      }
      case F_UP_F32:
        DN_TRY(add(pack_job(G_UP, deconv_fwd_view(w, L.cout), L.cin, L.cout, 4, ws + r.img, 0, 0, j), j));
        break;
      case F_BF16:
        if (L.k == 3)
          DN_TRY(add(pack_job_bf16(conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 3, ws + r.img, j), j));
        else  // nin_a, nin_b: launches of their own
          DN_TRY(launch_pack_bf16(conv_fwd_view(w, L.cin, 1), L.cin, L.cout, ws + r.img, s, 1));
        break;
      case F_X6:
        DN_TRY(add(pack_job_x6(conv_fwd_view(w, L.cin, 3), L.cin, L.cout, 0, ws + r.img, r.tail, j), j));
        break;
      case F_F32:
        DN_TRY(add(pack_job(L.k == 3 ? G_C3 : G_C1, conv_fwd_view(w, L.cin, L.k), L.cin, L.cout, 1,
                            ws + r.img, 0, 0, j), j));
        break;
      case F_HEAD:
        break;
    }
    // dec_conv1b's y-tile image for the Winograd pair pass: PK_W6 over the transposed taps
    if (i == D1B && R.w6_sel) {
      WView v = conv_fwd_view(w, L.cin, 3);
      v.flip = 2;
      DN_TRY(add(pack_job_x6(v, L.cin, L.cout, 0, ws + R.img_xv, X6_W6, j), j));
    }
  }
  if (R.head != H_BF16_3)  // (H_BF16_3: the three layers' own images, above)
    DN_TRY(pack_head_fwd(pb, R.head == H_NIN_X6 || R.head == H_NIN_BF16, prm + p.P.L[NINA].woff,
                         prm + p.P.L[NINB].woff, ws + R.head_img, s));
  DN_TIMED(s, "pack", 0, 0, 0, 0, 0, 0, pack_flush(pb, s));
  return DN_OK;
}

dn_status run_forward(const Plan& p, const FwdRoutes& R, const float* prm, const float* x,
                      float* y, float* ws, hipStream_t s, const uint8_t* sel_rd) {
  const int N = p.N, nf = p.nf, C = p.C;
  auto H = [&](int l) { return p.H >> l; };
  auto Wd = [&](int l) { return p.W >> l; };
  auto Bs = [&](int i) { return prm + p.P.L[i].woff + p.P.L[i].wcount; };
  auto V = [&](long off, int stride, int coff = 0) { return View{ws + off, stride, coff}; };
  const View none{nullptr, 0, 0};
  // Conv layer i (enc_conv1 .. nin_b; bias + LeakyReLU, NHWC) at its level, on the kernel and
  // image of its route.  pool: the 2x2 max-pool of `out` into that view, fused into the conv's
  // epilogue (bit-identical) or as its own launch
  auto conv_forward = [&](int i, const View& in, const View& out,
                          const View* pool = nullptr) -> hipError_t {
    const Layer& L = p.P.L[i];
    const FwdRoute& r = R.r[i];
    const int l = layer_level(i), h = H(l), w = Wd(l);
    hipError_t e = hipErrorInvalidValue;
    {
      const OpTimer timer(s, L.k == 3 ? "fwd3" : "fwd1",
                          2.0 * N * h * w * L.cin * L.cout * L.k * L.k, L.cin, L.cout, h, w, N);
      switch (r.kind) {
        case F_F32:  // (dec_conv1a: its c1k real channels)
          e = dn::conv_forward(in, N, h, w, L.cin, ws + r.img, Bs(i), L.cout, L.k, 1, out, OUT_NHWC, s);
          break;
        case F_X6: case F_BF16: {
          FwdArgs a = fwd_args(in, N, h, w, i == D1A ? p.c1kp : L.cin, L.cout, out, OUT_NHWC);
          a.wp = ws + r.img; a.bias = Bs(i); a.epi = EPI_BIAS_ACT;
          a.x6_tail = r.tail;
          if (r.tail & X6_T1) a.in_t1 = x;  // the image channel straight from the network input
          a.in_bf16 = r.in_bf16; a.out_bf16 = r.out_bf16;
          if (pool && r.pool) set_pool(a, *pool, R.pool_only);
          e = r.kind == F_X6 ? launch_fwd_x6(a, s) : launch_fwd_bf16(a, s, L.k);
          break;
        }
        default:
          break;
      }
    }
    if (e != hipSuccess || !pool || r.pool) return e;
    const OpTimer timer(s, "pool", 0);
    return launch_pool_fwd(out.p, N, h, w, L.cout, pool->p, pool->stride, pool->off, s);
  };
  // ConvTranspose2d(2,2) layer i (its input lives one level below its output)
  auto deconv_forward = [&](int i, const View& xin, const View& out) -> hipError_t {
    const Layer& L = p.P.L[i];
    const FwdRoute& r = R.r[i];
    const int l = layer_level(i) + 1, h = H(l), w = Wd(l);
    const OpTimer timer(s, "deconv", 2.0 * N * h * w * L.cin * L.cout * 4, L.cin, L.cout, h, w, N);
    FwdArgs a = fwd_args(xin, N, h, w, L.cin, L.cout, out, OUT_UP2);
    a.bias = Bs(i); a.epi = EPI_BIAS;
    switch (r.kind) {
      case F_UP_F32:
        return dn::deconv_forward(xin, N, h, w, L.cin, ws + r.img, Bs(i), L.cout, out, s);
      case F_UP_X6:  // bf16x6 parity GEMMs on the layer's pre-split images
        if (!deconv_x6_ok(a)) return hipErrorInvalidValue;
        return launch_deconv_x6(a, ws + r.img, s, r.plain);
      case F_UP_BF16:  // the bf16 1x1 kernel per output parity
        a.wp = ws + r.img; a.wp_z = bf16_pack_elems(L.cin, L.cout, 1);
        return launch_fwd_bf16(a, s, 1);
      default:
        return hipErrorInvalidValue;
    }
  };

  // the pair pass's cell lists first: they depend on the pair choices only, and built here they
  // run beside the other stream's work instead of alone right before the pair pass (~20 us of a
  // step in which nothing else ran, profiles/r6_step_timeline.txt)
  if (R.w6_sel)
    DN_TIMED(s, "sel_lists", 0, 0, 0, 0, 0, 0,
             launch_w6s_lists(sel_rd, N, H(0), Wd(0), reinterpret_cast<unsigned*>(ws + p.w6s_list),
                              reinterpret_cast<int*>(ws + p.w6s_cnt), s));
  // enc_conv0, fused with pool0 = x -> channels [2nf, 2nf+C) of the up1 concat buffer
  DN_TIMED(s, "enc0", 2.0 * N * p.H * p.W * C * nf * 9, C, nf, p.H, p.W, N,
           launch_enc0_fwd(x, N, C, p.H, p.W, prm + p.P.L[ENC0].woff, Bs(ENC0), ws + p.a0,
                           R.enc0_c1 ? ws + p.c1 : nullptr, p.c1s, 2 * nf, p.c1kp,
                           p.with_bwd ? ws + p.xin : nullptr, s, R.enc0_bf16));
  {  // enc_conv1 + pool1 -> skip slice of c2
    const View pv = V(p.c[1], p.cs[1], 2 * nf);
    DN_TRY(conv_forward(ENC1, V(p.a0, nf), V(p.a1, nf), &pv));
  }
  // enc_conv2..5 + pool2..5 (pool_k -> skip slice of c_{k+1}; pool5 -> p5)
  for (int l = 1; l <= 4; ++l) {
    const View in = (l == 4) ? V(p.c[4], p.cs[4], nf) : V(p.c[l], p.cs[l], 2 * nf);
    const View pv = l < 4 ? V(p.c[l + 1], p.cs[l + 1], (l + 1 == 4) ? nf : 2 * nf) : V(p.p5, nf, 0);
    DN_TRY(conv_forward(ENC2 + (l - 1), in, V(p.a[l], nf), &pv));
  }
  DN_TRY(conv_forward(ENC6, V(p.p5, nf), V(p.a6, nf)));
  // decoder: up5 (a6 -> c5[0:nf]); dec5a/b at level 4
  DN_TRY(deconv_forward(UP5, V(p.a6, nf), V(p.c[4], p.cs[4], 0)));
  const int up_idx[6] = {0, UP1, UP2, UP3, UP4, UP5};  // up_idx[k]: level k -> level k-1
  const int da_idx[5] = {0, D2A, D3A, D4A, D5A};
  for (int l = 4; l >= 1; --l) {
    if (l < 4)  // up_{l+1}: d_{l+1}b -> c_l[0:2nf]
      DN_TRY(deconv_forward(up_idx[l + 1], V(p.db[l + 1], 2 * nf), V(p.c[l], p.cs[l], 0)));
    const int ia = da_idx[l], ib = da_idx[l] + 1;
    // (dec_conv{l}a reduces over the concat's ck[l] channels == its cin; cs[l] is the stride)
    DN_TRY(conv_forward(ia, V(p.c[l], p.cs[l]), V(p.da[l], 2 * nf)));
    DN_TRY(conv_forward(ib, V(p.da[l], 2 * nf), V(p.db[l], 2 * nf)));
  }
  // up1: d2b -> c1[0:2nf], then dec_conv1a
  if (R.up1_fuse) {  // (the record carries dec_conv1a's algorithmic FLOPs, as the Winograd launches)
    FwdArgs a = fwd_args(V(p.db[1], 2 * nf), H(1), Wd(1), N, H(0), Wd(0), p.c1k, 96, V(p.d1a, 96),
                         OUT_NHWC);
    a.wp = ws + R.r[D1A].img; a.in_t1 = x; a.epi = EPI_BIAS_ACT;
    DN_TIMED(s, "fwd3", 2.0 * N * H(0) * Wd(0) * p.c1k * 96 * 9, p.c1k, 96, H(0), Wd(0), N,
             launch_upconv3_x6(a, s));
  } else {
    DN_TRY(deconv_forward(UP1, V(p.db[1], 2 * nf), V(p.c1, p.c1s, 0)));
    DN_TRY(conv_forward(D1A, V(p.c1, p.c1s), V(p.d1a, 96)));
  }

  // dec_conv1b and the head (arch_unet.py:251-257).  The pair pass (training_script.md:141-144
  // reads den at the pair pixels only) runs both on those pixels, through the [N, H/2, W, 96] pair
  // image in d1b's storage
  const int hh = R.sel ? H(0) / 2 : H(0);  // rows of the head's input
  HeadArgs h = head_args(prm, p.P.L[NINA], p.P.L[NINB], p.P.L[NINC], ws + R.head_img, y);
  // the intermediate activations are written only when a backward will read them
  if (p.with_bwd) { h.na = ws + p.na; h.nb = ws + p.nb; }
  // dec_conv1b where it is not conv_forward's: the pair pass, the fp32 head kernel
  FwdArgs ac = fwd_args(V(p.d1a, 96), N, H(0), Wd(0), 96, 96, V(p.d1b, 96), OUT_NHWC);
  ac.wp = ws + R.r[D1B].img; ac.bias = Bs(D1B); ac.epi = EPI_BIAS_ACT;
  if (R.sel) {
    const OpTimer timer(s, "fwd3sel", 2.0 * N * hh * Wd(0) * 96 * 96 * 9, 96, 96, hh, Wd(0), N);
    if (R.w6_sel) {  // the Winograd pass over the cells listed per tile orientation
      DN_TRY(launch_fwd_w6s(ac, reinterpret_cast<unsigned*>(ws + p.w6s_list),
                            reinterpret_cast<int*>(ws + p.w6s_cnt), ws + R.img_xv, s));
    } else {
      ac.sel_rd = sel_rd;
      DN_TRY(launch_fwd_x6_sel(ac, s));
    }
    h.rd = sel_rd;
  } else if (R.head != H_F32) {
    DN_TRY(conv_forward(D1B, V(p.d1a, 96), V(p.d1b, 96)));
  }
  switch (R.head) {
    case H_F32:  // dec_conv1b inside the head kernel, on its fp32 image
      if (p.with_bwd) h.d1b = ws + p.d1b;
      DN_TIMED(s, "fwd3+head", 2.0 * N * H(0) * Wd(0) * 96 * (9 * 96 + 2 * 96 + p.OC), 96, 96, H(0),
               Wd(0), N, launch_head(ac, h, s));
      break;
    case H_NIN: case H_NIN_X6:
      if (dn_status st = head_forward(h, ws + p.d1b, N, hh, Wd(0), R.head == H_NIN_X6, s)) return st;
      break;
    case H_NIN_BF16: {  // the head kernels' input: d1b, stored as bf16 by dec_conv1b
      FwdArgs a = fwd_args(V(p.d1b, 96), N, hh, Wd(0), 96, 96, none, OUT_NHWC);
      a.in_bf16 = R.r[D1B].out_bf16;
      DN_TIMED(s, "head", 2.0 * N * hh * Wd(0) * 96 * (2 * 96 + p.OC), 96, p.OC, hh, Wd(0), N,
               launch_nin_head_x6(a, h, ws + R.head_img, s, /*bf16=*/true));
      break;
    }
    case H_BF16_3: {
      DN_TRY(conv_forward(NINA, V(p.d1b, 96), V(p.na, 96)));
      DN_TRY(conv_forward(NINB, V(p.na, 96), V(p.nb, 96)));
      const Layer& Lc = p.P.L[NINC];  // 96 -> out_nc, no activation, NCHW into y
      DN_TRY(dn::conv_forward(V(p.nb, 96), N, H(0), Wd(0), Lc.cin, ws + R.r[NINC].img, Bs(NINC),
                              Lc.cout, Lc.k, 0, View{y, p.OC, 0}, OUT_NCHW, s));
      break;
    }
  }
  return DN_OK;
}

}  // namespace

dn_status unet_forward(const Plan& p, const float* prm, const float* x, float* y, float* ws,
                       hipStream_t s, int prec, const uint8_t* sel_rd, int pack) {
  const StreamDeviceGuard device_guard(s);
  const FwdRoutes R = fwd_routes(p, prec, sel_rd != nullptr);
  // (a prepacked forward: dn_unet_pack_weights left the images in ws)
  if (pack != RUN_ONLY) {
    const dn_status st = pack_forward(p, R, prm, ws, s);
    if (st != DN_OK) return st;
  }
  return pack == PACK_ONLY ? DN_OK : run_forward(p, R, prm, x, y, ws, s, sel_rd);
}

// ------------------------------------------------------------------------------------
// backward: the autograd graph of the forward above, in reverse.  Data gradients fuse
// LeakyReLU' into their epilogue (mask = the layer input, which is the previous layer's
// post-activation output); skip gradients are accumulated into the concat-gradient buffers.
// ------------------------------------------------------------------------------------
// Weight gradients and slab reductions on their own streams: BwdStreams (exec_common.h).
long tail_begin(const Plan& p) { return p.P.L[D5A].woff; }

// The data-gradient route of every layer (enc_conv1 .. dec_conv1b), decided once: the pack loop
// writes the image the launch reads.  Convs: dgrad_route (CV_F32: Plan::packB, CV_X6: packXB)
namespace {
// deconv data gradient on the fp32 kernel | of the 96-channel deconvs in bf16x6 (packUXB)
enum BwdKind { B_UP_F32 = CV_END, B_UP_X6 };
struct BwdRoutes {
  ConvRoute r[NL];
  bool head_x6;  // the head's data gradients in the bf16x6 arithmetic (k_head_bwd_x6)
};
BwdRoutes bwd_routes(const Plan& p, int prec) {
  const bool x6 = prec == DN_PREC_FP32_X6;
  BwdRoutes B{};
  for (int i = ENC1; i < NINA; ++i) {
    const Layer& L = p.P.L[i];
    const int l = layer_level(i);
    if (L.deconv)
      B.r[i] = x6 && p.packUXB[i] >= 0 ? ConvRoute{B_UP_X6, p.packUXB[i]} : ConvRoute{B_UP_F32, p.packB[i]};
    else
      B.r[i] = dgrad_route(x6, p.packB[i], p.packXB[i], p.N, p.H >> l, p.W >> l, L, dgrad_nout(p, i));
  }
  B.head_x6 = x6 && p.OC <= X6_HEAD_BWD_OCMAX;
  return B;
}
}  // namespace

dn_status unet_backward(const Plan& p, const float* prm, const float* dy, float* dprm, float* dx,
                        float* ws, hipStream_t s, int prec, hipEvent_t tail_ready) {
  const StreamDeviceGuard device_guard(s);
  const bool x6 = prec == DN_PREC_FP32_X6;
  const int N = p.N, nf = p.nf, C = p.C;
  auto H = [&](int l) { return p.H >> l; };
  auto Wd = [&](int l) { return p.W >> l; };
  auto G = [&](int i) { return dprm + p.P.L[i].woff; };
  auto V = [&](long off, int stride, int coff = 0) { return View{ws + off, stride, coff}; };
  const BwdRoutes B = bwd_routes(p, prec);
  // deconv layer i: dy at the layer's output level -> dx one level below (* leaky'(mask))
  auto deconv_dgrad = [&](int i, const View& dy, const View& mask, int epi, const View& dx,
                          hipStream_t st) -> hipError_t {
    const Layer& L = p.P.L[i];
    const ConvRoute& r = B.r[i];
    const int l = layer_level(i) + 1, h = H(l), w = Wd(l);
    const OpTimer timer(st, "deconv_dgrad", 2.0 * N * h * w * L.cin * L.cout * 4, L.cout, L.cin, h,
                        w, N);
    if (r.kind == B_UP_F32)
      return dn::deconv_dgrad(dy, N, h, w, L.cout, ws + r.img, L.cin, mask, epi, dx, st);
    FwdArgs a = fwd_args(dy, 2 * h, 2 * w, N, h, w, L.cout, L.cin, dx, OUT_NHWC);
    a.epi = epi;
    set_mask(a, mask);
    return launch_deconv_dgrad_x6(a, ws + r.img, st);
  };
  {  // the data gradients' flipped / transposed images, the head's, the zero padding: one launch
    PackBatch pb;
    for (int i = ENC1; i < NINA; ++i) {
      const Layer& L = p.P.L[i];
      const ConvRoute& r = B.r[i];
      const float* w = prm + L.woff;
      PackJob j;
      switch (r.kind) {
        case B_UP_X6:
          DN_TRY(pack_add(pb, pack_job_deconv_dgrad_x6(w, ws + r.img), s));
          break;
        case B_UP_F32:
          DN_TRY(pack_job(G_DN2, deconv_dgrad_view(w, L.cout), L.cout, L.cin, 1, ws + r.img, 0, 0, j)
                     ? pack_add(pb, j, s) : hipErrorInvalidValue);
          break;
        default:
          DN_TRY(pack_dgrad(pb, r, w, L, dgrad_nout(p, i), ws, s));
          break;
      }
    }
    DN_TRY(pack_head_bwd(pb, B.head_x6, prm + p.P.L[NINA].woff, prm + p.P.L[NINB].woff,
                         ws + p.packHB, ws + p.zeros, s));
    DN_TIMED(s, "pack", 0, 0, 0, 0, 0, 0, pack_flush(pb, s));
  }
  BwdStreams bs(s);
  const float* Z = ws + p.zeros;
  auto SL = [&](int i) { return ws + p.slab[i]; };
  auto dst = [&](int i) { return WgradDst{G(i), SL(i), p.splits[i]}; };
  // layer i's weight gradient on stream st: g (cout channels) against xv (cin channels), level l
  auto wg = [&](int i, int mode, const View& g, const View& xv, int l, int cout, int cin, bool x6_,
                hipStream_t st) -> dn_status {
    return wgrad_run(wgrad_route(mode, g, xv, N, H(l), Wd(l), cout, cin, x6_), g.p, xv.p, G(i),
                     SL(i), Z, st, &bs.rb);
  };
  // layer i: dz (the layer's cout channels) -> dx, channels [0, dgrad_nout(p, i)) of its input
  auto conv_dgrad = [&](int i, const View& dz, int epi, const View& mask, const View& dx,
                        hipStream_t st) -> hipError_t {
    const int l = layer_level(i);
    return run_dgrad(B.r[i], ws, dz, N, H(l), Wd(l), p.P.L[i], dgrad_nout(p, i), epi, mask, dx, st);
  };
  const View none{nullptr, 0, 0};
  const int OC = p.OC;
  const TailShape tail{N, H(0), Wd(0), x6, Z};

  // dy arrives NCHW; OC == 1: that is NHWC.  OC > 1: transposed into g_c1's storage (free here)
  View dyv{const_cast<float*>(dy), OC, 0};
  if (OC > 1) {
    DN_TRY(launch_nchw_to_slice(dy, N, OC, p.H, p.W, ws + p.g_c1, OC, 0, OC, s));
    dyv = V(p.g_c1, OC);
  }
  {  // nin_c .. nin_a: data gradients in one kernel, then the three 1x1 weight gradients
    HeadBwdArgs h{};
    h.wp = ws + p.packHB;
    h.wc = prm + p.P.L[NINC].woff; h.oc = OC;
    h.dy = dyv.p; h.dy_stride = dyv.stride;
    h.nb = ws + p.nb; h.na = ws + p.na; h.d1b = ws + p.d1b;
    h.g_nb = ws + p.g_nb; h.g_na = ws + p.g_na; h.g_d1b = ws + p.g_d1b;
    h.npx = (long)N * H(0) * Wd(0);
    if (dn_status st = head_backward(bs, tail, h, B.head_x6, dst(NINA), dst(NINB), dst(NINC))) return st;
  }
  DN_TRY(bs.fork());
  if (dn_status st_ = wg(D1B, W_C3, V(p.g_d1b, 96), V(p.d1a, 96), 0, 96, 96, x6, bs.s2)) return st_;
  DN_TRY(conv_dgrad(D1B, V(p.g_d1b, 96), EPI_MASK, V(p.d1a, 96), V(p.g_d1a, 96), s));
  // dec_conv1a's weight gradient: up1's channels [0, 2nf) and the network input's [2nf, 2nf + C)
  if (dn_status st = d1a_wgrad(bs, tail, ws + p.g_d1a, V(p.c1, p.c1s), p.c1k, ws + p.xin, C, dst(D1A)))
    return st;
  // only the up1 part of the concat needs a gradient (pool0 is the network input)
  DN_TRY(conv_dgrad(D1A, V(p.g_d1a, 96), EPI_PLAIN, none, V(p.g_c1, 2 * nf), s));

  // decoder levels 1..4: up_{l}(d_{l+1}b ...) ; here "dU" for level l-1's deconv
  const int up_idx[6] = {UP1, UP2, UP3, UP4, UP5, 0};
  const int da_idx[5] = {0, D2A, D3A, D4A, D5A};
  View dU = V(p.g_c1, 2 * nf);  // gradient of up1's output
  for (int l = 1; l <= 4; ++l) {
    const int iu = up_idx[l - 1];  // deconv producing level l-1 from level l
    // deconv wgrad: x = d_l b (level l), dU at level l-1
    DN_TRY(bs.fork());
    if (dn_status st_ = wg(iu, W_UP2, dU, V(p.db[l], 2 * nf), l, 2 * nf, 2 * nf, x6, bs.s2))
      return st_;
    DN_TRY(deconv_dgrad(iu, dU, V(p.db[l], 2 * nf), EPI_MASK, V(p.g_db[l], 2 * nf), s));
    const int ia = da_idx[l], ib = ia + 1;
    DN_TRY(bs.fork());
    if (dn_status st_ = wg(ib, W_C3, V(p.g_db[l], 2 * nf), V(p.da[l], 2 * nf), l, 2 * nf, 2 * nf, x6, bs.s2))
      return st_;
    DN_TRY(conv_dgrad(ib, V(p.g_db[l], 2 * nf), EPI_MASK, V(p.da[l], 2 * nf), V(p.g_da[l], 2 * nf),
                      s));
    DN_TRY(bs.fork());
    // channel count ck (the layer's cin, what G(ia) and the dgrad pack are sized for); cs is
    // only the pixel stride (larger under a DN_C1S_ALIGN override)
    if (dn_status st_ = wg(ia, W_C3, V(p.g_da[l], 2 * nf), V(p.c[l], p.cs[l]), l, 2 * nf, p.ck[l], x6, bs.s2))
      return st_;
    DN_TRY(conv_dgrad(ia, V(p.g_da[l], 2 * nf), EPI_PLAIN, none, V(p.g_c[l], p.cs[l]), s));
    dU = V(p.g_c[l], p.cs[l], 0);  // [u_{l+1} grad | skip grad]
  }
  // the head's and the decoder's reductions on the side stream now, behind their weight
  // gradients, overlapping the encoder's data gradients
  DN_TRY(bs.flush_reductions());
  if (bs.side && tail_ready) {  // dprm[tail_begin ..] (dec_conv5a .. nin_c) is final behind this flush
    DN_TRY(hipEventRecord(tail_ready, bs.side->rst));
    tail_ready = nullptr;
  }
  // up5: x = a6 (level 5), dU = g_c5[0:nf]
  DN_TRY(bs.fork());
  if (dn_status st_ = wg(UP5, W_UP2, V(p.g_c[4], p.cs[4], 0), V(p.a6, nf), 5, nf, nf, false, bs.s2))
    return st_;
  DN_TRY(deconv_dgrad(UP5, V(p.g_c[4], p.cs[4], 0), V(p.a6, nf), EPI_MASK, V(p.g_a6, nf), s));
  // enc_conv6 (input p5, level 5)
  DN_TRY(bs.fork());
  if (dn_status st_ = wg(ENC6, W_C3, V(p.g_a6, nf), V(p.p5, nf), 5, nf, nf, x6, bs.s2)) return st_;
  DN_TRY(conv_dgrad(ENC6, V(p.g_a6, nf), EPI_PLAIN, none, V(p.g_p5, nf), s));
  // pool5 backward -> g_a5 (level 4)
  DN_TIMED(s, "pool_bwd", 0, 0, 0, 0, 0, 0, launch_pool_bwd(ws + p.a[4], N, H(4), Wd(4), nf, ws + p.g_p5, nf, 0, 1, ws + p.g_a[4], s));
  // enc_conv5..2: input p_{l} = skip slice of c_l; gradient accumulates into g_c_l's skip slice
  for (int l = 4; l >= 1; --l) {
    const int li = ENC2 + (l - 1);
    const int skip = (l == 4) ? nf : 2 * nf;
    DN_TRY(bs.fork());
    if (dn_status st_ = wg(li, W_C3, V(p.g_a[l], nf), V(p.c[l], p.cs[l], skip), l, nf, nf, x6, bs.s2))
      return st_;
    DN_TRY(conv_dgrad(li, V(p.g_a[l], nf), EPI_ACCUM, none, V(p.g_c[l], p.cs[l], skip), s));
    // pool_l backward: d p_l (skip slice) -> gradient of the level l-1 activation
    if (l > 1) {
      DN_TIMED(s, "pool_bwd", 0, 0, 0, 0, 0, 0, launch_pool_bwd(ws + p.a[l - 1], N, H(l - 1), Wd(l - 1), nf, ws + p.g_c[l], p.cs[l],
                             skip, 1, ws + p.g_a[l - 1], s));
    } else {
      DN_TIMED(s, "pool_bwd", 0, 0, 0, 0, 0, 0, launch_pool_bwd(ws + p.a1, N, H(0), Wd(0), nf, ws + p.g_c[1], p.cs[1], skip, 1,
                             ws + p.g_a1, s));
    }
  }
  // the encoder's deep-level reductions (up5, enc_conv6 .. enc_conv2) on the side stream now,
  // beside enc_conv1's data gradient, so the serial tail of the step (after the last data
  // gradient) only reduces enc_conv1's and enc_conv0's slabs
  DN_TRY(bs.flush_reductions());
  // enc_conv1 (input a0), enc_conv0 (input x = c1 slice; no data gradient needed).  Two
  // streams: enc_conv1's weight gradient on the main stream behind its data gradient and
  // enc_conv0's beside it on the side stream, which is still working through the encoder's
  // weight gradients (both streams end together instead of the side stream alone for ~0.5 ms,
  // profiles/r6_step_timeline.txt)
  DN_TRY(conv_dgrad(ENC1, V(p.g_a1, nf), EPI_MASK, V(p.a0, nf), V(p.g_a0, nf), s));
  DN_TRY(bs.fork());
  DN_TIMED(bs.s2, "wgrad3_thin", 2.0 * N * H(0) * Wd(0) * nf * C * 9, C, nf, H(0), Wd(0), N,
           launch_enc0_wgrad(ws + p.g_a0, nf, ws + p.xin, N, C, H(0), Wd(0), SL(ENC0) + 64,
                             p.splits[ENC0], G(ENC0), bs.s2, &bs.rb));
  if (dn_status st_ = wg(ENC1, W_C3, V(p.g_a1, nf), V(p.a0, nf), 0, nf, nf, x6, s)) return st_;
  DN_TRY(bs.join());  // the weight-gradient and reduction branches, before the last reduction
  DN_TIMED(s, "reduce", 0, 0, 0, 0, 0, 0, red_flush(bs.rb, s));
  if (tail_ready) DN_TRY(hipEventRecord(tail_ready, s));  // one stream: everything is final here
  // dL/dx: the network input feeds enc_conv0 and (as pool0) dec_conv1a's last C channels
  if (dx)
    DN_TIMED(s, "dgrad_input", 0, 0, 0, 0, 0, 0, launch_dgrad_input(ws + p.g_a0, prm + p.P.L[ENC0].woff, ws + p.g_d1a,
                              prm + p.P.L[D1A].woff, p.c1k, 2 * nf, N, C, H(0), Wd(0), dx, s));
  return DN_OK;
}

}  // namespace dn
