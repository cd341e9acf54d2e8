// dec_conv1a(up1(d2b)) as ONE launch in forward-only plans, in the bf16x6 arithmetic of
// conv_x6.hip (see its header and x6_core.h).
//
// UpsampleCat (arch_unet.py:51-62) applies no activation between its ConvTranspose2d(96, 96, 2, 2)
// and the concat, so the 96 up1 channels of dec_conv1a's input are a linear map of d2b and the
// conv of them is, per output parity (py, px), a 2x2-tap convolution over the LOW-resolution
// d2b: four 96 x 96 taps per parity instead of nine, no deconv launch and no 96-channel
// high-resolution tensor written and read back.  The pack job (pk_upconv_x6, conv_x6.hip) forms
// the 16 composed matrices and the border-dependent bias in fp64; the image channels stay a 3x3
// conv of the network input at high resolution.
//
//   * Workgroup = 4 waves, two workgroups per CU; tile = 8 x 8 low-resolution pixels + 1 halo:
//     10 x 10 pixels x 96 channels, loaded and split ONCE into three bf16 planes (57.6 KB:
//     [plane][32-channel block][pixel][4 quads of 8], quad q of tile pixel (y, x) at
//     q ^ ((x & 1) | (y & 1) << 1): every ds_read_b128 lane group of a pixel fragment reads 16
//     distinct 16-B slots at any tap shift).
//   * Wave = one output parity: 96 outputs x the tile's four pixel fragments (2 rows x 8 pixels),
//     one 128-B output line (two output fragments) at a time: 4 taps x 3 blocks, each weight
//     fragment straight from L2 into registers (one block ahead) and used by all four pixel
//     fragments; the carried-correction accumulation of x6_block_c.
//   * Image channels on the matrix cores: K = 9 taps x 6 split products x C packed into
//     ceil(54 C / 32) blocks; the lane's B operand gathered from the split 18 x 18 input tile in
//     LDS through a K -> offset table; summed from zero, joined by a round-to-nearest add.
//   * Epilogue: bias by the pixel's border class (which of the deconv bias's taps are in range),
//     LeakyReLU, then k_deconv_x6's whole-line stores: adjacent lanes swap a fragment's registers
//     by DPP, so each store writes 128 B of one pixel per lane pair.
#include "conv_epi.h"
#include "x6_core.h"

namespace dn {

constexpr int UPC_TP = 100;                  // tile pixels (10 x 10)
constexpr int UPC_XT = 18 * 18 * 3;          // bf16 per image channel of the split input tile

__global__ __launch_bounds__(256, 2) void k_upconv3_x6(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 lx[3 * 3 * UPC_TP * 32];
  __shared__ __attribute__((aligned(16))) float lbias[UPC_BIAS_F];
  __shared__ __attribute__((aligned(16))) __bf16 xt[4 * UPC_XT];
  __shared__ short ktab[UPC_XKB * 32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int h = a.IHt, w = a.IWt, C = a.K - 96;
  const int tiles_x = (w + 7) / 8;
  int bxr, byr;
  xcd_tile(bxr, byr);
  const int ty0 = (bxr / tiles_x) * 8, tx0 = (bxr % tiles_x) * 8, n = byr;
  const __bf16* wimg = reinterpret_cast<const __bf16*>(a.wp);
  const __bf16* ximg = wimg + UPC_W_BF;
  const float* bimg = reinterpret_cast<const float*>(ximg + UPC_X_BF);

  // ---- stage: the low-resolution tile (split), the input tile (split), bias table, K table ----
  {
    float4 v[5][2];
    const float* inb = a.in + (long)n * h * w * a.in_stride + a.in_off;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int it = tid + 256 * r, p = it / 12, oc = it - 12 * p;
      const int y = p / 10, x = p - 10 * y, gy = ty0 - 1 + y, gx = tx0 - 1 + x;
      v[r][0] = v[r][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < UPC_TP && gy >= 0 && gy < h && gx >= 0 && gx < w) {
        const float4* src = reinterpret_cast<const float4*>(inb + ((long)gy * w + gx) * a.in_stride + 8 * oc);
        v[r][0] = src[0];
        v[r][1] = src[1];
      }
    }
    for (int e = tid; e < UPC_BIAS_F; e += 256) lbias[e] = bimg[e];
    for (int k = tid; k < UPC_XKB * 32; k += 256) {
      // K index k = slot + 6 (c + C tap) -> the lane-relative offset of its operand piece in xt
      const int slot = k % 6, ct = k / 6, c = ct % C, tap = ct / C;
      const int piece = slot == 1 || slot == 5 ? 1 : (slot == 3 ? 2 : 0);  // (h,m,h,l,h,m)
      ktab[k] = tap < 9 ? (short)(c * UPC_XT + ((tap / 3) * 18 + tap % 3) * 3 + piece) : (short)0;
    }
    const int OH = a.OH, OW = a.OW;
    for (int e = tid; e < 324 * C; e += 256) {
      const int c = e / 324, r = e - 324 * c, yy = r / 18, xx = r - 18 * yy;
      const int gy = 2 * ty0 - 1 + yy, gx = 2 * tx0 - 1 + xx;
      float xv = 0.f;
      if (gy >= 0 && gy < OH && gx >= 0 && gx < OW) xv = a.in_t1[(((long)n * C + c) * OH + gy) * OW + gx];
      __bf16 ph, pm, pl;
      split3(xv, ph, pm, pl);
      xt[3 * e] = ph; xt[3 * e + 1] = pm; xt[3 * e + 2] = pl;
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int it = tid + 256 * r, p = it / 12, oc = it - 12 * p;
      if (p >= UPC_TP) continue;
      const int y = p / 10, x = p - 10 * y;
      const float v8[8] = {v[r][0].x, v[r][0].y, v[r][0].z, v[r][0].w,
                           v[r][1].x, v[r][1].y, v[r][1].z, v[r][1].w};
      bf16x8 p0, p1, p2;
      split3x8(v8, p0, p1, p2);
      const int o = ((oc >> 2) * UPC_TP + p) * 32 + (((oc & 3) ^ ((x & 1) | ((y & 1) << 1))) * 8);
      *reinterpret_cast<bf16x8*>(lx + o) = p0;
      *reinterpret_cast<bf16x8*>(lx + 3 * UPC_TP * 32 + o) = p1;
      *reinterpret_cast<bf16x8*>(lx + 6 * UPC_TP * 32 + o) = p2;
    }
  }
  __syncthreads();

  // ---- the wave's parity: three output lines of two fragments each ----
  const int py = wave >> 1, px = wave & 1;
  const int ly = li >> 3, lxx = li & 7;  // the lane's pixel in a fragment (2 rows x 8 pixels)
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<__bf16*>(wimg), (short)0, UPC_W_BF * 2, 0x00020000);
  const int wvoff = (li * 32 + lg * 8) * 2;
  // the lane's operand address per tap (tile pixel of fragment 0, swizzled quad); fragments,
  // blocks and planes are constant offsets from it (the swizzle's row bit is the same for every
  // fragment: fragments are two rows apart)
  int xo[4];
#pragma unroll
  for (int tap = 0; tap < 4; ++tap) {
    const int y = ly + py + (tap >> 1), x = lxx + px + (tap & 1);
    xo[tap] = (y * 10 + x) * 32 + ((lg ^ ((x & 1) | ((y & 1) << 1))) * 8);
  }
  const int nkb = (54 * C + 31) / 32;
  const long out_px = a.out_stride;
  float* outn = a.out + (long)n * a.OH * a.OW * out_px + a.out_off;
#pragma unroll 1
  for (int fp = 0; fp < 3; ++fp) {
    f32x4 acc[2][4], accl[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[m][q] = accl[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // weight fragments of (tap, block) step s = 3 tap + b: [plane][output fragment]; through a
    // buffer resource, the step's offset in the scalar offset (one lane offset register for all
    // 72 loads of a line; as flat addresses each load's 64-bit address was hoisted and spilled)
    auto load_w = [&](int s, bf16x8 (&wv)[3][2]) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int m = 0; m < 2; ++m)
          wv[pl][m] = __builtin_bit_cast(
              bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                          wrs, wvoff, ((((wave * 12 + s) * 3 + pl) * 96 + (2 * fp + m) * 16) * 32) * 2, 0));
    };
    bf16x8 wv[2][3][2];
    load_w(0, wv[0]);
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      const int tap = s / 3, b = s % 3;
      if (s + 1 < 12) load_w(s + 1, wv[(s + 1) & 1]);
      bf16x8 xv[3][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          xv[pl][q] = *reinterpret_cast<const bf16x8*>(lx + xo[tap] + ((pl * 3 + b) * UPC_TP + 20 * q) * 32);
      }
      // (one step's operands at a time: unfenced, the scheduler hoists every step's loads and spills)
      __builtin_amdgcn_sched_barrier(0);
      x6_block_c<2, 4, 1>(acc, accl, wv[s & 1], xv);
      // the running sums materialised here: otherwise the fp32 adds of the leading products sink
      // past the loop and every step's MFMA results stay live (k_deconv_dgrad_x6)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[m][q]));
      __builtin_amdgcn_sched_barrier(0);
    }
    x6_fold<2, 4>(acc, accl);
    // the image channels: one MFMA per K block and fragment pair, summed from zero
    {
      f32x4 hi[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) hi[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kb = 0; kb < nkb; ++kb) {
        bf16x8 wx[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          wx[m] = *reinterpret_cast<const bf16x8*>(ximg + (kb * 96 + (2 * fp + m) * 16 + li) * 32 + lg * 8);
        int ko[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ko[j] = ktab[kb * 32 + lg * 8 + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int base = ((2 * (2 * q + ly) + py) * 18 + 2 * lxx + px) * 3;
          bf16x8 xb;
#pragma unroll
          for (int j = 0; j < 8; ++j) xb[j] = xt[base + ko[j]];
#pragma unroll
          for (int m = 0; m < 2; ++m) hi[m][q] = mfma_bf16(wx[m], xb, hi[m][q]);
        }
      }
      x6_fold<2, 4>(acc, hi);
    }
    // epilogue: bias by border class, LeakyReLU, whole 128-B lines (see k_deconv_x6)
    const bool ev = (li & 1) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gy = ty0 + 2 * q + ly, gx = tx0 + lxx;
      const int Y = 2 * gy + py, X = 2 * gx + px;
      const int cls = (Y == 0 ? 0 : (Y == a.OH - 1 ? 2 : 1)) * 3 + (X == 0 ? 0 : (X == a.OW - 1 ? 2 : 1));
      f32x4 o[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float4 bv = *reinterpret_cast<const float4*>(lbias + cls * 96 + (2 * fp + m) * 16 + 4 * lg);
        o[m] = f32x4{acc[m][q][0] + bv.x, acc[m][q][1] + bv.y, acc[m][q][2] + bv.z, acc[m][q][3] + bv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) o[m][r] = o[m][r] > 0.f ? o[m][r] : o[m][r] * 0.2f;
      }
      f32x4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        t[r] = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                                             __builtin_bit_cast(int, ev ? o[1][r] : o[0][r]), 0xB1, 0xF, 0xF, false));
      // the pair's even pixel: the even lane its fragment-0 quad, the odd lane that pixel's
      // fragment-1 quad; then the odd pixel likewise
      const f32x4 va = ev ? o[0] : t, vb = ev ? t : o[1];
      const int gxa = gx - (li & 1);
      float* row = outn + (long)Y * a.OW * out_px + 32 * fp + 4 * lg + (ev ? 0 : 16);
      if (gy < h && gxa < w)
        *reinterpret_cast<f32x4*>(row + (long)(2 * gxa + px) * out_px) = va;
      if (gy < h && gxa + 1 < w)
        *reinterpret_cast<f32x4*>(row + (long)(2 * gxa + 2 + px) * out_px) = vb;
    }
  }
}

bool upconv3_x6_ok(const FwdArgs& a) {  // float4 views, C image channels in [1, 4]
  return a.NOUT == 96 && a.K > 96 && a.K <= 100 && a.OH == 2 * a.IHt && a.OW == 2 * a.IWt &&
         a.in_t1 && a.wp && a.out_layout == OUT_NHWC &&
         !((a.in_stride | a.in_off | a.out_stride | a.out_off) & 3) && a.in_stride >= 96 &&
         a.out_stride >= 96 && (long)((a.IHt + 7) / 8) * ((a.IWt + 7) / 8) < (1L << 31) && a.N < 65536;
}

hipError_t launch_upconv3_x6(const FwdArgs& a, hipStream_t s) {
  if (!upconv3_x6_ok(a)) return hipErrorInvalidValue;
  prof_kernel("k_upconv3_x6");
  const dim3 grid((unsigned)(((a.IHt + 7) / 8) * ((a.IWt + 7) / 8)), (unsigned)a.N);
  hipLaunchKernelGGL(k_upconv3_x6, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dn
