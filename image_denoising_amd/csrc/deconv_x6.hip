// ConvTranspose2d(96, 96, 2, 2) forward and data gradient in the bf16x6 arithmetic of
// conv_x6.hip (see its header and x6_core.h); the weight images are packed by pk_deconv_x6 and
// pk_deconv_dgrad_x6 (k_pack_batch, conv_x6.hip).
#include "conv_epi.h"
#include "x6_core.h"

namespace dn {

// ------------------------------------------------------------------------------------
// ConvTranspose2d(96, 96, 2, 2) forward (UpsampleCat's deconv, arch_unet.py:51-62) in the
// bf16x6 arithmetic: out(2y+a, 2x+b, co) = bias[co] + sum_ci x(y, x, ci) W[ci][co][a][b].
// Each parity's 96x96 weight matrix is pre-split ([plane][K block][co][32 ci], 64-B rows,
// swizzled quads; 54 KiB) and DMA'd into LDS.  A lane's B operand is 8 consecutive input
// channels of its pixel (two float4 loads, split in registers); the 16x16 C/D tile (rows =
// output channels, columns = pixels) is stored as float4 channel quads at the scattered
// output pixel.
// ------------------------------------------------------------------------------------
// Persistent: one 8-wave workgroup per CU holds two parity images, (a, 0) and (a, 1), waves 0-3 /
// 4-7 computing those parities; the two workgroups of a group (blockIdx.x bit 3 = a, the other
// bits = group; same XCD) cover the four parities of the same wave-tiles -- one low-res row of
// 16 pixels -- so three of the four reads of an input row hit that XCD's L2.  The next row's
// input is loaded into registers while the current one computes; the images are read from L2
// once per workgroup.
// B1: plain bf16 products (the bf16 base's autocast arithmetic, as k_nin_head_x6's B1): the input
// rounded to bf16, the images' leading planes (the weights rounded to bf16), one MFMA per block
// chained in fp32 -- a sixth of the MFMAs, so the launch is bound by its output stores
template <bool B1 = false>
__global__ __launch_bounds__(512, 1) void k_deconv_x6(FwdArgs a, const __bf16* wimg, int nwt) {
  __shared__ __attribute__((aligned(16))) __bf16 lw[2 * X6_HEAD_BF];
  __shared__ __attribute__((aligned(16))) float lbias[96];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int pa = (blockIdx.x >> 3) & 1, pb = wave >> 2, wq = wave & 3;
  const int grp = ((blockIdx.x >> 4) << 3) | (blockIdx.x & 7), ngrp = gridDim.x >> 1;
  const __bf16* src = wimg + 2 * pa * X6_HEAD_BF;  // parities 2a, 2a + 1
  for (int q = wave; q < 2 * X6_HEAD_BF * 2 / 1024; q += 8)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(src + q * 512 + lane * 8),
        (__attribute__((address_space(3))) void*)(lw + q * 512), 16, 0, 0);
  if (threadIdx.x < 96) lbias[threadIdx.x] = a.bias[threadIdx.x];
  const __bf16* img = lw + pb * X6_HEAD_BF;
  const int tiles_x = (a.OW + 15) / 16;
  const int wstride = ngrp * 4;
  // loads and stores through per-row buffer resources: out-of-range lanes (past the row or the
  // last wave-tile) get an out-of-range offset instead of a branch, so every wave-tile issues the
  // same 6 loads and 6 stores and the compiler's counted waits cover exactly the loads they need.
  // Constant offsets go into the vector offset (folded into the instruction's offset field), never
  // into soffset: a 16-byte buffer store with an SGPR soffset whose data registers were rewritten
  // by the very next instruction (an LDS read) stored a corrupted last dword on some lanes.
  const long in_row = (long)a.IWt * a.in_stride, out_row = 2L * a.OW * a.out_stride;
  auto load = [&](int wt, float4 (&v)[6]) {
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x, gx = (r - gy * tiles_x) * 16 + li;
    const bool ok = wt < nwt && gx < a.OW;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.in + ((long)n * a.IHt + gy) * in_row + a.in_off), (short)0,
        (int)(in_row * 4), 0x00020000);
    const int off = ok ? (gx * a.in_stride + 8 * lg) * 4 : 0x7fffffff;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      v[2 * b] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 128 * b, 0, 0));
      v[2 * b + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 128 * b + 16, 0, 0));
    }
  };
  // one wave-tile; two register sets alternate (see k_nin_head_x6)
  auto tile = [&](int wt, const float4 (&xin)[6]) {
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x, gx = (r - gy * tiles_x) * 16 + li;
    f32x4 out[6][1];
#pragma unroll
    for (int f = 0; f < 6; ++f) out[f][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float4 u0 = xin[2 * b], u1 = xin[2 * b + 1];
      const float v8[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
      if constexpr (B1) {
        bf16x8 x0;
#pragma unroll
        for (int j = 0; j < 8; ++j) x0[j] = (__bf16)v8[j];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          const int row = b * 96 + f * 16 + li;
          const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(img + row * 32 + x6_swz(row, lg) * 8);
          out[f][0] = mfma_bf16(w0, x0, out[f][0]);
        }
        continue;
      }
      bf16x8 xv[3][1];
      split3x8(v8, xv[0][0], xv[1][0], xv[2][0]);
      // one output fragment at a time, its three weight planes read one fragment ahead: 24
      // operand registers live instead of 72, which leaves room for the third input set below
      bf16x8 wv[2][3];
      auto read_w = [&](int f, bf16x8 (&w)[3]) {
        const int row = b * 96 + f * 16 + li;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          w[pl] = *reinterpret_cast<const bf16x8*>(img + (pl * 3 * 96 + row) * 32 + x6_swz(row, lg) * 8);
      };
      read_w(0, wv[0]);
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        if (f + 1 < 6) read_w(f + 1, wv[(f + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        // x6_group's product order (hi = w0 x0; lo = w0 x1, w1 x0, w0 x2, w1 x1, w2 x0)
        const bf16x8(&w)[3] = wv[f & 1];
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 hi = mfma_bf16(w[0], xv[0][0], z);
        f32x4 lo = mfma_bf16(w[0], xv[1][0], z);
        lo = mfma_bf16(w[1], xv[0][0], lo);
        lo = mfma_bf16(w[0], xv[2][0], lo);
        lo = mfma_bf16(w[1], xv[1][0], lo);
        lo = mfma_bf16(w[2], xv[0][0], lo);
        x6_acc_add(out[f][0], hi, lo);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        a.out + ((long)n * 2 * a.OH + 2 * gy + pa) * out_row + a.out_off, (short)0,
        (int)(out_row * 4), 0x00020000);
    // Whole 128-B lines per store: a lane holds 4 channels of fragments f and f + 1 of its own
    // pixel, so one store per fragment wrote only 64 B of each pixel's 32-channel line, and the
    // L2 filled the other half from HBM before the second store came (0.75 GB of extra fetch per
    // 256^2 launch, profiles/r5a_pmc_step.json).  Adjacent lanes (pixels 2p, 2p + 1 of the
    // wave-tile) swap one fragment's registers (DPP quad_perm [1,0,3,2]), and each store
    // instruction writes the full line (channels 32k .. 32k + 31) of one pixel per lane pair:
    // the even lane its fragment-f quad, the odd lane the even pixel's fragment-(f + 1) quad.
    const bool ev = (li & 1) == 0;
    const int gxa = gx - (li & 1);  // the pair's even pixel; gxa + 1 the odd one
    const int offa = gxa < a.OW ? ((2 * gxa + pb) * a.out_stride + 4 * lg + (ev ? 0 : 16)) * 4 : 0x7fffffff;
    const int offb = gxa + 1 < a.OW ? ((2 * gxa + 2 + pb) * a.out_stride + 4 * lg + (ev ? 0 : 16)) * 4
                                     : 0x7fffffff;
#pragma unroll
    for (int f = 0; f < 6; f += 2) {
      const float4 b0 = *reinterpret_cast<const float4*>(lbias + f * 16 + 4 * lg);
      const float4 b1 = *reinterpret_cast<const float4*>(lbias + f * 16 + 16 + 4 * lg);
      const f32x4 o0 = {out[f][0][0] + b0.x, out[f][0][1] + b0.y, out[f][0][2] + b0.z, out[f][0][3] + b0.w};
      const f32x4 o1 = {out[f + 1][0][0] + b1.x, out[f + 1][0][1] + b1.y, out[f + 1][0][2] + b1.z,
                        out[f + 1][0][3] + b1.w};
      f32x4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        t[r] = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                                             __builtin_bit_cast(int, ev ? o1[r] : o0[r]), 0xB1, 0xF, 0xF, false));
      const f32x4 va = ev ? o0 : t, vb = ev ? t : o1;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, va), rs, offa + 64 * f, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, vb), rs, offb + 64 * f, 0, 0);
    }
  };
  // three input register sets: a wave-tile's input is requested two tiles before it is used
  // (one tile of MFMA work did not cover the HBM latency: 0.8 ms at 64 x 128^2 -> 256^2 against
  // ~0.4 ms of HBM traffic)
  int wt = grp * 4 + wq;
  float4 xa[6], xb[6], xc[6];
  load(wt, xa);
  load(wt + wstride, xb);
  __syncthreads();  // parity images and bias landed
  for (; wt < nwt; wt += 3 * wstride) {
    load(wt + 2 * wstride, xc);
    tile(wt, xa);
    if (wt + wstride >= nwt) break;
    load(wt + 3 * wstride, xa);
    tile(wt + wstride, xb);
    if (wt + 2 * wstride >= nwt) break;
    load(wt + 4 * wstride, xb);
    tile(wt + 2 * wstride, xc);
  }
}

bool deconv_x6_ok(const FwdArgs& a) {  // float4 views; per-row buffer extents below 2^31 bytes
  return a.K == 96 && a.NOUT == 96 && !((a.in_stride | a.in_off | a.out_stride | a.out_off) & 3) &&
         (long)a.IWt * a.in_stride * 4 < 0x7fffffffL && 2L * a.OW * a.out_stride * 4 < 0x7fffffffL;
}

// raw deconv weight (96, 96, 2, 2) -> four pre-split parity images (4 x X6_HEAD_BF bf16)
hipError_t launch_pack_deconv_x6(const float* w, void* out, hipStream_t s) {
  PackBatch b;
  b.j[b.n++] = pack_job_deconv_x6(w, out);
  return pack_flush(b, s);
}

// a: in = x (IHt = OH = h, IWt = OW = w), out = the 2h x 2w view, bias; K = NOUT = 96; b1: plain
// bf16 products (the bf16 base)
hipError_t launch_deconv_x6(const FwdArgs& a, const void* wimg, hipStream_t s, bool b1) {
  if (!deconv_x6_ok(a)) return hipErrorInvalidValue;
  const long nwt = (long)a.N * a.OH * ((a.OW + 15) / 16);  // one low-res 16-pixel row per wave-tile
  if (nwt >= (1L << 31) - (1L << 20)) return hipErrorInvalidValue;
  // groups of two workgroups (one per parity row a), a multiple of 8 groups (one per XCD)
  long groups = (nwt + 3) / 4;
  if (groups > 128) groups = 128;
  groups = (groups + 7) / 8 * 8;
  if (b1) {
    prof_kernel("k_deconv_x6<true>");
    hipLaunchKernelGGL(k_deconv_x6<true>, dim3((unsigned)(2 * groups)), dim3(512), 0, s, a,
                       static_cast<const __bf16*>(wimg), (int)nwt);
  } else {
    prof_kernel("k_deconv_x6<false>");
    hipLaunchKernelGGL(k_deconv_x6<false>, dim3((unsigned)(2 * groups)), dim3(512), 0, s, a,
                       static_cast<const __bf16*>(wimg), (int)nwt);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Data gradient of the 96-channel ConvTranspose2d(2, 2) (arch_unet.py:51-62) in the bf16x6
// arithmetic: dx(y, x, ci) = sum_{a,b} sum_co dy(2y+a, 2x+b, co) W[ci][co][a][b] (x leaky'(mask)),
// a GEMM with K = 4 parities x 96.  Persistent, one 8-wave workgroup per CU holding the images of
// one input-channel half h for all four parities (4 x 27 KiB; the two halves' workgroups of a
// group share an XCD and the same wave-tiles, so the second read of dy hits L2); a wave-tile is
// one row of 16 output pixels x 48 channels, computed in four parity steps whose dy rows are
// loaded one step ahead (two alternating register sets), the mask with the last step.
// ------------------------------------------------------------------------------------
template <bool MASKED>
__global__ __launch_bounds__(512, 1) void k_deconv_dgrad_x6(FwdArgs a, const __bf16* wimg, int nwt) {
  __shared__ __attribute__((aligned(16))) __bf16 lw[4 * X6_DG_BF];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int h = (blockIdx.x >> 3) & 1;
  const int grp = ((blockIdx.x >> 4) << 3) | (blockIdx.x & 7), ngrp = gridDim.x >> 1;
  const __bf16* src = wimg + (long)h * 4 * X6_DG_BF;
  for (int q = wave; q < 4 * X6_DG_BF * 2 / 1024; q += 8)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(src + q * 512 + lane * 8),
        (__attribute__((address_space(3))) void*)(lw + q * 512), 16, 0, 0);
  const int tiles_x = (a.OW + 15) / 16;
  const int wstride = ngrp * 8;
  // per-row buffer resources, constant offsets in the vector offset (see k_deconv_x6)
  const long in_row = (long)a.IWt * a.in_stride;
  auto load = [&](int wt, int par, float4 (&v)[6]) {  // dy row 2gy + a, pixels 2gx + b
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x, gx = (r - gy * tiles_x) * 16 + li;
    const bool ok = wt < nwt && gx < a.OW;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.in + ((long)n * a.IHt + 2 * gy + (par >> 1)) * in_row + a.in_off),
        (short)0, (int)(in_row * 4), 0x00020000);
    const int off = ok ? ((2 * gx + (par & 1)) * a.in_stride + 8 * lg) * 4 : 0x7fffffff;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      v[2 * b] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 128 * b, 0, 0));
      v[2 * b + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 128 * b + 16, 0, 0));
    }
  };
  auto row_rsrc = [&](const float* base, int stride, int wt) {  // output-resolution row of wt
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x;
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(base + ((long)n * a.OH + gy) * a.OW * stride), (short)0,
        a.OW * stride * 4, 0x00020000);
  };
  auto pix_off = [&](int wt, int stride, int coff) {  // this lane's channel quad, or out of range
    const int r = wt % (a.OH * tiles_x), gx = (r % tiles_x) * 16 + li;
    return wt < nwt && gx < a.OW ? (gx * stride + coff + 48 * h + 4 * lg) * 4 : 0x7fffffff;
  };
  auto mload = [&](int wt, float4 (&m)[3]) {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(a.mask, a.mask_stride, wt);
    const int off = pix_off(wt, a.mask_stride, a.mask_off);
#pragma unroll
    for (int f = 0; f < 3; ++f)
      m[f] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 64 * f, 0, 0));
  };
  auto step = [&](int par, const float4 (&xin)[6], f32x4 (&acc)[3][1]) {
    const __bf16* img = lw + par * X6_DG_BF;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float4 u0 = xin[2 * b], u1 = xin[2 * b + 1];
      const float v8[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
      bf16x8 xv[3][1];
      split3x8(v8, xv[0][0], xv[1][0], xv[2][0]);
      bf16x8 wv[3][3];
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const int row = b * 48 + f * 16 + li;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          wv[pl][f] = *reinterpret_cast<const bf16x8*>(img + (pl * 3 * 48 + row) * 32 + x6_swz(row, lg) * 8);
      }
      x6_block<3, 1, 1>(acc, wv, xv);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the running sums materialised here: otherwise the compiler defers the fp32 adds of the
    // block sums to the epilogue and keeps every step's MFMA results live (it spills)
#pragma unroll
    for (int f = 0; f < 3; ++f) asm volatile("" : "+v"(acc[f][0]));
  };
  auto epilogue = [&](int wt, const f32x4 (&acc)[3][1], const float4 (&m)[3]) {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(a.out, a.out_stride, wt);
    const int off = pix_off(wt, a.out_stride, a.out_off);
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      float4 o = make_float4(acc[f][0][0], acc[f][0][1], acc[f][0][2], acc[f][0][3]);
      if constexpr (MASKED) {
        o.x *= m[f].x > 0.f ? 1.f : 0.2f; o.y *= m[f].y > 0.f ? 1.f : 0.2f;
        o.z *= m[f].z > 0.f ? 1.f : 0.2f; o.w *= m[f].w > 0.f ? 1.f : 0.2f;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, o), rs, off + 64 * f, 0, 0);
    }
  };
  int wt = grp * 8 + wave;
  float4 xa[6], xb[6], m[3] = {};
  load(wt, 0, xa);
  __syncthreads();  // images landed
  for (; wt < nwt; wt += wstride) {
    f32x4 acc[3][1];
#pragma unroll
    for (int f = 0; f < 3; ++f) acc[f][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(wt, 1, xb);
    step(0, xa, acc);
    load(wt, 2, xa);
    step(1, xb, acc);
    load(wt, 3, xb);
    if constexpr (MASKED) mload(wt, m);
    step(2, xa, acc);
    load(wt + wstride, 0, xa);
    step(3, xb, acc);
    epilogue(wt, acc, m);
  }
}

bool deconv_dgrad_x6_ok(const FwdArgs& a) {  // float4 views; per-row buffer extents below 2^31
  return a.K == 96 && a.NOUT == 96 && a.IHt == 2 * a.OH && a.IWt == 2 * a.OW &&
         !((a.in_stride | a.in_off | a.out_stride | a.out_off) & 3) &&
         (a.epi == EPI_PLAIN || (a.epi == EPI_MASK && a.mask && !((a.mask_stride | a.mask_off) & 3))) &&
         (long)a.IWt * a.in_stride * 4 < 0x7fffffffL && (long)a.OW * a.out_stride * 4 < 0x7fffffffL &&
         (a.epi != EPI_MASK || (long)a.OW * a.mask_stride * 4 < 0x7fffffffL);
}

hipError_t launch_deconv_dgrad_x6(const FwdArgs& a, const void* wimg, hipStream_t s) {
  if (!deconv_dgrad_x6_ok(a)) return hipErrorInvalidValue;
  const long nwt = (long)a.N * a.OH * ((a.OW + 15) / 16);  // one 16-pixel output row per wave-tile
  if (nwt >= (1L << 31) - (1L << 20)) return hipErrorInvalidValue;
  // groups of two workgroups (one per input-channel half), a multiple of 8 groups (one per XCD)
  long groups = (nwt + 7) / 8;
  if (groups > 128) groups = 128;
  groups = (groups + 7) / 8 * 8;
  const dim3 grid((unsigned)(2 * groups)), block(512);
  const __bf16* w = static_cast<const __bf16*>(wimg);
  if (a.epi == EPI_MASK) hipLaunchKernelGGL(k_deconv_dgrad_x6<true>, grid, block, 0, s, a, w, (int)nwt);
  else hipLaunchKernelGGL(k_deconv_dgrad_x6<false>, grid, block, 0, s, a, w, (int)nwt);
  return hipGetLastError();
}

}  // namespace dn
