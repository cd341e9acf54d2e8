// The fused nin head (nin_a -> nin_b -> nin_c) and its backward in the bf16x6 arithmetic of
// conv_x6.hip (see its header and x6_core.h); the weight images are packed by pk_head_x6
// (k_pack_batch, conv_x6.hip).
#include <type_traits>

#include "conv_epi.h"
#include "x6_core.h"

namespace dn {

// ------------------------------------------------------------------------------------
// The nin head (nin_a -> nin_b -> nin_c, arch_unet.py:186-190, 257-259) on the activated
// dec_conv1b output, with the two 96x96 1x1 GEMMs in the bf16x6 arithmetic.  As in k_nin_head
// the tile lives in the 16x16 MFMA C/D map (rows = channels, columns = 16 pixels), which is
// directly the B operand of the next GEMM: for K block b (32 channels) lane group g supplies
// channels {32b + 4g + r, 32b + 16 + 4g + r} (r < 4) = registers 2b and 2b+1 of its tile
// fragment, split into three bf16x8 planes in registers.  The weight images are pre-split
// in the same permuted K order (pk_head_x6: [plane][b][out][32], 64-B rows, quads
// swizzled) and DMA'd into LDS once per workgroup (54 KiB per layer).
// ------------------------------------------------------------------------------------
// Persistent: one 8-wave workgroup per CU keeps both images (108 KiB) and the biases / nin_c
// weights in LDS for the whole launch; wave-tiles are single 16-pixel rows, taken in a wave-
// strided loop, the next row's input loaded into registers while the current one computes
// (the images are read from L2 once per CU, not once per tile).
// SAVE: na / nb written for the backward; PAIR: the input is a pair image (hd.rd); B1: plain
// bf16 products (the bf16 base's autocast arithmetic): the input rounded to bf16, the images'
// leading planes (the weights rounded to bf16), one MFMA per block chained in fp32
// IBF (with B1): the input activation is stored as bf16 (FwdArgs::in_bf16), 8 bytes per lane and
// 4 channels, taken as the operand without conversion
// RES: the network input hd.res (NCHW, oc channels, y's layout) added to nin_c's output in the
// epilogue (the RESNET's global residual)
template <bool SAVE, bool PAIR, bool B1 = false, bool IBF = false, bool RES = false>
__global__ __launch_bounds__(512, 1) void k_nin_head_x6(FwdArgs a, HeadArgs hd, const __bf16* wimg,
                                                      int nwt) {
  static_assert(!IBF || B1, "bf16 input only in the plain-bf16 head");
  static_assert(!RES || (!PAIR && !B1), "the residual head is the full-image split-product head");
  __shared__ __attribute__((aligned(16))) __bf16 lw[2 * X6_HEAD_BF];
  __shared__ __attribute__((aligned(16))) float lb[2 * 96 + X6_HEAD_OCMAX * 97];  // ba|bb|wc|bc
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  for (int q = wave; q < 2 * X6_HEAD_BF * 2 / 1024; q += 8)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(wimg + q * 512 + lane * 8),
        (__attribute__((address_space(3))) void*)(lw + q * 512), 16, 0, 0);
  for (int e = threadIdx.x; e < 2 * 96 + hd.oc * 97; e += 512) {
    float v;
    if (e < 96) v = hd.ba[e];
    else if (e < 192) v = hd.bb[e - 96];
    else if (e < 192 + hd.oc * 96) v = hd.wc[e - 192];
    else v = hd.bc[e - 192 - hd.oc * 96];
    lb[e] = v;
  }
  const float* lbc = lb + 192 + hd.oc * 96;
  const int tiles_x = (a.OW + 15) / 16;
  const int wstride = gridDim.x * 8;
  // per-row buffer resources, out-of-range offsets instead of branches (see k_deconv_x6)
  const long in_row = (long)a.IWt * a.in_stride;
  auto load = [&](int wt, f32x4 (&v)[6], int& rd) {
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x, gx = (r - gy * tiles_x) * 16 + li;
    const bool ok = wt < nwt && gx < a.OW;
    constexpr int EB = IBF ? 2 : 4;  // bytes per stored activation
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(a.in) +
                                   (((long)n * a.IHt + gy) * in_row + a.in_off) * EB),
        (short)0, (int)(in_row * EB), 0x00020000);
    const int off = ok ? (gx * a.in_stride + 4 * lg) * EB : 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      if constexpr (IBF) {  // bf16 bits of channels 16q + 4lg .. +3 in v[q][0..1]
        typedef unsigned u32x2h __attribute__((ext_vector_type(2)));
        const u32x2h d = __builtin_bit_cast(u32x2h, __builtin_amdgcn_raw_buffer_load_b64(rs, off + 32 * q, 0, 0));
        v[q] = f32x4{__uint_as_float(d[0]), __uint_as_float(d[1]), 0.f, 0.f};
      } else {
        v[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 64 * q, 0, 0));
      }
    }
    if constexpr (PAIR) {  // the cell's pair choice, loaded with the row (no wait of its own later)
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<unsigned char*>(hd.rd + ((long)n * a.OH + gy) * (a.OW / 2)), (short)0,
          a.OW / 2, 0x00020000);
      rd = __builtin_amdgcn_raw_buffer_load_b8(rr, ok ? gx >> 1 : 0x7fffffff, 0, 0);
    }
  };
  auto bias_act = [](f32x4& v, float4 b) {
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : v[r] * 0.2f;
  };
  auto save = [&](float* dst, long row, int off, const f32x4& v, int q) {  // 16 px x 96 ch
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst + row * a.OW * 96, (short)0,
                                                                        a.OW * 96 * 4, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs, off + 64 * q, 0, 0);
  };
  // out = W (LDS image at `img`) x in, three 32-channel K blocks of six split products each
  // (INB: `in` holds bf16 bits as loaded by load() under IBF)
  auto gemm96 = [&](auto inb_tag, const __bf16* img, const f32x4 (&in)[6], f32x4 (&out)[6][1]) {
    constexpr bool INB = decltype(inb_tag)::value;
#pragma unroll
    for (int f = 0; f < 6; ++f) out[f][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      bf16x8 xv[3][1];
      const float v8[8] = {in[2 * b][0], in[2 * b][1], in[2 * b][2], in[2 * b][3],
                           in[2 * b + 1][0], in[2 * b + 1][1], in[2 * b + 1][2], in[2 * b + 1][3]};
      if constexpr (B1) {
        if constexpr (INB) {
          const u32x4_t d = {__float_as_uint(in[2 * b][0]), __float_as_uint(in[2 * b][1]),
                             __float_as_uint(in[2 * b + 1][0]), __float_as_uint(in[2 * b + 1][1])};
          xv[0][0] = __builtin_bit_cast(bf16x8, d);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xv[0][0][j] = (__bf16)v8[j];
        }
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          const int row = b * 96 + f * 16 + li;
          const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(img + row * 32 + x6_swz(row, lg) * 8);
          out[f][0] = mfma_bf16(w0, xv[0][0], out[f][0]);
        }
        continue;
      }
      split3x8(v8, xv[0][0], xv[1][0], xv[2][0]);
      bf16x8 wv[3][6];
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const int row = b * 96 + f * 16 + li;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          wv[pl][f] = *reinterpret_cast<const bf16x8*>(img + (pl * 3 * 96 + row) * 32 + x6_swz(row, lg) * 8);
      }
      x6_block<6, 1, 1>(out, wv, xv);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // one wave-tile; two register sets (xa, xb) alternate so that the next tile's loads are in
  // flight while this one computes and no copy forces a wait for them (or for the stores)
  auto tile = [&](int wt, const f32x4 (&xin)[6], int rd) {
    const int n = wt / (a.OH * tiles_x), r = wt - n * a.OH * tiles_x;
    const int gy = r / tiles_x, gx = (r - gy * tiles_x) * 16 + li;
    const bool ok = gx < a.OW;
    const long row = (long)n * a.OH + gy;
    const int soff = ok ? (gx * 96 + 4 * lg) * 4 : 0x7fffffff;
    f32x4 u[6][1], h[6];
    gemm96(std::integral_constant<bool, IBF>{}, lw, xin, u);  // nin_a
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      bias_act(u[f][0], *reinterpret_cast<const float4*>(lb + f * 16 + 4 * lg));
      h[f] = u[f][0];
    }
    if constexpr (SAVE)
#pragma unroll
      for (int f = 0; f < 6; ++f) save(hd.na, row, soff, h[f], f);
    gemm96(std::false_type{}, lw + X6_HEAD_BF, h, u);  // nin_b
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      bias_act(u[f][0], *reinterpret_cast<const float4*>(lb + 96 + f * 16 + 4 * lg));
      if constexpr (SAVE) save(hd.nb, row, soff, u[f][0], f);
    }
    // nin_c (fp32 VALU): per-lane partial over its 24 channels, then across the lane groups;
    // lane group 0 stores (the others get an out-of-range offset)
    // PAIR: pair image pixel (gy, gx) -> pixel pair[rd][gx & 1] of cell (gy, gx / 2), i.e. y's
    // rows 2gy, 2gy + 1
    int yoff = 0x7fffffff;
    if (lg == 0 && ok) {
      if constexpr (PAIR) {
        constexpr unsigned kPair = 0xB721ED84u;
        const int k = (kPair >> (4 * (rd & 7) + 2 * (gx & 1))) & 3;
        yoff = ((k >> 1) * a.OW + (gx & ~1) + (k & 1)) * 4;
      } else {
        yoff = gx * 4;
      }
    }
    constexpr int YR = PAIR ? 2 : 1;  // y rows per wave-tile
    for (int o = 0; o < hd.oc; ++o) {
      float t = 0.f;
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const float4 w = *reinterpret_cast<const float4*>(lb + 192 + o * 96 + f * 16 + 4 * lg);
        t = fmaf(w.x, u[f][0][0], t); t = fmaf(w.y, u[f][0][1], t);
        t = fmaf(w.z, u[f][0][2], t); t = fmaf(w.w, u[f][0][3], t);
      }
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
          hd.y + (((long)n * hd.oc + o) * YR * a.OH + YR * gy) * a.OW, (short)0, YR * a.OW * 4,
          0x00020000);
      float yv = t + lbc[o];
      if constexpr (RES) {  // (out-of-range lanes read zero and drop their store)
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(hd.res) + (((long)n * hd.oc + o) * a.OH + gy) * a.OW, (short)0,
            a.OW * 4, 0x00020000);
        yv += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, yoff, 0, 0));
      }
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), ry, yoff, 0, 0);
    }
  };
  int wt = blockIdx.x * 8 + wave;
  f32x4 xa[6], xb[6];
  int ra = 0, rb = 0;
  load(wt, xa, ra);
  __syncthreads();  // images, biases and nin_c weights landed
  for (; wt < nwt; wt += 2 * wstride) {
    load(wt + wstride, xb, rb);
    tile(wt, xa, ra);
    if (wt + wstride >= nwt) break;
    load(wt + 2 * wstride, xa, ra);
    tile(wt + wstride, xb, rb);
  }
}


// ------------------------------------------------------------------------------------
// Backward of the fused head in the bf16x6 arithmetic (k_head_bwd's products on the fp32
// matrix cores, arch_unet.py:186-190 differentiated):
//   g_nb = leaky'(nb) * (Wc^T dy)      (fp32 VALU, K = oc, nin_c's weights in LDS)
//   g_na = leaky'(na) * (Wb^T g_nb)    (bf16x6 GEMM, image Wb^T)
//   g_d1b = leaky'(d1b) * (Wa^T g_na)  (bf16x6 GEMM, image Wa^T)
// The tile stays in the MFMA C/D map (rows = channels, columns = 16 pixels), which is the B
// operand of the next GEMM as in k_nin_head_x6; the transposed images (pk_head_x6 with flip) are
// DMA'd into LDS once per workgroup.  One 8-wave workgroup per CU walks 16-pixel wave-tiles of
// the flattened pixel range; a tile's nb / dy / na / d1b loads are issued together at its start
// (the other wave on the SIMD computes meanwhile).  Every 16-pixel tile addresses its rows
// through its own buffer resource (pixel ranges beyond 2 GiB, out-of-range lanes read zeros and
// drop their stores).
// ------------------------------------------------------------------------------------
template <int OCM>  // nin_c outputs at most (registers of dy)
__global__ __launch_bounds__(512, 1) void k_head_bwd_x6(HeadBwdArgs h, const __bf16* wimg, long nwt) {
  __shared__ __attribute__((aligned(16))) __bf16 lw[2 * X6_HEAD_BF];
  __shared__ __attribute__((aligned(16))) float lc[X6_HEAD_OCMAX * 96];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  for (int q = wave; q < 2 * X6_HEAD_BF * 2 / 1024; q += 8)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(wimg + q * 512 + lane * 8),
        (__attribute__((address_space(3))) void*)(lw + q * 512), 16, 0, 0);
  for (int e = threadIdx.x; e < h.oc * 96; e += 512) lc[e] = h.wc[e];
  __syncthreads();
  auto rsrc = [&](const float* base, long px0, int npx_t) {  // 16 pixels x 96 channels
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + px0 * 96), (short)0,
                                             npx_t * 96 * 4, 0x00020000);
  };
  auto mask = [](f32x4& v, const f32x4& m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = m[r] > 0.f ? v[r] : v[r] * 0.2f;
  };
  // out = W (LDS image at `img`) x in: three 32-channel K blocks of six split products each
  // (k_nin_head_x6's gemm96)
  auto gemm96 = [&](const __bf16* img, const f32x4 (&in)[6], f32x4 (&out)[6][1]) {
#pragma unroll
    for (int f = 0; f < 6; ++f) out[f][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      bf16x8 xv[3][1];
      const float v8[8] = {in[2 * b][0], in[2 * b][1], in[2 * b][2], in[2 * b][3],
                           in[2 * b + 1][0], in[2 * b + 1][1], in[2 * b + 1][2], in[2 * b + 1][3]};
      split3x8(v8, xv[0][0], xv[1][0], xv[2][0]);
      bf16x8 wv[3][6];
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const int row = b * 96 + f * 16 + li;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          wv[pl][f] = *reinterpret_cast<const bf16x8*>(img + (pl * 3 * 96 + row) * 32 + x6_swz(row, lg) * 8);
      }
      x6_block<6, 1, 1>(out, wv, xv);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  const int loff = (li * 96 + 4 * lg) * 4;  // lane's bytes within a tile row set
  for (long wt = (long)blockIdx.x * 8 + wave; wt < nwt; wt += (long)gridDim.x * 8) {
    const long px0 = wt * 16;
    const int npx_t = h.npx - px0 < 16 ? (int)(h.npx - px0) : 16;
    const bool ok = li < npx_t;
    const int off = ok ? loff : 0x7fffffff;
    const __amdgpu_buffer_rsrc_t rnb = rsrc(h.nb, px0, npx_t), rna = rsrc(h.na, px0, npx_t),
                                 rd1 = rsrc(h.d1b, px0, npx_t);
    f32x4 nb[6], na[6], d1[6];
#pragma unroll
    for (int q = 0; q < 6; ++q)
      nb[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rnb, off + 64 * q, 0, 0));
    float dy[OCM];
    const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(h.dy + px0 * h.dy_stride), (short)0, npx_t * h.dy_stride * 4, 0x00020000);
#pragma unroll
    for (int o = 0; o < OCM; ++o)
      if (o < h.oc)
        dy[o] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                              rdy, ok ? (li * h.dy_stride + o) * 4 : 0x7fffffff, 0, 0));
#pragma unroll
    for (int q = 0; q < 6; ++q)
      na[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rna, off + 64 * q, 0, 0));
    // g_nb (K = oc, k_head_bwd's order)
    f32x4 t[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) t[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < OCM; ++o) {
      if (o >= h.oc) break;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const float4 w = *reinterpret_cast<const float4*>(lc + o * 96 + q * 16 + 4 * lg);
        t[q][0] = fmaf(w.x, dy[o], t[q][0]); t[q][1] = fmaf(w.y, dy[o], t[q][1]);
        t[q][2] = fmaf(w.z, dy[o], t[q][2]); t[q][3] = fmaf(w.w, dy[o], t[q][3]);
      }
    }
    // (h.g_nb null: k_wgrad1p<., GNB> recomputes g_nb from dy and nb, nothing stores it)
    const __amdgpu_buffer_rsrc_t wnb = rsrc(h.g_nb ? h.g_nb : h.nb, px0, h.g_nb ? npx_t : 0);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      mask(t[q], nb[q]);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, t[q]), wnb, off + 64 * q, 0, 0);
    }
    f32x4 u[6][1];
    gemm96(lw, t, u);  // Wb^T g_nb
    // d1b's loads behind the first GEMM (registers), in flight during the second
#pragma unroll
    for (int q = 0; q < 6; ++q)
      d1[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd1, off + 64 * q, 0, 0));
    const __amdgpu_buffer_rsrc_t wna = rsrc(h.g_na, px0, npx_t);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      mask(u[q][0], na[q]);
      t[q] = u[q][0];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, t[q]), wna, off + 64 * q, 0, 0);
    }
    gemm96(lw + X6_HEAD_BF, t, u);  // Wa^T g_na
    const __amdgpu_buffer_rsrc_t wd1 = rsrc(h.g_d1b, px0, npx_t);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      mask(u[q][0], d1[q]);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, u[q][0]), wd1, off + 64 * q, 0, 0);
    }
  }
}

// wimg = pack_job_head_bwd_x6's images; every tensor NHWC stride 96 (dy: dy_stride, oc <=
// X6_HEAD_BWD_OCMAX: dy in registers; more outputs spill, k_head_bwd takes them)
hipError_t launch_head_bwd_x6(const HeadBwdArgs& h, const void* wimg, hipStream_t s) {
  if (h.oc < 1 || h.oc > X6_HEAD_BWD_OCMAX || h.npx < 1 || h.dy_stride < h.oc) return hipErrorInvalidValue;
  const long nwt = (h.npx + 15) / 16;
  const long blocks = (nwt + 7) / 8 < 256 ? (nwt + 7) / 8 : 256;  // one workgroup per CU
  prof_kernel("k_head_bwd_x6<4>");
  hipLaunchKernelGGL(k_head_bwd_x6<4>, dim3((unsigned)blocks), dim3(512), 0, s, h,
                     static_cast<const __bf16*>(wimg), nwt);
  return hipGetLastError();
}

// nin_a / nin_b weights (OIHW 96x96x1x1, contiguous) -> the two pre-split head images
hipError_t launch_pack_head_x6(const float* wa, const float* wb, void* out, hipStream_t s) {
  PackBatch b;
  b.j[b.n++] = pack_job_head_x6(wa, wb, out);
  return pack_flush(b, s);
}

hipError_t launch_nin_head_x6(const FwdArgs& a, const HeadArgs& h, const void* wimg, hipStream_t s,
                              bool bf16) {
  if ((bf16 && (h.rd || (h.na && h.nb))) || (a.in_bf16 && !bf16) || a.K != 96 || h.oc < 1 ||
      h.oc > X6_HEAD_OCMAX || ((a.in_stride | a.in_off) & 3) ||
      (long)a.IWt * a.in_stride * 4 >= 0x7fffffffL || (long)a.OW * 96 * 4 * 2 >= 0x7fffffffL)
    return hipErrorInvalidValue;
  const long nwt = (long)a.N * a.OH * ((a.OW + 15) / 16);  // one 16-pixel row per wave-tile
  if (nwt >= (1L << 31) - (1L << 20)) return hipErrorInvalidValue;
  long blocks = (nwt + 7) / 8;
  if (blocks > 256) blocks = 256;  // one workgroup per CU
  const __bf16* w = static_cast<const __bf16*>(wimg);
  const dim3 grid((unsigned)blocks), block(512);
  const bool save = h.na && h.nb;
  if (save && h.rd) return hipErrorInvalidValue;  // the pair pass saves nothing
  if (h.res && (h.rd || bf16)) return hipErrorInvalidValue;
  if (h.res && save)
    hipLaunchKernelGGL((k_nin_head_x6<true, false, false, false, true>), grid, block, 0, s, a, h, w, (int)nwt);
  else if (h.res)
    hipLaunchKernelGGL((k_nin_head_x6<false, false, false, false, true>), grid, block, 0, s, a, h, w, (int)nwt);
  else if (h.rd) hipLaunchKernelGGL((k_nin_head_x6<false, true>), grid, block, 0, s, a, h, w, (int)nwt);
  else if (save) hipLaunchKernelGGL((k_nin_head_x6<true, false>), grid, block, 0, s, a, h, w, (int)nwt);
  else if (bf16 && a.in_bf16)
    hipLaunchKernelGGL((k_nin_head_x6<false, false, true, true>), grid, block, 0, s, a, h, w, (int)nwt);
  else if (bf16) hipLaunchKernelGGL((k_nin_head_x6<false, false, true>), grid, block, 0, s, a, h, w, (int)nwt);
  else hipLaunchKernelGGL((k_nin_head_x6<false, false>), grid, block, 0, s, a, h, w, (int)nwt);
  return hipGetLastError();
}

}  // namespace dn
