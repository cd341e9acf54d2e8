// Pieces shared by the direct bf16x6 3x3 kernels of conv_x6.hip: profiling labels of template
// instantiations, the counted waits and the barrier of the pipelined kernels, and the parts that
// are the same for every tile shape (tile origin, x-tile staging), each templated
// on the kernel's config struct C (XCfg / PCfg / SCfg / HCfg).
#pragma once

#include <string>

#include "x6_core.h"

namespace dn {

// profiling label of a template instantiation ("k_c3x6p<6,0>"; -1 = parameter absent)
static std::string x6_kname(const char* k, int p0, int p1, int p2) {
  std::string n = std::string(k) + "<" + std::to_string(p0);
  for (int v : {p1, p2})
    if (v >= 0) n += "," + std::to_string(v);
  return n + ">";
}
// the same with one more template argument spelled out: x6_kmore(x6_kname(...), "false")
static std::string x6_kmore(std::string n, const char* last) {
  n.back() = ',';
  return n.append(last).append(">");
}

#define X6_WAITCNT_VM(n) \
  __builtin_amdgcn_s_waitcnt(((n) & 0xF) | (((n) >> 4) << 14) | (0x7 << 4) | (0xF << 8))
// the same with lgkmcnt(0): at a stage's end every LDS read has been consumed, so the wait is
// free, and it clears the compiler's view of the stage's weight DMAs as pending LGKM events --
// otherwise the next stage's first MFMA waits lgkmcnt(0) for all of its operand reads instead
// of the counted lgkmcnt(N) for the first few (the waitcnt pass treats global_load_lds as an
// out-of-order LGKM event)
#define X6_WAITCNT_VM_LGKM0(n) \
  __builtin_amdgcn_s_waitcnt(((n) & 0xF) | (((n) >> 4) << 14) | (0x7 << 4))

__device__ __forceinline__ void x6_barrier() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // no compiler motion of LDS accesses across it
  __builtin_amdgcn_s_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// Where a workgroup's tile lies: first output row / column (ty0, tx0) of image n in the
// XCD-aware tile order (conv_epi.h xcd_tile), first input row / column with the halo (iy0, ix0),
// the image's input view and the packed weight image (ZBLOCK: that of output-channel block
// blockIdx.z; false for a kernel that has no blocks).
struct X6Tile {
  int ty0, tx0, n, iy0, ix0;
  const float* inb;
  const __bf16* wimg;
};
template <class C, bool ZBLOCK>
__device__ __forceinline__ X6Tile x6_tile(const FwdArgs& a) {
  const int tiles_x = (a.OW + C::TW - 1) / C::TW;
  int bxr, byr;
  xcd_tile(bxr, byr);
  X6Tile t;
  t.ty0 = (bxr / tiles_x) * C::TH;
  t.tx0 = (bxr % tiles_x) * C::TW;
  t.n = byr;
  t.iy0 = t.ty0 - 1;
  t.ix0 = t.tx0 - 1;
  t.inb = a.in + (long)t.n * a.IHt * a.IWt * a.in_stride + a.in_off;
  t.wimg = reinterpret_cast<const __bf16*>(a.wp);
  if constexpr (ZBLOCK) t.wimg += (long)blockIdx.z * a.wp_z;
  return t;
}

// The tile's input rows [ry0, ry1) through a 32-bit buffer resource based at row ry0, so its
// byte extent and offsets stay below 2^31 for any image height (the launchers check
// C::IH * IWt * in_stride * 4 < 2^31); 0x7fffffff is then always out of range.
struct X6XRows {
  __amdgpu_buffer_rsrc_t rs;
  int ry0;
};
template <class C>
__device__ __forceinline__ X6XRows x6_x_rows(const FwdArgs& a, const X6Tile& tl) {
  const int ry0 = tl.iy0 > 0 ? tl.iy0 : 0, ry1 = tl.iy0 + C::IH < a.IHt ? tl.iy0 + C::IH : a.IHt;
  const long row_floats = (long)a.IWt * a.in_stride;
  return {__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(tl.inb + ry0 * row_floats), (short)0,
                                            (int)((ry1 - ry0) * row_floats * 4), 0x00020000),
          ry0};
}

// Channels [k0, k0 + 32) of the x tile (halo included) into registers: exactly C::XITEMS buffer
// loads per thread (items outside the tile or the image get an out-of-range offset, for which
// the buffer unit returns zeros), so the callers' vmcnt counts are compile-time constants.
template <class C>
__device__ __forceinline__ void x6_load_x(const FwdArgs& a, const X6Tile& tl, const X6XRows& xs,
                                          int tid, int k0, f32x4 (&xr)[C::XITEMS]) {
#pragma unroll
  for (int it = 0; it < C::XITEMS; ++it) {
    const int e = tid + it * C::WAVES * 64;
    const int q = e % (C::KC / 4), pix = e / (C::KC / 4);
    const int iy = pix / C::IW, ix = pix - iy * C::IW;
    const int gy = tl.iy0 + iy, gx = tl.ix0 + ix, k = k0 + 4 * q;
    const bool ok = e < C::XQ && gy >= 0 && gy < a.IHt && gx >= 0 && gx < a.IWt && k < a.K;
    const int off = ok ? (((gy - xs.ry0) * a.IWt + gx) * a.in_stride + k) * 4 : 0x7fffffff;
    xr[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs.rs, off, 0, 0));
  }
}

// The registers of x6_load_x split into the three bf16 planes of the x tile in LDS (rows of 32
// bf16 per pixel, quads swizzled by x6_swz)
template <class C>
__device__ __forceinline__ void x6_store_x(__bf16* lx, int tid, const f32x4 (&xr)[C::XITEMS]) {
#pragma unroll
  for (int it = 0; it < C::XITEMS; ++it) {
    const int e = tid + it * C::WAVES * 64;
    if (e < C::XQ) {
      const int q = e % (C::KC / 4), pix = e / (C::KC / 4);
      const float f[4] = {xr[it][0], xr[it][1], xr[it][2], xr[it][3]};
      bf16x4 h, m, l;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        __bf16 hj, mj, lj;
        split3(f[j], hj, mj, lj);
        h[j] = hj; m[j] = mj; l[j] = lj;
      }
      const int off = pix * C::KC + x6_swz(pix, q >> 1) * 8 + (q & 1) * 4;
      *reinterpret_cast<bf16x4*>(lx + off) = h;
      *reinterpret_cast<bf16x4*>(lx + C::XPL + off) = m;
      *reinterpret_cast<bf16x4*>(lx + 2 * C::XPL + off) = l;
    }
  }
}

}  // namespace dn
