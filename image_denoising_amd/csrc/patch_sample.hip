// Device-resident paired patch sampler: the loader of finetune.py:100-150 (DenoisePatchDataset:
// one random ps x ps crop of a clean / noisy image pair per item, / 255) as one gather launch
// over image pools that live in HBM.  DESIGN.md §19.
//
//   k_patch_sample   out[i, c, y, x] = pool[off_m + c*h*w + (top_i + y)*w + left_i + x] / 255.0f
//                    for item i of image m = img_idx[i]; the same window for the clean and the
//                    noisy pool.  (top, left) come from origins_in (parity mode, as rd_idx) or
//                    from Philox keyed on the item's global ordinal g = item_base + i:
//                      top  = (u32(seed, offset, 2g)     * (h - ps + 1)) >> 32
//                      left = (u32(seed, offset, 2g + 1) * (w - ps + 1)) >> 32
//                    Multiply-shift maps the 32-bit word onto [0, range) without a rejection
//                    step: every value gets floor or ceil of 2^32 / range words, so its
//                    probability is off from 1 / range by at most 1 / 2^32 (a relative bias of
//                    at most range / 2^32, 1.6e-7 for a 704-pixel range).  The key is the global
//                    ordinal, so a rank's shard is its slice of the single-process batch.
//
// Bandwidth-bound: 4 bytes read and 4 written per output element and pool.  A lane owns four
// consecutive elements of the flat output (one 16-byte store; the outputs are 16-byte aligned and
// a quad starts at a multiple of four elements).  Where the four lie in one patch row -- always
// when ps % 4 == 0 -- the lane decodes one position and issues four dword loads; the source row
// starts at an arbitrary `left`, so nothing wider is aligned, and a wave's loads cover one
// contiguous run of each source row.  A quad that crosses a row, a channel or an item (ps % 4
// != 0) decodes each element; the last total % 4 elements are stored one by one.
//
// The kernel never reads outside an image: an item whose img_idx is outside [0, M), whose table
// row does not lie inside the pool, whose image is smaller than ps, or whose explicit origin is
// outside [0, h - ps] x [0, w - ps] gets zeros and the origin (-1, -1).  All offsets are 64-bit.
#include "dn_internal.h"
#include "philox.h"

namespace dn {

namespace {

struct PatchArgs {
  const float* clean_pool;
  const float* noisy_pool;  // nullable: clean-only set
  long pool_elems;          // floats in each pool
  const long* table;        // [M][3]: element offset, h, w
  int M, C;
  const int* img_idx;  // [N]
  long N;
  int ps;
  unsigned long long seed, offset, item_base;
  const int* origins_in;  // nullable [N][2]
  float* clean_out;
  float* noisy_out;
  int* origins_out;  // nullable [N][2]
};

struct PatchItem {
  long base;   // pool offset of the window's first pixel in channel 0
  long plane;  // h * w
  int w;
  int top, left;  // (-1, -1): invalid item, zeros
};

__device__ __forceinline__ PatchItem patch_item(const PatchArgs& p, long i) {
  PatchItem it;
  it.base = 0; it.plane = 0; it.w = 0; it.top = -1; it.left = -1;
  const int m = p.img_idx[i];
  if (m < 0 || m >= p.M) return it;
  const long off = p.table[3 * (long)m], h = p.table[3 * (long)m + 1], w = p.table[3 * (long)m + 2];
  if (off < 0 || h < p.ps || w < p.ps || h > 0x7fffffffL || w > 0x7fffffffL) return it;
  if (h * w > (p.pool_elems - off) / p.C) return it;  // the image lies inside the pool
  long top, left;
  if (p.origins_in) {
    top = p.origins_in[2 * i];
    left = p.origins_in[2 * i + 1];
    if (top < 0 || left < 0 || top > h - p.ps || left > w - p.ps) return it;
  } else {
    // words 2g and 2g + 1 share Philox block g >> 1
    const unsigned long long g = p.item_base + (unsigned long long)i;
    const unsigned long long blk = g >> 1;
    const U32x4 o = philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)p.offset,
                                  (uint32_t)(p.offset >> 32), (uint32_t)p.seed,
                                  (uint32_t)(p.seed >> 32));
    const int k = (int)(g & 1) * 2;
    top = (long)(((unsigned long long)o.v[k] * (unsigned long long)(h - p.ps + 1)) >> 32);
    left = (long)(((unsigned long long)o.v[k + 1] * (unsigned long long)(w - p.ps + 1)) >> 32);
  }
  it.base = off + top * w + left;
  it.plane = h * w;
  it.w = (int)w;
  it.top = (int)top;
  it.left = (int)left;
  return it;
}

// flat element e -> (item, r = offset inside the item's [C, ps, ps] patch)
__device__ __forceinline__ void split_elem(long e, int per, long& i, int& r) {
  i = e / per;
  r = (int)(e - i * per);
}

__global__ __launch_bounds__(256) void k_patch_sample(const PatchArgs p) {
  const int ps = p.ps, pp = ps * ps, per = p.C * pp;
  const long total = p.N * per, nq = (total + 3) >> 2;
  const bool pair = p.noisy_pool != nullptr;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long e0 = q << 2;
    const int n = total - e0 < 4 ? (int)(total - e0) : 4;
    float cv[4] = {0.f, 0.f, 0.f, 0.f}, nv[4] = {0.f, 0.f, 0.f, 0.f};
    long i;
    int r;
    split_elem(e0, per, i, r);
    const int c = r / pp, r2 = r - c * pp, y = r2 / ps, x = r2 - y * ps;
    if (x + n <= ps) {  // the quad lies in one patch row
      const PatchItem it = patch_item(p, i);
      if (it.top >= 0) {
        const long s = it.base + c * it.plane + (long)y * it.w + x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) {
            cv[k] = p.clean_pool[s + k] / 255.0f;
            if (pair) nv[k] = p.noisy_pool[s + k] / 255.0f;
          }
      }
      if (r == 0 && p.origins_out) {
        p.origins_out[2 * i] = it.top;
        p.origins_out[2 * i + 1] = it.left;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
          long ik;
          int rk;
          split_elem(e0 + k, per, ik, rk);
          const int ck = rk / pp, rk2 = rk - ck * pp, yk = rk2 / ps, xk = rk2 - yk * ps;
          const PatchItem it = patch_item(p, ik);
          if (it.top >= 0) {
            const long s = it.base + ck * it.plane + (long)yk * it.w + xk;
            cv[k] = p.clean_pool[s] / 255.0f;
            if (pair) nv[k] = p.noisy_pool[s] / 255.0f;
          }
          if (rk == 0 && p.origins_out) {
            p.origins_out[2 * ik] = it.top;
            p.origins_out[2 * ik + 1] = it.left;
          }
        }
    }
    if (n == 4) {
      *reinterpret_cast<float4*>(p.clean_out + e0) = make_float4(cv[0], cv[1], cv[2], cv[3]);
      if (pair) *reinterpret_cast<float4*>(p.noisy_out + e0) = make_float4(nv[0], nv[1], nv[2], nv[3]);
    } else {
      for (int k = 0; k < n; ++k) {
        p.clean_out[e0 + k] = cv[k];
        if (pair) p.noisy_out[e0 + k] = nv[k];
      }
    }
  }
}

}  // namespace

hipError_t launch_patch_sample(const float* clean_pool, const float* noisy_pool, long pool_elems,
                               const long* table, int M, int C, const int* img_idx, int N, int ps,
                               unsigned long long seed, unsigned long long offset,
                               unsigned long long item_base, const int* origins_in,
                               float* clean_out, float* noisy_out, int* origins_out,
                               hipStream_t s) {
  PatchArgs p;
  p.clean_pool = clean_pool; p.noisy_pool = noisy_pool; p.pool_elems = pool_elems;
  p.table = table; p.M = M; p.C = C; p.img_idx = img_idx; p.N = N; p.ps = ps;
  p.seed = seed; p.offset = offset; p.item_base = item_base; p.origins_in = origins_in;
  p.clean_out = clean_out; p.noisy_out = noisy_out; p.origins_out = origins_out;
  const long nq = ((long)N * C * ps * ps + 3) / 4;
  const long nb = (nq + 255) / 256;
  hipLaunchKernelGGL(k_patch_sample, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace dn
