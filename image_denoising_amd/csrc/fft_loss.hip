// L1FFT (util.py:5-38 of the reference): alpha * L1(pred, target) + beta * mean|fft2(pred) -
// fft2(target)|, loss and gradient, by three passes over the real difference D = pred - target:
//
//   k_l1fft_rows_fwd   D formed on load, real -> half-spectrum FFT along W (two real rows ride one
//                      complex transform), H x (W/2+1) complex rows to the workspace, sum|D| partials
//   k_l1fft_cols       per tile of adjacent spectrum columns: FFT along H in LDS, weighted sum|F|
//                      partial, U = F / |F| (0 at |F| = 0) in place, inverse FFT along H, back to
//                      the workspace -- the full spectrum never reaches HBM
//   k_l1fft_rows_inv   half-spectrum -> real inverse along W, dpred = ga * sgn(D) + gb * result
//   k_l1fft_finalize   fixed-order sum of the per-block fp64 partials -> loss3
//
// Every transform is radix-2 over an LDS tile whose fastest index is the batch lane (a spectrum
// column / a row pair), so the 32 lanes of an LDS lane group read one contiguous 256-byte bank
// row at every butterfly stride.  The forward is decimation in frequency (natural in, bit-reversed
// out) and the inverse decimation in time (bit-reversed in, natural out): the column pass needs
// no reordering at all, the row passes reverse bits while they unpack / pack the row pair.
// Twiddles are sincospi in fp64, rounded once to fp32, per block in LDS.
#include <hip/hip_runtime.h>

#include "dn_internal.h"

namespace dn {
namespace {

constexpr int kFftTile = 4096;      // complex elements of a tile: batch lanes x transform length
constexpr int kFftLds = 5120;       // ... plus the row passes' one-lane row padding (L = 1024)
constexpr int kFftMaxL = 1024;

// One LDS tile of TC batch lanes x L points: element (h, c) at s[slot(h) * pitch + c].
// TC = min(32, kFftTile / L).  With TC < 32 an LDS lane group of 32 holds G = 32 / TC butterflies
// whose rows must fall on different 1/G-ths of the 64 banks: slot() mirrors the low bits of every
// odd aligned block of G rows, after which the rows a group touches at any stage (r .. r+G-1 for
// half-size m >= G, every 2m-th pair inside one aligned 2G block below) take G distinct values
// mod G.  The row passes pad the pitch by one lane so that their transposed fill (consecutive
// lanes = consecutive h) is conflict-free as well.
struct FftTile {
  int L, logL, TC, logTC, pitch, g, gm;
};

FftTile fft_tile_for(int L, int pad) {
  FftTile t{};
  t.L = L;
  while ((1 << t.logL) < L) ++t.logL;
  t.TC = kFftTile / L < 32 ? kFftTile / L : 32;
  while ((1 << t.logTC) < t.TC) ++t.logTC;
  t.pitch = t.TC + pad;
  const int G = 32 / t.TC;
  while ((1 << t.g) < G) ++t.g;
  t.gm = G - 1;
  return t;
}

__device__ __forceinline__ int fft_slot(int h, const FftTile& t) {
  return h ^ (((h >> t.g) & 1) * t.gm);
}

__device__ __forceinline__ int fft_brev(int k, int logL) {
  return (int)(__brev((unsigned)k) >> (32 - logL));
}

// tw[k] = exp(-2 pi i k / L), k < L / 2 (2k / L is exact: L is a power of two)
__device__ __forceinline__ void fft_twiddles(float2* tw, int L) {
  for (int k = threadIdx.x; k < L / 2; k += 256) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)L, &sn, &cs);
    tw[k] = make_float2((float)cs, (float)sn);
  }
}

// INV = false: forward DIF, X[k] left at point brev(k).  INV = true: unnormalised inverse DIT of
// a spectrum stored at brev(k), natural order out.  The caller synchronises before the call; the
// tile is synchronised on return.
template <bool INV>
__device__ __forceinline__ void fft_run(float2* s, const float2* tw, const FftTile& t) {
  const int nb = (t.L >> 1) << t.logTC;
  for (int st = 0; st < t.logL; ++st) {
    const int lm = INV ? st : t.logL - 1 - st;
    const int m = 1 << lm;
    for (int b = threadIdx.x; b < nb; b += 256) {
      const int c = b & (t.TC - 1), j = b >> t.logTC;
      const int i = j & (m - 1);
      const int r0 = ((j >> lm) << (lm + 1)) + i;
      float2* p0 = s + fft_slot(r0, t) * t.pitch + c;
      float2* p1 = s + fft_slot(r0 + m, t) * t.pitch + c;
      const float2 w = tw[i << (t.logL - 1 - lm)];
      const float2 a = *p0, q = *p1;
      if (!INV) {
        const float dx = a.x - q.x, dy = a.y - q.y;
        *p0 = make_float2(a.x + q.x, a.y + q.y);
        *p1 = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
      } else {  // q * conj(w)
        const float bx = q.x * w.x + q.y * w.y, by = q.y * w.x - q.x * w.y;
        *p0 = make_float2(a.x + bx, a.y + by);
        *p1 = make_float2(a.x - bx, a.y - by);
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float l1fft_sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// the block's sum in a fixed order -> *out (one double per block)
__device__ __forceinline__ void l1fft_block_sum(double v, double* out) {
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((red[0] + red[1]) + red[2]) + red[3];
}

// Row pair rp = rows 2rp, 2rp+1 of the flattened [N*C*H][W] image (H is even, so a pair never
// straddles two planes).  z = rowA + i rowB; with Z = FFT(z): FA[k] = (Z[k] + conj Z[W-k]) / 2,
// FB[k] = (Z[k] - conj Z[W-k]) / 2i.
__global__ __launch_bounds__(256) void k_l1fft_rows_fwd(const float* __restrict__ pred,
                                                        const float* __restrict__ tgt, long R,
                                                        int W, FftTile t,
                                                        float2* __restrict__ spec,
                                                        double* __restrict__ partials) {
  __shared__ float2 s[kFftLds];
  __shared__ float2 tw[kFftMaxL / 2];
  const int Wh = W / 2 + 1;
  const long rp0 = (long)blockIdx.x * t.TC;
  fft_twiddles(tw, W);
  double acc = 0.0;
  const int n = t.TC << t.logL;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int w = idx & (W - 1), p = idx >> t.logL;
    const long rp = rp0 + p;
    float2 v = make_float2(0.f, 0.f);
    if (rp < R) {
      const long e = 2 * rp * W + w;
      v.x = pred[e] - tgt[e];
      v.y = pred[e + W] - tgt[e + W];
      acc += fabs((double)v.x) + fabs((double)v.y);
    }
    s[fft_slot(w, t) * t.pitch + p] = v;
  }
  __syncthreads();
  fft_run<false>(s, tw, t);
  const int nh = t.TC * Wh;
  for (int idx = threadIdx.x; idx < nh; idx += 256) {
    const int p = idx / Wh, k = idx - p * Wh;
    const long rp = rp0 + p;
    if (rp >= R) break;  // p grows with idx
    const float2 z1 = s[fft_slot(fft_brev(k, t.logL), t) * t.pitch + p];
    const float2 z2 = s[fft_slot(fft_brev((W - k) & (W - 1), t.logL), t) * t.pitch + p];
    spec[(2 * rp) * Wh + k] = make_float2(0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y));
    spec[(2 * rp + 1) * Wh + k] = make_float2(0.5f * (z1.y + z2.y), 0.5f * (z2.x - z1.x));
  }
  l1fft_block_sum(acc, partials + blockIdx.x);
}

// Block = (plane, tile of TC adjacent half-spectrum columns); the last tile of a plane is ragged
// (W/2+1 is odd) and its missing columns are zeros, which normalise to zeros.  Column k of the
// half spectrum stands for columns k and W-k of the full one: weight 2, but 1 for k = 0 and W/2.
__global__ __launch_bounds__(256) void k_l1fft_cols(float2* __restrict__ spec, int H, int W,
                                                    int ntile, FftTile t,
                                                    double* __restrict__ partials) {
  __shared__ float2 s[kFftTile];
  __shared__ float2 tw[kFftMaxL / 2];
  const int Wh = W / 2 + 1;
  const int plane = blockIdx.x / ntile, tile = blockIdx.x - plane * ntile;
  const int k0 = tile * t.TC;
  float2* base = spec + (long)plane * H * Wh;
  fft_twiddles(tw, H);
  const int n = t.TC << t.logL;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int c = idx & (t.TC - 1), h = idx >> t.logTC;
    const int k = k0 + c;
    s[fft_slot(h, t) * t.pitch + c] = k < Wh ? base[(long)h * Wh + k] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  fft_run<false>(s, tw, t);
  double acc = 0.0;
  for (int idx = threadIdx.x; idx < n; idx += 256) {  // pointwise: any order of the points
    const int k = k0 + (idx & (t.TC - 1));
    const float2 v = s[idx];
    const float mag = sqrtf(v.x * v.x + v.y * v.y);
    if (k < Wh) acc += (double)((k == 0 || k == W / 2) ? mag : 2.f * mag);
    s[idx] = mag > 0.f ? make_float2(v.x / mag, v.y / mag) : make_float2(0.f, 0.f);
  }
  __syncthreads();
  fft_run<true>(s, tw, t);
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int c = idx & (t.TC - 1), h = idx >> t.logTC;
    const int k = k0 + c;
    if (k < Wh) base[(long)h * Wh + k] = s[fft_slot(h, t) * t.pitch + c];
  }
  l1fft_block_sum(acc, partials + blockIdx.x);
}

// V (the column-inverse of U) is Hermitian along k in every row, so rows A and B of a pair come
// back from one complex inverse of Z[k] = VA[k] + i VB[k], Z[W-k] = conj VA[k] + i conj VB[k]:
// z = a + i b.  The imaginary parts of bins 0 and W/2 are rounding noise of a real value: dropped.
__global__ __launch_bounds__(256) void k_l1fft_rows_inv(const float2* __restrict__ spec,
                                                        const float* __restrict__ pred,
                                                        const float* __restrict__ tgt, long R,
                                                        int W, FftTile t, float ga, float gb,
                                                        float* __restrict__ dpred) {
  __shared__ float2 s[kFftLds];
  __shared__ float2 tw[kFftMaxL / 2];
  const int Wh = W / 2 + 1;
  const long rp0 = (long)blockIdx.x * t.TC;
  fft_twiddles(tw, W);
  const int nh = t.TC * Wh;
  for (int idx = threadIdx.x; idx < nh; idx += 256) {
    const int p = idx / Wh, k = idx - p * Wh;
    const long rp = rp0 + p;
    float2 a = make_float2(0.f, 0.f), b = a;
    if (rp < R) {
      a = spec[(2 * rp) * Wh + k];
      b = spec[(2 * rp + 1) * Wh + k];
    }
    if (k == 0 || k == W / 2) a.y = b.y = 0.f;
    s[fft_slot(fft_brev(k, t.logL), t) * t.pitch + p] = make_float2(a.x - b.y, a.y + b.x);
    if (k > 0 && k < W / 2)
      s[fft_slot(fft_brev(W - k, t.logL), t) * t.pitch + p] = make_float2(a.x + b.y, b.x - a.y);
  }
  __syncthreads();
  fft_run<true>(s, tw, t);
  const int n = t.TC << t.logL;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int w = idx & (W - 1), p = idx >> t.logL;
    const long rp = rp0 + p;
    if (rp >= R) break;
    const float2 z = s[fft_slot(w, t) * t.pitch + p];
    const long e = 2 * rp * W + w;
    dpred[e] = ga * l1fft_sgn(pred[e] - tgt[e]) + gb * z.x;
    dpred[e + W] = ga * l1fft_sgn(pred[e + W] - tgt[e + W]) + gb * z.y;
  }
}

// beta == 0: no transform; dpred = ga * sgn(D) exactly as the pixel term of the other losses
__global__ __launch_bounds__(256) void k_l1fft_pixel(const float* __restrict__ pred,
                                                     const float* __restrict__ tgt, long total,
                                                     float ga, float* __restrict__ dpred,
                                                     double* __restrict__ partials) {
  double acc = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const float d = pred[e] - tgt[e];
    acc += fabs((double)d);
    dpred[e] = ga * l1fft_sgn(d);
  }
  l1fft_block_sum(acc, partials + blockIdx.x);
}

// thread t adds blocks t, t + 256, ... in order, then a fixed tree: sums[0] over the first n0
// partials (sum|D|), sums[1] over the next n1 (weighted sum|F|)
__global__ __launch_bounds__(256) void k_l1fft_finalize(const double* __restrict__ partials,
                                                        long n0, long n1, double denom,
                                                        float alpha, float beta,
                                                        float* __restrict__ loss3) {
  __shared__ double sh[2][256];
  const int t = threadIdx.x;
  double v0 = 0.0, v1 = 0.0;
  for (long b = t; b < n0; b += 256) v0 += partials[b];
  for (long b = t; b < n1; b += 256) v1 += partials[n0 + b];
  sh[0][t] = v0;
  sh[1][t] = v1;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t != 0) return;
  const float pix = (float)(sh[0][0] / denom), frq = (float)(sh[1][0] / denom);
  loss3[0] = pix;
  loss3[1] = frq;
  loss3[2] = alpha * pix + beta * frq;
}

constexpr int kL1Blocks = 1024;  // the beta == 0 path's fixed grid

bool l1fft_pow2(int v) { return v >= 8 && v <= kFftMaxL && (v & (v - 1)) == 0; }

struct L1fftPlan {
  FftTile rows, cols;
  long R, nblk_rows, nblk_cols;
  int ntile;
  size_t spec_bytes, total_bytes;
};

bool l1fft_plan(int N, int C, int H, int W, L1fftPlan& p) {
  if (N < 1 || C < 1 || !l1fft_pow2(H) || !l1fft_pow2(W)) return false;
  const long planes = (long)N * C;
  p.rows = fft_tile_for(W, 1);
  p.cols = fft_tile_for(H, 0);
  p.R = planes * (H / 2);
  p.nblk_rows = (p.R + p.rows.TC - 1) / p.rows.TC;
  const int Wh = W / 2 + 1;
  p.ntile = (Wh + p.cols.TC - 1) / p.cols.TC;
  p.nblk_cols = planes * p.ntile;
  if (p.nblk_rows >= (1L << 31) || p.nblk_cols >= (1L << 31)) return false;
  p.spec_bytes = (size_t)planes * H * Wh * sizeof(float2);
  const long nparts = p.nblk_rows + p.nblk_cols > kL1Blocks ? p.nblk_rows + p.nblk_cols : kL1Blocks;
  p.total_bytes = p.spec_bytes + (size_t)nparts * sizeof(double);
  return true;
}

}  // namespace

size_t l1fft_ws_bytes(int N, int C, int H, int W) {
  L1fftPlan p;
  return l1fft_plan(N, C, H, W, p) ? p.total_bytes : 0;
}

hipError_t launch_l1fft_loss(const float* pred, const float* tgt, int N, int C, int H, int W,
                             float alpha, float beta, bool reduction_sum, float* dpred,
                             float* loss3, void* ws, hipStream_t s) {
  L1fftPlan p;
  if (!l1fft_plan(N, C, H, W, p)) return hipErrorInvalidValue;
  const double M = (double)N * C * H * W;
  const double denom = reduction_sum ? 1.0 : M;
  // d/dpred of alpha * mean|D| = alpha / M * sgn(D); of beta * mean|F| = beta / M * (the
  // unnormalised inverse of U = H W ifft2(U))
  const float ga = reduction_sum ? alpha : alpha / (float)M;
  const float gb = reduction_sum ? beta : beta / (float)M;
  float2* spec = static_cast<float2*>(ws);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + p.spec_bytes);
  hipError_t e;
  if (beta == 0.f) {
    hipLaunchKernelGGL(k_l1fft_pixel, dim3(kL1Blocks), dim3(256), 0, s, pred, tgt,
                       (long)N * C * H * W, ga, dpred, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_l1fft_finalize, dim3(1), dim3(256), 0, s, part, (long)kL1Blocks, 0L,
                       denom, alpha, beta, loss3);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_l1fft_rows_fwd, dim3((unsigned)p.nblk_rows), dim3(256), 0, s, pred, tgt,
                     p.R, W, p.rows, spec, part);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_l1fft_cols, dim3((unsigned)p.nblk_cols), dim3(256), 0, s, spec, H, W,
                     p.ntile, p.cols, part + p.nblk_rows);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_l1fft_rows_inv, dim3((unsigned)p.nblk_rows), dim3(256), 0, s, spec, pred,
                     tgt, p.R, W, p.rows, ga, gb, dpred);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_l1fft_finalize, dim3(1), dim3(256), 0, s, part, p.nblk_rows, p.nblk_cols,
                     denom, alpha, beta, loss3);
  return hipGetLastError();
}

}  // namespace dn
