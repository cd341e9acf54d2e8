// L1FFT (util.py:5-38 of the reference): alpha * L1(pred, target) + beta * mean|fft2(pred) -
// fft2(target)|, loss and gradient, by three passes over the real difference D = pred - target:
//
//   k_l1fft_rows_fwd   D formed on load, real -> half-spectrum FFT along W (two real rows ride one
//                      complex transform), H x (W/2+1) complex rows to the workspace, sum|D| partials
//   k_l1fft_cols       per tile of adjacent spectrum columns: FFT along H in LDS, weighted sum|F|
//                      partial, U = F / |F| (0 at |F| = 0) in place, inverse FFT along H, back to
//                      the workspace -- the full spectrum never reaches HBM
//   k_l1fft_rows_inv   half-spectrum -> real inverse along W, dpred = ga * sgn(D) + gb * result
//   k_l1fft_finalize   the sum of the per-block fp64 partials -> loss3
//
// A transform length is L = m P with m odd, 1 <= m <= 31, and P = 2^k >= 8 (L <= 1024): one
// Cooley-Tukey split in front of a radix-2 network.  With input index n = P n1 + n2 and output
// bin k = k1 + m k2 the forward is (a) the m-point DFT over n1 of the rows n1 P + n2, times the
// twiddle exp(-2 pi i n2 k1 / L), to row k1 P + n2, then (b) radix-2 decimation in frequency
// inside every aligned block of P rows, which leaves bin k at row
//     pos(k) = (k mod m) P + brev_P(k div m).
// The inverse is the transpose: radix-2 decimation in time per block (bins at pos(k) in), the
// conjugate twiddles, the unnormalised inverse m-point DFT, natural order out.  m = 1 skips (a)
// and is the plain radix-2 transform.  The column pass applies |F| and F / |F| pointwise and
// needs no reordering at all; the row passes place bins by pos(k) while they unpack / pack the
// row pair.
//
// The LDS tile's fastest index is the batch lane (a spectrum column / a row pair), so the 32 lanes
// of an LDS lane group read one contiguous 256-byte bank row at every butterfly stride.
// Twiddles are one table tw[j] = exp(-2 pi i j / L), j < L: sincospi in fp64, rounded once to
// fp32, per block in LDS.  The radix-2 stages read it at multiples of m, the odd stage's twiddle
// is tw[n2 k1] (n2 k1 < L) and its m-point DFT matrix tw[(n1 k1 mod m) P].
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "dn_internal.h"

namespace dn {
namespace {

constexpr int kFftTile = 4096;      // complex elements of a tile: batch lanes x transform length
constexpr int kFftLds = 5120;       // ... plus the row passes' one-lane row padding (L = 1024)
constexpr int kFftMaxL = 1024;
constexpr int kFftMaxOdd = 31;      // the odd factor m of L

// One LDS tile of TC batch lanes x L points: element (h, c) at s[slot(h) * pitch + c].
// TC = the largest power of two <= min(32, kFftTile / L).  With TC < 32 an LDS lane group of 32
// holds G = 32 / TC butterflies whose rows must fall on different 1/G-ths of the 64 banks: slot()
// mirrors the low bits of every odd aligned block of G rows, after which the rows a group touches
// at any stage (r .. r+G-1 for half-size >= G, every pair inside one aligned 2G block below)
// take G distinct values mod G.  slot() permutes rows inside aligned blocks of 2G rows, and 2G
// divides P (so every accepted L, and every block of P rows) wherever G > 1: G > 1 means L > 128,
// which with m <= 31 forces P >= 8 = 2G at G <= 4, and G = 8 means L > 512, which forces P >= 32.
// The row passes pad the pitch by one lane so that their transposed fill (consecutive lanes =
// consecutive h) is conflict-free as well.
struct FftTile {
  int L, mo, P, logP, TC, logTC, pitch, g, gm;  // L = mo * P, mo odd, P = 1 << logP
};

FftTile fft_tile_for(int L, int pad) {
  FftTile t{};
  t.L = L;
  while (((L >> t.logP) & 1) == 0) ++t.logP;
  t.P = 1 << t.logP;
  t.mo = L >> t.logP;
  t.TC = 32;
  while (t.TC * L > kFftTile) t.TC >>= 1;
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

// the row of bin k after the forward transform (and where the inverse expects it)
__device__ __forceinline__ int fft_pos(int k, const FftTile& t) {
  const int k2 = k / t.mo, k1 = k - k2 * t.mo;
  return (k1 << t.logP) + (int)(__brev((unsigned)k2) >> (32 - t.logP));
}

// tw[j] = exp(-2 pi i j / L), j < L
__device__ __forceinline__ void fft_twiddles(float2* tw, int L) {
  for (int k = threadIdx.x; k < L; k += 256) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)L, &sn, &cs);
    tw[k] = make_float2((float)cs, (float)sn);
  }
}

// The odd stage: thread = (n2 < P, batch lane c), its M points rows j P + n2 in registers.
// The M-point DFT is direct, in its real-symmetric form: with a_j = x_j + x_{M-j},
// b_j = x_j - x_{M-j}, c = cos(2 pi j k / M), s = sin(2 pi j k / M) for j, k = 1 .. (M-1)/2,
//     y_k, y_{M-k} = x_0 + sum_j a_j c  -/+  i sum_j b_j s        (+/- for the inverse)
// which is (M-1)^2 real multiply-adds instead of 4 M^2.  The loop over j is unrolled over the
// compile-time M, so x, a, b are registers at constant indices; the loop over k is a real loop,
// and cos, sin of (j k mod M) come from the table row r P = (cos, -sin)(2 pi r / M), r stepped
// by k mod M: one address per wave, an LDS broadcast.  No array is indexed dynamically.
// Forward: y_k times tw[n2 k] to row k P + n2.  Inverse: x_k = row k P + n2 times conj tw[n2 k]
// on load.  A thread reads and writes the same M elements: no barrier inside the stage.
// LDS banks (derived by the 64-bank rule, not measured): a 32-lane group covers G consecutive n2
// of TC lanes each, which slot() keeps inside one aligned block of G rows; in the column pass
// (pitch TC) these are 256 contiguous bytes, conflict-free for loads and stores; in the row
// passes (pitch TC + 1) each row is shifted by two banks, so at G > 1 the last 2 (G - 1) banks of
// the group wrap onto its first: up to G - 1 lanes two-way, conflict-free at TC = 32.  The
// twiddle loads tw[n2 k] are G distinct addresses per group (one, broadcast, at TC = 32) at
// banks (2 n2 k) mod 64: two of them meet only where k times their distance < G is a multiple
// of 32, that is k = 16 at G >= 4 and k = 8, 24 at G = 8 (two-way; k = 16 at G = 8 four-way),
// conflict-free for every other k.  The DFT-matrix loads are one address per wave (broadcast).
template <int M, bool INV>
__device__ __forceinline__ void fft_odd_m(float2* s, const float2* tw, const FftTile& t) {
  constexpr int Hf = (M - 1) / 2;
  const int ng = t.P << t.logTC;
  for (int b = threadIdx.x; b < ng; b += 256) {
    const int c = b & (t.TC - 1), n2 = b >> t.logTC;
    float2 x[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      x[j] = s[fft_slot((j << t.logP) + n2, t) * t.pitch + c];
      if (INV && j > 0) {  // times conj tw[n2 j]
        const float2 w = tw[n2 * j], v = x[j];
        x[j] = make_float2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y);
      }
    }
    float2 y0 = x[0];
#pragma unroll
    for (int j = 1; j <= Hf; ++j) {
      const float2 p = x[j], q = x[M - j];
      x[j] = make_float2(p.x + q.x, p.y + q.y);      // a_j
      x[M - j] = make_float2(p.x - q.x, p.y - q.y);  // b_j
      y0.x += x[j].x;
      y0.y += x[j].y;
    }
    s[fft_slot(n2, t) * t.pitch + c] = y0;
#pragma unroll 1
    for (int k = 1; k <= Hf; ++k) {
      float2 A = x[0], B = make_float2(0.f, 0.f);
      int r = 0;
#pragma unroll
      for (int j = 1; j <= Hf; ++j) {
        r += k;
        r -= r >= M ? M : 0;  // j k mod M
        const float2 w = tw[r << t.logP];
        A.x += x[j].x * w.x;
        A.y += x[j].y * w.x;
        B.x -= x[M - j].x * w.y;
        B.y -= x[M - j].y * w.y;
      }
      // forward: y_k = A - i B, y_{M-k} = A + i B; inverse: the other way round
      float2 yk = INV ? make_float2(A.x - B.y, A.y + B.x) : make_float2(A.x + B.y, A.y - B.x);
      float2 ym = INV ? make_float2(A.x + B.y, A.y - B.x) : make_float2(A.x - B.y, A.y + B.x);
      if (!INV) {  // times tw[n2 k], tw[n2 (M - k)]
        const float2 w = tw[n2 * k], u = tw[n2 * (M - k)];
        yk = make_float2(yk.x * w.x - yk.y * w.y, yk.x * w.y + yk.y * w.x);
        ym = make_float2(ym.x * u.x - ym.y * u.y, ym.x * u.y + ym.y * u.x);
      }
      s[fft_slot((k << t.logP) + n2, t) * t.pitch + c] = yk;
      s[fft_slot(((M - k) << t.logP) + n2, t) * t.pitch + c] = ym;
    }
  }
}

template <bool INV>
__device__ __forceinline__ void fft_odd(float2* s, const float2* tw, const FftTile& t) {
  switch (t.mo) {  // uniform over the grid
#define DN_FFT_ODD(M) case M: fft_odd_m<M, INV>(s, tw, t); break;
    DN_FFT_ODD(3) DN_FFT_ODD(5) DN_FFT_ODD(7) DN_FFT_ODD(9) DN_FFT_ODD(11) DN_FFT_ODD(13)
    DN_FFT_ODD(15) DN_FFT_ODD(17) DN_FFT_ODD(19) DN_FFT_ODD(21) DN_FFT_ODD(23) DN_FFT_ODD(25)
    DN_FFT_ODD(27) DN_FFT_ODD(29) DN_FFT_ODD(31)
#undef DN_FFT_ODD
    default: break;  // m = 1
  }
}

// INV = false: forward (odd stage, then DIF per block of P rows), X[k] left at row pos(k).
// INV = true: unnormalised inverse (DIT per block, then the odd stage) of a spectrum stored at
// pos(k), natural order out.  The radix-2 butterflies of half-size < P stay inside aligned blocks
// of P rows, so one index space j < L / 2 serves the m blocks at once.  The caller synchronises
// before the call; the tile is synchronised on return.
template <bool INV>
__device__ __forceinline__ void fft_run(float2* s, const float2* tw, const FftTile& t) {
  if (!INV && t.mo > 1) {
    fft_odd<false>(s, tw, t);
    __syncthreads();
  }
  const int nb = (t.L >> 1) << t.logTC;
  for (int st = 0; st < t.logP; ++st) {
    const int lm = INV ? st : t.logP - 1 - st;
    const int hs = 1 << lm;
    for (int b = threadIdx.x; b < nb; b += 256) {
      const int c = b & (t.TC - 1), j = b >> t.logTC;
      const int i = j & (hs - 1);
      const int r0 = ((j >> lm) << (lm + 1)) + i;
      float2* p0 = s + fft_slot(r0, t) * t.pitch + c;
      float2* p1 = s + fft_slot(r0 + hs, t) * t.pitch + c;
      const float2 w = tw[(i << (t.logP - 1 - lm)) * t.mo];
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
  if (INV && t.mo > 1) {
    fft_odd<true>(s, tw, t);
    __syncthreads();
  }
}

// The block partials go through block_sum_store (block_reduce.h).  The transform kernels lend it
// their twiddle table, dead by then, as its four doubles of LDS: that keeps the column pass at
// 40 KiB, four workgroups per CU.

// Row pair rp = rows 2rp, 2rp+1 of the flattened [N*C*H][W] image (H is even, so a pair never
// straddles two planes).  z = rowA + i rowB; with Z = FFT(z): FA[k] = (Z[k] + conj Z[W-k]) / 2,
// FB[k] = (Z[k] - conj Z[W-k]) / 2i.
__global__ __launch_bounds__(256) void k_l1fft_rows_fwd(const float* __restrict__ pred,
                                                        const float* __restrict__ tgt, long R,
                                                        int W, FftTile t,
                                                        float2* __restrict__ spec,
                                                        double* __restrict__ partials) {
  __shared__ float2 s[kFftLds];
  __shared__ float2 tw[kFftMaxL];
  const int Wh = W / 2 + 1;
  const long rp0 = (long)blockIdx.x * t.TC;
  fft_twiddles(tw, W);
  double acc = 0.0;
  const int n = t.TC * t.L;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int p = idx / W, w = idx - p * W;
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
    const float2 z1 = s[fft_slot(fft_pos(k, t), t) * t.pitch + p];
    const float2 z2 = s[fft_slot(fft_pos(k ? W - k : 0, t), t) * t.pitch + p];
    spec[(2 * rp) * Wh + k] = make_float2(0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y));
    spec[(2 * rp + 1) * Wh + k] = make_float2(0.5f * (z1.y + z2.y), 0.5f * (z2.x - z1.x));
  }
  block_sum_store(acc, partials + blockIdx.x, reinterpret_cast<double*>(tw));
}

// Block = (plane, tile of TC adjacent half-spectrum columns); the last tile of a plane is ragged
// (W/2+1 is odd) and its missing columns are zeros, which normalise to zeros.  Column k of the
// half spectrum stands for columns k and W-k of the full one: weight 2, but 1 for k = 0 and W/2.
// waves_per_eu(4, 4): 40 KiB of LDS fit four workgroups per CU, and the odd stage (m = 31: 62
// registers of points) stays inside the 128 registers that allows without scratch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_l1fft_cols(float2* __restrict__ spec, int H, int W,
                                                    int ntile, FftTile t,
                                                    double* __restrict__ partials) {
  __shared__ float2 s[kFftTile];
  __shared__ float2 tw[kFftMaxL];
  const int Wh = W / 2 + 1;
  const int plane = blockIdx.x / ntile, tile = blockIdx.x - plane * ntile;
  const int k0 = tile * t.TC;
  float2* base = spec + (long)plane * H * Wh;
  fft_twiddles(tw, H);
  const int n = t.TC * t.L;
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
  block_sum_store(acc, partials + blockIdx.x, reinterpret_cast<double*>(tw));
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
  __shared__ float2 tw[kFftMaxL];
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
    s[fft_slot(fft_pos(k, t), t) * t.pitch + p] = make_float2(a.x - b.y, a.y + b.x);
    if (k > 0 && k < W / 2)
      s[fft_slot(fft_pos(W - k, t), t) * t.pitch + p] = make_float2(a.x + b.y, b.x - a.y);
  }
  __syncthreads();
  fft_run<true>(s, tw, t);
  const int n = t.TC * t.L;
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    const int p = idx / W, w = idx - p * W;
    const long rp = rp0 + p;
    if (rp >= R) break;
    const float2 z = s[fft_slot(w, t) * t.pitch + p];
    const long e = 2 * rp * W + w;
    dpred[e] = ga * sgn(pred[e] - tgt[e]) + gb * z.x;
    dpred[e + W] = ga * sgn(pred[e + W] - tgt[e + W]) + gb * z.y;
  }
}

// beta == 0: no transform; dpred = ga * sgn(D) exactly as the pixel term of the other losses
__global__ __launch_bounds__(256) void k_l1fft_pixel(const float* __restrict__ pred,
                                                     const float* __restrict__ tgt, long total,
                                                     float ga, float* __restrict__ dpred,
                                                     double* __restrict__ partials) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const float d = pred[e] - tgt[e];
    acc += fabs((double)d);
    dpred[e] = ga * sgn(d);
  }
  block_sum_store(acc, partials + blockIdx.x, red);
}

// v[0] over the first n0 partials (sum|D|), v[1] over the next n1 (weighted sum|F|).  The two
// segments differ in length, so the gather (thread t adds blocks t, t + 256, ... in order) is
// written out here in place of sum_partials; the tree is the shared one.
__global__ __launch_bounds__(256) void k_l1fft_finalize(const double* __restrict__ partials,
                                                        long n0, long n1, double denom,
                                                        float alpha, float beta,
                                                        float* __restrict__ loss3) {
  __shared__ double sh[2][256];
  double v[2] = {0.0, 0.0};
  for (long b = threadIdx.x; b < n0; b += 256) v[0] += partials[b];
  for (long b = threadIdx.x; b < n1; b += 256) v[1] += partials[n0 + b];
  block_tree_sum(v, sh);
  if (threadIdx.x != 0) return;
  const float pix = (float)(v[0] / denom), frq = (float)(v[1] / denom);
  loss3[0] = pix;
  loss3[1] = frq;
  loss3[2] = alpha * pix + beta * frq;
}

// L = m 2^k with m odd, m <= 31, k >= 3, L <= 1024
bool l1fft_len_ok(int v) {
  if (v < 8 || v > kFftMaxL || (v & 7) != 0) return false;
  while ((v & 1) == 0) v >>= 1;
  return v <= kFftMaxOdd;
}

struct L1fftPlan {
  FftTile rows, cols;
  long R, nblk_rows, nblk_cols;
  int ntile;
  size_t spec_bytes, total_bytes;
};

bool l1fft_plan(int N, int C, int H, int W, L1fftPlan& p) {
  if (N < 1 || C < 1 || !l1fft_len_ok(H) || !l1fft_len_ok(W)) return false;
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
  const long nparts = p.nblk_rows + p.nblk_cols > kLossBlocks ? p.nblk_rows + p.nblk_cols : kLossBlocks;
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
    hipLaunchKernelGGL(k_l1fft_pixel, dim3(kLossBlocks), dim3(256), 0, s, pred, tgt,
                       (long)N * C * H * W, ga, dpred, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_l1fft_finalize, dim3(1), dim3(256), 0, s, part, (long)kLossBlocks, 0L,
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
