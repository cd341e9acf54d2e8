// The fixed-order fp64 reduction of every loss and metric kernel, once.
// The block forms assume 256 threads = four 64-lane waves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dn {

// The fixed-grid losses (N2N, Structure, finetune, IQSL, L1FFT at beta == 0) launch kLossBlocks
// blocks.  Those that write the shared partials buffer (dn_loss_partials_size()) put block b's
// terms at partials[b * kLossStride + k]; a user asserts that its terms fit the stride.
constexpr int kLossBlocks = 1024;
constexpr int kLossStride = 4;
constexpr size_t kLossPartialsBytes = sizeof(double) * kLossBlocks * kLossStride;

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// xor butterfly over the 64 lanes: every lane ends with the wave's sum
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// dst[k] = the block's sum of v[k], the four waves added as ((w0 + w1) + w2) + w3.
// red: 4 * T doubles of LDS that no thread reads or writes any more.
template <int T>
__device__ __forceinline__ void block_sum_store(double (&v)[T], double* dst, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < T; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < T; ++k) red[wv * T + k] = v[k];
  __syncthreads();
  if (threadIdx.x < T) {
    const int k = threadIdx.x;
    dst[k] = ((red[k] + red[T + k]) + red[2 * T + k]) + red[3 * T + k];
  }
}

template <int T>
__device__ __forceinline__ void block_sum_store(double (&v)[T], double* dst) {
  __shared__ double red[4 * T];
  block_sum_store(v, dst, red);
}

__device__ __forceinline__ void block_sum_store(double v, double* dst, double* red) {
  double a[1] = {v};
  block_sum_store(a, dst, red);
}

// the same sum returned to all 256 threads; red: 4 doubles.  The leading barrier lets two calls
// share red back to back.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// v[k] = sum over the 256 threads of v[k] by a halving tree in LDS (thread t adds entry t + w for
// w = 128, 64, ..., 1), returned to all threads
template <typename V, int T>
__device__ __forceinline__ void block_tree_sum(V (&v)[T], V (*sh)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < T; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
#pragma unroll
      for (int k = 0; k < T; ++k) sh[k][t] += sh[k][t + w];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < T; ++k) v[k] = sh[k][0];
}

template <typename V>
__device__ __forceinline__ V block_tree_sum(V v, V* sh) {
  V a[1] = {v};
  block_tree_sum(a, reinterpret_cast<V(*)[256]>(sh));
  return a[0];
}

// out[k] = sum over b < nblk of partials[b * stride + k] by one 256-thread block: thread t adds
// blocks t, t + 256, ... in order, then the tree
template <int T>
__device__ __forceinline__ void sum_partials(const double* __restrict__ partials, int nblk,
                                             int stride, double (&out)[T]) {
  __shared__ double sh[T][256];
#pragma unroll
  for (int k = 0; k < T; ++k) out[k] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int k = 0; k < T; ++k) out[k] += partials[b * stride + k];
  block_tree_sum(out, sh);
}

}  // namespace dn
