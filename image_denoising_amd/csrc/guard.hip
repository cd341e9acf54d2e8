// The guarded optimizer step for gfx950 (train_opt.py:128-157): the fp64 norm of
// the flat gradient, the one-block decision (skip on loss, skip on norm, clip) that also keeps
// Adam's step count, and the Adam kernel that reads the decision from device memory.  Three
// launches on one stream; the host never reads any of it.
#include <math.h>
#include <cstdint>

#include "block_reduce.h"
#include "denoise_hip.h"
#include "dn_internal.h"

namespace dn {

// The caller-owned state: kLossBlocks fp64 partials, then the dn_guard_stats the host may read.
struct GuardState {
  double partials[kLossBlocks];
  dn_guard_stats st;
};
static_assert(sizeof(GuardState) == sizeof(double) * kLossBlocks + sizeof(dn_guard_stats), "");

size_t guard_state_bytes() { return sizeof(GuardState); }

// One pass of the full grid covers kLossBlocks * 256 * 4 elements.
constexpr int kQuad = 4;

int guard_norm_blocks(int64_t n) {
  const int64_t per_block = 256 * kQuad;
  int64_t b = (n + per_block - 1) / per_block;
  if (b > kLossBlocks) b = kLossBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ double sq_term(float g, float gscale) {
  const float x = gscale == 1.f ? g : g * gscale;  // k_adam's gg
  return (double)x * x;
}

// partials[b] = block b's sum of (double)x * x, x = g[i] (* gscale in fp32).  Thread t of block b
// takes the quads b * 256 + t, + gridDim.x * 256, ... and adds a quad's four terms in index order,
// so the float4 kernel (VEC, 16-byte aligned g) and its scalar twin form the same sum bit for
// bit.  Every index read is below n.
template <bool VEC>
__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, int64_t n,
                                                    float gscale, double* __restrict__ partials) {
  const long nq = (long)((n + kQuad - 1) / kQuad);
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long i = q * kQuad;
    if (i + kQuad <= n) {
      float4 v;
      if (VEC) {
        v = reinterpret_cast<const float4*>(g)[q];
      } else {
        v = make_float4(g[i], g[i + 1], g[i + 2], g[i + 3]);
      }
      acc += sq_term(v.x, gscale);
      acc += sq_term(v.y, gscale);
      acc += sq_term(v.z, gscale);
      acc += sq_term(v.w, gscale);
    } else {
      for (long j = i; j < n; ++j) acc += sq_term(g[j], gscale);
    }
  }
  __shared__ double red[4];
  block_sum_store(acc, partials + blockIdx.x, red);
}

// norm = sqrt(fixed-order sum of the partials): the reduction alone (dn_grad_norm)
__global__ __launch_bounds__(256) void k_guard_norm(GuardState* __restrict__ gs, int nblk,
                                                    double* __restrict__ norm_out) {
  double s[1];
  sum_partials(gs->partials, nblk, 1, s);
  if (threadIdx.x == 0) {
    const double norm = sqrt(s[0]);
    gs->st.last_norm = norm;
    if (norm_out) *norm_out = norm;
  }
}

__global__ void k_guard_init(GuardState* __restrict__ gs, int64_t step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dn_guard_stats z{};
    z.step = step;
    z.last_coef = 1.f;
    gs->st = z;
  }
}

// The decision, in train_opt.py's order: loss (:136), gradient norm (:149), clip (:155).
// max_loss / max_norm_skip / clip <= 0: that guard is off (the launcher maps NaN to 0).
__global__ __launch_bounds__(256) void k_guard_decide(GuardState* __restrict__ gs, int nblk,
                                                      const float* __restrict__ loss,
                                                      float max_loss, float max_norm_skip,
                                                      float clip, float gscale, double lr,
                                                      double b1, double b2) {
  double s[1];
  sum_partials(gs->partials, nblk, 1, s);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(s[0]);
  dn_guard_stats st = gs->st;
  st.last_norm = norm;
  st.last_loss = loss ? *loss : 0.f;
  const bool norm_bad = !isfinite(norm);
  if (loss && max_loss > 0.f &&
      (!isfinite(st.last_loss) || (double)st.last_loss > (double)max_loss)) {
    st.apply = 0;
    ++st.skipped_loss;
  } else if ((norm_bad && (max_norm_skip > 0.f || clip > 0.f)) ||
             (max_norm_skip > 0.f && norm > (double)max_norm_skip)) {
    st.apply = 0;
    ++st.skipped_norm;
  } else {
    st.apply = 1;
    ++st.applied;
    ++st.step;
  }
  if (st.apply) {
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
    double coef = 1.0;
    if (clip > 0.f) coef = fmin(1.0, (double)clip / (norm + 1e-6));
    const double bc1 = 1.0 - pow(b1, (double)st.step);
    const double bc2 = 1.0 - pow(b2, (double)st.step);
    st.last_coef = (float)coef;
    st.gscale = (float)(coef * (double)gscale);
    st.step_size = (float)(lr / bc1);
    st.bc2s = (float)sqrt(bc2);
  } else {
    st.last_coef = 0.f;
    st.gscale = 0.f;
    st.step_size = 0.f;
    st.bc2s = 1.f;
  }
  gs->st = st;
}

// k_adam's body with gscale, step_size, bc2s and the apply flag read from the guard state; the
// whole grid returns at once on a skipped step.
__global__ __launch_bounds__(256) void k_adam_guarded(float* __restrict__ p,
                                                      const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      int64_t n, float w1, float b2, float w2,
                                                      float eps,
                                                      const GuardState* __restrict__ gs) {
#pragma clang fp contract(off)
  if (gs->st.apply == 0) return;
  const float gscale = gs->st.gscale, step_size = gs->st.step_size, bc2s = gs->st.bc2s;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float gg = gscale == 1.f ? g[i] : g[i] * gscale;
    const float mo = m[i];
    const float mm = fmaf(w1, gg - mo, mo);     // ATen lerp_vec: fmadd(weight, end-start, start)
    const float vv = v[i] * b2 + (w2 * gg) * gg;  // addcmul: self + (value*t1)*t2
    const float denom = sqrtf(vv) / bc2s + eps;
    p[i] = p[i] + (-step_size * mm) / denom;      // addcdiv: self + (value*t1)/t2
    m[i] = mm;
    v[i] = vv;
  }
}

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
hipError_t launch_guard_init(void* state, int64_t step, hipStream_t s) {
  hipLaunchKernelGGL(k_guard_init, dim3(1), dim3(64), 0, s, static_cast<GuardState*>(state), step);
  return hipGetLastError();
}

hipError_t launch_grad_sumsq(const float* g, int64_t n, float gscale, void* state, hipStream_t s) {
  GuardState* gs = static_cast<GuardState*>(state);
  const int blocks = guard_norm_blocks(n);
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0)
    hipLaunchKernelGGL(k_grad_sumsq<true>, dim3(blocks), dim3(256), 0, s, g, n, gscale,
                       gs->partials);
  else  // unaligned views: the scalar twin, the same sum
    hipLaunchKernelGGL(k_grad_sumsq<false>, dim3(blocks), dim3(256), 0, s, g, n, gscale,
                       gs->partials);
  return hipGetLastError();
}

hipError_t launch_grad_norm(const float* g, int64_t n, float gscale, void* state, double* norm_out,
                            hipStream_t s) {
  hipError_t e = launch_grad_sumsq(g, n, gscale, state, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_guard_norm, dim3(1), dim3(256), 0, s, static_cast<GuardState*>(state),
                     guard_norm_blocks(n), norm_out);
  return hipGetLastError();
}

hipError_t launch_adam_guarded(float* p, const float* g, float* m, float* v, int64_t n, float w1,
                               float b2f, float w2, float eps, float gscale, double lr, double b1,
                               double b2, const float* loss, float max_loss, float max_norm_skip,
                               float clip, void* state, hipStream_t s) {
  GuardState* gs = static_cast<GuardState*>(state);
  hipError_t e = launch_grad_sumsq(g, n, gscale, state, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_guard_decide, dim3(1), dim3(256), 0, s, gs, guard_norm_blocks(n), loss,
                     max_loss, max_norm_skip, clip, gscale, lr, b1, b2);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;  // launch_adam's grid
  hipLaunchKernelGGL(k_adam_guarded, dim3((unsigned)blocks), dim3(256), 0, s, p, g, m, v, n, w1,
                     b2f, w2, eps, gs);
  return hipGetLastError();
}

hipError_t guard_state_read(const void* state, void* out, hipStream_t s) {
  const GuardState* gs = static_cast<const GuardState*>(state);
  hipError_t e = hipMemcpyAsync(out, &gs->st, sizeof(dn_guard_stats), hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(s);
}

}  // namespace dn
