// Memory-bank adapter finetune (finetune_memory.py, evaluation_704_iqsl_memory.py) for gfx950.
//
// 1. Nearest-patch selection over an IMPLICIT bank.  The reference unfolds n_img images into
//    N = n_img * ny * nx overlapping P x P windows (1 GB at its shipped settings) and scans them
//    with a GEMM.  Here the bank stays the images: a lane owns one window n = (img, iy, ix) and
//    walks its pixels in place, forming sum (q - b)^2 directly in fp32 for MS_Q queries at a time
//    (the query values are wave-uniform: scalar loads).  The four waves of a workgroup split the
//    C * P patch rows and add their partial sums in a fixed order, so no query or window tile is
//    ever staged in LDS and any D = C * P * P works.  Where windows x queries alone give too few
//    workgroups the patch rows are also split over blockIdx.z.  Stage 1 leaves every window's
//    distance shares; stage 2 adds them in a fixed order and takes the argmin per query.  Ties go
//    to the lowest n.
// 2. HyperGatedResidualAdapter(_FFT): statistics / row-DFT features (fp64), the hyper MLP, three
//    thin 3x3 convolutions on the vector ALUs, and the parameter gradients (slab rows per
//    workgroup, summed in a fixed order in fp64), and the gradient into base_out (direct, local
//    and hyper routes; the hyper route is the fp64 adjoint of the features).  No atomics anywhere.
// 3. The Hann-window blend of patchwise inference in gather form.
#include "block_reduce.h"
#include "dn_internal.h"

namespace dn {

// ---- selection --------------------------------------------------------------------------------
constexpr int MS_Q = 4;     // queries per workgroup
constexpr int MS_WIN = 64;  // windows per workgroup (one per lane)

__device__ __forceinline__ const float* mem_window(const float* img, const MemGeom& g, long n) {
  const int per = g.ny * g.nx;
  const int im = (int)(n / per);
  const int r = (int)(n - (long)im * per);
  const int iy = r / g.nx, ix = r - iy * g.nx;
  return img + ((long)im * g.C * g.H + (long)iy * g.s) * g.W + (long)ix * g.s;
}

// stage 1: dpart[(b * RS + z) * N + n] = the share of sum (q_b - window_n)^2 over the patch rows
// [z R / RS, (z + 1) R / RS), R = C * P; blockIdx = (64-window block, query group, row split z)
__global__ __launch_bounds__(256) void k_mem_dist(const float* __restrict__ q,
                                                  const float* __restrict__ img, MemGeom g, int B,
                                                  int RS, float* __restrict__ dpart) {
  __shared__ float sred[4][MS_Q][MS_WIN];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long n = (long)blockIdx.x * MS_WIN + lane;
  const bool valid = n < g.N;
  const float* win = mem_window(img, g, valid ? n : g.N - 1);  // an invalid lane reads window N-1
  const int b0 = blockIdx.y * MS_Q, z = blockIdx.z;
  const long D = (long)g.C * g.P * g.P;
  const float* qp[MS_Q];
#pragma unroll
  for (int j = 0; j < MS_Q; ++j) qp[j] = q + (long)(b0 + j < B ? b0 + j : B - 1) * D;
  const int R = g.C * g.P;  // patch rows: this workgroup's share [z0, z1), this wave's [r0, r1)
  const int z0 = (int)((long)R * z / RS), z1 = (int)((long)R * (z + 1) / RS);
  const int r0 = z0 + (int)((long)(z1 - z0) * wv / 4), r1 = z0 + (int)((long)(z1 - z0) * (wv + 1) / 4);
  float acc[MS_Q];
#pragma unroll
  for (int j = 0; j < MS_Q; ++j) acc[j] = 0.f;
  for (int r = r0; r < r1; ++r) {
    const int c = r / g.P, py = r - c * g.P;
    const float* row = win + ((long)c * g.H + py) * g.W;
    const long qo = (long)r * g.P;
#pragma unroll 4
    for (int px = 0; px < g.P; ++px) {
      const float v = row[px];
#pragma unroll
      for (int j = 0; j < MS_Q; ++j) {
        const float d = qp[j][qo + px] - v;
        acc[j] = fmaf(d, d, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MS_Q; ++j) sred[wv][j][lane] = acc[j];
  __syncthreads();
  // wave j finishes query b0 + j: the four waves' shares in order
  const int b = b0 + wv;
  const float d = ((sred[0][wv][lane] + sred[1][wv][lane]) + sred[2][wv][lane]) + sred[3][wv][lane];
  if (valid && b < B) dpart[((long)b * RS + z) * g.N + n] = d;
}

// stage 2: one workgroup per query adds every window's RS shares in order and takes the argmin
__global__ __launch_bounds__(256) void k_mem_argmin(const float* __restrict__ dpart, int RS, long N,
                                                    int64_t* __restrict__ idx) {
  __shared__ float sd[256];
  __shared__ int si[256];
  const int t = threadIdx.x;
  const float* base = dpart + (long)blockIdx.x * RS * N;
  float d = __builtin_inff();
  int bi = 0x7fffffff;
  for (long n = t; n < N; n += 256) {
    float d2 = base[n];
    for (int z = 1; z < RS; ++z) d2 += base[(long)z * N + n];
    if (d2 < d || (d2 == d && (int)n < bi)) {
      d = d2;
      bi = (int)n;
    }
  }
  sd[t] = d;
  si[t] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const float d2 = sd[t + w];
      const int i2 = si[t + w];
      if (d2 < sd[t] || (d2 == sd[t] && i2 < si[t])) {
        sd[t] = d2;
        si[t] = i2;
      }
    }
    __syncthreads();
  }
  // every distance NaN: window 0 (torch's argmin would return the first NaN)
  if (t == 0) idx[blockIdx.x] = si[0] == 0x7fffffff ? 0 : si[0];
}

__global__ __launch_bounds__(256) void k_mem_gather(const float* __restrict__ img, MemGeom g,
                                                    const int64_t* __restrict__ idx, int B,
                                                    float* __restrict__ out) {
  const long D = (long)g.C * g.P * g.P, total = D * B;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int b = (int)(e / D);
    const int r = (int)(e - (long)b * D);
    const int c = r / (g.P * g.P), p = r - c * g.P * g.P;
    const int py = p / g.P, px = p - py * g.P;
    long n = idx[b];
    n = n < 0 ? 0 : (n >= g.N ? g.N - 1 : n);  // an index outside the bank is not followed
    out[e] = mem_window(img, g, n)[((long)c * g.H + py) * g.W + px];
  }
}

int mem_select_blocks(const MemGeom& g) { return (int)((g.N + MS_WIN - 1) / MS_WIN); }

// row splits: enough workgroups for about four per CU when windows x query groups alone are few
// (the training step: 254 x 1), each split at least four patch rows
int mem_select_splits(const MemGeom& g, int B) {
  const long wgs = (long)mem_select_blocks(g) * ((B + MS_Q - 1) / MS_Q);
  long rs = (1024 + wgs - 1) / wgs;
  const long cap = (long)g.C * g.P / 4;
  rs = rs > 8 ? 8 : rs;
  rs = rs > cap ? cap : rs;
  return (int)(rs < 1 ? 1 : rs);
}

size_t mem_select_ws_bytes(const MemGeom& g, int B) {
  return sizeof(float) * (size_t)B * mem_select_splits(g, B) * (size_t)g.N;
}

hipError_t launch_mem_select(const float* q, const float* img, const MemGeom& g, int B,
                             int64_t* idx, void* ws, hipStream_t s) {
  const int RS = mem_select_splits(g, B);
  float* dpart = static_cast<float*>(ws);
  const dim3 grid(mem_select_blocks(g), (B + MS_Q - 1) / MS_Q, RS);
  hipLaunchKernelGGL(k_mem_dist, grid, dim3(256), 0, s, q, img, g, B, RS, dpart);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mem_argmin, dim3(B), dim3(256), 0, s, dpart, RS, g.N, idx);
  return hipGetLastError();
}

hipError_t launch_mem_gather(const float* img, const MemGeom& g, const int64_t* idx, int B,
                             float* out, hipStream_t s) {
  const long total = (long)B * g.C * g.P * g.P;
  const int nb = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_mem_gather, dim3(nb), dim3(256), 0, s, img, g, idx, B, out);
  return hipGetLastError();
}

// ---- adapter: features --------------------------------------------------------------------------
constexpr int MA_T = 16;         // tile edge of the convolutions
constexpr int MA_WMAX = 1024;    // widest row whose DFT twiddle table lives in LDS (else global)
constexpr int MA_NBMAX = 8;      // most frequency bands
constexpr int MA_WG_BLOCKS = 256;  // most workgroups (slab rows) of a weight-gradient launch

// (cos, sin)(2 pi k / W), k < W, for rows too wide for the LDS table
__global__ __launch_bounds__(256) void k_ma_twiddle(int W, double* __restrict__ tw) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= W) return;
  const double a = 2.0 * (double)k / (double)W;
  tw[2 * k] = cospi(a);
  tw[2 * k + 1] = sinpi(a);
}

// feat[b] = [mean_n, std_n, mean_b, std_b, mean_m, std_m, fft_n (nb), fft_b (nb), fft_m (nb)]:
// one workgroup per (sample, tensor), everything in fp64.  gtw: the twiddle table in global
// memory (W > MA_WMAX), else it is built in LDS.
__global__ __launch_bounds__(256) void k_ma_stats(const float* __restrict__ noisy,
                                                  const float* __restrict__ base,
                                                  const float* __restrict__ mem, int C, int H,
                                                  int W, int nb, const double* __restrict__ gtw,
                                                  float* __restrict__ feat) {
  constexpr int FC = MA_WMAX / 2;  // bins per pass
  __shared__ double red[4];
  __shared__ double tw[2 * MA_WMAX];
  __shared__ double spow[FC];
  const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const long M = (long)C * H * W;
  const float* x = (t == 0 ? noisy : (t == 1 ? base : mem)) + (long)b * M;
  const int NF = 6 + 3 * nb;
  double s = 0.0;
  for (long e = tid; e < M; e += 256) s += (double)x[e];
  const double mean = block_sum(s, red) / (double)M;
  s = 0.0;
  for (long e = tid; e < M; e += 256) {
    const double d = (double)x[e] - mean;
    s += d * d;
  }
  const double var = block_sum(s, red) / (double)(M - 1);  // unbiased, torch.std's default
  if (tid == 0) {
    feat[(long)b * NF + 2 * t] = (float)mean;
    feat[(long)b * NF + 2 * t + 1] = (float)sqrt(var);
  }
  if (nb == 0) return;
  const int F = W / 2 + 1, rows = C * H;
  if (!gtw)
    for (int k = tid; k < W; k += 256) {
      const double a = 2.0 * (double)k / (double)W;
      tw[2 * k] = cospi(a);
      tw[2 * k + 1] = sinpi(a);
    }
  const double* T = gtw ? gtw : tw;
  __syncthreads();
  int G = 256 / F;  // row groups per bin (F * G <= 256 tasks, or one group of all rows)
  G = G < 1 ? 1 : (G > rows ? rows : G);
  const int bs = F / nb;
  double band[MA_NBMAX];  // thread 0: the bands' sums of the row-mean power, bins in order
  for (int k = 0; k < MA_NBMAX; ++k) band[k] = 0.0;
  for (int f0 = 0; f0 < F; f0 += FC) {
    const int nf = F - f0 < FC ? F - f0 : FC;
    for (int task = tid; task < nf * G; task += 256) {
      const int f = f0 + task % nf, g = task / nf;
      double ps = 0.0;
      for (int r = g; r < rows; r += G) {
        const float* xr = x + (long)r * W;
        double re = 0.0, im = 0.0;
        int k = 0;
        for (int w = 0; w < W; ++w) {
          const double v = (double)xr[w];
          re += v * T[2 * k];
          im += v * T[2 * k + 1];
          k += f;
          if (k >= W) k -= W;
        }
        ps += re * re + im * im;
      }
      spow[task] = ps;
    }
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < nf; ++j) {  // mean over the rows, groups added in order
        double p = 0.0;
        for (int g = 0; g < G; ++g) p += spow[g * nf + j];
        int k = (f0 + j) / bs;
        k = k < nb - 1 ? k : nb - 1;
        band[k] += p / (double)rows;
      }
    __syncthreads();
  }
  if (tid != 0) return;
  double bm = 0.0;
  for (int k = 0; k < nb; ++k) {
    const int st = k * bs, en = k < nb - 1 ? (k + 1) * bs : F;
    band[k] = log1p(band[k] / (double)(en - st));
    bm += band[k];
  }
  bm = bm / (double)nb + 1e-6;
  for (int k = 0; k < nb; ++k) feat[(long)b * NF + 6 + t * nb + k] = (float)(band[k] / bm);
}

// parameter offsets (floats) in state_dict order: local_net.0/2/4 weight, bias; hyper_mlp.0/2
struct MaLayout {
  int w1, b1, w2, b2, w3, b3, m0w, m0b, m1w, m1b, np, nf;
};

MaLayout ma_layout(int C, int HID, int nb) {
  MaLayout L;
  L.nf = 6 + 3 * nb;
  L.w1 = 0;
  L.b1 = L.w1 + HID * 2 * C * 9;
  L.w2 = L.b1 + HID;
  L.b2 = L.w2 + HID * HID * 9;
  L.w3 = L.b2 + HID;
  L.b3 = L.w3 + C * HID * 9;
  L.m0w = L.b3 + C;
  L.m0b = L.m0w + HID * L.nf;
  L.m1w = L.m0b + HID;
  L.m1b = L.m1w + 2 * C * HID;
  L.np = L.m1b + 2 * C;
  return L;
}

// hidden = relu(W0 feat + b0) of sample b into sh[HID] (threads < HID), no barrier
__device__ __forceinline__ void ma_mlp_hidden(const float* __restrict__ prm, const MaLayout& L,
                                              const float* __restrict__ f, int HID, float* sh) {
  const int j = threadIdx.x;
  if (j >= HID) return;
  float a = prm[L.m0b + j];
  for (int k = 0; k < L.nf; ++k) a = fmaf(prm[L.m0w + j * L.nf + k], f[k], a);
  sh[j] = fmaxf(a, 0.f);
}

// gb[b] = [gamma (C) | beta (C) | tanh(beta_raw) (C)]
__global__ __launch_bounds__(64) void k_ma_hyper(const float* __restrict__ prm, MaLayout L,
                                                 const float* __restrict__ feat, int C, int HID,
                                                 float* __restrict__ gb) {
  __shared__ float sh[16];
  const int b = blockIdx.x, j = threadIdx.x;
  ma_mlp_hidden(prm, L, feat + (long)b * L.nf, HID, sh);
  __syncthreads();
  if (j >= 2 * C) return;
  float a = prm[L.m1b + j];
  for (int k = 0; k < HID; ++k) a = fmaf(prm[L.m1w + j * HID + k], sh[k], a);
  if (j < C) {
    gb[(long)b * 3 * C + j] = 1.f / (1.f + expf(-a));
  } else {
    const float th = tanhf(a);
    gb[(long)b * 3 * C + j] = 0.1f * th;
    gb[(long)b * 3 * C + C + j] = th;
  }
}

// sample b's gradients at the hyper MLP's two pre-activations: sdh[2C] (gamma | beta rows) and
// sdk[HID] = dz0, from the tile sums part[((b * C + c) * ntiles + t) * 2 + {0, 1}] of r * dpre and
// dpre.  Ends with a barrier; sh, sdh and sdk are then readable by every thread.
__device__ __forceinline__ void ma_hyper_dz0(const float* __restrict__ prm, const MaLayout& L,
                                             const float* __restrict__ f,
                                             const float* __restrict__ gb,
                                             const double* __restrict__ part, int ntiles, int b,
                                             int C, int HID, float* sh, float* sdh, float* sdk) {
  const int tid = threadIdx.x;
  ma_mlp_hidden(prm, L, f, HID, sh);
  if (tid < 2 * C) {
    const int which = tid / C, c = tid - which * C;
    const double* p = part + ((long)(b * C + c) * ntiles) * 2 + which;
    double S = 0.0;
    for (int t = 0; t < ntiles; ++t) S += p[2 * t];
    if (which == 0) {
      const float g = gb[(long)b * 3 * C + c];
      sdh[tid] = (float)S * g * (1.f - g);
    } else {
      const float th = gb[(long)b * 3 * C + 2 * C + c];
      sdh[tid] = (float)S * 0.1f * (1.f - th * th);
    }
  }
  __syncthreads();
  if (tid < HID) {
    float a = 0.f;
    for (int j = 0; j < 2 * C; ++j) a = fmaf(prm[L.m1w + j * HID + tid], sdh[j], a);
    sdk[tid] = sh[tid] > 0.f ? a : 0.f;
  }
  __syncthreads();
}

// gradients of the hyper MLP's parameters: one workgroup walks the samples in order.
__global__ __launch_bounds__(256) void k_ma_hyper_bwd(const float* __restrict__ prm, MaLayout L,
                                                      const float* __restrict__ feat,
                                                      const float* __restrict__ gb,
                                                      const double* __restrict__ part, int ntiles,
                                                      int N, int C, int HID,
                                                      float* __restrict__ dprm) {
  __shared__ float sh[16], sdh[8], sdk[16];
  const int tid = threadIdx.x;
  const int NPM = L.np - L.m0w;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < N; ++b) {
    const float* f = feat + (long)b * L.nf;
    ma_hyper_dz0(prm, L, f, gb, part, ntiles, b, C, HID, sh, sdh, sdk);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int e = tid + 256 * jj;
      if (e >= NPM) continue;
      float v;
      if (e < HID * L.nf) v = sdk[e / L.nf] * f[e % L.nf];
      else if (e < HID * L.nf + HID) v = sdk[e - HID * L.nf];
      else if (e < HID * L.nf + HID + 2 * C * HID) {
        const int r = e - HID * L.nf - HID;
        v = sdh[r / HID] * sh[r % HID];
      } else v = sdh[e - HID * L.nf - HID - 2 * C * HID];
      acc[jj] += (double)v;
    }
    __syncthreads();
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int e = tid + 256 * jj;
    if (e < NPM) dprm[L.m0w + e] = (float)acc[jj];
  }
}

// dfe[b] = the gradient at base_out's features of sample b, (W0^T dz0)[2, 3, 6 + nb + k]:
// [dmean, dstd, dphi_0 .. dphi_{nb-1}], the HID products added in order in fp64
__global__ __launch_bounds__(64) void k_ma_hyper_dfeat(const float* __restrict__ prm, MaLayout L,
                                                       const float* __restrict__ feat,
                                                       const float* __restrict__ gb,
                                                       const double* __restrict__ part, int ntiles,
                                                       int C, int HID, int nb,
                                                       double* __restrict__ dfe) {
  __shared__ float sh[16], sdh[8], sdk[16];
  const int b = blockIdx.x, j = threadIdx.x;
  ma_hyper_dz0(prm, L, feat + (long)b * L.nf, gb, part, ntiles, b, C, HID, sh, sdh, sdk);
  if (j >= 2 + nb) return;
  const int col = j < 2 ? 2 + j : 6 + nb + (j - 2);
  double a = 0.0;
  for (int h = 0; h < HID; ++h) a += (double)prm[L.m0w + h * L.nf + col] * (double)sdk[h];
  dfe[(long)b * (2 + MA_NBMAX) + j] = a;
}

// ---- adapter: thin 3x3 convolutions (NCHW, pad 1) ------------------------------------------------
enum MaMode {
  MA_RELU = 0,   // out = relu(conv + bias)
  MA_MASKT = 1,  // out = aux > 0 ? convT : 0    (data gradient through a ReLU; w transposed)
  MA_FINAL = 2,  // pre = base + (gamma * (conv + bias) + beta); out = clamp ? clamp(pre) : pre
  MA_DFINAL = 3, // out = dr = gamma * dpre, part = the tile's sums of r * dpre and dpre
  MA_DINT = 4,   // out += convT over output channels [CO, 2 CO) of w [CI][2 CO][9]: no mask (the
                 // data gradient of local_net.0 into base_out, added to the dpre already in out)
};

struct MaConvArgs {
  const float* in0; const float* in1; int c0;  // input channels [0, c0) from in0, the rest from in1
  const float* w; const float* bias;
  int N, H, W;
  float* out;
  const float* aux;   // MA_MASKT: the ReLU's output; MA_FINAL / MA_DFINAL: base_out
  const float* gb;    // [N][3C]
  const float* dout;  // MA_DFINAL
  double* part;       // MA_DFINAL
  float* dpre;        // MA_DFINAL, nullable: dpre itself (the direct route of the input gradient)
  int clamp;
};

template <int CI>
__device__ __forceinline__ void ma_load_tile(const MaConvArgs& a, int n, int y0, int x0, float* sx) {
  constexpr int E = MA_T + 2;
  for (int e = threadIdx.x; e < CI * E * E; e += 256) {
    const int i = e / (E * E), r = e - i * E * E;
    const int gy = y0 + r / E, gx = x0 + r % E;
    float v = 0.f;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      v = i < a.c0 ? a.in0[(((long)n * a.c0 + i) * a.H + gy) * a.W + gx]
                   : a.in1[(((long)n * (CI - a.c0) + (i - a.c0)) * a.H + gy) * a.W + gx];
    }
    sx[e] = v;
  }
}

template <int CI, int CO, int MODE>
__global__ __launch_bounds__(256) void k_ma_conv(MaConvArgs a) {
  constexpr int E = MA_T + 2;
  __shared__ float sx[CI * E * E];
  __shared__ double red[4];
  const int tiles_x = (a.W + MA_T - 1) / MA_T;
  const int ty0 = (blockIdx.x / tiles_x) * MA_T, tx0 = (blockIdx.x % tiles_x) * MA_T;
  const int n = blockIdx.y;
  ma_load_tile<CI>(a, n, ty0 - 1, tx0 - 1, sx);
  __syncthreads();
  const int py = threadIdx.x / MA_T, px = threadIdx.x % MA_T;
  const int gy = ty0 + py, gx = tx0 + px;
  const bool in = gy < a.H && gx < a.W;
  float acc[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) acc[o] = 0.f;
#pragma unroll 1
  for (int i = 0; i < CI; ++i) {
    float x[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) x[t] = sx[i * E * E + (py + t / 3) * E + px + t % 3];
#pragma unroll
    for (int o = 0; o < CO; ++o)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        // transposed: w is [CI][CO][9] and the taps run backwards (the data gradient)
        const float wv = MODE == MA_MASKT  ? a.w[(i * CO + o) * 9 + 8 - t]
                         : MODE == MA_DINT ? a.w[(i * 2 * CO + CO + o) * 9 + 8 - t]
                                           : a.w[(o * CI + i) * 9 + t];
        acc[o] = fmaf(wv, x[t], acc[o]);
      }
  }
  if (MODE == MA_RELU || MODE == MA_MASKT || MODE == MA_DINT) {
    if (!in) return;
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      const long e = (((long)n * CO + o) * a.H + gy) * a.W + gx;
      if (MODE == MA_RELU) a.out[e] = fmaxf(acc[o] + a.bias[o], 0.f);
      else if (MODE == MA_MASKT) a.out[e] = a.aux[e] > 0.f ? acc[o] : 0.f;
      else a.out[e] = __fadd_rn(a.out[e], acc[o]);
    }
    return;
  }
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    float rd = 0.f, dp = 0.f;
    if (in) {
      const long e = (((long)n * CO + o) * a.H + gy) * a.W + gx;
      const float gamma = a.gb[(long)n * 3 * CO + o], beta = a.gb[(long)n * 3 * CO + CO + o];
      const float r = acc[o] + a.bias[o];
      const float pre = __fadd_rn(a.aux[e], __fadd_rn(__fmul_rn(gamma, r), beta));
      if (MODE == MA_FINAL) {
        a.out[e] = a.clamp ? fminf(fmaxf(pre, 0.f), 1.f) : pre;
      } else {
        dp = (!a.clamp || (pre >= 0.f && pre <= 1.f)) ? a.dout[e] : 0.f;
        rd = r * dp;
        a.out[e] = gamma * dp;
        if (a.dpre) a.dpre[e] = dp;
      }
    }
    if (MODE == MA_DFINAL) {
      const double s0 = block_sum((double)rd, red);
      const double s1 = block_sum((double)dp, red);
      if (threadIdx.x == 0) {
        double* p = a.part + (((long)n * CO + o) * gridDim.x + blockIdx.x) * 2;
        p[0] = s0;
        p[1] = s1;
      }
    }
  }
}

// dW[o][i][ky][kx] = sum_p g[o][p] * in[i][p + (ky-1, kx-1)], db[o] = sum_p g[o][p]: a workgroup
// walks a fixed set of tiles, sums a tile in fp32 and the tiles in fp64, and writes one slab row
// [W | b]; thread task = one kernel row (o, i, ky) or one bias
template <int CI, int CO>
__global__ __launch_bounds__(256) void k_ma_wgrad(MaConvArgs a, const float* __restrict__ g,
                                                  float* __restrict__ slab) {
  constexpr int E = MA_T + 2, TA = MA_T * MA_T, GP = TA + 4;
  constexpr int T = CO * CI * 3, NT = T + CO, TPT = (NT + 255) / 256, ROW = CO * CI * 9 + CO;
  __shared__ float sx[CI * E * E];
  __shared__ float sg[CO * GP];
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + MA_T - 1) / MA_T, tiles_y = (a.H + MA_T - 1) / MA_T;
  const long ntiles = (long)a.N * tiles_x * tiles_y;
  double acc[TPT][3];
#pragma unroll
  for (int j = 0; j < TPT; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = (int)(tile / ((long)tiles_x * tiles_y));
    const int r = (int)(tile - (long)n * tiles_x * tiles_y);
    const int ty0 = (r / tiles_x) * MA_T, tx0 = (r % tiles_x) * MA_T;
    ma_load_tile<CI>(a, n, ty0 - 1, tx0 - 1, sx);
    for (int e = tid; e < CO * TA; e += 256) {
      const int o = e / TA, p = e - o * TA;
      const int gy = ty0 + p / MA_T, gx = tx0 + p % MA_T;
      sg[o * GP + p] = (gy < a.H && gx < a.W) ? g[(((long)n * CO + o) * a.H + gy) * a.W + gx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int k = tid + 256 * j;
      if (k >= NT) continue;
      if (k < T) {
        const int o = k / (CI * 3), i = (k / 3) % CI, ky = k % 3;
        const float* gs = sg + o * GP;
        const float* xs = sx + i * E * E + ky * E;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 1
        for (int rr = 0; rr < MA_T; ++rr) {
          float xv[E];
#pragma unroll
          for (int cc = 0; cc < E; ++cc) xv[cc] = xs[rr * E + cc];
#pragma unroll
          for (int cc = 0; cc < MA_T; ++cc) {
            const float d = gs[rr * MA_T + cc];
            a0 = fmaf(d, xv[cc], a0);
            a1 = fmaf(d, xv[cc + 1], a1);
            a2 = fmaf(d, xv[cc + 2], a2);
          }
        }
        acc[j][0] += (double)a0;
        acc[j][1] += (double)a1;
        acc[j][2] += (double)a2;
      } else {
        const float* gs = sg + (k - T) * GP;
        double a0 = 0.0;
        for (int p = 0; p < TA; ++p) a0 += (double)gs[p];
        acc[j][0] += a0;
      }
    }
    __syncthreads();
  }
  float* row = slab + (long)blockIdx.x * ROW;
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int k = tid + 256 * j;
    if (k >= NT) continue;
    if (k < T) {
      const int o = k / (CI * 3), i = (k / 3) % CI, ky = k % 3;
      for (int kx = 0; kx < 3; ++kx) row[(o * CI + i) * 9 + ky * 3 + kx] = (float)acc[j][kx];
    } else {
      row[CO * CI * 9 + k - T] = (float)acc[j][0];
    }
  }
}

// out[e] = sum over the slab rows in order, in fp64
__global__ __launch_bounds__(256) void k_ma_reduce(const float* __restrict__ slab, int row, int nrows,
                                                   float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= row) return;
  double s = 0.0;
  for (int r = 0; r < nrows; ++r) s += (double)slab[(long)r * row + e];
  out[e] = (float)s;
}

// ---- adapter: the hyper route of the input gradient ----------------------------------------------
// base_out also reaches the output through its own features (mean, unbiased std, row-DFT bands),
// which feed the hyper MLP.  Per sample, x = base_out[b] as R = C H rows of W, M = R W:
//   A[r,f] = sum_w x[r,w] cos(2 pi f w / W),  S[r,f] = sum_w x[r,w] sin(2 pi f w / W)
//   P_f = (1/R) sum_r (A^2 + S^2),  B_k = band mean of P_f,  L_k = log1p(B_k),  m = mean_k L_k
//   dL_k = dphi_k / (m + eps) - (sum_j dphi_j L_j) / (nb (m + eps)^2),  dB_k = dL_k / (1 + B_k)
//   hyper[r,w] = dmean / M + dstd (x[r,w] - mean) / ((M - 1) std)
//              + sum_f c_f (A[r,f] cos(2 pi f w / W) + S[r,f] sin(2 pi f w / W)),
//   c_f = dB_band(f) * 2 / (R len_band(f))          (one-sided power: DC and Nyquist take the 2 too)
// Three launches, everything in fp64, every sum in a fixed order, one writer per element:
//   k_ma_adj_power  a workgroup walks a fixed set of row passes: sum (x - x0), sum (x - x0)^2 and
//                   its rows' share of every bin's power (the band powers cannot be recovered from
//                   feat: it holds only phi_k)
//   k_ma_adj_coef   one workgroup per sample adds the shares in order: mean, std, c of every band
//   k_ma_adj_apply  the same row passes again: analysis A, S into LDS, then the synthesis
// A pass stages as many rows as fit (MA_ADJ_X floats of x, MA_ADJ_F (row, bin) pairs of A and S);
// a thread's task is one (row, bin) of the analysis and one (row, w) of the synthesis, both
// O(W) / O(F) long.  Rows wider than MA_WMAX go one at a time with x, the twiddles and A, S in
// global memory (WIDE).  A constant sample has std = 0 and no defined gradient (inf / nan), as in
// the reference.
constexpr int MA_ADJ_X = 4096;                   // floats of x staged per pass
constexpr int MA_ADJ_F = 2 * (MA_WMAX / 2 + 1);  // (row, bin) pairs of A and of S per pass
constexpr int MA_ADJ_CO = 4 + MA_NBMAX;          // doubles per sample: dmean/M, dstd/((M-1) std), mean, -, c_k
constexpr int MA_ADJ_DF = 2 + MA_NBMAX;          // doubles per sample: dmean, dstd, dphi_k

struct MaAdj {
  int R, W, F, ri, iters, G;  // rows, width, bins, rows per pass, passes, workgroups per sample
};

static MaAdj ma_adj_plan(int N, int C, int H, int W) {
  MaAdj p;
  p.R = C * H; p.W = W; p.F = W / 2 + 1;
  if (W > MA_WMAX) {
    p.ri = 1;
  } else {
    const int a = MA_ADJ_F / p.F, b = MA_ADJ_X / W;
    p.ri = a < b ? a : b;
    p.ri = p.ri < p.R ? p.ri : p.R;
  }
  p.iters = (p.R + p.ri - 1) / p.ri;
  int g = 1024 / N;  // about four workgroups per CU over the batch, 16 .. 256 per sample
  g = g < 16 ? 16 : (g > 256 ? 256 : g);
  p.G = g < p.iters ? g : p.iters;
  return p;
}

template <bool WIDE>
struct MaAdjLds {
  double tw[WIDE ? 2 : 2 * MA_WMAX];
  double as[WIDE ? 2 : 2 * MA_ADJ_F];
  float x[WIDE ? 2 : MA_ADJ_X];
};

// A[s * F + f], S[s * F + f] of the nr rows at xs, bins f < F; T = (cos, sin)(2 pi k / W)
__device__ __forceinline__ void ma_adj_analysis(const float* xs, int nr, int W, int F,
                                                const double* T, double* A, double* S) {
  for (int task = threadIdx.x; task < nr * F; task += 256) {
    const int s = task / F, f = task - s * F;
    const float* xr = xs + (long)s * W;
    double re = 0.0, im = 0.0;
    int k = 0;
    for (int w = 0; w < W; ++w) {
      const double v = (double)xr[w];
      re += v * T[2 * k];
      im += v * T[2 * k + 1];
      k += f;
      if (k >= W) k -= W;
    }
    A[task] = re;
    S[task] = im;
  }
}

// the pass's rows into LDS (or, WIDE, where they are) and the pointers of its A and S
template <bool WIDE>
__device__ __forceinline__ const float* ma_adj_stage(MaAdjLds<WIDE>& l, const float* xg, int n) {
  if (WIDE) return xg;
  for (int e = threadIdx.x; e < n; e += 256) l.x[e] = xg[e];
  __syncthreads();
  return l.x;
}

template <bool WIDE>
__device__ __forceinline__ const double* ma_adj_twiddles(MaAdjLds<WIDE>& l, int W, int nb,
                                                         const double* gtw) {
  if (WIDE) return gtw;
  if (nb > 0) {
    for (int k = threadIdx.x; k < W; k += 256) {
      const double a = 2.0 * (double)k / (double)W;
      l.tw[2 * k] = cospi(a);
      l.tw[2 * k + 1] = sinpi(a);
    }
    __syncthreads();
  }
  return l.tw;
}

// part[(b * G + g) * (2 + F)] = [sum d, sum d^2 (d = x - x[0]), the power of bins 0 .. F-1] over
// workgroup g's passes g, g + G, ...; gas (WIDE): 2 F doubles per workgroup
template <bool WIDE>
__global__ __launch_bounds__(256) void k_ma_adj_power(const float* __restrict__ base, MaAdj p,
                                                      int nb, const double* __restrict__ gtw,
                                                      double* gas, double* part) {
  __shared__ MaAdjLds<WIDE> l;
  __shared__ double red[4];
  const int g = blockIdx.x, b = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  const int W = p.W, F = p.F;
  const float* x = base + (long)b * p.R * W;
  const double x0 = (double)x[0];
  const double* T = ma_adj_twiddles<WIDE>(l, W, nb, gtw);
  double* A = WIDE ? gas + ((long)b * G + g) * 2 * F : l.as;
  double* S = A + (WIDE ? F : MA_ADJ_F);
  double* pp = part + ((long)b * G + g) * (2 + F);
  double sd = 0.0, sdd = 0.0;
  bool first = true;
  for (int it = g; it < p.iters; it += G) {
    const int r0 = it * p.ri, nr = p.R - r0 < p.ri ? p.R - r0 : p.ri;
    const float* xs = ma_adj_stage<WIDE>(l, x + (long)r0 * W, nr * W);
    for (int e = tid; e < nr * W; e += 256) {
      const double d = (double)xs[e] - x0;
      sd += d;
      sdd += d * d;
    }
    if (nb > 0) {
      ma_adj_analysis(xs, nr, W, F, T, A, S);
      __syncthreads();
      for (int f = tid; f < F; f += 256) {
        double pw = 0.0;
        for (int s = 0; s < nr; ++s) pw += A[s * F + f] * A[s * F + f] + S[s * F + f] * S[s * F + f];
        pp[2 + f] = first ? pw : pp[2 + f] + pw;
      }
    }
    first = false;
    __syncthreads();
  }
  const double s0 = block_sum(sd, red);
  const double s1 = block_sum(sdd, red);
  if (tid == 0) {
    pp[0] = s0;
    pp[1] = s1;
  }
}

// coef[b] = [dmean / M, dstd / ((M - 1) std), mean, 0, c_0 .. c_{nb-1}]; the gradient at the
// features comes from dfd (doubles, MA_ADJ_DF per sample) or, if null, dff (floats, 2 + nb per
// sample); pf: F doubles per sample
__global__ __launch_bounds__(256) void k_ma_adj_coef(const float* __restrict__ base, MaAdj p, int G,
                                                     int nb, const double* part,
                                                     const double* __restrict__ dfd,
                                                     const float* __restrict__ dff, double* pf,
                                                     double* __restrict__ coef) {
  const int b = blockIdx.x, tid = threadIdx.x, F = p.F;
  const double* pb = part + (long)b * G * (2 + F);
  double* P = pf + (long)b * F;
  if (nb > 0)
    for (int f = tid; f < F; f += 256) {
      double s = 0.0;
      for (int g = 0; g < G; ++g) s += pb[(long)g * (2 + F) + 2 + f];
      P[f] = s / (double)p.R;
    }
  __syncthreads();
  if (tid != 0) return;
  const double M = (double)p.R * (double)p.W;
  double sd = 0.0, sdd = 0.0;
  for (int g = 0; g < G; ++g) {
    sd += pb[(long)g * (2 + F)];
    sdd += pb[(long)g * (2 + F) + 1];
  }
  const double mean = (double)base[(long)b * p.R * p.W] + sd / M;
  const double sdev = sqrt((sdd - sd * sd / M) / (M - 1.0));
  double df[MA_ADJ_DF];
  for (int k = 0; k < 2 + nb; ++k)
    df[k] = dfd ? dfd[(long)b * MA_ADJ_DF + k] : (double)dff[(long)b * (2 + nb) + k];
  double* co = coef + (long)b * MA_ADJ_CO;
  co[0] = df[0] / M;
  co[1] = df[1] / ((M - 1.0) * sdev);
  co[2] = mean;
  co[3] = 0.0;
  if (nb == 0) return;
  const int bs = F / nb;
  double Bk[MA_NBMAX], Lk[MA_NBMAX];
  double m = 0.0, dot = 0.0;
  for (int k = 0; k < nb; ++k) {
    const int st = k * bs, en = k < nb - 1 ? (k + 1) * bs : F;
    double s = 0.0;
    for (int f = st; f < en; ++f) s += P[f];
    Bk[k] = s / (double)(en - st);
    Lk[k] = log1p(Bk[k]);
    m += Lk[k];
    dot += df[2 + k] * Lk[k];
  }
  m = m / (double)nb + 1e-6;
  for (int k = 0; k < nb; ++k) {
    const int st = k * bs, en = k < nb - 1 ? (k + 1) * bs : F;
    const double dL = df[2 + k] / m - dot / ((double)nb * m * m);
    co[4 + k] = dL / (1.0 + Bk[k]) * 2.0 / ((double)p.R * (double)(en - st));
  }
}

// out[b, r, w] (+)= hyper[r, w]
template <bool WIDE>
__global__ __launch_bounds__(256) void k_ma_adj_apply(const float* __restrict__ base, MaAdj p,
                                                      int nb, const double* __restrict__ gtw,
                                                      double* gas, const double* __restrict__ coef,
                                                      float* out, int accumulate) {
  __shared__ MaAdjLds<WIDE> l;
  const int g = blockIdx.x, b = blockIdx.y, G = gridDim.x, tid = threadIdx.x;
  const int W = p.W, F = p.F;
  const long M = (long)p.R * W;
  const float* x = base + (long)b * M;
  const double* co = coef + (long)b * MA_ADJ_CO;
  const double a0 = co[0], a1 = co[1], mean = co[2];
  const double* T = ma_adj_twiddles<WIDE>(l, W, nb, gtw);
  double* A = WIDE ? gas + ((long)b * G + g) * 2 * F : l.as;
  double* S = A + (WIDE ? F : MA_ADJ_F);
  const int bs = nb > 0 ? F / nb : 0;
  for (int it = g; it < p.iters; it += G) {
    const int r0 = it * p.ri, nr = p.R - r0 < p.ri ? p.R - r0 : p.ri;
    const float* xs = ma_adj_stage<WIDE>(l, x + (long)r0 * W, nr * W);
    if (nb > 0) {
      ma_adj_analysis(xs, nr, W, F, T, A, S);
      __syncthreads();
    }
    for (int task = tid; task < nr * W; task += 256) {
      const int s = task / W, w = task - s * W;
      double acc = 0.0;
      int k = 0;
      for (int kb = 0; kb < nb; ++kb) {
        const int st = kb * bs, en = kb < nb - 1 ? (kb + 1) * bs : F;
        double ab = 0.0;
        for (int f = st; f < en; ++f) {
          ab += A[s * F + f] * T[2 * k] + S[s * F + f] * T[2 * k + 1];
          k += w;
          if (k >= W) k -= W;
        }
        acc += co[4 + kb] * ab;
      }
      const double h = a0 + a1 * ((double)xs[task] - mean) + acc;
      const long e = (long)b * M + (long)r0 * W + task;
      out[e] = accumulate ? __fadd_rn(out[e], (float)h) : (float)h;
    }
    __syncthreads();
  }
}

static int ma_tiles(int H, int W) { return ((H + MA_T - 1) / MA_T) * ((W + MA_T - 1) / MA_T); }

static int ma_wg_blocks(int N, int H, int W) {
  const long t = (long)N * ma_tiles(H, W);
  return (int)(t < MA_WG_BLOCKS ? t : MA_WG_BLOCKS);
}

static size_t ma_align(size_t floats) { return (floats + 63) / 64 * 64; }

// workspace (floats): gb | tw (doubles, W > MA_WMAX) | part (doubles) | h1 | h2 | [dr | g2 | g1 | slab]
// and, for the input gradient (mode 2), doubles: [dfe | coef | pf | apart | gas (W > MA_WMAX)]
struct MaWs {
  size_t gb, tw, part, h1, h2, dr, g2, g1, slab, dfe, coef, pf, apart, gas, total;
};

// mode: 0 forward, 1 parameter gradient, 2 parameter and input gradient
static MaWs ma_ws(int N, int C, int H, int W, int HID, int mode) {
  const bool bwd = mode != 0;
  MaWs w;
  const size_t px = (size_t)N * H * W;
  size_t o = 0;
  w.gb = o; o += ma_align((size_t)N * 3 * C);
  w.tw = o; o += W > MA_WMAX ? ma_align((size_t)W * 2 * 2) : 0;  // doubles: wide rows' twiddles
  w.part = o; o += ma_align((size_t)N * C * ma_tiles(H, W) * 2 * 2);
  w.h1 = o; o += ma_align(px * HID);
  w.h2 = o; o += ma_align(px * HID);
  w.dr = w.g2 = w.g1 = w.slab = o;
  if (bwd) {
    w.dr = o; o += ma_align(px * C);
    w.g2 = o; o += ma_align(px * HID);
    w.g1 = o; o += ma_align(px * HID);
    const int mc = 2 * C > HID ? 2 * C : HID;
    w.slab = o; o += ma_align((size_t)MA_WG_BLOCKS * ((size_t)HID * mc * 9 + HID));
  }
  w.dfe = w.coef = w.pf = w.apart = w.gas = o;
  if (mode == 2) {
    const MaAdj p = ma_adj_plan(N, C, H, W);
    w.dfe = o; o += ma_align((size_t)N * MA_ADJ_DF * 2);
    w.coef = o; o += ma_align((size_t)N * MA_ADJ_CO * 2);
    w.pf = o; o += ma_align((size_t)N * p.F * 2);
    w.apart = o; o += ma_align((size_t)N * p.G * (2 + p.F) * 2);
    w.gas = o; o += W > MA_WMAX ? ma_align((size_t)N * p.G * 2 * p.F * 2) : 0;
  }
  w.total = o;
  return w;
}

bool memadapter_supported(int C, int HID, int nb) {
  return (C == 1 || C == 3) && (HID == 8 || HID == 16) && nb >= 0 && nb <= MA_NBMAX;
}

long memadapter_param_count(int C, int HID, int nb) {
  return memadapter_supported(C, HID, nb) ? ma_layout(C, HID, nb).np : -1;
}

size_t memadapter_ws_bytes(int N, int C, int H, int W, int HID, int nb, int mode) {
  if (!memadapter_supported(C, HID, nb) || N < 1 || H < 1 || W < 1) return 0;
  return sizeof(float) * ma_ws(N, C, H, W, HID, mode).total;
}

#define MA_CHECK()                        \
  do {                                    \
    hipError_t e_ = hipGetLastError();    \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

template <int C, int HID>
static hipError_t ma_features_and_convs(const float* prm, const MaLayout& L, const float* noisy,
                                        const float* base, const float* feat, int N, int H, int W,
                                        float* wsf, const MaWs& ws, hipStream_t s) {
  hipLaunchKernelGGL(k_ma_hyper, dim3(N), dim3(64), 0, s, prm, L, feat, C, HID, wsf + ws.gb);
  MA_CHECK();
  const dim3 grid(ma_tiles(H, W), N);
  MaConvArgs a{};
  a.N = N; a.H = H; a.W = W;
  a.in0 = noisy; a.in1 = base; a.c0 = C;
  a.w = prm + L.w1; a.bias = prm + L.b1; a.out = wsf + ws.h1;
  hipLaunchKernelGGL((k_ma_conv<2 * C, HID, MA_RELU>), grid, dim3(256), 0, s, a);
  MA_CHECK();
  a.in0 = wsf + ws.h1; a.in1 = nullptr; a.c0 = HID;
  a.w = prm + L.w2; a.bias = prm + L.b2; a.out = wsf + ws.h2;
  hipLaunchKernelGGL((k_ma_conv<HID, HID, MA_RELU>), grid, dim3(256), 0, s, a);
  MA_CHECK();
  return hipSuccess;
}

template <int C, int HID>
static hipError_t ma_fwd(const float* prm, const float* noisy, const float* base, const float* mem,
                         float* out, float* feat, int N, int H, int W, int nb, int clamp, float* wsf,
                         hipStream_t s) {
  const MaLayout L = ma_layout(C, HID, nb);
  const MaWs ws = ma_ws(N, C, H, W, HID, 0);
  const double* gtw = nullptr;
  if (nb > 0 && W > MA_WMAX) {
    double* tw = reinterpret_cast<double*>(wsf + ws.tw);
    hipLaunchKernelGGL(k_ma_twiddle, dim3((W + 255) / 256), dim3(256), 0, s, W, tw);
    MA_CHECK();
    gtw = tw;
  }
  hipLaunchKernelGGL(k_ma_stats, dim3(N, 3), dim3(256), 0, s, noisy, base, mem, C, H, W, nb, gtw,
                     feat);
  MA_CHECK();
  hipError_t e = ma_features_and_convs<C, HID>(prm, L, noisy, base, feat, N, H, W, wsf, ws, s);
  if (e != hipSuccess) return e;
  MaConvArgs a{};
  a.N = N; a.H = H; a.W = W;
  a.in0 = wsf + ws.h2; a.c0 = HID;
  a.w = prm + L.w3; a.bias = prm + L.b3; a.out = out;
  a.aux = base; a.gb = wsf + ws.gb; a.clamp = clamp;
  hipLaunchKernelGGL((k_ma_conv<HID, C, MA_FINAL>), dim3(ma_tiles(H, W), N), dim3(256), 0, s, a);
  return hipGetLastError();
}

// out (+)= the hyper route: dfd (doubles, MA_ADJ_DF per sample) or dff (floats, 2 + nb per sample)
// is the gradient at base_out's features; wsf regions tw, dfe.. of a mode-2 workspace
static hipError_t ma_adjoint(const float* base, const double* dfd, const float* dff, float* out,
                             int accumulate, int N, int C, int H, int W, int nb, float* wsf,
                             const MaWs& ws, hipStream_t s) {
  const MaAdj p = ma_adj_plan(N, C, H, W);
  const bool wide = W > MA_WMAX;
  double* tw = nullptr;
  if (nb > 0 && wide) {
    tw = reinterpret_cast<double*>(wsf + ws.tw);
    hipLaunchKernelGGL(k_ma_twiddle, dim3((W + 255) / 256), dim3(256), 0, s, W, tw);
    MA_CHECK();
  }
  double* coef = reinterpret_cast<double*>(wsf + ws.coef);
  double* pf = reinterpret_cast<double*>(wsf + ws.pf);
  double* apart = reinterpret_cast<double*>(wsf + ws.apart);
  double* gas = reinterpret_cast<double*>(wsf + ws.gas);
  const dim3 grid(p.G, N);
  if (wide) hipLaunchKernelGGL(k_ma_adj_power<true>, grid, dim3(256), 0, s, base, p, nb, tw, gas, apart);
  else hipLaunchKernelGGL(k_ma_adj_power<false>, grid, dim3(256), 0, s, base, p, nb, tw, gas, apart);
  MA_CHECK();
  hipLaunchKernelGGL(k_ma_adj_coef, dim3(N), dim3(256), 0, s, base, p, p.G, nb, apart, dfd, dff, pf,
                     coef);
  MA_CHECK();
  if (wide)
    hipLaunchKernelGGL(k_ma_adj_apply<true>, grid, dim3(256), 0, s, base, p, nb, tw, gas, coef, out,
                       accumulate);
  else
    hipLaunchKernelGGL(k_ma_adj_apply<false>, grid, dim3(256), 0, s, base, p, nb, tw, gas, coef, out,
                       accumulate);
  return hipGetLastError();
}

// dprm (nullable) = the parameter gradient; dbase (nullable) = dpre + the data gradient of
// local_net.0 into base_out's channels + the hyper route.  One shared chain; the launches that
// form dprm are the same with and without dbase.
template <int C, int HID>
static hipError_t ma_bwd(const float* prm, const float* noisy, const float* base, const float* feat,
                         const float* dout, float* dprm, float* dbase, int N, int H, int W, int nb,
                         int clamp, float* wsf, hipStream_t s) {
  const MaLayout L = ma_layout(C, HID, nb);
  const MaWs ws = ma_ws(N, C, H, W, HID, dbase ? 2 : 1);
  hipError_t e = ma_features_and_convs<C, HID>(prm, L, noisy, base, feat, N, H, W, wsf, ws, s);
  if (e != hipSuccess) return e;
  const int ntiles = ma_tiles(H, W), wgb = ma_wg_blocks(N, H, W);
  const dim3 grid(ntiles, N);
  double* part = reinterpret_cast<double*>(wsf + ws.part);
  float* slab = wsf + ws.slab;
  MaConvArgs a{};
  a.N = N; a.H = H; a.W = W;
  // r, pre, dpre; dr and the (gamma, beta) sums; dpre itself opens dbase
  a.in0 = wsf + ws.h2; a.c0 = HID;
  a.w = prm + L.w3; a.bias = prm + L.b3; a.out = wsf + ws.dr;
  a.aux = base; a.gb = wsf + ws.gb; a.dout = dout; a.part = part; a.clamp = clamp;
  a.dpre = dbase;
  hipLaunchKernelGGL((k_ma_conv<HID, C, MA_DFINAL>), grid, dim3(256), 0, s, a);
  MA_CHECK();
  if (dprm) {
    hipLaunchKernelGGL(k_ma_hyper_bwd, dim3(1), dim3(256), 0, s, prm, L, feat, wsf + ws.gb, part,
                       ntiles, N, C, HID, dprm);
    MA_CHECK();
  }
  // layer 3: weights from (dr, h2), then the gradient into h2's pre-activation
  constexpr int ROW3 = C * HID * 9 + C, ROW2 = HID * HID * 9 + HID, ROW1 = HID * 2 * C * 9 + HID;
  if (dprm) {
    hipLaunchKernelGGL((k_ma_wgrad<HID, C>), dim3(wgb), dim3(256), 0, s, a, wsf + ws.dr, slab);
    MA_CHECK();
    hipLaunchKernelGGL(k_ma_reduce, dim3((ROW3 + 255) / 256), dim3(256), 0, s, slab, ROW3, wgb, dprm + L.w3);
    MA_CHECK();
  }
  MaConvArgs t{};
  t.N = N; t.H = H; t.W = W;
  t.in0 = wsf + ws.dr; t.c0 = C; t.w = prm + L.w3; t.aux = wsf + ws.h2; t.out = wsf + ws.g2;
  hipLaunchKernelGGL((k_ma_conv<C, HID, MA_MASKT>), grid, dim3(256), 0, s, t);
  MA_CHECK();
  // layer 2
  a.in0 = wsf + ws.h1; a.c0 = HID;
  if (dprm) {
    hipLaunchKernelGGL((k_ma_wgrad<HID, HID>), dim3(wgb), dim3(256), 0, s, a, wsf + ws.g2, slab);
    MA_CHECK();
    hipLaunchKernelGGL(k_ma_reduce, dim3((ROW2 + 255) / 256), dim3(256), 0, s, slab, ROW2, wgb, dprm + L.w2);
    MA_CHECK();
  }
  t.in0 = wsf + ws.g2; t.c0 = HID; t.w = prm + L.w2; t.aux = wsf + ws.h1; t.out = wsf + ws.g1;
  hipLaunchKernelGGL((k_ma_conv<HID, HID, MA_MASKT>), grid, dim3(256), 0, s, t);
  MA_CHECK();
  // layer 1
  if (dprm) {
    a.in0 = noisy; a.in1 = base; a.c0 = C;
    hipLaunchKernelGGL((k_ma_wgrad<2 * C, HID>), dim3(wgb), dim3(256), 0, s, a, wsf + ws.g1, slab);
    MA_CHECK();
    hipLaunchKernelGGL(k_ma_reduce, dim3((ROW1 + 255) / 256), dim3(256), 0, s, slab, ROW1, wgb, dprm + L.w1);
    MA_CHECK();
  }
  if (!dbase) return hipSuccess;
  // dbase += g1 through local_net.0's base_out channels (transposed, taps reversed, no mask)
  t.in0 = wsf + ws.g1; t.c0 = HID; t.w = prm + L.w1; t.aux = nullptr; t.out = dbase;
  hipLaunchKernelGGL((k_ma_conv<HID, C, MA_DINT>), grid, dim3(256), 0, s, t);
  MA_CHECK();
  // dbase += the hyper route
  double* dfe = reinterpret_cast<double*>(wsf + ws.dfe);
  hipLaunchKernelGGL(k_ma_hyper_dfeat, dim3(N), dim3(64), 0, s, prm, L, feat, wsf + ws.gb, part,
                     ntiles, C, HID, nb, dfe);
  MA_CHECK();
  return ma_adjoint(base, dfe, nullptr, dbase, 1, N, C, H, W, nb, wsf, ws, s);
}

#define MA_DISPATCH(fn, ...)                                  \
  do {                                                        \
    if (C == 1 && HID == 16) return fn<1, 16>(__VA_ARGS__);   \
    if (C == 3 && HID == 16) return fn<3, 16>(__VA_ARGS__);   \
    if (C == 1 && HID == 8) return fn<1, 8>(__VA_ARGS__);     \
    if (C == 3 && HID == 8) return fn<3, 8>(__VA_ARGS__);     \
    return hipErrorInvalidValue;                              \
  } while (0)

hipError_t launch_memadapter_fwd(const float* prm, const float* noisy, const float* base,
                                 const float* mem, float* out, float* feat, int N, int C, int H,
                                 int W, int HID, int nb, int clamp, void* ws, hipStream_t s) {
  MA_DISPATCH(ma_fwd, prm, noisy, base, mem, out, feat, N, H, W, nb, clamp, static_cast<float*>(ws), s);
}

hipError_t launch_memadapter_bwd(const float* prm, const float* noisy, const float* base,
                                 const float* feat, const float* dout, float* dprm, float* dbase,
                                 int N, int C, int H, int W, int HID, int nb, int clamp, void* ws,
                                 hipStream_t s) {
  MA_DISPATCH(ma_bwd, prm, noisy, base, feat, dout, dprm, dbase, N, H, W, nb, clamp,
              static_cast<float*>(ws), s);
}

hipError_t launch_memadapter_feature_adjoint(const float* base, const float* dfeat, float* hyper,
                                             int N, int C, int H, int W, int nb, void* ws,
                                             hipStream_t s) {
  const MaWs w = ma_ws(N, C, H, W, 8, 2);
  return ma_adjoint(base, nullptr, dfeat, hyper, 0, N, C, H, W, nb, static_cast<float*>(ws), w, s);
}

// ---- Hann-window blend of patchwise inference ------------------------------------------------------
// out[c][y][x] = sum_k pred_k * w / (sum_k w + 1e-8) over the patches k = iy * nx + ix that cover
// the pixel, in that order (the order the reference adds them), w = max(hann[py] * hann[px], 1e-3)
__global__ __launch_bounds__(256) void k_hann_blend(const float* __restrict__ pred,
                                                    const float* __restrict__ hann,
                                                    const int* __restrict__ ys,
                                                    const int* __restrict__ xs, int ny, int nx, int C,
                                                    int H, int W, int P, float* __restrict__ out) {
  const long total = (long)C * H * W;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int x = (int)(e % W), y = (int)((e / W) % H), c = (int)(e / ((long)W * H));
    float acc = 0.f, wsum = 0.f;
    for (int iy = 0; iy < ny; ++iy) {
      const int py = y - ys[iy];
      if (py < 0 || py >= P) continue;
      for (int ix = 0; ix < nx; ++ix) {
        const int px = x - xs[ix];
        if (px < 0 || px >= P) continue;
        const float w = fmaxf(__fmul_rn(hann[py], hann[px]), 1e-3f);
        const float v = pred[(((long)(iy * nx + ix) * C + c) * P + py) * P + px];
        acc = __fadd_rn(acc, __fmul_rn(v, w));
        wsum = __fadd_rn(wsum, w);
      }
    }
    out[e] = __fdiv_rn(acc, __fadd_rn(wsum, 1e-8f));
  }
}

hipError_t launch_hann_blend(const float* pred, const float* hann, const int* ys, const int* xs,
                             int ny, int nx, int C, int H, int W, int P, float* out, hipStream_t s) {
  const long total = (long)C * H * W;
  const int nb = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_hann_blend, dim3(nb), dim3(256), 0, s, pred, hann, ys, xs, ny, nx, C, H, W, P,
                     out);
  return hipGetLastError();
}

}  // namespace dn
