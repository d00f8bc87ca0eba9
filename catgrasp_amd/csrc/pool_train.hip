// Training form of PointNet's pooled layer conv(k = 1) + BatchNorm (batch statistics) + [ReLU] + max over the points, in closed form
// (catgrasp_amd/include/catgrasp_amd_pool.h has the contract; catgrasp_amd/pool_autograd.py assembles the layer).  The (rows, c)
// activation z = x . W^T + bias is never stored: BatchNorm is monotone per channel, so the pooled output needs only the extremum of z
// per (cloud, channel) and where it is; the mean of z follows from the column mean of x, and its variance comes from a second sweep of
// the same tiles that sums (z - mean)^2 (or, without a sweep and less accurately, from the centred Gram matrix of x).
//
// Extrema.  The tile body of gemm.hip's gemm_bias_act_kernel (64 rows x 128 channels per step, x staged in LDS, W read in pack_b
// order, v_mfma_f32_32x32x2_f32) with another epilogue: a workgroup owns a chunk of CG_POOL_ROWS consecutive points of ONE cloud and
// 128 channels, its wave w the 32 channels of block 4 blockIdx.y + w.  A lane holds column lane & 31 of every 32 x 32 tile, 16 rows of
// it in ascending order, and keeps (max, argmax, min, argmin) of its column in four registers across the tiles of the chunk: strict
// comparisons over ascending rows keep the first occurrence.  The two half-waves are joined with one shuffle (equal values: the
// smaller row), and one partial per (chunk, channel) goes to the workspace.  Rows of the last tile past the cloud's end are loaded
// from the cloud's last row (in bounds) and masked out of the fold.  The second launch reduces the chunks of a cloud in ascending order.
//
// Variance sweep.  The same kernel with the fold sq = fmaf(d, d, sq), d = (acc + bias) - mean: one chain per lane over its rows of the
// chunk, the two half-waves added (lower + upper), one partial per (chunk, channel), the partials summed in ascending order.
//
// Statistics.  One wave per 64 channels, one lane per channel, its row of W in LDS (stride 129: conflict-free); xbar and s are read at
// wave-uniform addresses.
//
// Gather / scatter.  The sparse terms of the weight and the input gradient: per (cloud, channel) one selected row.
#include <limits.h>
#include <math.h>
#include "cg_common.hpp"
#include "../include/catgrasp_amd_pool.h"

namespace {

constexpr int PR = CG_POOL_ROWS;
constexpr int BM = 64;                      // rows per step: two 32-row MFMA tiles
constexpr int MAXK = CG_POOL_MAX_CIN;
constexpr long MAX_ROWS = 1L << 24;
static_assert(PR % BM == 0, "a chunk is a whole number of steps");

struct Ext { float vmax, vmin; int imax, imin; };

// fold the 32 x 32 tile c (rows t .. t + 31 of the chunk, this lane's column) into e; rows >= rows take no part
__device__ __forceinline__ void fold_tile(const f32x16& c, int t, int rows, float bias, int lane, Ext& e) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = t + acc_row(r, lane);
    const float v = c[r] + bias;
    if (i < rows) {
      if (v > e.vmax) { e.vmax = v; e.imax = i; }
      if (v < e.vmin) { e.vmin = v; e.imin = i; }
    }
  }
}

// the variance sweep's fold: sq = fmaf(d, d, sq) with d = (c[r] + bias) - mean over this lane's rows of the tile, ascending
__device__ __forceinline__ void fold_sq(const f32x16& c, int t, int rows, float bias, float mean, int lane, float& sq) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float d = (c[r] + bias) - mean;
    if (t + acc_row(r, lane) < rows) sq = fmaf(d, d, sq);
  }
}

// VAR = false: ws is four planes of parts * c words: max, argmax, min, argmin; part = cloud * cpc + chunk.
// VAR = true (the second sweep): ws is one plane, the chunk's sum of (z - mean)^2 per channel.
template <bool VAR>
__global__ __launch_bounds__(256) void pool_extrema_kernel(const float* __restrict__ x, long n, long cpc, int K, const float* __restrict__ wp,
                                                           const float* __restrict__ bias, int c, const float* __restrict__ mean,
                                                           float* __restrict__ ws, long parts) {
  __shared__ __attribute__((aligned(16))) float xs[BM * (MAXK + 4)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const long cloud = blockIdx.x / cpc, chunk = blockIdx.x - cloud * cpc;
  const long n0 = chunk * PR;
  const int rows = (int)min((long)PR, n - n0);                  // >= 1
  const float* xc = x + (size_t)(cloud * n + n0) * K;
  const int nb = blockIdx.y * 4 + w;
  const bool active = nb < c / 32;                              // wave-uniform
  const int SA = K + 4, kq = K / 4, nks = K / 8;
  const int col = nb * 32 + l31;
  const float bv0 = (active && bias) ? bias[col] : 0.f;
  Ext e = {-INFINITY, INFINITY, INT_MAX, INT_MAX};
  const float mu = (VAR && active) ? mean[col] : 0.f;
  float sq = 0.f;
  for (int t0 = 0; t0 < rows; t0 += BM) {
    __syncthreads();
    for (int i = tid; i < BM * kq; i += 256) {
      const int r = i / kq, cq = i - r * kq;
      const int row = min(t0 + r, rows - 1);                    // clamped inside the cloud; masked in the fold
      *(f32x4*)(xs + r * SA + cq * 4) = *(const f32x4*)(xc + (size_t)row * K + cq * 4);
    }
    __syncthreads();
    if (active) {
      f32x16 c0 = {0}, c1 = {0};
      const f32x4* bp = (const f32x4*)wp + (size_t)nb * nks * 64 + lane;
      const float* ar0 = xs + l31 * SA + lhi * 4;
      const float* ar1 = ar0 + 32 * SA;
      for (int ks = 0; ks < nks; ++ks) {
        const f32x4 bv = bp[ks * 64];
        const f32x4 a0 = *(const f32x4*)(ar0 + ks * 8);
        const f32x4 a1 = *(const f32x4*)(ar1 + ks * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { c0 = mfma32(a0[j], bv[j], c0); c1 = mfma32(a1[j], bv[j], c1); }
      }
      if (VAR) {
        fold_sq(c0, t0, rows, bv0, mu, lane, sq);
        fold_sq(c1, t0 + 32, rows, bv0, mu, lane, sq);
      } else {
        fold_tile(c0, t0, rows, bv0, lane, e);
        fold_tile(c1, t0 + 32, rows, bv0, lane, e);
      }
    }
  }
  if (!active) return;
  if (VAR) {                                                    // lower half-wave's rows first, then the upper's
    const float hi = __shfl_xor(sq, 32);
    if (!lhi) ws[(size_t)blockIdx.x * c + col] = sq + hi;
    return;
  }
  {                                                             // the other half-wave holds the other rows of this column
    const float ov = __shfl_xor(e.vmax, 32), uv = __shfl_xor(e.vmin, 32);
    const int oi = __shfl_xor(e.imax, 32), ui = __shfl_xor(e.imin, 32);
    if (ov > e.vmax || (ov == e.vmax && oi < e.imax)) { e.vmax = ov; e.imax = oi; }
    if (uv < e.vmin || (uv == e.vmin && ui < e.imin)) { e.vmin = uv; e.imin = ui; }
  }
  if (lhi) return;
  const size_t plane = (size_t)parts * c, at = (size_t)blockIdx.x * c + col;
  ws[at] = e.vmax;
  ((int*)ws)[plane + at] = (int)n0 + e.imax;
  ws[2 * plane + at] = e.vmin;
  ((int*)ws)[3 * plane + at] = (int)n0 + e.imin;
}

__global__ __launch_bounds__(256) void pool_select_kernel(const float* __restrict__ ws, long clouds, long cpc, int c, const float* __restrict__ sign,
                                                          float* __restrict__ zsel, int* __restrict__ idx) {
  const long el = (long)blockIdx.x * 256 + threadIdx.x;
  if (el >= clouds * c) return;
  const long b = el / c;
  const int ch = (int)(el - b * c);
  const bool take_max = !sign || sign[ch] >= 0.f;
  const size_t plane = (size_t)clouds * cpc * c;
  const float* pv = ws + (take_max ? 0 : 2 * plane) + (size_t)b * cpc * c + ch;
  const int* pi = (const int*)ws + (take_max ? plane : 3 * plane) + (size_t)b * cpc * c + ch;
  float best = pv[0];
  int bi = pi[0];
  for (long k = 1; k < cpc; ++k) {
    const float v = pv[(size_t)k * c];
    if (take_max ? v > best : v < best) { best = v; bi = pi[(size_t)k * c]; }
  }
  zsel[el] = best;
  idx[el] = bi;
}

// var[ch] = (the chunk partials in ascending (cloud, chunk) order) / m, clamped at 0
__global__ __launch_bounds__(256) void pool_var_total_kernel(const float* __restrict__ ws, long parts, int c, float m, float* __restrict__ var) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  float t = ws[ch];
  for (long k = 1; k < parts; ++k) t = t + ws[(size_t)k * c + ch];
  var[ch] = fmaxf(t / m, 0.f);
}

constexpr int SW = MAXK + 1;

__global__ __launch_bounds__(64) void pool_stats_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ xbar,
                                                        const float* __restrict__ s, const float* __restrict__ var_in, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, long clouds, float m, int cin, int c, const float* __restrict__ zsel, int relu,
                                                        float* __restrict__ mean_o, float* __restrict__ var_o, float* __restrict__ invstd_o,
                                                        float* __restrict__ scale_o, float* __restrict__ shift_o, float* __restrict__ out) {
  __shared__ float sw[64 * SW];
  const int lane = threadIdx.x, ch0 = blockIdx.x * 64;
  for (int i = lane; i < 64 * cin; i += 64) {
    const int r = i / cin, k = i - r * cin;
    sw[r * SW + k] = ch0 + r < c ? w[(size_t)(ch0 + r) * cin + k] : 0.f;
  }
  __syncthreads();
  const int ch = ch0 + lane;
  if (ch >= c) return;
  const float* wr = sw + lane * SW;
  float p = 0.f;
  for (int k = 0; k < cin; ++k) p = fmaf(wr[k], xbar[k], p);
  const float mean = p + (bias ? bias[ch] : 0.f);
  mean_o[ch] = mean;
  if (!var_in && !s) return;                                    // the mean alone: what the variance sweep needs
  float var;
  if (var_in) {
    var = var_in[ch];
  } else {
    float q = 0.f;
    for (int j = 0; j < cin; ++j) {
      float t = 0.f;
#pragma unroll 8
      for (int k = 0; k < cin; ++k) t = fmaf(wr[k], s[(size_t)k * cin + j], t);
      q = fmaf(t, wr[j], q);
    }
    var = fmaxf(q / m, 0.f);
  }
  const float invstd = 1.f / sqrtf(var + eps);
  const float scale = gamma[ch] * invstd;
  const float shift = beta[ch] - mean * scale;
  var_o[ch] = var; invstd_o[ch] = invstd; scale_o[ch] = scale; shift_o[ch] = shift;
  for (long b = 0; b < clouds; ++b) {
    const float v = zsel[(size_t)b * c + ch] * scale + shift;
    out[(size_t)b * c + ch] = relu ? fmaxf(v, 0.f) : v;
  }
}

__global__ __launch_bounds__(256) void pool_gather_kernel(const float* __restrict__ x, long clouds, long n, int cin, const float* __restrict__ coef,
                                                          const int* __restrict__ idx, int c, float* __restrict__ t) {
  const long el = (long)blockIdx.x * 256 + threadIdx.x;
  if (el >= (long)c * cin) return;
  const int ch = (int)(el / cin), k = (int)(el - (long)ch * cin);
  float p = 0.f;
  for (long b = 0; b < clouds; ++b) {
    const int i = idx[(size_t)b * c + ch];
    if (i < 0 || i >= n) continue;
    p = fmaf(coef[(size_t)b * c + ch], x[((size_t)b * n + i) * cin + k], p);
  }
  t[el] = p;
}

// one workgroup per cloud; wave w visits the channels w, w + 4, ...; the first channel that selects a row owns the row's whole chain
__global__ __launch_bounds__(256) void pool_scatter_kernel(const float* __restrict__ coef, const int* __restrict__ idx, const float* __restrict__ w,
                                                           long n, int cin, int c, float* __restrict__ dx) {
  __shared__ int sidx[CG_POOL_MAX_C];
  __shared__ float scoef[CG_POOL_MAX_C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  for (int i = tid; i < c; i += 256) { sidx[i] = idx[(size_t)b * c + i]; scoef[i] = coef[(size_t)b * c + i]; }
  __syncthreads();
  for (int ch = wave; ch < c; ch += 4) {                        // wave-uniform
    const int row = sidx[ch];
    if (row < 0 || row >= n) continue;
    bool owner = true;
    for (int base = 0; base < ch && owner; base += 64) {
      const int c2 = base + lane;
      if (__any(c2 < ch && sidx[c2] == row)) owner = false;
    }
    if (!owner) continue;
    float* drow = dx + ((size_t)b * n + row) * cin;
    float a0 = lane < cin ? drow[lane] : 0.f;
    float a1 = lane + 64 < cin ? drow[lane + 64] : 0.f;
    for (int base = ch & ~63; base < c; base += 64) {
      const int c2 = base + lane;
      unsigned long long hits = __ballot(c2 >= ch && c2 < c && sidx[c2] == row);
      while (hits) {
        const int o = base + __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const float f = scoef[o];
        if (lane < cin) a0 = fmaf(f, w[(size_t)o * cin + lane], a0);
        if (lane + 64 < cin) a1 = fmaf(f, w[(size_t)o * cin + lane + 64], a1);
      }
    }
    if (lane < cin) drow[lane] = a0;
    if (lane + 64 < cin) drow[lane + 64] = a1;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_counts(long clouds, long n) {
  if (clouds < 1 || n < 1 || clouds > MAX_ROWS || n > MAX_ROWS || clouds * n > MAX_ROWS || clouds * n < 2) return CG_ERR_ARG;
  return CG_OK;
}

int check_shape(long clouds, long n, int cin, int c) {
  if (check_counts(clouds, n) != CG_OK || cin <= 0 || c <= 0) return CG_ERR_ARG;
  if (cin % 8 != 0 || cin > CG_POOL_MAX_CIN || c % 32 != 0 || c > CG_POOL_MAX_C) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

}  // namespace

extern "C" long cg_pool_extrema_workspace(long clouds, long n, int c) {
  const int st = check_shape(clouds, n, 8, c);
  if (st != CG_OK) return st;
  return 4 * clouds * ((n + PR - 1) / PR) * c;
}

extern "C" int cg_pool_extrema(const float* x, long clouds, long n, int cin, const float* w_packed, const float* bias, int c, const float* sign,
                               float* workspace, float* zsel, int* idx, void* stream) {
  const int st = check_shape(clouds, n, cin, c);
  if (st != CG_OK) return st;
  if (!x || !w_packed || !workspace || !zsel || !idx || !aligned16(x) || !aligned16(w_packed)) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long cpc = (n + PR - 1) / PR, parts = clouds * cpc;     // parts <= 2^24
  hipLaunchKernelGGL(pool_extrema_kernel<false>, dim3((unsigned)parts, (unsigned)((c / 32 + 3) / 4)), dim3(256), 0, s, x, n, cpc, cin, w_packed, bias, c,
                     (const float*)nullptr, workspace, parts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pool_select_kernel, dim3((unsigned)((clouds * c + 255) / 256)), dim3(256), 0, s, (const float*)workspace, clouds, cpc, c, sign,
                     zsel, idx);
  return cg_hip_status(hipGetLastError());
}

extern "C" long cg_pool_var_workspace(long clouds, long n, int c) {
  const int st = check_shape(clouds, n, 8, c);
  if (st != CG_OK) return st;
  return clouds * ((n + PR - 1) / PR) * c;
}

extern "C" int cg_pool_var(const float* x, long clouds, long n, int cin, const float* w_packed, const float* bias, int c, const float* mean,
                           float* workspace, float* var, void* stream) {
  const int st = check_shape(clouds, n, cin, c);
  if (st != CG_OK) return st;
  if (!x || !w_packed || !mean || !workspace || !var || !aligned16(x) || !aligned16(w_packed)) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long cpc = (n + PR - 1) / PR, parts = clouds * cpc;
  hipLaunchKernelGGL(pool_extrema_kernel<true>, dim3((unsigned)parts, (unsigned)((c / 32 + 3) / 4)), dim3(256), 0, s, x, n, cpc, cin, w_packed, bias, c,
                     mean, workspace, parts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pool_var_total_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s, (const float*)workspace, parts, c, (float)(clouds * n), var);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_pool_stats(const float* w, const float* bias, const float* xbar, const float* sm, const float* var_in, const float* gamma,
                             const float* beta, float eps,
                             long clouds, long n, int cin, int c, const float* zsel, int relu, float* mean, float* var, float* invstd, float* scale,
                             float* shift, float* out, void* stream) {
  const int st = check_shape(clouds, n, cin, c);
  if (st != CG_OK) return st;
  if (!w || !xbar || !mean) return CG_ERR_ARG;
  if ((sm || var_in) && (!gamma || !beta || !zsel || !var || !invstd || !scale || !shift || !out)) return CG_ERR_ARG;
  hipLaunchKernelGGL(pool_stats_kernel, dim3((unsigned)((c + 63) / 64)), dim3(64), 0, (hipStream_t)stream, w, bias, xbar, sm, var_in, gamma, beta, eps, clouds,
                     (float)(clouds * n), cin, c, zsel, relu, mean, var, invstd, scale, shift, out);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_pool_wgrad_gather(const float* x, long clouds, long n, int cin, const float* coef, const int* idx, int c, float* t, void* stream) {
  const int st = check_shape(clouds, n, cin, c);
  if (st != CG_OK) return st;
  if (!x || !coef || !idx || !t) return CG_ERR_ARG;
  hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)(((long)c * cin + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, clouds, n, cin, coef, idx, c, t);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_pool_dgrad_scatter(const float* coef, const int* idx, const float* w, long clouds, long n, int cin, int c, float* dx, void* stream) {
  const int st = check_shape(clouds, n, cin, c);
  if (st != CG_OK) return st;
  if (!coef || !idx || !w || !dx) return CG_ERR_ARG;
  hipLaunchKernelGGL(pool_scatter_kernel, dim3((unsigned)clouds), dim3(256), 0, (hipStream_t)stream, coef, idx, w, n, cin, c, dx);
  return cg_hip_status(hipGetLastError());
}
