// The NUNOCS training objective: cross-entropy over coordinate bins, minimised over the category's symmetries, forward and backward
// (include/catgrasp_amd_loss.h has the contract: the bin chain, the order of every sum and the tree of the row sums, so the results
// are a function of the values and the shapes alone).  f32; no sum is left to arrival order.  Nothing of size n_sym x logits exists: per (point, axis)
// one log-sum-exp, per (point, axis, symmetry) one gathered logit.
//
// One workgroup of 4 waves per (sample, segment of CG_NOCS_SEG points) in every kernel that touches the logits; the decomposition
// inside follows the storage, so that a wave's loads and stores are 256-byte runs:
//
//   channel-major (B, 3*bins, N)   lanes over the segment's 64 points, the 4 waves over the rows k = w, w + 4, ... of one axis at a
//       forward  nocs_fwd_cm_kernel  time.  A wave puts its rows into an LDS tile [bins][64] (max on the way, then the sum of exp from
//                                    the tile) and has the next axis' rows in flight meanwhile; the partial max and sum of the waves meet in LDS.  The gather x_a[k_a] of a
//                                    (point, symmetry) is an LDS read at [k][lane]: the bank is the lane, whatever k is.  The waves
//                                    split the symmetries (s = w, w + 4, ...; tfs[s] is wave-uniform) and sum v over the 3 axes in LDS.
//       backward nocs_bwd_cm_kernel  the same lanes and rows; bins and lse of a lane's point are formed once.
//   point-major (B, N, 3*bins)     lanes over the bins (k = lane, lane + 64) of one point, the 4 waves over the points i = w, w + 4,
//       forward  nocs_fwd_pm_kernel  ...; max and sum by xor butterflies, the three axes interleaved.  For the gathers the lanes turn
//                                    to the symmetries (s = lane, lane + 64, their tfs rows in registers) and re-read three logits of
//                                    the row the wave has just loaded.  The next point's row is loaded before this one is reduced.
//       backward nocs_bwd_pm_kernel  the segment's rows are one contiguous run: a flat float4 sweep, the points' bins and lse in LDS.
//
// Both forwards leave v[s][point] in LDS (row stride 65: thread s reads its row conflict-free) and thread s runs the segment's chain
// and writes the partial to the workspace (ws[(sample, segment, s)]).  nocs_rows_kernel (one workgroup per sample) adds the segment
// partials in ascending order, divides by N and takes the first arg-min; nocs_mean_kernel runs the chain over the samples.
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_loss.h"

namespace {

constexpr int SEG = CG_NOCS_SEG, MAX_BINS = CG_NOCS_MAX_BINS, MAX_SYM = CG_NOCS_MAX_SYM, WAVES = 4, LANES = 64;
constexpr int ROWS_PER_WAVE = MAX_BINS / WAVES;
constexpr int VLD = SEG + 1;                      // row stride of v[s][point] in LDS
constexpr long MAX_N = 1L << 24;
static_assert(SEG == LANES && MAX_BINS <= 2 * LANES && MAX_SYM <= 2 * LANES, "one lane per point; two bins and two symmetries per lane");

// bin of one axis: T = row a of tfs[s] (rotation, then translation), c = target - 0.5f
__device__ __forceinline__ int bin_of(const float* __restrict__ T, float c0, float c1, float c2, int bins) {
  const float r = fmaf(T[2], c2, fmaf(T[1], c1, fmaf(T[0], c0, T[3]))) + 0.5f;
  const float q = r * (float)bins;
  return (int)fminf(fmaxf(q, 0.0f), (float)(bins - 1));
}

// v[s][0 .. cnt) in LDS -> the segment partial of symmetry s = threadIdx.x: one chain from +0, ascending
__device__ __forceinline__ void store_segment_partial(const float* __restrict__ v, int S, int cnt, float* __restrict__ out) {
  const int s = threadIdx.x;
  if (s < S) {
    float p = 0.f;
    for (int i = 0; i < cnt; ++i) p = p + v[s * VLD + i];
    out[s] = p;
  }
}

// dynamic LDS of the channel-major forward, in floats: the tile [bins][64], v [S][65], the waves' partial max and sum [2][4][64]
__host__ __device__ constexpr int cm_lds_floats(int bins, int S) { return bins * SEG + S * VLD + 2 * WAVES * LANES; }

__global__ __launch_bounds__(WAVES * LANES) void nocs_fwd_cm_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                   const float* __restrict__ tfs, long N, int bins, int S, long nseg,
                                                                   float* __restrict__ ws, float* __restrict__ lse_out) {
  extern __shared__ float lds[];
  float* tile = lds;                              // [bins][64] logits of one axis
  float* v = tile + bins * SEG;                   // [S][65], summed over the axes in place
  float* part_m = v + S * VLD;                    // [4][64]
  float* part_s = part_m + WAVES * LANES;         // [4][64]
  // w in a scalar register: the 32 row addresses of load_axis are then scalar too (as vector registers they cost 64 of them and the
  // kernel spilt to scratch).  The compiler still holds more scalars than it has registers for: 143 of them spill to the lanes of
  // vector registers (v_writelane / v_readlane), none to scratch.
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long b = blockIdx.y, seg = blockIdx.x, n0 = seg * SEG, n = n0 + lane;
  const bool live = n < N;
  const int col = live ? lane : (int)(N - 1 - n0);   // a lane past the end reads the last point again: no per-row lane mask, nothing used
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if (live) {
    const float* t = target + (b * N + n) * 3;
    c0 = t[0] - 0.5f, c1 = t[1] - 0.5f, c2 = t[2] - 0.5f;
  }
  // a wave's rows of one axis: up to ROWS_PER_WAVE loads in flight per lane, issued one axis ahead of their use
  float xv[ROWS_PER_WAVE];
  auto load_axis = [&](int a) {
    const float* xa = pred + (b * 3 * bins + (long)a * bins + w) * N + n0;          // wave-uniform; the lane adds its own 4 bytes
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) xv[i] = w + WAVES * i < bins ? xa[(long)(WAVES * i) * N + col] : 0.f;
  };
  load_axis(0);
  for (int a = 0; a < 3; ++a) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
      const int k = w + WAVES * i;
      if (k < bins) {
        tile[k * SEG + lane] = xv[i];
        m = fmaxf(m, xv[i]);
      }
    }
    if (a < 2) load_axis(a + 1);
    part_m[w * LANES + lane] = m;
    __syncthreads();
    m = fmaxf(fmaxf(part_m[lane], part_m[LANES + lane]), fmaxf(part_m[2 * LANES + lane], part_m[3 * LANES + lane]));
    float p = 0.f;
#pragma unroll 4
    for (int k = w; k < bins; k += WAVES) p = p + expf(tile[k * SEG + lane] - m);
    part_s[w * LANES + lane] = p;
    __syncthreads();
    const float lse = m + logf((part_s[lane] + part_s[LANES + lane]) + (part_s[2 * LANES + lane] + part_s[3 * LANES + lane]));
    if (w == 0 && live && lse_out) lse_out[(b * N + n) * 3 + a] = lse;
#pragma unroll 4
    for (int s = w; s < S; s += WAVES) {          // this wave's own v entries: no other wave touches them
      const float d = lse - tile[bin_of(tfs + s * 16 + a * 4, c0, c1, c2, bins) * SEG + lane];
      v[s * VLD + lane] = a == 0 ? d : v[s * VLD + lane] + d;
    }
    __syncthreads();                              // the tile and the partials are rewritten by the next axis; v is read below
  }
  const long left = N - n0;
  store_segment_partial(v, S, (int)(left < SEG ? left : SEG), ws + (b * nseg + seg) * S);
}

// the two logits of a lane (k = lane, lane + 64) on each axis of one point's row; a k past the end reads nothing and is -inf
struct Row { float lo[3], hi[3]; };
__device__ __forceinline__ Row load_row(const float* __restrict__ x, int bins, int lane) {
  Row r;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.lo[a] = lane < bins ? x[a * bins + lane] : -INFINITY;
    r.hi[a] = lane + LANES < bins ? x[a * bins + lane + LANES] : -INFINITY;
  }
  return r;
}

__global__ __launch_bounds__(WAVES * LANES) void nocs_fwd_pm_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                   const float* __restrict__ tfs, long N, int bins, int S, long nseg,
                                                                   float* __restrict__ ws, float* __restrict__ lse_out) {
  extern __shared__ float v[];                    // [S][65]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long b = blockIdx.y, seg = blockIdx.x, n0 = seg * SEG;
  const long left = N - n0;
  const int cnt = (int)(left < SEG ? left : SEG), C = 3 * bins;
  float T[2][12];                                 // rows 0..2 of tfs[lane] and of tfs[lane + 64]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 12; ++i) T[h][i] = lane + LANES * h < S ? tfs[(lane + LANES * h) * 16 + i] : 0.f;
  const float* xs = pred + (b * N + n0) * C;
  Row next = load_row(xs + (long)(w < cnt ? w : 0) * C, bins, lane);
  for (int i = w; i < cnt; i += WAVES) {
    const Row r = next;
    if (i + WAVES < cnt) next = load_row(xs + (long)(i + WAVES) * C, bins, lane);
    const float* x = xs + (long)i * C;
    const float* t = target + (b * N + n0 + i) * 3;
    const float c0 = t[0] - 0.5f, c1 = t[1] - 0.5f, c2 = t[2] - 0.5f;
    float m[3], u[3], lse[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = fmaxf(r.lo[a], r.hi[a]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] = fmaxf(m[a], __shfl_xor(m[a], d));
#pragma unroll
    for (int a = 0; a < 3; ++a)
      u[a] = (lane < bins ? expf(r.lo[a] - m[a]) : 0.f) + (lane + LANES < bins ? expf(r.hi[a] - m[a]) : 0.f);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
      for (int a = 0; a < 3; ++a) u[a] = u[a] + __shfl_xor(u[a], d);
#pragma unroll
    for (int a = 0; a < 3; ++a) lse[a] = m[a] + logf(u[a]);
    if (lane < 3 && lse_out) lse_out[(b * N + n0 + i) * 3 + lane] = lane == 0 ? lse[0] : lane == 1 ? lse[1] : lse[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int s = lane + LANES * h;
      if (s < S) {
        const float d0 = lse[0] - x[bin_of(T[h], c0, c1, c2, bins)];
        const float d1 = lse[1] - x[bins + bin_of(T[h] + 4, c0, c1, c2, bins)];
        const float d2 = lse[2] - x[2 * bins + bin_of(T[h] + 8, c0, c1, c2, bins)];
        v[s * VLD + i] = (d0 + d1) + d2;
      }
    }
  }
  __syncthreads();
  store_segment_partial(v, S, cnt, ws + (b * nseg + seg) * S);
}

// L[b, :] from the segment partials, and the first arg-min
__global__ __launch_bounds__(MAX_SYM) void nocs_rows_kernel(const float* __restrict__ ws, long N, int S, long nseg, float* __restrict__ L,
                                                           int* __restrict__ ids) {
  __shared__ float row[MAX_SYM];
  const long b = blockIdx.x;
  const int s = threadIdx.x;
  if (s < S) {
    const float* p = ws + b * nseg * S + s;
    float t = p[0];
    for (long g = 1; g < nseg; ++g) t = t + p[g * S];
    row[s] = L[b * S + s] = t / (float)N;
  }
  __syncthreads();
  if (s == 0) {
    int best = 0;
    for (int k = 1; k < S; ++k)
      if (row[k] < row[best]) best = k;
    ids[b] = best;
  }
}

// loss = (chain over the samples of L[b, ids[b]]) / B: the loads in parallel, 256 samples at a time, the chain by thread 0
__global__ __launch_bounds__(256) void nocs_mean_kernel(const float* __restrict__ L, const int* __restrict__ ids, long B, int S,
                                                       float* __restrict__ loss) {
  __shared__ float val[256];
  float p = 0.f;
  for (long b0 = 0; b0 < B; b0 += 256) {
    const long b = b0 + threadIdx.x;
    if (b < B) val[threadIdx.x] = L[b * S + ids[b]];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = (int)(B - b0 < 256 ? B - b0 : 256);
      for (int i = 0; i < cnt; ++i) p = p + val[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = p / (float)B;
}

// rows 0..2 of tfs[ids[b]]; an id outside [0, S) (never written by the forward) is clamped, so that nothing is read out of bounds
__device__ __forceinline__ const float* winner(const float* __restrict__ tfs, const int* __restrict__ ids, long b, int S) {
  int s = ids[b];
  s = s < 0 ? 0 : s >= S ? S - 1 : s;
  return tfs + s * 16;
}

__global__ __launch_bounds__(WAVES * LANES) void nocs_bwd_cm_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                   const float* __restrict__ tfs, const float* __restrict__ lse,
                                                                   const int* __restrict__ ids, const float* __restrict__ grad_loss, long B,
                                                                   long N, int bins, int S, float* __restrict__ grad) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long b = blockIdx.y, n = (long)blockIdx.x * SEG + lane;
  if (n >= N) return;
  const float coef = grad_loss[0] / ((float)B * (float)N);
  const float* T = winner(tfs, ids, b, S);
  const float* t = target + (b * N + n) * 3;
  const float c0 = t[0] - 0.5f, c1 = t[1] - 0.5f, c2 = t[2] - 0.5f;
  for (int a = 0; a < 3; ++a) {
    const int ka = bin_of(T + a * 4, c0, c1, c2, bins);
    const float la = lse[(b * N + n) * 3 + a];
    const long base = (b * 3 * bins + (long)a * bins) * N + n;
#pragma unroll 8
    for (int k = w; k < bins; k += WAVES)
      grad[base + (long)k * N] = coef * (expf(pred[base + (long)k * N] - la) - (k == ka ? 1.0f : 0.0f));
  }
}

// VEC: the segment's rows are one contiguous run of cnt * 3 * bins floats; with 3 * bins a multiple of 4 and 16-byte aligned pointers it is
// swept as float4 (a float4 never straddles two points), the bins and lse of the segment's points waiting in LDS.  Otherwise one float
// per lane.  The arithmetic per element is the same, so both give the same bits.
template <bool VEC>
__global__ __launch_bounds__(WAVES * LANES) void nocs_bwd_pm_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                   const float* __restrict__ tfs, const float* __restrict__ lse,
                                                                   const int* __restrict__ ids, const float* __restrict__ grad_loss, long B,
                                                                   long N, int bins, int S, float* __restrict__ grad) {
  __shared__ float lse_s[SEG * 3];
  __shared__ int bin_s[SEG * 3];
  const long b = blockIdx.y, n0 = (long)blockIdx.x * SEG;
  const long left = N - n0;
  const int cnt = (int)(left < SEG ? left : SEG), C = 3 * bins;
  const float coef = grad_loss[0] / ((float)B * (float)N);
  const float* T = winner(tfs, ids, b, S);
  if ((int)threadIdx.x < cnt * 3) {                // thread -> (point, axis)
    const int i = threadIdx.x / 3, a = threadIdx.x - 3 * i;
    const float* t = target + (b * N + n0 + i) * 3;
    bin_s[threadIdx.x] = bin_of(T + a * 4, t[0] - 0.5f, t[1] - 0.5f, t[2] - 0.5f, bins);
    lse_s[threadIdx.x] = lse[(b * N + n0) * 3 + threadIdx.x];
  }
  __syncthreads();
  const long base = (b * N + n0) * C;
  const int total = cnt * C;
  if (VEC) {
    const f32x4* src = (const f32x4*)(pred + base);
    f32x4* dst = (f32x4*)(grad + base);
#pragma unroll 4
    for (int f = threadIdx.x; f < total / 4; f += WAVES * LANES) {
      const f32x4 x = src[f];
      const int i = (4 * f) / C, c = 4 * f - i * C;
      f32x4 g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int a = (c + j) / bins, k = (c + j) - a * bins;
        g[j] = coef * (expf(x[j] - lse_s[3 * i + a]) - (k == bin_s[3 * i + a] ? 1.0f : 0.0f));
      }
      dst[f] = g;
    }
  } else {
    for (int e = threadIdx.x; e < total; e += WAVES * LANES) {
      const int i = e / C, c = e - i * C, a = c / bins, k = c - a * bins;
      grad[base + e] = coef * (expf(pred[base + e] - lse_s[3 * i + a]) - (k == bin_s[3 * i + a] ? 1.0f : 0.0f));
    }
  }
}

int check_shape(long B, long N, int bins, int S) {
  if (B < 1 || N < 1 || N > MAX_N || bins < 1 || S < 1) return CG_ERR_ARG;
  if (bins > MAX_BINS || S > MAX_SYM || B > 65535) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

}  // namespace

extern "C" long cg_nocs_symce_workspace_floats(long B, long N, int bins, int S) {
  const int st = check_shape(B, N, bins, S);
  if (st != CG_OK) return st;
  return B * ((N + SEG - 1) / SEG) * S;
}

extern "C" int cg_nocs_symce_forward(const float* pred, int layout, const float* target, const float* tfs, long B, long N, int bins, int S,
                                     float* workspace, float* loss, int* ids, float* L, float* lse, void* stream) {
  const int st = check_shape(B, N, bins, S);
  if (st != CG_OK) return st;
  if (layout != CG_NOCS_CHANNEL_MAJOR && layout != CG_NOCS_POINT_MAJOR) return CG_ERR_ARG;
  if (!pred || !target || !tfs || !workspace || !loss || !ids || !L) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long nseg = (N + SEG - 1) / SEG;
  const dim3 grid((unsigned)nseg, (unsigned)B), block(WAVES * LANES);
  if (layout == CG_NOCS_CHANNEL_MAJOR) {
    const size_t bytes = (size_t)cm_lds_floats(bins, S) * sizeof(float);
    if (bytes > 64 * 1024) {                      // only with bins and S both near their caps
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess) return CG_ERR_UNSUPPORTED;
      const int ok = cg_allow_dynamic_lds<nocs_fwd_cm_kernel>(dev, (size_t)cm_lds_floats(MAX_BINS, MAX_SYM) * sizeof(float));
      if (ok != CG_OK) return ok;
    }
    hipLaunchKernelGGL(nocs_fwd_cm_kernel, grid, block, bytes, s, pred, target, tfs, N, bins, S, nseg, workspace, lse);
  } else
    hipLaunchKernelGGL(nocs_fwd_pm_kernel, grid, block, (size_t)S * VLD * sizeof(float), s, pred, target, tfs, N, bins, S, nseg, workspace, lse);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nocs_rows_kernel, dim3((unsigned)B), dim3(MAX_SYM), 0, s, (const float*)workspace, N, S, nseg, L, ids);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(nocs_mean_kernel, dim3(1), dim3(256), 0, s, (const float*)L, (const int*)ids, B, S, loss);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_nocs_symce_backward(const float* pred, int layout, const float* target, const float* tfs, const float* lse, const int* ids,
                                      const float* grad_loss, long B, long N, int bins, int S, float* grad_pred, void* stream) {
  const int st = check_shape(B, N, bins, S);
  if (st != CG_OK) return st;
  if (layout != CG_NOCS_CHANNEL_MAJOR && layout != CG_NOCS_POINT_MAJOR) return CG_ERR_ARG;
  if (!pred || !target || !tfs || !lse || !ids || !grad_loss || !grad_pred) return CG_ERR_ARG;
  const dim3 grid((unsigned)((N + SEG - 1) / SEG), (unsigned)B), block(WAVES * LANES);
  if (layout == CG_NOCS_CHANNEL_MAJOR)
    hipLaunchKernelGGL(nocs_bwd_cm_kernel, grid, block, 0, (hipStream_t)stream, pred, target, tfs, lse, ids, grad_loss, B, N, bins, S, grad_pred);
  else if ((3 * bins) % 4 == 0 && (((uintptr_t)pred | (uintptr_t)grad_pred) & 15) == 0)
    hipLaunchKernelGGL(nocs_bwd_pm_kernel<true>, grid, block, 0, (hipStream_t)stream, pred, target, tfs, lse, ids, grad_loss, B, N, bins, S, grad_pred);
  else
    hipLaunchKernelGGL(nocs_bwd_pm_kernel<false>, grid, block, 0, (hipStream_t)stream, pred, target, tfs, lse, ids, grad_loss, B, N, bins, S, grad_pred);
  return cg_hip_status(hipGetLastError());
}
