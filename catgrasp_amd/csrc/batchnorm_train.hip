// BatchNorm in batch-statistics mode fused with ReLU, forward and backward (include/catgrasp_amd_bn.h has the contract: every
// per-channel sum is a stated tree of f32 chains -- 64-row segments, 1024-row chunks, chunks in ascending order -- so the results are
// a function of the values and n alone).  f32, no atomics.
//
// Every kernel has the same layout: one workgroup of 16 waves per (chunk of CG_BN_ROWS rows, 64 channels), one wave per segment of
// CG_BN_SEG rows, one lane per channel, so a row read is one 256-byte run (64 bytes at c = 16).  A lane runs the chain of its channel
// over its segment's rows; the 16 segment partials meet in LDS, wave 0 adds them in ascending order and writes the chunk partial to
// the workspace (ws[(sum, chunk, channel)]).  The pass that needs a total re-adds the chunk partials of its own 64 channels (wave 0,
// ascending, handed to the other waves through LDS) instead of a launch of its own: n / 1024 dependent adds per workgroup, a dozen
// at the network's sizes.
//
//   forward    bn_sum_kernel<SUM_X>   S(x)                     -> ws[0]
//              bn_sum_kernel<SUM_DD>  mean; S((x - mean)^2)    -> ws[1]
//              bn_apply_kernel        mean, var, invstd, scale, shift (chunk 0 writes them); y
//   backward   bn_sum_kernel<SUM_G>   S(g) -> ws[0], S(g*xhat) -> ws[1]
//              bn_dx_kernel           dbeta, dgamma (chunk 0 writes them); dx (one chunk of workgroups and no row work when dx is NULL)
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_bn.h"
#include "../include/catgrasp_amd_dense.h"

namespace {

constexpr int SEG = CG_BN_SEG, ROWS = CG_BN_ROWS, WAVES = ROWS / SEG, LANES = 64;
constexpr long MAX_N = 1L << 24;
constexpr int NARROW_C = 224;
static_assert(WAVES == 16 && SEG == 64, "one wave per segment, 16 waves per workgroup");

enum { SUM_X, SUM_DD, SUM_G };

// total of channel ch: the partial of chunk 0, then those of chunks 1, 2, ... added in ascending order
__device__ __forceinline__ float total_of(const float* __restrict__ part, long chunks, int c, int ch) {
  float t = part[ch];
  for (long k = 1; k < chunks; ++k) t = t + part[k * c + ch];
  return t;
}

struct Where { long chunk, row0; int rows, nseg, wave, lane, ch; bool live; };

// this thread's place: rows [row0, row0 + rows) of channel ch (rows <= 0: the segment lies past the end), nseg segments in the chunk
__device__ __forceinline__ Where where(long n, int c) {
  Where w;
  w.chunk = blockIdx.x;
  w.wave = threadIdx.x >> 6, w.lane = threadIdx.x & 63;
  w.ch = blockIdx.y * LANES + w.lane;
  w.live = w.ch < c;
  const long left = n - w.chunk * ROWS;                       // >= 1: the grid has ceil(n / ROWS) chunks
  w.nseg = (int)((left < ROWS ? left : ROWS) + SEG - 1) / SEG;
  w.row0 = w.chunk * ROWS + (long)w.wave * SEG;
  const long mine = n - w.row0;
  w.rows = (int)(mine < SEG ? mine : SEG);
  return w;
}

// segment partials in LDS -> the chunk partial of this workgroup's channels, by wave 0
__device__ __forceinline__ void store_chunk_partial(const float (*part)[LANES], const Where& w, float* __restrict__ out, int c) {
  if (w.wave == 0 && w.live) {
    float t = part[0][w.lane];
    for (int s = 1; s < w.nseg; ++s) t = t + part[s][w.lane];
    out[w.chunk * c + w.ch] = t;
  }
}

template <int WHAT>
__global__ __launch_bounds__(ROWS) void bn_sum_kernel(const float* __restrict__ x, const float* __restrict__ dy, long n, int c, long chunks,
                                                      const float* __restrict__ mean_in, const float* __restrict__ invstd,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ ws) {
  __shared__ float part[2][WAVES][LANES];
  __shared__ float cst[LANES];
  const Where w = where(n, c);
  if (WHAT == SUM_DD) {
    if (w.wave == 0 && w.live) cst[w.lane] = total_of(ws, chunks, c, w.ch) / (float)n;
    __syncthreads();
  }
  float p = 0.f, q = 0.f;
  if (w.live && w.rows > 0) {
    const float* xp = x + w.row0 * c + w.ch;
    if (WHAT == SUM_X) {
#pragma unroll 8
      for (int i = 0; i < w.rows; ++i) p = p + xp[(long)i * c];
    } else if (WHAT == SUM_DD) {
      const float mean = cst[w.lane];
#pragma unroll 8
      for (int i = 0; i < w.rows; ++i) {
        const float d = xp[(long)i * c] - mean;
        p = fmaf(d, d, p);
      }
    } else {
      const float* gp = dy + w.row0 * c + w.ch;
      const float mean = mean_in[w.ch], is = invstd[w.ch], sc = scale[w.ch], sh = shift[w.ch];
#pragma unroll 8
      for (int i = 0; i < w.rows; ++i) {
        const float xv = xp[(long)i * c];
        const float z = xv * sc + sh;
        const float g = z > 0.f ? gp[(long)i * c] : 0.f;
        const float xhat = (xv - mean) * is;
        p = p + g;
        q = fmaf(g, xhat, q);
      }
    }
  }
  part[0][w.wave][w.lane] = p;
  if (WHAT == SUM_G) part[1][w.wave][w.lane] = q;
  __syncthreads();
  store_chunk_partial(part[0], w, ws + (WHAT == SUM_DD ? chunks * c : 0), c);
  if (WHAT == SUM_G) store_chunk_partial(part[1], w, ws + chunks * c, c);
}

__global__ __launch_bounds__(ROWS) void bn_apply_kernel(const float* __restrict__ x, long n, int c, long chunks, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, const float* __restrict__ ws,
                                                        float* __restrict__ mean_out, float* __restrict__ var_out, float* __restrict__ invstd_out,
                                                        float* __restrict__ scale_out, float* __restrict__ shift_out, float* __restrict__ y) {
  __shared__ float cst[2][LANES];
  const Where w = where(n, c);
  if (w.wave == 0 && w.live) {
    const float mean = total_of(ws, chunks, c, w.ch) / (float)n;
    const float var = total_of(ws + chunks * c, chunks, c, w.ch) / (float)n;
    const float is = 1.0f / sqrtf(var + eps);
    const float sc = gamma[w.ch] * is;
    const float sh = beta[w.ch] - mean * sc;
    cst[0][w.lane] = sc, cst[1][w.lane] = sh;
    if (w.chunk == 0) {
      mean_out[w.ch] = mean, var_out[w.ch] = var, invstd_out[w.ch] = is, scale_out[w.ch] = sc, shift_out[w.ch] = sh;
    }
  }
  __syncthreads();
  if (!w.live || w.rows <= 0) return;
  const float sc = cst[0][w.lane], sh = cst[1][w.lane];
  const float* xp = x + w.row0 * c + w.ch;
  float* yp = y + w.row0 * c + w.ch;
#pragma unroll 8
  for (int i = 0; i < w.rows; ++i) yp[(long)i * c] = fmaxf(xp[(long)i * c] * sc + sh, 0.f);
}

__global__ __launch_bounds__(ROWS) void bn_dx_kernel(const float* __restrict__ x, const float* __restrict__ dy, long n, int c, long chunks,
                                                     const float* __restrict__ mean_in, const float* __restrict__ invstd,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     const float* __restrict__ ws, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     float* __restrict__ dx) {
  __shared__ float cst[2][LANES];
  const Where w = where(n, c);
  if (w.wave == 0 && w.live) {
    const float db = total_of(ws, chunks, c, w.ch);
    const float dg = total_of(ws + chunks * c, chunks, c, w.ch);
    cst[0][w.lane] = db / (float)n, cst[1][w.lane] = dg / (float)n;
    if (w.chunk == 0) dbeta[w.ch] = db, dgamma[w.ch] = dg;
  }
  if (!dx) return;                                            // uniform: the gradient of the input is not asked for
  __syncthreads();
  if (!w.live || w.rows <= 0) return;
  const float k1 = cst[0][w.lane], k2 = cst[1][w.lane];
  const float mean = mean_in[w.ch], is = invstd[w.ch], sc = scale[w.ch], sh = shift[w.ch];
  const float* xp = x + w.row0 * c + w.ch;
  const float* gp = dy + w.row0 * c + w.ch;
  float* dp = dx + w.row0 * c + w.ch;
#pragma unroll 8
  for (int i = 0; i < w.rows; ++i) {
    const float xv = xp[(long)i * c];
    const float z = xv * sc + sh;
    const float g = z > 0.f ? gp[(long)i * c] : 0.f;
    const float xhat = (xv - mean) * is;
    dp[(long)i * c] = sc * ((g - k1) - xhat * k2);
  }
}

// max_c: 224 for the entry points of catgrasp_amd_bn.h, CG_DENSE_MAX_C for the wide ones of catgrasp_amd_dense.h -- the one difference
int check_shape(long n, int c, int max_c) {
  if (n < 2 || n > MAX_N || c <= 0) return CG_ERR_ARG;
  if (c % 16 != 0 || c > max_c) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

long workspace_size(long n, int c, int max_c) {
  const int st = check_shape(n, c, max_c);
  if (st != CG_OK) return st;
  return 2L * c * ((n + ROWS - 1) / ROWS);
}

int forward(const float* x, long n, int c, const float* gamma, const float* beta, float eps, float* workspace, float* mean, float* var,
            float* invstd, float* scale, float* shift, float* y, void* stream, int max_c) {
  const int st = check_shape(n, c, max_c);
  if (st != CG_OK) return st;
  if (!x || !gamma || !beta || !workspace || !mean || !var || !invstd || !scale || !shift || !y) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (n + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)chunks, (unsigned)((c + LANES - 1) / LANES)), block(ROWS);
  const float* none = nullptr;
  hipLaunchKernelGGL(bn_sum_kernel<SUM_X>, grid, block, 0, s, x, none, n, c, chunks, none, none, none, none, workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bn_sum_kernel<SUM_DD>, grid, block, 0, s, x, none, n, c, chunks, none, none, none, none, workspace);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bn_apply_kernel, grid, block, 0, s, x, n, c, chunks, gamma, beta, eps, (const float*)workspace, mean, var, invstd, scale,
                     shift, y);
  return cg_hip_status(hipGetLastError());
}

int backward(const float* x, const float* dy, long n, int c, const float* mean, const float* invstd, const float* scale, const float* shift,
             float* workspace, float* dgamma, float* dbeta, float* dx, void* stream, int max_c) {
  const int st = check_shape(n, c, max_c);
  if (st != CG_OK) return st;
  if (!x || !dy || !mean || !invstd || !scale || !shift || !workspace || !dgamma || !dbeta) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (n + ROWS - 1) / ROWS;
  const unsigned groups = (unsigned)((c + LANES - 1) / LANES);
  const dim3 block(ROWS);
  hipLaunchKernelGGL(bn_sum_kernel<SUM_G>, dim3((unsigned)chunks, groups), block, 0, s, x, dy, n, c, chunks, mean, invstd, scale, shift, workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bn_dx_kernel, dim3(dx ? (unsigned)chunks : 1u, groups), block, 0, s, x, dy, n, c, chunks, mean, invstd, scale, shift,
                     (const float*)workspace, dgamma, dbeta, dx);
  return cg_hip_status(hipGetLastError());
}

}  // namespace

extern "C" long cg_bn_workspace(long n, int c) { return workspace_size(n, c, NARROW_C); }

extern "C" int cg_bn_relu_train_forward(const float* x, long n, int c, const float* gamma, const float* beta, float eps, float* workspace,
                                        float* mean, float* var, float* invstd, float* scale, float* shift, float* y, void* stream) {
  return forward(x, n, c, gamma, beta, eps, workspace, mean, var, invstd, scale, shift, y, stream, NARROW_C);
}

extern "C" int cg_bn_relu_train_backward(const float* x, const float* dy, long n, int c, const float* mean, const float* invstd,
                                         const float* scale, const float* shift, float* workspace, float* dgamma, float* dbeta, float* dx,
                                         void* stream) {
  return backward(x, dy, n, c, mean, invstd, scale, shift, workspace, dgamma, dbeta, dx, stream, NARROW_C);
}

// The same functions up to CG_DENSE_MAX_C channels (catgrasp_amd_dense.h): the widths of PointNetSeg's per-point head.
extern "C" long cg_bn_wide_workspace(long n, int c) { return workspace_size(n, c, CG_DENSE_MAX_C); }

extern "C" int cg_bn_relu_train_forward_wide(const float* x, long n, int c, const float* gamma, const float* beta, float eps, float* workspace,
                                             float* mean, float* var, float* invstd, float* scale, float* shift, float* y, void* stream) {
  return forward(x, n, c, gamma, beta, eps, workspace, mean, var, invstd, scale, shift, y, stream, CG_DENSE_MAX_C);
}

extern "C" int cg_bn_relu_train_backward_wide(const float* x, const float* dy, long n, int c, const float* mean, const float* invstd,
                                              const float* scale, const float* shift, float* workspace, float* dgamma, float* dbeta, float* dx,
                                              void* stream) {
  return backward(x, dy, n, c, mean, invstd, scale, shift, workspace, dgamma, dbeta, dx, stream, CG_DENSE_MAX_C);
}
