// Gradients of a dense per-row layer y = x . W^T + bias [+ row_bias[row / rows_per_group]] (catgrasp_amd/include/catgrasp_amd_dense.h
// has the contract): weight and bias gradient (cg_dense_wgrad), input gradient (cg_dense_dgrad) and the per-group column sums that
// are the gradient of row_bias (cg_dense_group_sums).  Exact f32 on v_mfma_f32_32x32x2_f32, every result element a fixed-order chain
// written by exactly one thread.
//
// Weight gradient.  dw (cout, cin) = dy^T . x: the reduction index (the rows) is the MFMA's k dimension, the output channels are its
// M and the input channels its N, and both operands are row-contiguous: lane l feeds A[m = l&31][l>>5] = dy[row 2s + (l>>5)][o0 + (l&31)]
// and B[l>>5][n = l&31] = x[row 2s + (l>>5)][c0 + (l&31)].  D = fma(a1, b1, fma(a0, b0, C)): the rows enter every element's chain in
// ascending order.  A 32 x 32 tile fed from global memory would read 256 B per operand for 4096 flops; so a workgroup of four waves
// owns (chunk of CG_DENSE_GRAD_ROWS rows, 128 output channels, 32 NJ input channels, NJ = 1, 2 or 4 by cin), stages 32 rows of both
// operands in LDS at a time (ds_read_b32 of 32 consecutive floats per half wave: conflict-free without padding) and its wave w holds
// the NJ accumulator tiles of output channels [32w, 32w + 32): one A read and NJ B reads per NJ MFMAs, 2 x 16 KB of global reads per
// 64 MFMAs of the workgroup.  The next stage's rows are requested before this stage's products and written to LDS after them.
// Rows past the end and channels past the edge are staged as zeros: fmaf(0, 0, p) = p.
// The bias gradient is the chain p = fmaf(1, dy, p) over the staged rows, one thread per output channel, in the workgroups of input
// tile 0.  Every partial tile goes to the workspace; dense_wgrad_reduce_kernel sums the chunks in ascending order.
//
// Input gradient.  dx (n, cin) = dy . W is the forward operator with the transposed weight: the tile body of gemm.hip's
// gemm_bias_act_kernel (64 rows x 128 columns per workgroup, dy staged in LDS 64 columns at a time), with the B operand read from W
// as it is stored (W[o][c0 + (l&31)]: a row of W is the operand's layout) and the contraction padded with zeros to whole steps of 8.
//
// Group sums.  The layout of batchnorm_train.hip's bn_sum_kernel per group: one workgroup of 16 waves per (group, chunk of
// CG_BN_ROWS rows of the group, 64 channels), one wave per segment of CG_BN_SEG rows, one lane per channel.
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_bn.h"
#include "../include/catgrasp_amd_dense.h"

namespace {

constexpr int ROWS = CG_DENSE_GRAD_ROWS;
constexpr int ST = 32;                      // rows per LDS stage: 16 MFMA steps of two rows
constexpr int TO = 128;                     // output channels per workgroup: 32 per wave
constexpr long MAX_N = 1L << 24;
static_assert(ROWS % ST == 0, "a chunk is a whole number of stages");

// ws: per chunk, cout*cin floats of dw partials [o][ci], then cout floats of db partials
template <int NJ>
__global__ __launch_bounds__(256) void dense_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, long n, int cin, int cout,
                                                          int do_w, int do_b, float* __restrict__ ws) {
  constexpr int TI = 32 * NJ;               // input channels per workgroup
  __shared__ __attribute__((aligned(16))) float sa[ST * TO];
  __shared__ __attribute__((aligned(16))) float sb[ST * TI];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const long row0 = (long)blockIdx.x * ROWS;
  const int nrows = (int)min((long)ROWS, n - row0);
  const int o0 = blockIdx.y * TO, c0 = blockIdx.z * TI;
  const bool bias_wg = do_b && blockIdx.z == 0;
  const bool wave_ok = do_w && o0 + wave * 32 < cout;          // wave-uniform

  // the loader's place: float4 q of this thread covers row (tid >> 5) + 8 q, columns 4 (tid & 31) .. + 3 of the dy tile, and row
  // (tid + 256 q) / (8 NJ), columns 4 ((tid + 256 q) % (8 NJ)) .. + 3 of the x tile; cout and cin are multiples of 4
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 va[4], vb[NJ];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + (tid >> 5) + 8 * q, o = o0 + 4 * (tid & 31);
      va[q] = zero;
      if (r < nrows && o < cout) va[q] = *(const f32x4*)(dy + (size_t)(row0 + r) * cout + o);
    }
    if (do_w) {
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const int e = tid + 256 * q;
        const int r = r0 + e / (8 * NJ), c = c0 + 4 * (e % (8 * NJ));
        vb[q] = zero;
        if (r < nrows && c < cin) vb[q] = *(const f32x4*)(x + (size_t)(row0 + r) * cin + c);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) *(f32x4*)(sa + ((tid >> 5) + 8 * q) * TO + 4 * (tid & 31)) = va[q];
    if (do_w) {
#pragma unroll
      for (int q = 0; q < NJ; ++q) *(f32x4*)(sb + 4 * (tid + 256 * q)) = vb[q];      // row-major (ST, TI): element index 4 e
    }
  };

  f32x16 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float pb = 0.f;

  fetch(0);
  for (int r0 = 0; r0 < nrows; r0 += ST) {
    __syncthreads();                        // the previous stage has been read
    stage();
    __syncthreads();
    if (r0 + ST < nrows) fetch(r0 + ST);
    if (wave_ok) {
      const float* ap = sa + h * TO + wave * 32 + i;
      const float* bp = sb + h * TI + i;
#pragma unroll 4
      for (int s = 0; s < ST / 2; ++s) {
        const float a = ap[2 * s * TO];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = mfma32(a, bp[2 * s * TI + 32 * j], acc[j]);
      }
    }
    if (bias_wg && tid < TO) {
#pragma unroll 8
      for (int r = 0; r < ST; ++r) pb = fmaf(1.f, sa[r * TO + tid], pb);
    }
  }

  const size_t cc = (size_t)cout * cin;
  float* part = ws + (size_t)blockIdx.x * (cc + cout);
  if (bias_wg && tid < TO && o0 + tid < cout) part[cc + o0 + tid] = pb;
  if (!wave_ok) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = c0 + 32 * j + i;
    if (c >= cin) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = o0 + wave * 32 + acc_row(r, lane);
      if (o < cout) part[(size_t)o * cin + c] = acc[j][r];
    }
  }
}

// element e of [dw (cc floats) | db (cout floats)]: the chunks' partials in ascending order
__global__ __launch_bounds__(256) void dense_wgrad_reduce_kernel(const float* __restrict__ ws, long chunks, long cc, int cout, float* __restrict__ dw,
                                                                 float* __restrict__ db) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= cc + cout) return;
  float* dst = e < cc ? (dw ? dw + e : nullptr) : (db ? db + (e - cc) : nullptr);
  if (!dst) return;
  const size_t stride = (size_t)cc + cout;
  float s = ws[e];
#pragma unroll 4
  for (long ch = 1; ch < chunks; ++ch) s += ws[ch * stride + e];
  *dst = s;
}

constexpr int BM = 64;       // rows per workgroup
constexpr int BK = 64;       // columns of dy staged in LDS
constexpr int SA = BK + 4;   // LDS row stride (floats)

__global__ __launch_bounds__(256) void dense_dgrad_kernel(const float* __restrict__ dy, long n, int cout, const float* __restrict__ w, int cin,
                                                          float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float ys[BM * SA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const long row0 = (long)blockIdx.x * BM;
  const int cb = blockIdx.y * 128 + wave * 32;
  const bool active = cb < cin;                                // wave-uniform
  const int col = cb + l31;
  const float* wcol = w + min(col, cin - 1);                   // clamped: a column past the edge is not stored
  const int kpad = (cout + 7) & ~7;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x16 c0 = {0}, c1 = {0};
  for (int k0 = 0; k0 < kpad; k0 += BK) {
    const int kc = min(BK, kpad - k0);
    __syncthreads();
    // stage dy[row0 : row0 + 64, k0 : k0 + kc] (rows clamped; columns >= cout are zeros; cout is a multiple of 4)
    for (int e = tid; e < BM * (BK / 4); e += 256) {
      const int r = e / (BK / 4), cq = e - r * (BK / 4);
      if (cq * 4 < kc) {
        const long row = min(row0 + r, n - 1);
        f32x4 v = zero;
        if (k0 + cq * 4 < cout) v = *(const f32x4*)(dy + (size_t)row * cout + k0 + cq * 4);
        *(f32x4*)(ys + r * SA + cq * 4) = v;
      }
    }
    __syncthreads();
    if (active) {
      const float* ar0 = ys + l31 * SA + lhi * 4;
      const float* ar1 = ar0 + 32 * SA;
      const int nks = kc / 8;
#pragma unroll 4
      for (int ks = 0; ks < nks; ++ks) {
        const int kb = k0 + ks * 8 + lhi * 4;
        float bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = wcol[(size_t)min(kb + j, cout - 1) * cin];
          bv[j] = kb + j < cout ? t : 0.f;
        }
        const f32x4 a0 = *(const f32x4*)(ar0 + ks * 8);
        const f32x4 a1 = *(const f32x4*)(ar1 + ks * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { c0 = mfma32(a0[j], bv[j], c0); c1 = mfma32(a1[j], bv[j], c1); }
      }
    }
  }
  if (!active || col >= cin) return;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long row = row0 + half * 32 + acc_row(r, lane);
      if (row < n) dx[(size_t)row * cin + col] = half ? c1[r] : c0[r];
    }
  }
}

constexpr int SEG = CG_BN_SEG, BROWS = CG_BN_ROWS, WAVES = BROWS / SEG;
static_assert(WAVES == 16 && SEG == 64, "one wave per segment, 16 waves per workgroup");

// out[(g * cpg + chunk) * c + ch]: the chunk partial of channel ch over rows [chunk * BROWS, ...) of group g (cpg chunks per group)
__global__ __launch_bounds__(BROWS) void dense_group_sum_kernel(const float* __restrict__ dy, long rpg, long cpg, int c, float* __restrict__ out) {
  __shared__ float part[WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long g = blockIdx.x / cpg, chunk = blockIdx.x - g * cpg;
  const int ch = blockIdx.y * 64 + lane;
  const long left = rpg - chunk * BROWS;                        // >= 1
  const int nseg = (int)((left < BROWS ? left : BROWS) + SEG - 1) / SEG;
  const long r0 = chunk * BROWS + (long)wave * SEG;             // within the group
  const long mine = rpg - r0;
  const int rows = (int)(mine < SEG ? mine : SEG);
  float p = 0.f;
  if (ch < c && rows > 0) {
    const float* yp = dy + (size_t)(g * rpg + r0) * c + ch;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) p = p + yp[(size_t)r * c];
  }
  part[wave][lane] = p;
  __syncthreads();
  if (wave == 0 && ch < c) {
    float t = part[0][lane];
    for (int s = 1; s < nseg; ++s) t = t + part[s][lane];
    out[(size_t)blockIdx.x * c + ch] = t;
  }
}

// sums[g][ch]: the chunk partials of group g in ascending order
__global__ __launch_bounds__(256) void dense_group_total_kernel(const float* __restrict__ ws, long groups, long cpg, int c, float* __restrict__ sums) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= groups * c) return;
  const long g = e / c;
  const int ch = (int)(e - g * c);
  const float* p = ws + (size_t)g * cpg * c + ch;
  float t = p[0];
  for (long k = 1; k < cpg; ++k) t = t + p[(size_t)k * c];
  sums[e] = t;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_wgrad(long n, int cin, int cout) {
  if (n < 1 || n > MAX_N || cin <= 0 || cout <= 0) return CG_ERR_ARG;
  if (cin % 8 != 0 || cin > CG_DENSE_MAX_C || cout % 4 != 0 || cout > CG_DENSE_MAX_C) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

int check_group_sums(long groups, long rpg, int c) {
  if (groups < 1 || rpg < 1 || groups > MAX_N || rpg > MAX_N || groups * rpg > MAX_N || c <= 0) return CG_ERR_ARG;
  if (c % 4 != 0 || c > CG_DENSE_MAX_C) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

}  // namespace

extern "C" long cg_dense_wgrad_workspace(long n, int cin, int cout) {
  const int st = check_wgrad(n, cin, cout);
  if (st != CG_OK) return st;
  return (n + ROWS - 1) / ROWS * ((long)cout * cin + cout);
}

extern "C" int cg_dense_wgrad(const float* x, const float* dy, long n, int cin, int cout, float* workspace, float* dw, float* db, void* stream) {
  const int st = check_wgrad(n, cin, cout);
  if (st != CG_OK) return st;
  if ((!dw && !db) || !dy || !workspace || (dw && !x) || !aligned16(dy) || !aligned16(x) || !aligned16(workspace)) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (n + ROWS - 1) / ROWS;                    // at most 2^14
  const int nj = cin <= 32 ? 1 : cin <= 64 ? 2 : 4;
  const dim3 grid((unsigned)chunks, (unsigned)((cout + TO - 1) / TO), (unsigned)(dw ? (cin + 32 * nj - 1) / (32 * nj) : 1));
  const int do_w = dw != nullptr, do_b = db != nullptr;
  if (nj == 1) hipLaunchKernelGGL(dense_wgrad_kernel<1>, grid, dim3(256), 0, s, x, dy, n, cin, cout, do_w, do_b, workspace);
  else if (nj == 2) hipLaunchKernelGGL(dense_wgrad_kernel<2>, grid, dim3(256), 0, s, x, dy, n, cin, cout, do_w, do_b, workspace);
  else hipLaunchKernelGGL(dense_wgrad_kernel<4>, grid, dim3(256), 0, s, x, dy, n, cin, cout, do_w, do_b, workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long cc = (long)cout * cin;
  hipLaunchKernelGGL(dense_wgrad_reduce_kernel, dim3((unsigned)((cc + cout + 255) / 256)), dim3(256), 0, s, (const float*)workspace, chunks, cc, cout,
                     dw, db);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_dense_dgrad(const float* dy, long n, int cout, const float* w, int cin, float* dx, void* stream) {
  if (n < 1 || n > MAX_N || cin <= 0 || cout <= 0) return CG_ERR_ARG;
  if (cin % 4 != 0 || cin > CG_DENSE_MAX_C || cout % 4 != 0 || cout > CG_DENSE_MAX_C) return CG_ERR_UNSUPPORTED;
  if (!dy || !w || !dx || !aligned16(dy)) return CG_ERR_ARG;
  const dim3 grid((unsigned)((n + BM - 1) / BM), (unsigned)((cin + 127) / 128));
  hipLaunchKernelGGL(dense_dgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, dy, n, cout, w, cin, dx);
  return cg_hip_status(hipGetLastError());
}

extern "C" long cg_dense_group_sums_workspace(long groups, long rows_per_group, int c) {
  const int st = check_group_sums(groups, rows_per_group, c);
  if (st != CG_OK) return st;
  return groups * c * ((rows_per_group + BROWS - 1) / BROWS);
}

extern "C" int cg_dense_group_sums(const float* dy, long groups, long rows_per_group, int c, float* workspace, float* sums, void* stream) {
  const int st = check_group_sums(groups, rows_per_group, c);
  if (st != CG_OK) return st;
  const long cpg = (rows_per_group + BROWS - 1) / BROWS;
  if (!dy || !sums || (cpg > 1 && !workspace)) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(groups * cpg), (unsigned)((c + 63) / 64));      // groups * cpg < 2^25
  hipLaunchKernelGGL(dense_group_sum_kernel, grid, dim3(BROWS), 0, s, dy, rows_per_group, cpg, c, cpg > 1 ? workspace : sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || cpg == 1) return cg_hip_status(e);
  hipLaunchKernelGGL(dense_group_total_kernel, dim3((unsigned)((groups * c + 255) / 256)), dim3(256), 0, s, (const float*)workspace, groups, cpg, c, sums);
  return cg_hip_status(hipGetLastError());
}
