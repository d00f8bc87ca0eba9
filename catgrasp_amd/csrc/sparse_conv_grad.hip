// Gradients of the sparse 3-D convolution layers (include/catgrasp_amd_sparse_grad.h): weight and bias gradient
// (cg_sparse_conv_wgrad) and input gradient (cg_sparse_conv_dgrad), on v_mfma_f32_32x32x2_f32 (exact f32: every result element is a
// fixed-order fmaf chain), without atomics.
//
// Weight gradient.  dw[k] (cin, cout) = sum_i x[nbr[i,k]]^T dy[i]: the reduction index (the rows) is the MFMA's k dimension, the
// input channels are its M and the output channels its N.  One instruction takes two rows: lane l feeds A[m = l&31][l>>5] =
// x[source of row 2s + (l>>5)][c0 + (l&31)] and B[l>>5][n = l&31] = dy[row 2s + (l>>5)][o0 + (l&31)], both straight from global
// memory (two 128-byte segments per operand: no LDS tile is needed, the MFMA's operand layout is the row layout).  D = fma(a1, b1,
// fma(a0, b0, C)): the rows enter every element's chain in ascending order.
// A workgroup owns (chunk of CG_SPARSE_GRAD_ROWS rows, offset k, 32 input channels); its wave w owns output channels [32w, 32w+32)
// and one accumulator tile.  Wave 0 first compacts the chunk's rows that have a neighbour at k into an LDS list, in row order, so
// the MFMA count follows the neighbours that exist (most of the 27 offsets are absent on surface-like scenes: an offset that no
// row of the chunk uses costs one pass over its rule-book column).  Skipping a row and feeding zeros for it give the same bits
// (fmaf(0, b, acc) = acc for finite b and acc != -0, and a chain from +0 never reaches -0 in the normal range), which is what the
// padding of the list to whole steps relies on.
// The bias gradient is the same chain with A = 1 over every row: the pseudo-offset k = K of the same launch.
// Every partial tile is stored to the workspace; sparse_wgrad_reduce_kernel sums the chunks in ascending order.
//
// Input gradient.  The forward operator over the transposed rule book with transposed weights (the header has the table), so the
// kernel is the tile body of csrc/sparse_conv.hip -- 32 rows per workgroup, the gathered rows in LDS with the same layout, the same
// ballot that skips an offset no row of the tile uses -- for the transposed channel sets: dy has cout in {3, 16..112} channels (3
// handled as the forward handles 6: scalar gather, zero padding to 8) and dx has cin in {6, 16..224} columns, in blocks of 128 on
// blockIdx.y (a workgroup holds at most four 32-column waves).  There is no prologue, bias or residual.  The forward kernel is
// left as it is: its bits are pinned (tests/test_sparse_conv_exact_gpu.py), so its body is restated here, not shared.
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_sparse.h"
#include "../../include/catgrasp_amd_sparse_grad.h"

namespace {

constexpr int ROWS = CG_SPARSE_GRAD_ROWS;
constexpr int STEP = 8;                     // list entries per loop iteration: four MFMAs of two rows
static_assert(ROWS % 64 == 0 && ROWS % STEP == 0, "the compaction works on whole waves, the product loop on whole steps");

// ws: per chunk, K*cin*cout floats of dw partials [k][ci][o], then cout floats of db partials.  k_first = K: the bias only.
__global__ __launch_bounds__(256) void sparse_wgrad_kernel(const float* __restrict__ feats, long n_in, const int* __restrict__ nbr, long n_out, int K,
                                                           int k_first, const float* __restrict__ dy, int cin, int cout, float* __restrict__ ws) {
  __shared__ int lsrc[ROWS + STEP], lrow[ROWS + STEP];
  __shared__ int lcnt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int k = k_first + blockIdx.y;
  const bool bias_mode = k == K;
  if (bias_mode && blockIdx.z != 0) return;                  // the whole workgroup: no barrier is left unmatched
  const long row0 = (long)blockIdx.x * ROWS;
  const int nrows = (int)min((long)ROWS, n_out - row0);

  if (wave == 0) {
    // all loads first (one latency), then the ballots in row order
    int src[ROWS / 64];
#pragma unroll
    for (int j = 0; j < ROWS / 64; ++j) {
      const int r = j * 64 + lane;
      src[j] = -1;
      if (r < nrows) src[j] = bias_mode ? 0 : nbr[(row0 + r) * K + k];
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < ROWS / 64; ++j) {
      const bool ok = src[j] >= 0 && (bias_mode || src[j] < n_in);
      const unsigned long long m = __ballot(ok);
      if (ok) {
        const int p = cnt + __popcll(m & ((1ull << lane) - 1ull));          // p < nrows <= ROWS
        lsrc[p] = src[j];
        lrow[p] = j * 64 + lane;
      }
      cnt += __popcll(m);
    }
    if (lane < STEP) {                                     // cnt <= ROWS: inside the arrays
      lsrc[cnt + lane] = -1;
      lrow[cnt + lane] = 0;
    }
    if (lane == 0) lcnt = cnt;
  }
  __syncthreads();
  const int cnt = lcnt;

  const int c0 = blockIdx.z * 32;
  const int c = min(c0 + i, cin - 1), o = min(wave * 32 + i, cout - 1);          // clamped: a tile element past the edge is not stored
  const float* xcol = feats + c;
  const float* ycol = dy + (size_t)row0 * cout + o;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // entry e = 2s + h of the list is this lane's row of MFMA s.  The next iteration's operands are loaded before this one's products.
  auto load = [&](int e0, float (&a)[4], float (&b)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = lsrc[e0 + 2 * j + h], r = lrow[e0 + 2 * j + h];
      a[j] = 0.f;
      b[j] = 0.f;
      if (s >= 0) {
        a[j] = bias_mode ? 1.f : xcol[(size_t)s * cin];
        b[j] = ycol[(size_t)r * cout];
      }
    }
  };
  float a[4], b[4];
  if (cnt > 0) load(0, a, b);
  for (int e0 = 0; e0 < cnt; e0 += STEP) {
    float an[4] = {0.f, 0.f, 0.f, 0.f}, bn[4] = {0.f, 0.f, 0.f, 0.f};
    if (e0 + STEP < cnt) load(e0 + STEP, an, bn);
    __builtin_amdgcn_sched_barrier(0);          // keep the loads above in front of the products
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = mfma32(a[j], b[j], acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = an[j];
      b[j] = bn[j];
    }
  }

  const size_t kcc = (size_t)K * cin * cout;
  float* part = ws + (size_t)blockIdx.x * (kcc + cout);
  const int col = wave * 32 + i;
  if (col >= cout) return;
  if (bias_mode) {
    if (h == 0) part[kcc + col] = acc[0];                    // row 0 of the tile: every row holds the same sum
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ci = c0 + acc_row(r, lane);
    if (ci < cin) part[((size_t)k * cin + ci) * cout + col] = acc[r];
  }
}

// element e of [dw (kcc floats) | db (cout floats)]: the chunks' partials in ascending order
__global__ __launch_bounds__(256) void sparse_wgrad_reduce_kernel(const float* __restrict__ ws, long chunks, long kcc, int cout, float* __restrict__ dw,
                                                                  float* __restrict__ db) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= kcc + cout) return;
  float* dst = e < kcc ? (dw ? dw + e : nullptr) : (db ? db + (e - kcc) : nullptr);
  if (!dst) return;
  const size_t stride = (size_t)kcc + cout;
  float s = ws[e];
#pragma unroll 4
  for (long ch = 1; ch < chunks; ++ch) s += ws[ch * stride + e];
  *dst = s;
}

// The tile body of sparse_conv_kernel (csrc/sparse_conv.hip) over dy (n_out, cy) and the transposed book nbr_t (n_in, K):
// dx (n_in, cx), weight_t (K, cy, cx); workgroup = 32 rows of dx x the column block [128 blockIdx.y, +128).
__global__ __launch_bounds__(256) void sparse_dgrad_kernel(const float* __restrict__ dy, long n_out, const int* __restrict__ nbr_t, long n_in, int K,
                                                           const float* __restrict__ wt, int cy, int cx, float* __restrict__ dx) {
  extern __shared__ float4 tile4[];
  float* tile = (float*)tile4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int cp = (cy + 7) & ~7, S = cp + 4, chunks = cp >> 2;
  const bool vec = (cy & 3) == 0;
  const long row0 = (long)blockIdx.x * 32;
  const int col = blockIdx.y * 128 + wave * 32 + i;
  const bool col_ok = col < cx;
  const bool wave_ok = blockIdx.y * 128 + wave * 32 < cx;          // wave-uniform: a wave with no column gathers and waits, no more

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int k = 0; k < K; ++k) {
    int idx = -1;
    if (lane < 32 && row0 + lane < n_in) {
      idx = nbr_t[(row0 + lane) * K + k];
      if (idx < 0 || idx >= n_out) idx = -1;
    }
    if (__ballot(idx >= 0) == 0) continue;          // wave-uniform, and the same in every wave of the workgroup
    __syncthreads();                                // the previous offset's tile has been read
    for (int t = threadIdx.x; t < 32 * chunks; t += blockDim.x) {      // 32*chunks and blockDim.x are multiples of 64: no wave splits
      const int r = t / chunks, ch = t - r * chunks;
      const int src = __shfl(idx, r);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src >= 0) {
        const float* p = dy + (size_t)src * cy + ch * 4;
        if (vec && ch * 4 + 4 <= cy) {
          v = *(const float4*)p;
        } else {
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = ch * 4 + j < cy ? p[j] : 0.f;
          v = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      *(float4*)(tile + r * S + ch * 4) = v;
    }
    __syncthreads();
    if (!wave_ok) continue;
    // as in the forward: unmasked weight loads at clamped addresses; a column >= cx is never stored, a row >= cy (cy = 3 only)
    // meets the zeros that pad the tile
    const float* wcol = wt + (size_t)k * cy * cx + (col_ok ? col : 0);
    const float* arow = tile + i * S + h * 4;
    const int nq = cp >> 3;
    float4 a = *(const float4*)arow;
    float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = wcol[(size_t)min(h * 4 + j, cy - 1) * cx];
    for (int q = 0; q < nq; ++q) {
      float4 an = a;
      float bn[4] = {b[0], b[1], b[2], b[3]};
      if (q + 1 < nq) {
        an = *(const float4*)(arow + (q + 1) * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) bn[j] = wcol[(size_t)min((q + 1) * 8 + h * 4 + j, cy - 1) * cx];
      }
      __builtin_amdgcn_sched_barrier(0);          // keep the loads above in front of the products
      acc = mfma32(a.x, b[0], acc);
      acc = mfma32(a.y, b[1], acc);
      acc = mfma32(a.z, b[2], acc);
      acc = mfma32(a.w, b[3], acc);
      a = an;
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = bn[j];
    }
  }

  if (!col_ok) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long row = row0 + acc_row(r, lane);
    if (row < n_in) dx[(size_t)row * cx + col] = acc[r];
  }
}

bool cin_ok(int c) { return c == 6 || (c > 0 && c % 16 == 0 && c <= CG_SPARSE_MAX_CIN); }
bool cout_ok(int c) { return c == 3 || (c > 0 && c % 16 == 0 && c <= CG_SPARSE_MAX_COUT); }

int check_shape(long n_in, long n_out, int K, int cin, int cout) {
  if (n_in < 0 || n_out < 0 || n_in > (1L << 26) || n_out > (1L << 26) || (K != 1 && K != 8 && K != 27) || cin <= 0 || cout <= 0) return CG_ERR_ARG;
  if (!cin_ok(cin) || !cout_ok(cout)) return CG_ERR_UNSUPPORTED;
  return CG_OK;
}

}  // namespace

extern "C" long cg_sparse_wgrad_workspace(long n_out, int K, int cin, int cout) {
  const int st = check_shape(0, n_out, K, cin, cout);
  if (st != CG_OK) return st;
  return (n_out + ROWS - 1) / ROWS * ((long)K * cin * cout + cout);
}

extern "C" int cg_sparse_conv_wgrad(const float* feats, long n_in, const int* nbr, long n_out, int K, const float* dy, int cin, int cout,
                                    float* workspace, float* dw, float* db, void* stream) {
  const int st = check_shape(n_in, n_out, K, cin, cout);
  if (st != CG_OK) return st;
  if (!dw && !db) return CG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long kcc = (long)K * cin * cout;
  if (n_out == 0) {
    hipError_t e = dw ? hipMemsetAsync(dw, 0, (size_t)kcc * sizeof(float), s) : hipSuccess;
    if (e == hipSuccess && db) e = hipMemsetAsync(db, 0, (size_t)cout * sizeof(float), s);
    return cg_hip_status(e);
  }
  if (!dy || !workspace || (dw && (!nbr || (n_in > 0 && !feats)))) return CG_ERR_ARG;
  const long chunks = (n_out + ROWS - 1) / ROWS;                    // at most 2^16
  const int waves = (cout + 31) / 32, ctiles = (cin + 31) / 32;     // 1 .. 4 and 1 .. 7
  const dim3 grid((unsigned)chunks, (unsigned)((dw ? K : 0) + (db ? 1 : 0)), (unsigned)(dw ? ctiles : 1));
  hipLaunchKernelGGL(sparse_wgrad_kernel, grid, dim3(64 * waves), 0, s, feats, n_in, nbr, n_out, K, dw ? 0 : K, dy, cin, cout, workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sparse_wgrad_reduce_kernel, dim3((unsigned)((kcc + cout + 255) / 256)), dim3(256), 0, s, workspace, chunks, kcc, cout, dw, db);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_sparse_conv_dgrad(const float* dy, long n_out, const int* nbr_t, long n_in, int K, const float* weight_t, int cin, int cout,
                                    float* dx, void* stream) {
  const int st = check_shape(n_in, n_out, K, cin, cout);
  if (st != CG_OK) return st;
  if (n_in == 0) return CG_OK;
  if (!nbr_t || !weight_t || !dx || (n_out > 0 && !dy)) return CG_ERR_ARG;
  const int waves = min(4, (cin + 31) / 32);
  const int cp = (cout + 7) & ~7;
  const size_t lds = (size_t)32 * (cp + 4) * sizeof(float);      // at most 14,848 B
  hipLaunchKernelGGL(sparse_dgrad_kernel, dim3((unsigned)((n_in + 31) / 32), (unsigned)((cin + 127) / 128)), dim3(64 * waves), lds,
                     (hipStream_t)stream, dy, n_out, nbr_t, n_in, K, weight_t, cout, cin, dx);
  return cg_hip_status(hipGetLastError());
}
