// Fused gather-GEMM of the sparse 3-D convolution layers (include/catgrasp_amd_sparse.h, cg_sparse_conv): submanifold, strided and
// inverse convolution are the same kernel over different rule books.
//
// Output-stationary.  A workgroup owns 32 output rows; its wave w owns the 32 x 32 tile of output channels [32w, 32w+32) and keeps
// it in the 16 accumulator registers of one v_mfma_f32_32x32x2_f32 chain (exact f32, a fixed-order fmaf chain per element).  For
// k = 0 .. K-1 in order:
//   - lanes 0..31 of every wave read column k of the tile's rule-book rows; if no row has a neighbour there the offset is skipped
//     (one ballot: the same decision in every wave, so the barriers below stay matched);
//   - the waves gather the 32 neighbour rows into LDS, 16 B per lane, applying the optional prologue max(x*scale + shift, 0) to
//     rows that exist and writing zeros for rows that do not (an absent neighbour contributes nothing, not relu(shift));
//   - each wave multiplies the LDS tile by its 32 columns of weight[k], read from global memory (L1/L2 resident: every workgroup
//     reads the same K*cin*cout floats).
// Then bias and the optional residual row are added and every output element is stored once.  No scatter, no atomics.
//
// LDS tile: 32 rows of S = cp + 4 floats, cp = cin rounded up to 8.  Lane (i = lane & 31, h = lane >> 5) reads the 16 bytes at
// row i, floats 8q + 4h .. 8q + 4h + 3 with one ds_read_b128 and feeds element j to the MFMA of step (q, j): the A operand of that
// step is A[i][kk = h] = X[i][8q + 4h + j], so the B operand is weight[k][8q + 4h + j][col].  S/4 is odd, so the 16 lanes that a
// ds_read_b128 services together fall on 16 different bank quadruples.
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_sparse.h"
#include "../../include/catgrasp_amd_pointgroup.h"

namespace {

__device__ __forceinline__ float prologue(float x, float s, float b) { return fmaxf(x * s + b, 0.f); }

// TWO: the input rows are the concatenation [feats | feats_b] of two matrices with the same row order, cin_a and cin - cin_a
// channels wide (both multiples of 16): a 16-byte chunk below cin_a is read from feats, the others from feats_b.  Nothing else
// differs, so every output element is the same fmaf chain as over the concatenated matrix (cg_sparse_conv_cat).
template <bool TWO>
__global__ __launch_bounds__(256) void sparse_conv_kernel(const float* __restrict__ feats, const float* __restrict__ feats_b, int cin_a, long n_in,
                                                          const int* __restrict__ nbr, long n_out, int K,
                                                          const float* __restrict__ weight, const float* __restrict__ bias,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const float* __restrict__ residual, int cin, int cout, float* __restrict__ out) {
  extern __shared__ float4 tile4[];
  float* tile = (float*)tile4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int cp = (cin + 7) & ~7, S = cp + 4, chunks = cp >> 2;
  const bool vec = (cin & 3) == 0;
  const long row0 = (long)blockIdx.x * 32;
  const int col = wave * 32 + i;
  const bool col_ok = col < cout;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int k = 0; k < K; ++k) {
    int idx = -1;
    if (lane < 32 && row0 + lane < n_out) {
      idx = nbr[(row0 + lane) * K + k];
      if (idx < 0 || idx >= n_in) idx = -1;
    }
    if (__ballot(idx >= 0) == 0) continue;          // wave-uniform, and the same in every wave of the workgroup
    __syncthreads();                                // the previous offset's tile has been read
    for (int t = threadIdx.x; t < 32 * chunks; t += blockDim.x) {      // 32*chunks and blockDim.x are multiples of 64: no wave splits
      const int r = t / chunks, ch = t - r * chunks;
      const int src = __shfl(idx, r);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src >= 0) {
        const float* p = feats + (size_t)src * cin + ch * 4;
        if constexpr (TWO) p = ch * 4 < cin_a ? feats + (size_t)src * cin_a + ch * 4 : feats_b + (size_t)src * (cin - cin_a) + (ch * 4 - cin_a);
        if (vec && ch * 4 + 4 <= cin) {
          v = *(const float4*)p;
          if (scale) {
            const float4 s = *(const float4*)(scale + ch * 4), b = *(const float4*)(shift + ch * 4);
            v.x = prologue(v.x, s.x, b.x); v.y = prologue(v.y, s.y, b.y); v.z = prologue(v.z, s.z, b.z); v.w = prologue(v.w, s.w, b.w);
          }
        } else {
          float e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = ch * 4 + j;
            float x = 0.f;
            if (c < cin) {
              x = p[j];
              if (scale) x = prologue(x, scale[c], shift[c]);
            }
            e[j] = x;
          }
          v = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      *(float4*)(tile + r * S + ch * 4) = v;
    }
    __syncthreads();
    // One step = 8 input channels: this lane's 16 bytes of the tile and its four weights.  The next step's loads are issued before
    // this step's four products (two register sets), so their latency hides under 256 cycles of MFMA.  The weight loads carry no
    // mask, only clamped addresses: a column >= cout computes a result that is never stored, and a row >= cin (cin = 6 only)
    // meets the zeros that pad the tile.
    const float* wcol = weight + (size_t)k * cin * cout + (col_ok ? col : 0);
    const float* arow = tile + i * S + h * 4;
    const int nq = cp >> 3;
    float4 a = *(const float4*)arow;
    float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = wcol[(size_t)min(h * 4 + j, cin - 1) * cout];
    for (int q = 0; q < nq; ++q) {
      float4 an = a;
      float bn[4] = {b[0], b[1], b[2], b[3]};
      if (q + 1 < nq) {
        an = *(const float4*)(arow + (q + 1) * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) bn[j] = wcol[(size_t)min((q + 1) * 8 + h * 4 + j, cin - 1) * cout];
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
  const float bv = bias ? bias[col] : 0.f;
  float res[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) res[r] = 0.f;
  if (residual) {
#pragma unroll
    for (int r = 0; r < 16; ++r) res[r] = residual[(size_t)min(row0 + acc_row(r, lane), n_out - 1) * cout + col];      // clamped row: not stored
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long row = row0 + acc_row(r, lane);
    if (row < n_out) out[(size_t)row * cout + col] = (acc[r] + bv) + res[r];
  }
}

bool cin_ok(int c) { return c == 6 || (c > 0 && c % 16 == 0 && c <= CG_SPARSE_MAX_CIN); }
bool cout_ok(int c) { return c == 3 || (c > 0 && c % 16 == 0 && c <= CG_SPARSE_MAX_COUT); }

}  // namespace

extern "C" int cg_sparse_conv(const float* feats, long n_in, const int* nbr, long n_out, int K, const float* weight, const float* bias,
                              const float* scale, const float* shift, const float* residual, int cin, int cout, float* out, void* stream) {
  if (n_in < 0 || n_out < 0 || n_in > (1L << 26) || n_out > (1L << 26) || (K != 1 && K != 8 && K != 27) || cin <= 0 || cout <= 0 ||
      (scale == nullptr) != (shift == nullptr))
    return CG_ERR_ARG;
  if (!cin_ok(cin) || !cout_ok(cout)) return CG_ERR_UNSUPPORTED;
  if (n_out == 0) return CG_OK;
  if (!nbr || !weight || !out || (n_in > 0 && !feats)) return CG_ERR_ARG;
  const int waves = (cout + 31) / 32;                       // 1 .. 4: one per 32 output channels
  const int cp = (cin + 7) & ~7;
  const size_t lds = (size_t)32 * (cp + 4) * sizeof(float);      // at most 29,184 B
  hipLaunchKernelGGL(sparse_conv_kernel<false>, dim3((unsigned)((n_out + 31) / 32)), dim3(64 * waves), lds, (hipStream_t)stream, feats,
                     (const float*)nullptr, cin, n_in, nbr, n_out, K, weight, bias, scale, shift, residual, cin, cout, out);
  return cg_hip_status(hipGetLastError());
}

// cg_sparse_conv over the row-wise concatenation [feats_a | feats_b], which is never formed (include/catgrasp_amd_pointgroup.h).
extern "C" int cg_sparse_conv_cat(const float* feats_a, int cin_a, const float* feats_b, int cin_b, long n_in, const int* nbr, long n_out, int K,
                                  const float* weight, const float* bias, const float* scale, const float* shift, const float* residual,
                                  int cout, float* out, void* stream) {
  if (n_in < 0 || n_out < 0 || n_in > (1L << 26) || n_out > (1L << 26) || (K != 1 && K != 8 && K != 27) || cin_a <= 0 || cin_b <= 0 || cout <= 0 ||
      (scale == nullptr) != (shift == nullptr))
    return CG_ERR_ARG;
  if (cin_a % 16 || cin_b % 16 || (long)cin_a + cin_b > CG_SPARSE_MAX_CIN || !cout_ok(cout)) return CG_ERR_UNSUPPORTED;
  if (n_out == 0) return CG_OK;
  if (!nbr || !weight || !out || (n_in > 0 && (!feats_a || !feats_b))) return CG_ERR_ARG;
  const int cin = cin_a + cin_b, waves = (cout + 31) / 32;
  const size_t lds = (size_t)32 * (cin + 4) * sizeof(float);
  hipLaunchKernelGGL(sparse_conv_kernel<true>, dim3((unsigned)((n_out + 31) / 32)), dim3(64 * waves), lds, (hipStream_t)stream, feats_a, feats_b,
                     cin_a, n_in, nbr, n_out, K, weight, bias, scale, shift, residual, cin, cout, out);
  return cg_hip_status(hipGetLastError());
}
