// Rule books of the sparse 3-D convolution layers (include/catgrasp_amd_sparse.h): output-stationary neighbour tables built by
// binary search in the sorted linear keys of the input sites.  No dense grid, no hash table, no atomics except the OR into the
// error flag: every table entry is a pure function of the inputs, so the tables are the same on every run.
//
//   keys      one i64 per row, ((b*s0 + d0)*s1 + d1)*s2 + d2; the caller sorts them (stable) and keeps the permutation
//   subm      one thread per (row, offset): neighbour coordinate, range check PER AXIS (so the last voxel of a row never finds
//             the first voxel of the next row, and batch items never touch), key, lower bound, perm
//   down      one thread per (output, offset) of the kernel-2 stride-2 layer: child site 2*o + k, the same lookup
//   inverse   one thread per fine row: its parent's row in the ascending output keys, stored at offset (d0%2, d1%2, d2%2)
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_sparse.h"
#include <limits.h>

namespace {

constexpr long long NO_KEY = LLONG_MAX;

// position of `key` in the ascending array a[0..n), or -1
__device__ __forceinline__ long find_key(const long long* __restrict__ a, long n, long long key) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(256) void keys_kernel(const int* __restrict__ indices, long n, int batch, int s0, int s1, int s2, int coarse,
                                                   long long* __restrict__ keys, int* __restrict__ err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = indices[i * 4], d0 = indices[i * 4 + 1], d1 = indices[i * 4 + 2], d2 = indices[i * 4 + 3];
  if (b < 0 || b >= batch || d0 < 0 || d0 >= s0 || d1 < 0 || d1 >= s1 || d2 < 0 || d2 >= s2) {
    atomicOr(err, CG_SPARSE_ERR_RANGE);
    keys[i] = NO_KEY;
    return;
  }
  if (!coarse) {
    keys[i] = (((long long)b * s0 + d0) * s1 + d1) * s2 + d2;
    return;
  }
  const int o0 = (s0 - 2) / 2 + 1, o1 = (s1 - 2) / 2 + 1, o2 = (s2 - 2) / 2 + 1;
  const int p0 = d0 >> 1, p1 = d1 >> 1, p2 = d2 >> 1;
  keys[i] = (p0 < o0 && p1 < o1 && p2 < o2) ? (((long long)b * o0 + p0) * o1 + p1) * o2 + p2 : NO_KEY;
}

__device__ __forceinline__ void flag_duplicate(const long long* __restrict__ sorted, long n, long i, int* __restrict__ err) {
  if (i + 1 < n && sorted[i] == sorted[i + 1] && sorted[i] != NO_KEY) atomicOr(err, CG_SPARSE_ERR_DUPLICATE);
}

__global__ __launch_bounds__(256) void rules_subm_kernel(const int* __restrict__ indices, const long long* __restrict__ sorted,
                                                         const long long* __restrict__ perm, long n, int s0, int s1, int s2,
                                                         int* __restrict__ nbr, int* __restrict__ err) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * 27) return;
  const long i = t / 27;
  const int k = (int)(t - i * 27);
  if (k == 0) flag_duplicate(sorted, n, i, err);
  const int b = indices[i * 4];
  const int d0 = indices[i * 4 + 1] + k / 9 - 1, d1 = indices[i * 4 + 2] + (k / 3) % 3 - 1, d2 = indices[i * 4 + 3] + k % 3 - 1;
  int r = -1;
  if (d0 >= 0 && d0 < s0 && d1 >= 0 && d1 < s1 && d2 >= 0 && d2 < s2) {
    const long p = find_key(sorted, n, (((long long)b * s0 + d0) * s1 + d1) * s2 + d2);
    if (p >= 0) r = (int)perm[p];
  }
  nbr[t] = r;
}

__global__ __launch_bounds__(256) void rules_down_kernel(const long long* __restrict__ out_keys, long n_out, const long long* __restrict__ sorted,
                                                         const long long* __restrict__ perm, long n_in, int s0, int s1, int s2,
                                                         int* __restrict__ out_indices, int* __restrict__ nbr, int* __restrict__ err) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < n_in) flag_duplicate(sorted, n_in, t, err);
  if (t >= n_out * 8) return;
  const long o = t >> 3;
  const int k = (int)(t & 7);
  const int o0 = (s0 - 2) / 2 + 1, o1 = (s1 - 2) / 2 + 1, o2 = (s2 - 2) / 2 + 1;
  long long key = out_keys[o];
  const int p2 = (int)(key % o2); key /= o2;
  const int p1 = (int)(key % o1); key /= o1;
  const int p0 = (int)(key % o0);
  const int b = (int)(key / o0);
  if (k == 0) {
    out_indices[o * 4] = b; out_indices[o * 4 + 1] = p0; out_indices[o * 4 + 2] = p1; out_indices[o * 4 + 3] = p2;
  }
  const int d0 = 2 * p0 + (k >> 2), d1 = 2 * p1 + ((k >> 1) & 1), d2 = 2 * p2 + (k & 1);      // < 2*o <= s on every axis
  const long p = find_key(sorted, n_in, (((long long)b * s0 + d0) * s1 + d1) * s2 + d2);
  nbr[t] = p >= 0 ? (int)perm[p] : -1;
}

__global__ __launch_bounds__(256) void rules_inverse_kernel(const int* __restrict__ indices, long n_in, const long long* __restrict__ out_keys,
                                                            long n_out, int s0, int s1, int s2, int* __restrict__ nbr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_in) return;
  const int o0 = (s0 - 2) / 2 + 1, o1 = (s1 - 2) / 2 + 1, o2 = (s2 - 2) / 2 + 1;
  const int b = indices[i * 4], d0 = indices[i * 4 + 1], d1 = indices[i * 4 + 2], d2 = indices[i * 4 + 3];
  const int p0 = d0 >> 1, p1 = d1 >> 1, p2 = d2 >> 1;
  long parent = -1;
  if (b >= 0 && d0 >= 0 && d1 >= 0 && d2 >= 0 && p0 < o0 && p1 < o1 && p2 < o2)
    parent = find_key(out_keys, n_out, (((long long)b * o0 + p0) * o1 + p1) * o2 + p2);
  const int mine = ((d0 & 1) << 2) | ((d1 & 1) << 1) | (d2 & 1);
#pragma unroll
  for (int k = 0; k < 8; ++k) nbr[i * 8 + k] = (k == mine) ? (int)parent : -1;
}

// the grid's cell count must leave an i64 key far from LLONG_MAX (the "no key" value)
bool grid_ok(int batch, int s0, int s1, int s2, int smin) {
  if (batch < 1 || s0 < smin || s1 < smin || s2 < smin) return false;
  long long cells = batch;
  return !__builtin_mul_overflow(cells, (long long)s0, &cells) && !__builtin_mul_overflow(cells, (long long)s1, &cells) &&
         !__builtin_mul_overflow(cells, (long long)s2, &cells) && cells < (1LL << 62);
}

unsigned blocks_for(long threads) { return (unsigned)((threads + 255) / 256); }
constexpr long MAX_ROWS = 1L << 26;       // 27 table entries per row stay far inside an i32 grid and i32 row numbers

}  // namespace

extern "C" int cg_sparse_keys(const int* indices, long n, int batch_size, int s0, int s1, int s2, int coarse, long long* keys, int* err_flag,
                              void* stream) {
  if (n < 0 || n > MAX_ROWS || (coarse != 0 && coarse != 1) || !grid_ok(batch_size, s0, s1, s2, coarse ? 2 : 1)) return CG_ERR_ARG;
  if (n == 0) return CG_OK;
  if (!indices || !keys || !err_flag) return CG_ERR_ARG;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, indices, n, batch_size, s0, s1, s2, coarse, keys,
                     err_flag);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_sparse_rules_subm(const int* indices, const long long* sorted_keys, const long long* perm, long n, int s0, int s1, int s2,
                                    int* nbr, int* err_flag, void* stream) {
  if (n < 0 || n > MAX_ROWS || !grid_ok(1, s0, s1, s2, 1)) return CG_ERR_ARG;
  if (n == 0) return CG_OK;
  if (!indices || !sorted_keys || !perm || !nbr || !err_flag) return CG_ERR_ARG;
  hipLaunchKernelGGL(rules_subm_kernel, dim3(blocks_for(n * 27)), dim3(256), 0, (hipStream_t)stream, indices, sorted_keys, perm, n, s0, s1,
                     s2, nbr, err_flag);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_sparse_rules_down(const long long* out_keys, long n_out, const long long* sorted_keys, const long long* perm, long n_in,
                                    int s0, int s1, int s2, int* out_indices, int* nbr, int* err_flag, void* stream) {
  if (n_out < 0 || n_in < 0 || n_out > n_in || n_in > MAX_ROWS || !grid_ok(1, s0, s1, s2, 2)) return CG_ERR_ARG;
  if (n_in == 0) return CG_OK;
  if (!sorted_keys || !perm || !err_flag || (n_out > 0 && (!out_keys || !out_indices || !nbr))) return CG_ERR_ARG;
  const long threads = n_out * 8 > n_in ? n_out * 8 : n_in;
  hipLaunchKernelGGL(rules_down_kernel, dim3(blocks_for(threads)), dim3(256), 0, (hipStream_t)stream, out_keys, n_out, sorted_keys, perm,
                     n_in, s0, s1, s2, out_indices, nbr, err_flag);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_sparse_rules_inverse(const int* indices, long n_in, const long long* out_keys, long n_out, int s0, int s1, int s2, int* nbr,
                                       void* stream) {
  if (n_in < 0 || n_out < 0 || n_in > MAX_ROWS || n_out > MAX_ROWS || !grid_ok(1, s0, s1, s2, 2)) return CG_ERR_ARG;
  if (n_in == 0) return CG_OK;
  if (!indices || !nbr || (n_out > 0 && !out_keys)) return CG_ERR_ARG;
  hipLaunchKernelGGL(rules_inverse_kernel, dim3(blocks_for(n_in)), dim3(256), 0, (hipStream_t)stream, indices, n_in, out_keys, n_out, s0, s1,
                     s2, nbr);
  return cg_hip_status(hipGetLastError());
}
