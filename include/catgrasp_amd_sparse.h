/* catgrasp_amd -- C ABI of the sparse 3-D convolution layers (submanifold, strided 2x2x2, inverse 2x2x2).
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * A sparse tensor is features (n, C) f32 and indices (n, 4) i32 rows [batch, d0, d1, d2] inside a grid of
 * batch_size x (s0, s1, s2).  The linear key of a site is ((batch*s0 + d0)*s1 + d1)*s2 + d2 (i64).
 *
 * A rule book is an output-stationary table nbr (n_out, K) i32: entry [i, k] is the input row that output
 * row i reads through kernel offset k (row-major (k0, k1, k2)), or -1.  The rule-book builders look sites
 * up by binary search in the ascending keys of the input sites: `sorted_keys` (n) i64 and `perm` (n) i64,
 * the row of every sorted key (a stable sort of the cg_sparse_keys output and its permutation).
 */
#ifndef CATGRASP_AMD_SPARSE_H
#define CATGRASP_AMD_SPARSE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* bits of *err_flag (i32, zeroed by the caller, only ever OR-ed into) */
#define CG_SPARSE_ERR_RANGE 1      /* a coordinate outside [0, shape) or a batch index outside [0, batch_size) */
#define CG_SPARSE_ERR_DUPLICATE 2  /* two rows name the same site */

/* channel limits of cg_sparse_conv */
#define CG_SPARSE_MAX_CIN 224
#define CG_SPARSE_MAX_COUT 112

/* Key and validation pass.  coarse = 0: keys[i] = linear key of row i in the grid (s0, s1, s2).
 * coarse = 1: keys[i] = linear key of the parent site [batch, d/2] in the grid ((s-2)/2+1 per axis) of a kernel-2 stride-2
 * convolution, or LLONG_MAX for a row that feeds no output (a coordinate >= 2*((s-2)/2+1): the last one of an odd axis).
 * Rows out of range set CG_SPARSE_ERR_RANGE and get key LLONG_MAX.  batch_size*s0*s1*s2 must fit an i64 with room to spare
 * (< 2^62), every s >= 1 (>= 2 for coarse). */
int cg_sparse_keys(const int* indices, long n, int batch_size, int s0, int s1, int s2, int coarse, long long* keys, int* err_flag,
                   void* stream);

/* Submanifold 3x3x3, padding 1: nbr (n, 27); outputs are the input rows in their order.  Offset k = (k0*3 + k1)*3 + k2 reads the
 * site at d + (k0-1, k1-1, k2-1) of the same batch item; a neighbour outside the grid on any axis is absent.  Equal adjacent
 * sorted keys set CG_SPARSE_ERR_DUPLICATE. */
int cg_sparse_rules_subm(const int* indices, const long long* sorted_keys, const long long* perm, long n, int s0, int s1, int s2,
                         int* nbr, int* err_flag, void* stream);

/* Kernel 2, stride 2, padding 0 over the input grid (s0, s1, s2).  out_keys: (n_out) i64 ascending distinct parent keys (the
 * coarse cg_sparse_keys output, made unique, without LLONG_MAX).  Writes out_indices (n_out, 4) i32 and nbr (n_out, 8): offset
 * k = (k0*2 + k1)*2 + k2 of output o reads the input site 2*o + (k0, k1, k2).  Equal adjacent sorted input keys set
 * CG_SPARSE_ERR_DUPLICATE. */
int cg_sparse_rules_down(const long long* out_keys, long n_out, const long long* sorted_keys, const long long* perm, long n_in,
                         int s0, int s1, int s2, int* out_indices, int* nbr, int* err_flag, void* stream);

/* Inverse of the kernel-2 stride-2 layer: outputs are its n_in input rows; nbr (n_in, 8) holds, at offset k = the row's
 * (d0%2, d1%2, d2%2), the row of its parent in out_keys, and -1 elsewhere; a row the strided layer dropped has no entry. */
int cg_sparse_rules_inverse(const int* indices, long n_in, const long long* out_keys, long n_out, int s0, int s1, int s2, int* nbr,
                            void* stream);

/* The fused gather-GEMM of all three layers:
 *   out[i] = bias + residual[i] + sum_k pro(feats[nbr[i,k]]) * weight[k]      (k ascending, absent entries skipped)
 * feats (n_in, cin) f32, nbr (n_out, K) i32 with entries in [-1, n_in), weight (K, cin, cout) f32, bias (cout) or NULL,
 * pro(x)[c] = max(x[c]*scale[c] + shift[c], 0) when scale and shift (cin) are given (both or neither), else x;
 * the product and the sum are rounded separately, and the max is C's fmaxf: a NaN in x, scale or shift gives 0, it is
 * not handed on as a ReLU on its own would (without a prologue a NaN reaches every column of the rows that read it);
 * the sum over k and the input channels is a chain of f32 fmaf from +0, then (sum + bias) + residual;
 * residual (n_out, cout) or NULL; out (n_out, cout), written once per row.  K in {1, 8, 27}.
 * cin in {6, multiples of 16 up to 224}, cout in {3, multiples of 16 up to 112}: anything else is CG_ERR_UNSUPPORTED.
 * Deterministic: every output row is one wave's fixed-order f32 sum, no atomics. */
int cg_sparse_conv(const float* feats, long n_in, const int* nbr, long n_out, int K, const float* weight, const float* bias,
                   const float* scale, const float* shift, const float* residual, int cin, int cout, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
