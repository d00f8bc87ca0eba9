/* catgrasp_amd -- C ABI of the training form of PointNet's pooled layer
 *   out[b] = act( batch_norm( x[b] . W^T + bias ) ) reduced by max over the n points of cloud b        (act = ReLU or identity)
 * in closed form: the (clouds * n, c) activation z = x . W^T + bias is never stored, forward or backward.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd_dense.h: every pointer is a DEVICE pointer, sizes are
 * element counts, `stream` is a hipStream_t passed as void*.  The functions are asynchronous on `stream`, never allocate, never
 * synchronise; they return 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * x (clouds, n, cin) point-major, W (c, cin): f32, row-major.  f32 only; no atomics anywhere: every result is a fixed-order f32
 * expression that depends on the values and the shapes alone.  The library is built with -ffp-contract=off.
 *
 * Limits of every function below: cin a multiple of 8 in 8 .. CG_POOL_MAX_CIN and c a multiple of 32 in 32 .. CG_POOL_MAX_C (else
 * CG_ERR_UNSUPPORTED); clouds >= 1, n >= 1, 2 <= clouds * n <= 16,777,216 (else CG_ERR_ARG, judged before the widths); a NULL
 * required pointer or a misaligned x / w_packed (16 bytes) is CG_ERR_ARG.  Non-finite inputs give unspecified results.
 */
#ifndef CATGRASP_AMD_POOL_H
#define CATGRASP_AMD_POOL_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* rows of one chunk of a cloud's points, counted from the cloud's first row */
#define CG_POOL_ROWS 1024
#define CG_POOL_MAX_CIN 128
#define CG_POOL_MAX_C 1024

/* Host only, launches nothing: the number of 4-byte words cg_pool_extrema needs in `workspace`,
 *   4 * clouds * ceil(n / CG_POOL_ROWS) * c
 * or a negative CG_ERR_* for the shapes it refuses. */
long cg_pool_extrema_workspace(long clouds, long n, int c);

/* Per cloud and channel, the extremum over the cloud's points of z[b,i,ch] = chain(x[b,i], W[ch]) + bias[ch], and where it is:
 *   zsel[b,ch] = max_i z[b,i,ch]  where sign[ch] >= 0 (zero of either sign included, or sign == NULL),  min_i z[b,i,ch]  otherwise
 *   idx[b,ch]  = the smallest i that attains zsel[b,ch]
 * z is the bits cg_gemm_bias_act (catgrasp_amd.h) returns for that element: one f32 fmaf chain from +0 over k in the order of its
 * MFMA steps (for each block of eight 8q: 8q, 8q+4, 8q+1, 8q+5, 8q+2, 8q+6, 8q+3, 8q+7), then one f32 add of bias[ch] (bias == NULL:
 * of +0).  w_packed is W in the B-fragment order cg_gemm_bias_act reads (c is a multiple of 32: no padding rows).
 * Two launches.  The first gives one workgroup a chunk of CG_POOL_ROWS consecutive points of ONE cloud and 128 channels; it walks the
 * chunk in 32 x 32 accumulator tiles that are folded in registers, not stored, and writes (max, argmax, min, argmin) per (chunk,
 * channel) to `workspace` (cg_pool_extrema_workspace words; contents unspecified afterwards).  The second picks by `sign` and
 * reduces a cloud's chunks in ascending order.  Every comparison is strict, candidates are visited so that equal values keep the
 * smaller i.  Rows of a tile past the cloud's last point take no part. */
int cg_pool_extrema(const float* x, long clouds, long n, int cin, const float* w_packed, const float* bias, int c, const float* sign,
                    float* workspace, float* zsel, int* idx, void* stream);

/* Host only, launches nothing: the number of floats cg_pool_var needs in `workspace`, clouds * ceil(n / CG_POOL_ROWS) * c, or a
 * negative CG_ERR_* for the shapes it refuses. */
long cg_pool_var_workspace(long clouds, long n, int c);

/* The biased batch variance of z by a second sweep of cg_pool_extrema's tiles, for a given mean (c):
 *   var[ch] = fmaxf( (sum over all m = clouds * n rows of (z[r,ch] - mean[ch])^2) / (float)m, 0 )
 * with z the bits of cg_pool_extrema's z and d = z - mean one f32 subtraction.  Order of the sum: the rows are cut into the chunks
 * of cg_pool_extrema; within a chunk, and within every 32 rows 32t .. 32t + 31 of it, the rows 0-3, 8-11, 16-19, 24-27 belong to the
 * lower chain and 4-7, 12-15, 20-23, 28-31 to the upper; each chain is p = fmaf(d, d, p) from +0 over its rows of the whole chunk in
 * ascending order; the chunk's partial is lower + upper; the partials are added in ascending (cloud, chunk) order, starting from
 * the first.  Two launches; `workspace` holds the partials. */
int cg_pool_var(const float* x, long clouds, long n, int cin, const float* w_packed, const float* bias, int c, const float* mean,
                float* workspace, float* var, void* stream);

/* Batch statistics of z and the pooled output, from the column mean xbar (cin) of the m = clouds * n rows of x and EITHER the variance
 * var_in (c) that cg_pool_var returns OR, with var_in == NULL, the centred Gram matrix s (cin, cin) of the rows.  One lane per channel
 * ch, every chain ascending in its index from +0:
 *   p = fmaf(W[ch,k], xbar[k], p) over k;                       mean = p + bias[ch]            (bias == NULL: p + 0)
 *   var = var_in[ch], or from s:
 *   t_j = chain over k of fmaf(W[ch,k], s[k,j], t);  q = fmaf(t_j, W[ch,j], q) over j;          var = fmaxf(q / (float)m, 0)
 *   invstd = 1 / sqrtf(var + eps);   scale = gamma * invstd;   shift = beta - mean * scale
 *   out[b,ch] = zsel[b,ch] * scale + shift (two roundings), then fmaxf(., 0) when relu != 0
 * mean, var, invstd, scale, shift (c each) and out (clouds, c) are written.  With s == NULL and var_in == NULL only mean is written
 * (what cg_pool_var needs) and every pointer but w, xbar and mean may be NULL.  The route through s costs no sweep, but its relative
 * error grows with |W[ch]|^2 lambda_max(s) / (m var[ch]): it is kept for inputs known to be well spread. */
int cg_pool_stats(const float* w, const float* bias, const float* xbar, const float* s, const float* var_in, const float* gamma,
                  const float* beta, float eps, long clouds, long n, int cin, int c, const float* zsel, int relu, float* mean, float* var,
                  float* invstd, float* scale, float* shift, float* out, void* stream);

/* t (c, cin)[ch,k] = sum over the clouds of coef[b,ch] * x[b, idx[b,ch], k]: one chain p = fmaf(coef[b,ch], x[b,idx[b,ch],k], p) from
 * +0 over b ascending.  coef (clouds, c), idx (clouds, c) with 0 <= idx < n (an index outside is skipped). */
int cg_pool_wgrad_gather(const float* x, long clouds, long n, int cin, const float* coef, const int* idx, int c, float* t, void* stream);

/* dx[b, idx[b,ch], k] = fmaf(coef[b,ch], W[ch,k], dx[b, idx[b,ch], k]) for every (b, ch), onto an existing dx (clouds, n, cin): for
 * each row the additions come in ascending ch (two channels of a cloud may select the same row; one wave owns the row's whole
 * chain).  An index outside 0 .. n-1 is skipped. */
int cg_pool_dgrad_scatter(const float* coef, const int* idx, const float* w, long clouds, long n, int cin, int c, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
