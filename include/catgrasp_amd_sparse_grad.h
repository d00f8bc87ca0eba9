/* catgrasp_amd -- C ABI of the gradients of the sparse 3-D convolution layers (weight, bias, input).
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd_sparse.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * The operator differentiated is cg_sparse_conv without prologue and residual:
 *   out[i] = bias + sum_k feats[nbr[i,k]] * weight[k]
 * feats (n_in, cin) f32, nbr (n_out, K) i32 with entries in [-1, n_in) (-1: absent, contributes nothing), weight (K, cin, cout)
 * f32, dy = d loss / d out (n_out, cout) f32.  K in {1, 8, 27}, cin in {6, multiples of 16 up to 224}, cout in {3, multiples of
 * 16 up to 112}, as in cg_sparse_conv: anything else is CG_ERR_UNSUPPORTED.  f32 only.  No atomics anywhere: every result is a
 * fixed-order f32 sum that depends on the shapes alone, never on the device, the grid or the timing.
 */
#ifndef CATGRASP_AMD_SPARSE_GRAD_H
#define CATGRASP_AMD_SPARSE_GRAD_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* rows of one chunk of the weight and bias gradients' reduction over the n_out rows */
#define CG_SPARSE_GRAD_ROWS 1024

/* Host only, launches nothing: the number of floats cg_sparse_conv_wgrad needs in `workspace`,
 *   chunks * (K*cin*cout + cout)   with chunks = ceil(n_out / CG_SPARSE_GRAD_ROWS)
 * (0 for n_out = 0), or a negative CG_ERR_* for the arguments cg_sparse_conv_wgrad refuses. */
long cg_sparse_wgrad_workspace(long n_out, int K, int cin, int cout);

/* Weight and bias gradient:
 *   dw[k] (cin, cout) = sum over the rows i with nbr[i,k] >= 0 of feats[nbr[i,k]]^T * dy[i]        db[o] = sum_i dy[i,o]
 * The rows are cut into chunks of CG_SPARSE_GRAD_ROWS consecutive rows (the last one may be shorter); the number of chunks depends
 * on n_out alone.  Order of every sum:
 *   partial of chunk c for dw[k,ci,o]: a chain of f32 fmaf from +0 over the chunk's rows in ascending row order,
 *       p = fmaf(feats[nbr[i,k], ci], dy[i,o], p), rows without a neighbour at k skipped (a chunk with none gives +0);
 *   partial of chunk c for db[o]: the same chain with 1 in the place of the feature, p = fmaf(1, dy[i,o], p) = p + dy[i,o], over
 *       every row of the chunk in ascending order;
 *   dw[k,ci,o] and db[o]: the partial of chunk 0, then the partials of chunks 1, 2, ... added to it in ascending chunk order, each
 *       add rounded to f32.
 * The partials are written to `workspace` (cg_sparse_wgrad_workspace floats; its contents afterwards are unspecified) by one
 * launch, one workgroup per (chunk, offset, 32 input channels), and summed by a second one.
 * dw (K, cin, cout) or NULL, db (cout) or NULL (not both NULL): a gradient that is not asked for is not computed.
 * n_out = 0 writes zeros to dw and db and is CG_OK; workspace may then be NULL.  feats may be NULL when n_in = 0. */
int cg_sparse_conv_wgrad(const float* feats, long n_in, const int* nbr, long n_out, int K, const float* dy, int cin, int cout,
                         float* workspace, float* dw, float* db, void* stream);

/* Input gradient, as the forward operator over the transposed rule book:
 *   dx[j] = sum_k dy[nbr_t[j,k]] * weight_t[k]      (k ascending, absent entries skipped)
 * nbr_t (n_in, K) i32 with entries in [-1, n_out): nbr_t[j,k'] = i exactly when nbr[i,k] = j, for the layer's pairing of k' with k;
 * weight_t (K, cout, cin): weight_t[k'] = weight[k]^T.  (Submanifold 3x3x3: nbr_t = nbr, k' = 26 - k.  Strided layer: nbr_t = the
 * table of cg_sparse_rules_inverse, k' = k.  Inverse layer: nbr_t = the strided layer's table, k' = k.  K = 1: nbr_t = nbr.)
 * dx (n_in, cin), every row written once by one wave (zeros for a row that no output read).  Every element is one chain of f32
 * fmaf from +0: k ascending, and inside an offset the channels of dy in the order of cg_sparse_conv's MFMA steps (for each
 * block of eight channels 8q: 8q, 8q+4, 8q+1, 8q+5, 8q+2, 8q+6, 8q+3, 8q+7, channels >= cout left out).
 * n_in = 0 is CG_OK; dy may be NULL when n_out = 0 (dx is then all zeros). */
int cg_sparse_conv_dgrad(const float* dy, long n_out, const int* nbr_t, long n_in, int K, const float* weight_t, int cin, int cout,
                         float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
