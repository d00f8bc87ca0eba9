/* catgrasp_amd -- C ABI of BatchNorm in batch-statistics mode fused with ReLU, forward and backward (the training-time form of the
 * `BatchNorm1d, ReLU` that the inference layers fold into a convolution's prologue).
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd_sparse_grad.h: every pointer is a DEVICE pointer, sizes
 * are element counts, `stream` is a hipStream_t passed as void*.  The functions are asynchronous on `stream`, never allocate,
 * never synchronise; they return 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive
 * hipError_t.
 *
 * x (n, c) f32, row-major.  c a multiple of 16 up to 224: anything else is CG_ERR_UNSUPPORTED.  2 <= n <= 16,777,216 (so that
 * (float)n is exact): anything else is CG_ERR_ARG.  A NULL pointer (but `dx`) is CG_ERR_ARG.  f32 only.  No atomics anywhere: every
 * result is a fixed-order f32 expression that depends on the values and the shapes alone, never on the device, the grid or the
 * timing.  The library is built with -ffp-contract=off: every operation written separately below is rounded separately, a product
 * and a sum are fused only where fmaf is written.  Divisions and square roots are the correctly rounded ones.
 *
 * Column sums.  Every per-channel sum S(t) over the n rows, of a term t(row) and a chain step, is formed as follows:
 *   the rows are cut into segments of CG_BN_SEG consecutive rows and chunks of CG_BN_ROWS consecutive rows (16 segments); the last
 *       segment and the last chunk may be shorter; the tree depends on n alone;
 *   a segment partial is one f32 chain from +0 over the segment's rows in ascending order, p = step(p, t(row));
 *   a chunk partial is the partial of its segment 0 with those of its segments 1, 2, ... added in ascending order;
 *   the total is the partial of chunk 0 with those of chunks 1, 2, ... added in ascending order; every add is rounded to f32.
 * The chunk partials go through `workspace` (cg_bn_workspace floats; its contents afterwards are unspecified).
 */
#ifndef CATGRASP_AMD_BN_H
#define CATGRASP_AMD_BN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* rows of one segment (one f32 chain) and of one chunk (CG_BN_ROWS / CG_BN_SEG segments) of the column sums */
#define CG_BN_SEG 64
#define CG_BN_ROWS 1024

/* Host only, launches nothing: the number of floats the two functions below need in `workspace`,
 *   2 * c * ceil(n / CG_BN_ROWS)
 * or a negative CG_ERR_* for the shapes they refuse. */
long cg_bn_workspace(long n, int c);

/* Forward.  Two passes over x for the statistics (not E[x^2] - mean^2), a third for y:
 *   mean   = S(x) / (float)n                 chain step p + x
 *   var    = S(d*d) / (float)n, d = x - mean chain step fmaf(d, d, p)             (the biased variance)
 *   invstd = 1.0f / sqrtf(var + eps)
 *   scale  = gamma * invstd
 *   shift  = beta - mean * scale
 *   y      = fmaxf(x * scale + shift, 0)
 * gamma, beta (c) inputs; mean, var, invstd, scale, shift (c) outputs; y (n, c).  Three launches, one workgroup per
 * (chunk, 64 channels); the second and third re-add the chunk partials of the pass before for their own channels. */
int cg_bn_relu_train_forward(const float* x, long n, int c, const float* gamma, const float* beta, float eps, float* workspace,
                             float* mean, float* var, float* invstd, float* scale, float* shift, float* y, void* stream);

/* Backward, for dy = d loss / d y (n, c) and the forward's mean, invstd, scale, shift:
 *   z      = x * scale + shift               exactly as in the forward: the mask is recomputed, not stored
 *   g      = z > 0 ? dy : 0
 *   xhat   = (x - mean) * invstd
 *   dbeta  = S(g)                            chain step p + g
 *   dgamma = S(g*xhat)                       chain step fmaf(g, xhat, p)
 *   k1     = dbeta / (float)n,  k2 = dgamma / (float)n
 *   dx     = scale * ((g - k1) - xhat * k2)
 * dgamma, dbeta (c) outputs; dx (n, c) or NULL: the input gradient is then not computed.  Two launches: the chunk partials, then
 * the totals (and dx, one workgroup per (chunk, 64 channels), each re-adding the partials of its own channels). */
int cg_bn_relu_train_backward(const float* x, const float* dy, long n, int c, const float* mean, const float* invstd,
                              const float* scale, const float* shift, float* workspace, float* dgamma, float* dbeta, float* dx,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
