/* catgrasp_amd -- C ABI of the gradients of a dense (per-row) layer y = x . W^T + bias [+ row_bias[row / rows_per_group]], and of
 * BatchNorm + ReLU in batch-statistics mode at the widths of PointNetSeg's per-point head.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd_bn.h: every pointer is a DEVICE pointer, sizes are element
 * counts, `stream` is a hipStream_t passed as void*.  The functions are asynchronous on `stream`, never allocate, never
 * synchronise; they return 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * x (n, cin), dy = d loss / d y (n, cout), W (cout, cin): f32, row-major, 16-byte aligned.  f32 only, on v_mfma_f32_32x32x2_f32
 * (exact f32: D = fmaf(a1, b1, fmaf(a0, b0, C))).  No atomics anywhere: every result is a fixed-order f32 expression that depends on
 * the values and the shapes alone, never on the device, the grid or the timing.  The library is built with -ffp-contract=off.
 * The forward of the layer is cg_gemm_bias_act (catgrasp_amd.h), unchanged.
 */
#ifndef CATGRASP_AMD_DENSE_H
#define CATGRASP_AMD_DENSE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* rows of one chunk of the weight and bias gradients' reduction over the n rows */
#define CG_DENSE_GRAD_ROWS 1024
/* widest layer (input or output channels) of every function below */
#define CG_DENSE_MAX_C 1024

/* Host only, launches nothing: the number of floats cg_dense_wgrad needs in `workspace`,
 *   chunks * (cout*cin + cout)   with chunks = ceil(n / CG_DENSE_GRAD_ROWS)
 * or a negative CG_ERR_* for the shapes cg_dense_wgrad refuses. */
long cg_dense_wgrad_workspace(long n, int cin, int cout);

/* Weight and bias gradient:
 *   dw (cout, cin) = dy^T . x        db (cout) = sum over the rows of dy
 * cin a multiple of 8 up to CG_DENSE_MAX_C, cout a multiple of 4 up to CG_DENSE_MAX_C: anything else is CG_ERR_UNSUPPORTED.
 * 1 <= n <= 16,777,216: anything else is CG_ERR_ARG, as is a NULL or misaligned x / dy / workspace.
 * The rows are cut into chunks of CG_DENSE_GRAD_ROWS consecutive rows (the last one may be shorter); the number of chunks depends on
 * n alone.  Order of every sum:
 *   partial of chunk c for dw[o,ci]: one chain of f32 fmaf from +0 over the chunk's rows in ascending row order,
 *       p = fmaf(dy[i,o], x[i,ci], p);
 *   partial of chunk c for db[o]: the same chain with 1 in the place of the input, p = fmaf(1, dy[i,o], p) = p + dy[i,o];
 *   dw[o,ci] and db[o]: the partial of chunk 0, then the partials of chunks 1, 2, ... added to it in ascending chunk order, each
 *       add rounded to f32.
 * The partials are written to `workspace` (cg_dense_wgrad_workspace floats; its contents afterwards are unspecified) by one launch,
 * one workgroup per (chunk, 128 output channels, up to 128 input channels), and summed by a second one.
 * dw (cout, cin) or NULL, db (cout) or NULL (not both NULL): a gradient that is not asked for is not computed (x may be NULL when
 * dw is). */
int cg_dense_wgrad(const float* x, const float* dy, long n, int cin, int cout, float* workspace, float* dw, float* db, void* stream);

/* Input gradient:
 *   dx (n, cin) = dy . W
 * cin and cout multiples of 4 up to CG_DENSE_MAX_C (else CG_ERR_UNSUPPORTED), 1 <= n <= 16,777,216 (else CG_ERR_ARG).  W is read as it
 * is stored (row-major (cout, cin): a row of W is the MFMA's operand layout, nothing is packed or transposed).
 * The contraction runs over the cout columns of dy, PADDED with zeros to a multiple of 8 inside the kernel (cout = 300 takes 38
 * steps of 8, the last with four columns of zeros): nothing is copied and a padded column adds a zero product, which leaves the
 * chain's value as it is.  Every element dx[i,ci] is one chain of f32 fmaf from +0, p = fmaf(dy[i,o], W[o,ci], p), with o in the
 * order of cg_gemm_bias_act's MFMA steps: for each block of eight columns 8q: 8q, 8q+4, 8q+1, 8q+5, 8q+2, 8q+6, 8q+3, 8q+7, columns
 * >= cout left out. */
int cg_dense_dgrad(const float* dy, long n, int cout, const float* w, int cin, float* dx, void* stream);

/* Host only, launches nothing: the number of floats cg_dense_group_sums needs in `workspace`,
 *   groups * c * ceil(rows_per_group / CG_BN_ROWS)
 * or a negative CG_ERR_* for the shapes it refuses. */
long cg_dense_group_sums_workspace(long groups, long rows_per_group, int c);

/* Per-group column sums, the gradient of the layer's row_bias:
 *   sums (groups, c)[g] = sum over the rows [g * rows_per_group, (g + 1) * rows_per_group) of dy (groups * rows_per_group, c)
 * c a multiple of 4 up to CG_DENSE_MAX_C (else CG_ERR_UNSUPPORTED); groups >= 1, rows_per_group >= 1, groups * rows_per_group <=
 * 16,777,216 (else CG_ERR_ARG).  Every sum is the column-sum tree of catgrasp_amd_bn.h applied to the group's rows alone: the
 * group's rows are cut into segments of CG_BN_SEG (64) and chunks of CG_BN_ROWS (1024) rows, counted from the group's first row; a
 * segment partial is one chain p = p + dy from +0 over its rows ascending; a chunk partial is the partial of its segment 0 with
 * the others added in ascending order; the sum is the partial of chunk 0 with the others added in ascending order.  One launch
 * for rows_per_group <= 1024 (workspace may then be NULL), two otherwise. */
int cg_dense_group_sums(const float* dy, long groups, long rows_per_group, int c, float* workspace, float* sums, void* stream);

/* BatchNorm + ReLU in batch-statistics mode for c a multiple of 16 up to CG_DENSE_MAX_C: the kernels, the arithmetic and the tree of
 * cg_bn_workspace / cg_bn_relu_train_forward / cg_bn_relu_train_backward (catgrasp_amd_bn.h has the contract; only the limit on c
 * differs).  At c <= 224 the results are the bits of those functions. */
long cg_bn_wide_workspace(long n, int c);
int cg_bn_relu_train_forward_wide(const float* x, long n, int c, const float* gamma, const float* beta, float eps, float* workspace,
                                  float* mean, float* var, float* invstd, float* scale, float* shift, float* y, void* stream);
int cg_bn_relu_train_backward_wide(const float* x, const float* dy, long n, int c, const float* mean, const float* invstd,
                                   const float* scale, const float* shift, float* workspace, float* dgamma, float* dbeta, float* dx,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
