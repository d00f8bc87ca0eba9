/* catgrasp_amd -- C ABI of what the assembled PointGroup network needs beyond the sparse layers of catgrasp_amd_sparse.h.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 */
#ifndef CATGRASP_AMD_POINTGROUP_H
#define CATGRASP_AMD_POINTGROUP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* cg_sparse_conv (catgrasp_amd_sparse.h) over the row-wise concatenation [feats_a | feats_b], which is never formed:
 *   out[i] = bias + residual[i] + sum_k pro([feats_a | feats_b][nbr[i,k]]) * weight[k]
 * feats_a (n_in, cin_a) f32 and feats_b (n_in, cin_b) f32 hold the same rows in the same order; weight (K, cin_a+cin_b, cout),
 * scale and shift (cin_a+cin_b, both or neither); nbr, bias, residual, out, K as for cg_sparse_conv.  The gather reads channels
 * [0, cin_a) of a row from feats_a and the others from feats_b; tile, product chain, offset order and epilogue are those of
 * cg_sparse_conv, so the result has the same bits as cg_sparse_conv on the concatenated matrix.
 * cin_a and cin_b positive (else CG_ERR_ARG); multiples of 16 with cin_a + cin_b <= 224 (CG_SPARSE_MAX_CIN), cout in
 * {3, multiples of 16 up to 112}: anything else is CG_ERR_UNSUPPORTED.  A null feats_a or feats_b with rows to read is CG_ERR_ARG. */
int cg_sparse_conv_cat(const float* feats_a, int cin_a, const float* feats_b, int cin_b, long n_in, const int* nbr, long n_out, int K,
                       const float* weight, const float* bias, const float* scale, const float* shift, const float* residual, int cout,
                       float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
