/* catgrasp_amd -- C ABI of the NUNOCS training objective: the cross-entropy over coordinate bins, minimised over an object
 * category's symmetries (NocsMinSymmetryCELoss, loss.py:16-45, called by trainer_nunocs.py:52,81), forward and backward.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd_bn.h: every pointer is a DEVICE pointer, sizes are element
 * counts, `stream` is a hipStream_t passed as void*.  The functions are asynchronous on `stream`, never allocate, never synchronise;
 * they return 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * pred    the logits, logically (B, N, 3, bins), f32, in one of two storages (`layout`):
 *           CG_NOCS_CHANNEL_MAJOR  (B, 3*bins, N) contiguous: element (b, n, a, k) at (b*3*bins + a*bins + k)*N + n
 *                                  (what conv4(h).permute(0, 2, 1) of the training forward is, pointnet2.py:231)
 *           CG_NOCS_POINT_MAJOR    (B, N, 3*bins) contiguous: element (b, n, a, k) at (b*N + n)*3*bins + a*bins + k
 *         Neither is copied or transposed; the gradient comes back in the storage of its input.
 * target  (B, N, 3) f32, the NOCS coordinates in [0, 1].  tfs (S, 4, 4) f32 row-major, the symmetry transforms.
 *
 * Limits.  1 <= bins <= CG_NOCS_MAX_BINS, 1 <= S <= CG_NOCS_MAX_SYM, B <= 65535: beyond them CG_ERR_UNSUPPORTED.  B >= 1,
 * 1 <= N <= 16,777,216 (so that (float)N is exact), `layout` one of the two, no NULL pointer (but `lse` of the forward): otherwise
 * CG_ERR_ARG.  Every index is 64-bit, so B*N*3*bins has no bound of its own.  f32 only.  No atomics anywhere: every result is a
 * fixed-order f32 expression of the values and the shapes, never of the device, the grid or the timing.  The library is built with
 * -ffp-contract=off: every operation written separately below is rounded separately, a product and a sum are fused only where fmaf is
 * written.  Divisions are the correctly rounded ones.
 *
 * The bins.  For point (b, n), symmetry s and axis a, with T = tfs[s] and t = target[b, n]:
 *   c_j = t_j - 0.5f                                                                  j = 0, 1, 2
 *   r_a = fmaf(T[a][2], c_2, fmaf(T[a][1], c_1, fmaf(T[a][0], c_0, T[a][3]))) + 0.5f
 *   q   = r_a * (float)bins
 *   k_a = (int)fminf(fmaxf(q, 0.0f), (float)(bins - 1))                               clamped, then truncated toward zero
 * (loss.py:31-33 forms r by a torch.matmul whose summation order torch does not state, and q by a division by 1/bins; this chain is
 * the definition here.  A NaN q gives bin 0.)
 *
 * The log-sum-exp of one (b, n, a), x = the row's `bins` logits:
 *   m   = the maximum of x
 *   e_k = expf(x_k - m)
 *   sum = channel-major: p_w = the chain from +0 over k = w, w + 4, w + 8, ... ascending, w = 0..3; sum = (p_0 + p_1) + (p_2 + p_3)
 *         point-major:   u_l = e_l + e_(l + 64), l = 0..63 (an e_k with k >= bins is +0); then six rounds d = 32, 16, 8, 4, 2, 1 of
 *                        u_l <- u_l + u_(l xor d); sum = u_0
 *   lse = m + logf(sum)
 * expf and logf are the device library's; the two storages sum in different orders, so their lse may differ in the last bits.
 *
 * The loss, from lse as stored:
 *   v[b, n, s] = ((lse_0 - x_0[k_0]) + (lse_1 - x_1[k_1])) + (lse_2 - x_2[k_2])        loss.py:38-40
 *   L[b, s]    = P(b, s) / (float)N                                                    loss.py:41
 *   ids[b]     = the first s at which L[b, s] is smallest (a NaN is never smaller)     loss.py:42
 *   loss       = (the chain from +0 over b ascending of L[b, ids[b]]) / (float)B       loss.py:43-44
 * Row sums.  P(b, s) is formed as follows: the N points are cut into segments of CG_NOCS_SEG consecutive points, the last may be
 * shorter; a segment partial is one f32 chain from +0 over the segment's points in ascending order, p = p + v; P is the partial of
 * segment 0 with those of segments 1, 2, ... added in ascending order.  The segment partials go through `workspace`
 * (cg_nocs_symce_workspace_floats; its contents afterwards are unspecified).  Given lse, the tree is the same in both storages.
 */
#ifndef CATGRASP_AMD_LOSS_H
#define CATGRASP_AMD_LOSS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* points of one segment (one f32 chain) of the row sums; the caps on bins (the decode's own, cg_nunocs_decode) and on symmetries */
#define CG_NOCS_SEG 64
#define CG_NOCS_MAX_BINS 128
#define CG_NOCS_MAX_SYM 128

/* storage of the logits and of their gradient */
#define CG_NOCS_CHANNEL_MAJOR 0
#define CG_NOCS_POINT_MAJOR 1

/* Host only, launches nothing: the number of floats the forward needs in `workspace`,
 *   B * ceil(N / CG_NOCS_SEG) * S
 * or a negative CG_ERR_* for the shapes it refuses (bins is not part of the size: pass the one of the call). */
long cg_nocs_symce_workspace_floats(long B, long N, int bins, int S);

/* Forward (loss.py:29-45).  Outputs: loss (1), ids (B) int32, L (B, S), lse (B, N, 3) or NULL: a forward-only call (the validation
 * loop, trainer_nunocs.py:81) keeps no lse.  Three launches: the segment partials (one read of pred), L and ids (one workgroup per
 * sample), loss. */
int cg_nocs_symce_forward(const float* pred, int layout, const float* target, const float* tfs, long B, long N, int bins, int S,
                          float* workspace, float* loss, int* ids, float* L, float* lse, void* stream);

/* Backward (what autograd derives from loss.py:35-44), for g = d / d loss read from grad_loss (1) on the device, the forward's lse
 * and ids, and the bins k_a of symmetry ids[b] recomputed by the chain above:
 *   coef = g / ((float)B * (float)N)
 *   grad_pred[b, n, a, k] = coef * (expf(x - lse_a) - (k == k_a ? 1.0f : 0.0f))
 * grad_pred has pred's storage; every element is written.  No gradient flows to target.  One launch: one read of pred, one write. */
int cg_nocs_symce_backward(const float* pred, int layout, const float* target, const float* tfs, const float* lse, const int* ids,
                           const float* grad_loss, long B, long N, int bins, int S, float* grad_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif
