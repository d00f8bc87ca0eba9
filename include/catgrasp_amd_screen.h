/* catgrasp_amd -- C ABI of the screened form of the fused per-point pass (cg_pointmlp_max of catgrasp_amd.h).
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE pointer, sizes are element
 * counts, `stream` is a hipStream_t passed as void*.  The function is asynchronous on `stream`, never allocates, never synchronises;
 * it returns 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 */
#ifndef CATGRASP_AMD_SCREEN_H
#define CATGRASP_AMD_SCREEN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cg_pointmlp_max with the SAME output bits at less matrix work.  On the throughput path (more than 256 workgroups) the 128 -> 1024
 * layer of a 64-point tile is screened with three bf16 MFMAs per 16 input channels; a (point, channel) pair is recomputed with the
 * exact f32 fmaf chain only if a proven error bound leaves it able to reach the channel's maximum.  A tile whose
 * list of such pairs overflows, whose activations leave the bound's range (row norm above 2^30 or not finite), or that is the first
 * of its workgroup runs the exact stream of cg_pointmlp_max inside the same kernel; smaller calls run cg_pointmlp_max's kernels.
 * w3_split: the bf16 hi / lo image of the 128 -> 1024 weights (folding.pack_b_split, as cg_pointmlp_max_bf16x3's w3_split), 16-byte
 * aligned.  w3_norm: (1025) f32, [c] an upper bound of ||W3[c]||_2 and [1024] their maximum (folding.screen_norms); above 2^30 every
 * tile runs the exact stream.  stats: optional device long long[8], zeroed by the caller, accumulated with atomics: [0] tiles
 * screened, [1] tiles sent to the exact stream by an overflowing list, [2] by the range, [3] as first tiles, [4] pairs recomputed,
 * [5] the f32 bits of max |screen value - exact value| / bound over those pairs, [6] tiles under force 1.  force: 0 normal, 1 exact
 * stream for every tile, 2 screen first tiles too (tests).  Other arguments as cg_pointmlp_max. */
int cg_pointmlp_max_screened(const float* x, int B, int N, const float* t3, const float* w1, const float* b1,
                             int mid_mode, const float* wm_packed, const float* bm, const float* t64,
                             const float* w2_packed, const float* b2, const float* w3_packed, const float* b3,
                             int relu3, int nsplit, float* out, float* pointfeat, const unsigned short* w3_split,
                             const float* w3_norm, long long* stats, int force, void* stream);

#ifdef __cplusplus
}
#endif
#endif
