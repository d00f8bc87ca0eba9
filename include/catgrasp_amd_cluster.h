/* catgrasp_amd -- C ABI of the scene-to-objects clustering step (MeanShift on the device).
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * They replace the body of sklearn.cluster.MeanShift.fit as the reference calls it
 * (predicter.py:332: MeanShift(bandwidth, cluster_all=True, seeds=None).fit_predict(xyz_shifted)).
 */
#ifndef CATGRASP_AMD_CLUSTER_H
#define CATGRASP_AMD_CLUSTER_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* cg_meanshift_climb `route` values.  AUTO stages the points in LDS when cg_meanshift_lds_max_points allows it;
 * LDS and STREAMED force one route (tests: both give bitwise identical outputs); LDS with too many points is CG_ERR_ARG. */
#define CG_MEANSHIFT_ROUTE_AUTO 0
#define CG_MEANSHIFT_ROUTE_LDS 1
#define CG_MEANSHIFT_ROUTE_STREAMED 2

/* Largest point count that the seed climb stages in LDS: 160 KiB / 12 B (f32 points) or / 24 B (f64 points).  Host only. */
int cg_meanshift_lds_max_points(int pts_is_f64);

/* The seed climb of mean shift with a flat kernel (_mean_shift_single_seed of scikit-learn, one wavefront per seed).
 * pts: (n,3) f32, or f64 if pts_is_f64.  seeds: (n_seeds,3) f64.  Per seed, all in float64, repeat: the points with
 * |p - mean|^2 <= bandwidth^2 are counted and averaged; no point -> stop (count 0, the seed is empty);
 * |mean - old mean| <= 1e-3 * bandwidth or completed iterations == max_iter -> stop; otherwise one more completed iteration.
 * means: (n_seeds,3) f64 final mean.  counts: (n_seeds) i32 size of the last radius query.  iters: (n_seeds) i32 completed
 * iterations.  The outputs depend on the inputs only: not on the grid, the workgroup size or the route. */
int cg_meanshift_climb(const void* pts, int pts_is_f64, int n, const double* seeds, long n_seeds, double bandwidth, int max_iter,
                       int route, double* means, int* counts, int* iters, void* stream);

/* The greedy duplicate removal of MeanShift.fit.  sorted_centers: (m,3) f64 in scikit-learn's order (by (count, (x,y,z))
 * descending).  Walking them in order, a center that no kept center has suppressed is kept and suppresses every later
 * center within `bandwidth` of it (float64, <=).  keep: (m) u8, 1 for a kept center.  One workgroup. */
int cg_meanshift_merge(const double* sorted_centers, int m, double bandwidth, unsigned char* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif
