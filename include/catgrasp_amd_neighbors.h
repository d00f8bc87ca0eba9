/* catgrasp_amd -- C ABI of the grid index: radius-bounded neighbour queries and oriented normals for ANY point cloud.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * They replace, for a cloud without a pixel grid, open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) +
 * correct_pcd_normal_direction (Utils.py:205-213; run_grasp_simulation.py:209,247), cKDTree.query(k=1, distance_upper_bound=) and
 * cKDTree.query_ball_point(..., return_length=True) (Utils.py:482-488).
 *
 * THE GRID.  A uniform lattice of `cell`-sized cells whose corner is `origin` (the per-axis minimum of the points).  The cell
 * coordinate of a value x on an axis is
 *     c(x) = min(max(floor(((x - origin) / cell)), 0), ext - 1)       in float64, every operation rounded once,
 * and the key of a point is (c(z) * ext_y + c(y)) * ext_x + c(x), which needs ext_x * ext_y * ext_z < 2^62.  The caller sorts the points
 * by (key, original index) and hands every query function the three sorted tables:
 *     sorted_points (n,3) f64   the coordinates (f32 coordinates widened: exact),
 *     sorted_index  (n)   i32   the original index of every sorted point,
 *     sorted_keys   (n)   i64   the keys, ascending.
 * A query at q with radius r looks, per axis, at the cells c(lo) .. c(hi), lo = the double below fl(q - r (1 + 2^-40)), hi = the double
 * above fl(q + r (1 + 2^-40)): c is monotone, so these cells hold every point whose d2 can pass the test below, rounding included.
 * With r <= cell (required) that is at most 4 cells per axis, 3 unless q +- r is within rounding of a cell face; the cells along x
 * have consecutive keys, so one binary search per (y, z) pair finds them.  No lookup reads outside the tables, wherever q lies.
 * The results depend on the points, the queries and the radius only: never on `cell`, the origin or the extents.
 *
 * IN RANGE, everywhere: d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius with d = p_j - q, in float64 from the exact coordinates, every
 * operation rounded separately (no fused multiply-add).  radius*radius must be a normal float64.
 */
#ifndef CATGRASP_AMD_NEIGHBORS_H
#define CATGRASP_AMD_NEIGHBORS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* The largest max_nn of cg_grid_normals: the selected neighbours of a query are kept as a list in LDS (12 bytes each, 64 queries per
 * workgroup: 48 KiB at the limit).  A larger max_nn is CG_ERR_UNSUPPORTED. */
#define CG_NB_MAX_NN 64

/* Keys of n points (or queries: a point outside the lattice takes the key of the nearest cell).  points: (n,3) f32, or f64 if
 * points_f64.  keys: (n) i64. */
int cg_grid_cell_keys(const void* points, int points_f64, long n, double origin_x, double origin_y, double origin_z, double cell, long ext_x,
                      long ext_y, long ext_z, long long* keys, void* stream);

/* Oriented normals of every point of the indexed cloud, written at the point's ORIGINAL index.  Per point q:
 *   candidates  every point j (q included; a duplicate of q is a candidate of its own) in range;
 *   neighbours  the max_nn candidates of smallest d2; exact ties at the last place go to the smaller original index;
 *   moments     sums of d and d d^T about q, accumulated in ASCENDING ORIGINAL INDEX;
 *   raw normal  (0,0,1) with fewer than 3 neighbours; otherwise the unit eigenvector of the smallest eigenvalue of the neighbours'
 *               covariance about their own mean (divided by their number), by cyclic Jacobi rotations;
 *   orientation n <- n / (|n| + 1e-10); n <- -n where ((vp - p) / |vp - p|) . n < 0, vp = (view_x, view_y, view_z).
 * These are the semantics of cg_organized_normals (catgrasp_amd_scene.h) with "row-major pixel index" read as "original index", and
 * the arithmetic after the search is the same code: on the used points of a depth image, in row-major order, the outputs are the
 * same bits.  normals: (n,3) f64.  nb_count: (n) i32 number of neighbours, nb_d2max: (n) f64 their largest d2; either may be NULL.
 * max_nn < 1 is CG_ERR_ARG, max_nn > CG_NB_MAX_NN is CG_ERR_UNSUPPORTED; radius > cell is CG_ERR_ARG. */
int cg_grid_normals(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                    double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, double radius, int max_nn,
                    double view_x, double view_y, double view_z, double* normals, int* nb_count, double* nb_d2max, void* stream);

/* Per query (any point, in the cloud or not): the in-range point of smallest d2, exact ties going to the smaller original index.
 * queries: (m,3) f32, or f64 if queries_f64.  query_order: (m) i32, a permutation of 0..m-1 -- thread t answers query query_order[t],
 * so that with the queries sorted by cg_grid_cell_keys the lanes of a wave scan the same cells; NULL is the identity.  The outputs
 * are written at the query's own index: nn_index (m) i32, -1 without a point in range; nn_d2 (m) f64, +infinity then. */
int cg_grid_nearest_within(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                           double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                           int queries_f64, const int* query_order, long m, double radius, int* nn_index, double* nn_d2, void* stream);

/* Per query, the number of points in range.  count: (m) i32; the other arguments as above. */
int cg_grid_count_within(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                         double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                         int queries_f64, const int* query_order, long m, double radius, int* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
