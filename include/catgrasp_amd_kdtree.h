/* catgrasp_amd -- C ABI of the exact searches on the grid index that a k-d tree is used for: the unbounded nearest neighbour
 * (cKDTree.query(x), no distance_upper_bound) and the index lists of cKDTree.query_ball_point.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE pointer, sizes are element
 * counts, `stream` is a hipStream_t passed as void*.  The functions are asynchronous on `stream`, never allocate, never synchronise;
 * they return 0 (CG_OK), a negative CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * THE GRID is the one of catgrasp_amd_neighbors.h: both functions take its three sorted tables (sorted_points (n,3) f64, sorted_index
 * (n) i32, sorted_keys (n) i64, sorted by (key, original index) with the keys of cg_grid_cell_keys) and its origin, cell and extents.
 * queries: (m,3) f32, or f64 if queries_f64 (f32 coordinates are widened: exact).  query_order: (m) i32, a permutation of 0..m-1 --
 * thread t answers query query_order[t], so that with the queries sorted by cg_grid_cell_keys the lanes of a wave scan the same
 * cells; NULL is the identity.  Every output is written at the query's own index.
 *
 * DISTANCE, everywhere: d2 = (dx*dx + dy*dy) + dz*dz with d = p_j - q, in float64 from the exact coordinates, every operation rounded
 * separately (no fused multiply-add): the expression of cg_grid_nearest_within and of cg_nearest_neighbor (catgrasp_amd.h), so equal
 * inputs give equal bits.  The cells decide only WHERE the kernels look: no result depends on `cell`, the origin or the extents.  No
 * lookup reads outside [0, n) of the tables, wherever q lies.
 *
 * Argument errors (CG_ERR_ARG, nothing launched): a NULL table, query or output pointer, n <= 0, m <= 0, a grid that
 * catgrasp_amd_neighbors.h refuses (non-finite origin, cell not positive and finite, an extent < 1, ext_x ext_y ext_z >= 2^62).
 * n or m above INT_MAX is CG_ERR_UNSUPPORTED (indices are i32).
 */
#ifndef CATGRASP_AMD_KDTREE_H
#define CATGRASP_AMD_KDTREE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* The largest number of box rounds of cg_grid_nearest per query: the round loop has this fixed trip count, after which the query is
 * finished by the linear pass.  |rounds| <= CG_KD_MAX_ROUNDS. */
#define CG_KD_MAX_ROUNDS 64

/* The exact nearest neighbour, unbounded: per query the point of smallest d2 among ALL n points, exact ties going to the smaller
 * original index.  With n >= 1 every query with finite coordinates has an answer.  These are the results of cg_nearest_neighbor
 * (catgrasp_amd.h), index for index.
 *
 * The search is boxes of doubling radius.  Round k = 0, 1, ... takes r_k = cell * 2^k (exact) and scans, per axis, the cells that
 * catgrasp_amd_neighbors.h gives for the radius r_k -- c(lo) .. c(hi) around q -+ r_k (1 + 2^-40) -- keeping the smallest (d2 bits,
 * original index) seen so far.  Those cells hold every point with d2 <= fl(r_k^2), rounding included, so the search stops as soon as
 * best d2 <= fl(r_k^2) (tested only while fl(r_k^2) is a normal, finite float64): nothing unseen can beat or tie the best.  It also
 * stops when the box covers the whole lattice on all three axes.  A round scans its box from the query's own row of cells outwards,
 * the inner boxes included (the running minimum is idempotent), and leaves out what the best so far rules out, by the same lemma
 * applied to the radius sqrt(best): the cells outside q -+ sqrt(best) on an axis, the rows of cells whose distance from q in (y, z)
 * alone exceeds it, and in a row the cells along x beyond what is left of it.  A point left out has d2 > best, strictly, rounding
 * included, so it can neither win nor tie.
 *
 * Two bounds hold for every query, however far away and however small the cell:
 *   WORK   a row of cells costs a binary search in the keys, a point costs one load.  Before every round after the first (round 0 is
 *          at most 4 x 4 rows), if the rows of its box (after the per-axis cut by the best so far) outnumber the indexed points
 *          (rows > n), the query is finished by ONE LINEAR PASS over the sorted table instead -- same d2 expression, same tie rule,
 *          so the same answer.
 *   TRIPS  after CG_KD_MAX_ROUNDS box rounds the query is finished by the linear pass as well.  No query can spin.
 *
 * nn_index (m) i32; nn_d2 (m) f64; rounds (m) i32, may be NULL: the number of box rounds the query scanned (>= 1), NEGATED when the
 * linear pass finished it.  It exists so that tests can show both paths taken. */
int cg_grid_nearest(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                    double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                    int queries_f64, const int* query_order, long m, int* nn_index, double* nn_d2, int* rounds, void* stream);

/* The index lists of query_ball_point: per query the original indices of the points with d2 <= radius*radius, the in-range test of
 * cg_grid_count_within, written into the query's own segment of `indices`.
 * radius: as in catgrasp_amd_neighbors.h (positive, finite, <= cell, radius*radius a normal float64; otherwise CG_ERR_ARG).
 * offsets: (m+1) i64, offsets[0] = 0 and offsets[q+1] - offsets[q] = the count cg_grid_count_within gives for query q at this radius
 * (the caller's cumulative sum); total = offsets[m], passed by value because offsets is device memory.  indices: (total) i32.  The
 * segment of query q is indices[offsets[q] .. offsets[q+1]), filled in the order the cells are scanned, NOT sorted; a thread never
 * writes outside its segment nor at or beyond `total`, whatever offsets holds.  NULL offsets, total < 0, or NULL indices with
 * total > 0 are CG_ERR_ARG.  With total == 0 nothing is launched. */
int cg_grid_ball_fill(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                      double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                      int queries_f64, const int* query_order, long m, double radius, const long long* offsets, long total,
                      int* indices, void* stream);

#ifdef __cplusplus
}
#endif
#endif
