/* catgrasp_amd -- C ABI of the scene front end: depth image -> organized point map -> oriented point normals.
 *
 * Same library (libcatgrasp_amd.so) and same conventions as catgrasp_amd.h: every pointer is a DEVICE
 * pointer, sizes are element counts, `stream` is a hipStream_t passed as void*.  The functions are
 * asynchronous on `stream`, never allocate, never synchronise; they return 0 (CG_OK), a negative
 * CG_ERR_* for argument errors (nothing is launched), or a positive hipError_t.
 *
 * They replace depth2xyzmap (Utils.py:239-251) and, for an organized cloud, open3d's
 * estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + correct_pcd_normal_direction (Utils.py:205-213) as the
 * reference calls them in compute_candidate_grasp (run_grasp_simulation.py:192-212).
 */
#ifndef CATGRASP_AMD_SCENE_H
#define CATGRASP_AMD_SCENE_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CG_OK
#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)
#endif

/* cg_organized_normals `route` values.  TILED stages, per workgroup of CG_SCENE_TILE x CG_SCENE_TILE query pixels, the tile and a halo
 * of halo_v rows and halo_u columns around it in LDS (16 bytes per pixel); DIRECT reads every neighbour from global memory and has no
 * window limit; AUTO takes TILED when cg_scene_halo_fits(halo_u, halo_v), DIRECT otherwise.  Both give bitwise identical outputs.
 * TILED with a halo that does not fit is CG_ERR_ARG. */
#define CG_SCENE_ROUTE_AUTO 0
#define CG_SCENE_ROUTE_TILED 1
#define CG_SCENE_ROUTE_DIRECT 2

#define CG_SCENE_TILE 16
/* The LDS budget of the TILED route: 64 KiB per workgroup (two workgroups share the 160 KiB of a CU), i.e.
 * (CG_SCENE_TILE + 2 halo_u) * (CG_SCENE_TILE + 2 halo_v) <= 4096 staged pixels -- a square halo of up to 24 pixels. */
#define CG_SCENE_LDS_BUDGET 65536

/* 1 if a halo of halo_u columns and halo_v rows fits CG_SCENE_LDS_BUDGET, 0 if not (or if either is negative).  Host only. */
int cg_scene_halo_fits(int halo_u, int halo_v);

/* depth2xyzmap.  depth: (H,W) f32, or f64 if depth_is_f64, in metres.  Per pixel (v,u), in float64: z = depth,
 * x = ((u - cx) * z) / fx, y = ((v - cy) * z) / fy, each operation rounded once, then rounded once to f32: the bits of the numpy
 * function.  A pixel with depth < 0.1 (compared in the depth's own type) is invalid: its xyz is (0,0,0) and its byte 0.
 * xyz_map: (H,W,3) f32.  valid: (H,W) u8, may be NULL. */
int cg_depth_to_xyz(const void* depth, int depth_is_f64, int H, int W, double fx, double fy, double cx, double cy, float* xyz_map,
                    unsigned char* valid, void* stream);

/* Oriented normals of an organized cloud.  xyz_map: (H,W,3) f32 as cg_depth_to_xyz writes it (x/z = (u - cx)/fx, y/z = (v - cy)/fy up
 * to f32 rounding).  use: (H,W) u8, non-zero for the pixels that take part (valid and not background).  normals: (H,W,3) f64, zero
 * where use is 0.  Per used pixel q, all in float64 from the f32 coordinates:
 *   candidates  every used pixel j (q included) with d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius, every operation rounded
 *               separately (no fused multiply-add);
 *   neighbours  the max_nn candidates of smallest d2; exact ties at the last place go to the smaller row-major pixel index;
 *   raw normal  (0,0,1) with fewer than 3 neighbours; otherwise the unit eigenvector of the smallest eigenvalue of the neighbours'
 *               covariance about their own mean (divided by their number), by cyclic Jacobi rotations;
 *   orientation n <- n / (|n| + 1e-10); n <- -n where ((vp - p) / |vp - p|) . n < 0, vp = (view_x, view_y, view_z), p the pixel's point.
 * The neighbours are searched in the pixel window |u_j - u_q| <= ceil((fx + |u_q - cx|) * radius / (z_q - radius)) + 1 (likewise in v
 * with fy, cy), which holds every point within `radius` of q (the whole image when z_q <= radius).
 * halo_u, halo_v: the halo of the TILED route; a query whose window is larger reads its neighbours from global memory, so they
 * affect speed, never results -- pass the largest window half-widths of the used pixels.  Ignored by DIRECT.
 * nb_count: (H,W) i32 number of neighbours, nb_d2max: (H,W) f64 their largest d2 (0 where use is 0); either may be NULL.
 * The outputs depend on the inputs only: not on the grid, the tile, the halo or the route. */
int cg_organized_normals(const float* xyz_map, const unsigned char* use, int H, int W, double fx, double fy, double cx, double cy,
                         double radius, int max_nn, double view_x, double view_y, double view_z, int route, int halo_u, int halo_v,
                         double* normals, int* nb_count, double* nb_d2max, void* stream);

#ifdef __cplusplus
}
#endif
#endif
