// The scene front end on the device (include/catgrasp_amd_scene.h): depth2xyzmap (Utils.py:239-251) and the oriented normals of
// an organized cloud -- open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + correct_pcd_normal_direction
// (Utils.py:205-213) as run_grasp_simulation.py:192-212 calls them, restated for a depth image.
//
// Normals: one thread per query pixel, 16 x 16 queries per workgroup.  A point within `radius` of the query lies in a small pixel
// window around it (bound and proof: DESIGN 4.11), so the hybrid search is a scan of that window -- exact, no tree.  The window is
// walked in row-major order by every pass:
//   1. accumulate over everything in range (d2 <= radius^2): count, largest d2, sums of d and d d^T with d = p_j - p_q.  With at
//      most max_nn in range the neighbour set is complete and the point is finished;
//   2. otherwise search the BIT PATTERN of d2 (non-negative doubles order like their bits) for the max_nn-th smallest d2, one
//      counting scan per probe, stopping early at a threshold with exactly max_nn at or below it.  The first probes interpolate
//      (the count grows about linearly with d2 on a surface), the rest bisect; with exact ties at the last place the search runs
//      out and the first (max_nn - count below) of the tied candidates in scan order, i.e. of smallest pixel index, are taken;
//   3. accumulate again over the selected set.
// The first scan walks the whole window; every later one walks the pixel rectangle of the candidates that can still be taken (those
// at or below the current upper end of the search), which the scan that found that end has recorded.
// No per-thread list exists, so nothing is indexed at run time and nothing goes to scratch.  The moments are taken about the QUERY
// point: |d| <= radius, so S2/n - m m^T subtracts terms of the covariance's own magnitude, never large equal ones.
//
// TILED stages the tile and its halo in LDS as float4 (x, y, z, used); DIRECT reads global memory.  Both fetch through one function and
// run the same arithmetic on the same candidates in the same order, so their outputs are the same bits.  A query whose window
// exceeds the staged halo reads global memory in the TILED kernel as well: the halo is a matter of speed, not of results.
#include "cg_common.hpp"
#include "cg_normals.hpp"
#include "../../include/catgrasp_amd_scene.h"
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int SC_TILE = CG_SCENE_TILE;
constexpr int SC_THREADS = SC_TILE * SC_TILE;
constexpr int SC_XYZ_THREADS = 256;
constexpr int SC_INTERPOLATED = 6;                        // value-interpolated probes of the selection before plain bisection

template <typename T>
__global__ __launch_bounds__(SC_XYZ_THREADS) void depth_to_xyz_kernel(const T* __restrict__ depth, int H, int W, double fx, double fy,
                                                                      double cx, double cy, float* __restrict__ xyz,
                                                                      unsigned char* __restrict__ valid) {
  const long n = (long)H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const T d = depth[i];
    const bool ok = !(d < (T)0.1);                          // the reference's invalid mask, in the depth's own type
    const int v = (int)(i / W), u = (int)(i - (long)v * W);
    const double z = (double)d;
    const double x = __ddiv_rn(__dmul_rn(__dsub_rn((double)u, cx), z), fx);
    const double y = __ddiv_rn(__dmul_rn(__dsub_rn((double)v, cy), z), fy);
    xyz[i * 3] = ok ? (float)x : 0.f;
    xyz[i * 3 + 1] = ok ? (float)y : 0.f;
    xyz[i * 3 + 2] = ok ? (float)z : 0.f;
    if (valid) valid[i] = ok ? 1 : 0;
  }
}

// where one query's candidates come from: the staged halo or global memory
struct Source {
  const float4* halo; int lw, gu0, gv0;                    // LDS: row length, image coordinates of its first entry
  const float* xyz; const unsigned char* use; int W;
  bool lds;
  __device__ __forceinline__ bool fetch(int ju, int jv, float& x, float& y, float& z) const {
    if (lds) {
      const float4 e = halo[(jv - gv0) * lw + (ju - gu0)];
      x = e.x; y = e.y; z = e.z;
      return e.w != 0.f;
    }
    const long p = (long)jv * W + ju;
    if (!use[p]) return false;
    x = xyz[p * 3]; y = xyz[p * 3 + 1]; z = xyz[p * 3 + 2];
    return true;
  }
};

struct Query { double x, y, z; int u0, u1, v0, v1; };      // the point and its window, clipped to the image

__device__ __forceinline__ long long d2_bits(const Source& s, const Query& q, int ju, int jv, double& dx, double& dy, double& dz, bool& ok) {
  float x, y, z;
  ok = s.fetch(ju, jv, x, y, z);
  dx = __dsub_rn((double)x, q.x); dy = __dsub_rn((double)y, q.y); dz = __dsub_rn((double)z, q.z);
  return __double_as_longlong(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// the pixel rectangle that holds the candidates a scan has taken
struct Box {
  int u0, u1, v0, v1;
  __device__ __forceinline__ void clear() { u0 = v0 = 0x7fffffff; u1 = v1 = -1; }
  __device__ __forceinline__ void add(int ju, int jv) { u0 = min(u0, ju); u1 = max(u1, ju); v0 = min(v0, jv); v1 = max(v1, jv); }
};

// number of candidates with d2 <= t (as bit patterns), and their rectangle
__device__ __forceinline__ int count_at_most(const Source& s, const Query& q, long long t, Box& box) {
  int c = 0;
  box.clear();
  for (int jv = q.v0; jv <= q.v1; ++jv)
    for (int ju = q.u0; ju <= q.u1; ++ju) {
      double dx, dy, dz; bool ok;
      const long long b = d2_bits(s, q, ju, jv, dx, dy, dz, ok);
      if (ok && b <= t) { ++c; box.add(ju, jv); }
    }
  return c;
}

struct Moments { int n; long long d2max; double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz; Box box; };

// moments of the candidates with d2 < t, and of the first `ties` candidates in scan order with d2 == t
__device__ __forceinline__ Moments accumulate(const Source& s, const Query& q, long long t, int ties) {
  Moments m = {0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, {0, 0, 0, 0}};
  m.box.clear();
  for (int jv = q.v0; jv <= q.v1; ++jv)
    for (int ju = q.u0; ju <= q.u1; ++ju) {
      double dx, dy, dz; bool ok;
      const long long b = d2_bits(s, q, ju, jv, dx, dy, dz, ok);
      if (!ok || b > t) continue;
      if (b == t) {
        if (ties <= 0) continue;
        --ties;
      }
      ++m.n;
      m.box.add(ju, jv);
      m.d2max = b > m.d2max ? b : m.d2max;
      m.sx += dx; m.sy += dy; m.sz += dz;
      m.sxx += dx * dx; m.sxy += dx * dy; m.sxz += dx * dz; m.syy += dy * dy; m.syz += dy * dz; m.szz += dz * dz;
    }
  return m;
}

template <bool TILED>
__global__ __launch_bounds__(SC_THREADS) void organized_normals_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ use,
                                                                       int H, int W, double fx, double fy, double cx, double cy,
                                                                       double radius, long long r2_bits, int max_nn, double vx, double vy,
                                                                       double vz, int halo_u, int halo_v, double* __restrict__ normals,
                                                                       int* __restrict__ nb_count, double* __restrict__ nb_d2max) {
  extern __shared__ __align__(16) unsigned char sc_smem[];
  float4* halo = (float4*)sc_smem;
  const int lw = SC_TILE + 2 * halo_u, lh = SC_TILE + 2 * halo_v;
  const int gu0 = (int)blockIdx.x * SC_TILE - halo_u, gv0 = (int)blockIdx.y * SC_TILE - halo_v;
  if (TILED) {
    for (int i = threadIdx.x; i < lw * lh; i += SC_THREADS) {
      const int lv = i / lw, lu = i - lv * lw, ju = gu0 + lu, jv = gv0 + lv;
      float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ju >= 0 && ju < W && jv >= 0 && jv < H) {
        const long p = (long)jv * W + ju;
        if (use[p]) e = make_float4(xyz[p * 3], xyz[p * 3 + 1], xyz[p * 3 + 2], 1.f);
      }
      halo[i] = e;
    }
    __syncthreads();
  }
  const int u = (int)blockIdx.x * SC_TILE + (threadIdx.x & (SC_TILE - 1)), v = (int)blockIdx.y * SC_TILE + (threadIdx.x / SC_TILE);
  if (u >= W || v >= H) return;
  const long pix = (long)v * W + u;
  if (!use[pix]) {
    normals[pix * 3] = 0.0; normals[pix * 3 + 1] = 0.0; normals[pix * 3 + 2] = 0.0;
    if (nb_count) nb_count[pix] = 0;
    if (nb_d2max) nb_d2max[pix] = 0.0;
    return;
  }
  Query q;
  q.x = (double)xyz[pix * 3]; q.y = (double)xyz[pix * 3 + 1]; q.z = (double)xyz[pix * 3 + 2];
  // the window: every point within radius of q lies in it (one pixel is added for the f32 rounding of the map)
  int hu = W, hv = H;
  const double zr = q.z - radius;
  if (zr > 0.0) {
    const double bu = ceil((fx + fabs((double)u - cx)) * radius / zr) + 1.0, bv = ceil((fy + fabs((double)v - cy)) * radius / zr) + 1.0;
    hu = bu < (double)W ? (int)bu : W;
    hv = bv < (double)H ? (int)bv : H;
  }
  q.u0 = max(u - hu, 0); q.u1 = min(u + hu, W - 1); q.v0 = max(v - hv, 0); q.v1 = min(v + hv, H - 1);
  Source s;
  s.halo = halo; s.lw = lw; s.gu0 = gu0; s.gv0 = gv0; s.xyz = xyz; s.use = use; s.W = W;
  s.lds = TILED && hu <= halo_u && hv <= halo_v;

  Moments m = accumulate(s, q, r2_bits, 0x7fffffff);
  if (m.n > max_nn) {
    // smallest t with count_at_most(t) >= max_nn: count_at_most(lo) = below < max_nn < above = count_at_most(hi) throughout.  On a
    // surface the count grows about linearly with d2, so the first probes interpolate in VALUE between the two ends, aiming
    // between the max_nn-th and the next candidate; after SC_INTERPOLATED probes the bit pattern is bisected, which ends.
    // Whichever probes are taken, the set that comes out is the same.
    // Every later scan only looks for candidates at or below the current `hi`, and the scan that set `hi` has seen their
    // rectangle: the window shrinks to it (the scan order of what remains, row-major, is unchanged).
    long long lo = -1, hi = r2_bits;
    int below = 0, above = m.n, ties = -1;
    q.u0 = m.box.u0; q.u1 = m.box.u1; q.v0 = m.box.v0; q.v1 = m.box.v1;
    for (int probe = 0; hi - lo > 1; ++probe) {
      long long mid = lo + ((hi - lo) >> 1);
      if (probe < SC_INTERPOLATED) {
        const double lv = lo < 0 ? 0.0 : __longlong_as_double(lo), hv = __longlong_as_double(hi);
        const double t = lv + (hv - lv) * (((double)(max_nn - below) + 0.5) / (double)(above - below));
        const long long g = __double_as_longlong(t);
        mid = g <= lo ? lo + 1 : g >= hi ? hi - 1 : g;
      }
      Box box;
      const int c = count_at_most(s, q, mid, box);
      if (c < max_nn) { lo = mid; below = c; continue; }
      q.u0 = box.u0; q.u1 = box.u1; q.v0 = box.v0; q.v1 = box.v1;
      hi = mid; above = c;
      if (c == max_nn) { ties = 0x7fffffff; break; }                  // exactly max_nn at or below mid: they are the set
    }
    if (ties < 0) ties = max_nn - below;
    m = accumulate(s, q, hi, ties);
  }

  double nx, ny, nz;
  oriented_normal(m, q.x, q.y, q.z, vx, vy, vz, nx, ny, nz);
  normals[pix * 3] = nx; normals[pix * 3 + 1] = ny; normals[pix * 3 + 2] = nz;
  if (nb_count) nb_count[pix] = m.n;
  if (nb_d2max) nb_d2max[pix] = __longlong_as_double(m.d2max);
}

size_t halo_bytes(int halo_u, int halo_v) { return (size_t)(SC_TILE + 2 * halo_u) * (size_t)(SC_TILE + 2 * halo_v) * sizeof(float4); }

}  // namespace

extern "C" int cg_scene_halo_fits(int halo_u, int halo_v) {
  if (halo_u < 0 || halo_v < 0 || halo_u > CG_SCENE_LDS_BUDGET || halo_v > CG_SCENE_LDS_BUDGET) return 0;
  return halo_bytes(halo_u, halo_v) <= (size_t)CG_SCENE_LDS_BUDGET ? 1 : 0;
}

extern "C" int cg_depth_to_xyz(const void* depth, int depth_is_f64, int H, int W, double fx, double fy, double cx, double cy, float* xyz_map,
                               unsigned char* valid, void* stream) {
  if (!depth || !xyz_map || H <= 0 || W <= 0) return CG_ERR_ARG;
  if (!(fx > 0.0) || !(fy > 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return CG_ERR_ARG;
  const long n = (long)H * W;
  long blocks = (n + SC_XYZ_THREADS - 1) / SC_XYZ_THREADS;
  if (blocks > 65536) blocks = 65536;
  if (depth_is_f64)
    hipLaunchKernelGGL(depth_to_xyz_kernel<double>, dim3((unsigned)blocks), dim3(SC_XYZ_THREADS), 0, (hipStream_t)stream, (const double*)depth,
                       H, W, fx, fy, cx, cy, xyz_map, valid);
  else
    hipLaunchKernelGGL(depth_to_xyz_kernel<float>, dim3((unsigned)blocks), dim3(SC_XYZ_THREADS), 0, (hipStream_t)stream, (const float*)depth,
                       H, W, fx, fy, cx, cy, xyz_map, valid);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_organized_normals(const float* xyz_map, const unsigned char* use, int H, int W, double fx, double fy, double cx, double cy,
                                    double radius, int max_nn, double view_x, double view_y, double view_z, int route, int halo_u, int halo_v,
                                    double* normals, int* nb_count, double* nb_d2max, void* stream) {
  if (!xyz_map || !use || !normals || H <= 0 || W <= 0 || max_nn < 1) return CG_ERR_ARG;
  if (!(fx > 0.0) || !(fy > 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return CG_ERR_ARG;
  if (!(radius > 0.0) || !isfinite(radius) || !isfinite(view_x) || !isfinite(view_y) || !isfinite(view_z)) return CG_ERR_ARG;
  if (route < CG_SCENE_ROUTE_AUTO || route > CG_SCENE_ROUTE_DIRECT) return CG_ERR_ARG;
  bool tiled = false;
  if (route != CG_SCENE_ROUTE_DIRECT) {
    if (halo_u < 0 || halo_v < 0) return CG_ERR_ARG;
    tiled = cg_scene_halo_fits(halo_u, halo_v) != 0;
    if (route == CG_SCENE_ROUTE_TILED && !tiled) return CG_ERR_ARG;
  }
  const double r2 = radius * radius;
  long long r2_bits;
  memcpy(&r2_bits, &r2, sizeof r2_bits);
  const dim3 grid((unsigned)((W + SC_TILE - 1) / SC_TILE), (unsigned)((H + SC_TILE - 1) / SC_TILE));
  if (grid.y > 65535u) return CG_ERR_UNSUPPORTED;
  if (tiled)
    hipLaunchKernelGGL(organized_normals_kernel<true>, grid, dim3(SC_THREADS), halo_bytes(halo_u, halo_v), (hipStream_t)stream, xyz_map, use, H,
                       W, fx, fy, cx, cy, radius, r2_bits, max_nn, view_x, view_y, view_z, halo_u, halo_v, normals, nb_count, nb_d2max);
  else
    hipLaunchKernelGGL(organized_normals_kernel<false>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, xyz_map, use, H, W, fx, fy, cx, cy,
                       radius, r2_bits, max_nn, view_x, view_y, view_z, 0, 0, normals, nb_count, nb_d2max);
  return cg_hip_status(hipGetLastError());
}
