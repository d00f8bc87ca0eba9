// MeanShift with a flat kernel on the device (include/catgrasp_amd_cluster.h): the per-seed climb and the ordered merge of
// sklearn.cluster.MeanShift.fit as the reference calls it (predicter.py:332).  Labels are cg_nearest_neighbor's (affordance.hip).
//
// Climb: one wavefront per seed.  Lane l visits points l, l+64, ...; squared distance, membership (d2 <= bandwidth^2), count and
// coordinate sums are float64 from the exact point coordinates; an xor butterfly adds the 64 partial sums in a fixed order, and
// since a + b == b + a bit for bit every lane holds the same totals, so the stop rule is wave-uniform without a broadcast.
// Nothing depends on which wave or workgroup a seed lands in: no atomics, no cross-wave traffic after the staging barrier.
//
// Points are staged once per workgroup in LDS as three coordinate arrays (lane-contiguous 4- or 8-byte reads: conflict-free)
// when they fit the 160 KiB of a CU: n <= 13653 f32 points, n <= 6826 f64 points.  One 1024-thread workgroup then owns a CU, its
// 16 waves (4 per SIMD) each walking seeds with a grid stride.  Larger clouds read the same values from global memory (a 15k-point
// cloud is 180 KB: L2-resident); the arithmetic is the same code, so both routes give the same bits.
#include "cg_common.hpp"
#include "../../include/catgrasp_amd_cluster.h"
#include <math.h>

namespace {

constexpr int MS_LDS_BYTES = 160 * 1024;
constexpr int MS_CLIMB_THREADS = 1024;
constexpr int MS_MERGE_THREADS = 1024;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(MS_CLIMB_THREADS) void meanshift_climb_kernel(const T* __restrict__ pts, int n, const double* __restrict__ seeds,
                                                                           long n_seeds, double bw2, double stop_thresh, int max_iter,
                                                                           double* __restrict__ means, int* __restrict__ counts,
                                                                           int* __restrict__ iters) {
  extern __shared__ __align__(16) unsigned char ms_smem[];
  T* sx = (T*)ms_smem; T* sy = sx + n; T* sz = sy + n;
  if (LDS) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      sx[i] = pts[(long)i * 3]; sy[i] = pts[(long)i * 3 + 1]; sz[i] = pts[(long)i * 3 + 2];
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long waves = (long)gridDim.x * (blockDim.x >> 6);
  for (long s = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < n_seeds; s += waves) {
    double mx = seeds[s * 3], my = seeds[s * 3 + 1], mz = seeds[s * 3 + 2];
    int it = 0, cnt;
    while (true) {
      double c = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll 4
      for (int i = lane; i < n; i += 64) {
        const double x = LDS ? (double)sx[i] : (double)pts[(long)i * 3];
        const double y = LDS ? (double)sy[i] : (double)pts[(long)i * 3 + 1];
        const double z = LDS ? (double)sz[i] : (double)pts[(long)i * 3 + 2];
        const double dx = x - mx, dy = y - my, dz = z - mz;
        const bool in = dx * dx + dy * dy + dz * dz <= bw2;
        c += in ? 1.0 : 0.0; ax += in ? x : 0.0; ay += in ? y : 0.0; az += in ? z : 0.0;
      }
      c = wave_sum(c); ax = wave_sum(ax); ay = wave_sum(ay); az = wave_sum(az);
      cnt = (int)c;                                         // exact: a sum of at most 2^31 ones
      if (cnt == 0) break;                                  // an empty seed keeps the mean it had
      const double nx = ax / c, ny = ay / c, nz = az / c;
      const double ex = nx - mx, ey = ny - my, ez = nz - mz;
      mx = nx; my = ny; mz = nz;
      if (sqrt(ex * ex + ey * ey + ez * ez) <= stop_thresh || it == max_iter) break;
      ++it;
    }
    if (lane == 0) {
      means[s * 3] = mx; means[s * 3 + 1] = my; means[s * 3 + 2] = mz;
      counts[s] = cnt; iters[s] = it;
    }
  }
}

// One workgroup; thread t owns centers t, t+T, ...: it alone reads and writes their keep bytes, so the only exchange between
// threads is the block-wide minimum of the next alive index.
__global__ __launch_bounds__(MS_MERGE_THREADS) void meanshift_merge_kernel(const double* __restrict__ c, int m, double bw2,
                                                                           unsigned char* __restrict__ keep) {
  __shared__ int wave_min[MS_MERGE_THREADS / 64];
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
  for (int i = tid; i < m; i += T) keep[i] = 1;
  int p = tid;                                              // this thread's first center that is alive and not yet walked
  while (true) {
    int best = p < m ? p : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0) wave_min[wave] = best;
    __syncthreads();
    best = wave_min[0];
    for (int w = 1; w < n_waves; ++w) best = min(best, wave_min[w]);
    __syncthreads();                                        // wave_min is rewritten in the next round
    if (best == 0x7fffffff) break;                          // block-uniform
    const double x = c[(long)best * 3], y = c[(long)best * 3 + 1], z = c[(long)best * 3 + 2];
    if (p == best) p += T;                                  // kept: stays 1
    // later centers only: an earlier one is kept (then `best` would not be alive) or already suppressed
    for (int i = p; i < m; i += T) {
      const double dx = c[(long)i * 3] - x, dy = c[(long)i * 3 + 1] - y, dz = c[(long)i * 3 + 2] - z;
      if (dx * dx + dy * dy + dz * dz <= bw2) keep[i] = 0;
    }
    while (p < m && !keep[p]) p += T;
  }
}

template <typename T>
int launch_climb(const void* pts, int n, const double* seeds, long n_seeds, double bandwidth, int max_iter, bool lds, double* means,
                 int* counts, int* iters, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const int n_cu = cg_device_cu_count(dev);
  if (n_cu <= 0) return CG_ERR_UNSUPPORTED;
  const int wpb = MS_CLIMB_THREADS / 64;
  long blocks = (n_seeds + wpb - 1) / wpb;
  const double bw2 = bandwidth * bandwidth, stop = 1e-3 * bandwidth;
  if (lds) {
    constexpr auto kern = meanshift_climb_kernel<T, true>;
    const int st = cg_allow_dynamic_lds<kern>(dev, MS_LDS_BYTES);
    if (st != CG_OK) return st;
    if (blocks > n_cu) blocks = n_cu;                       // one workgroup holds a CU's LDS: stage once, stride over the seeds
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(MS_CLIMB_THREADS), (size_t)n * 3 * sizeof(T), stream, (const T*)pts, n, seeds,
                       n_seeds, bw2, stop, max_iter, means, counts, iters);
  } else {
    if (blocks > 2L * n_cu) blocks = 2L * n_cu;
    hipLaunchKernelGGL((meanshift_climb_kernel<T, false>), dim3((unsigned)blocks), dim3(MS_CLIMB_THREADS), 0, stream, (const T*)pts, n,
                       seeds, n_seeds, bw2, stop, max_iter, means, counts, iters);
  }
  return cg_hip_status(hipGetLastError());
}

}  // namespace

extern "C" int cg_meanshift_lds_max_points(int pts_is_f64) { return MS_LDS_BYTES / (pts_is_f64 ? 24 : 12); }

extern "C" int cg_meanshift_climb(const void* pts, int pts_is_f64, int n, const double* seeds, long n_seeds, double bandwidth, int max_iter,
                                  int route, double* means, int* counts, int* iters, void* stream) {
  if (!pts || !seeds || !means || !counts || !iters || n <= 0 || n_seeds < 0 || max_iter < 0) return CG_ERR_ARG;
  if (!(bandwidth > 0.0) || !isfinite(bandwidth)) return CG_ERR_ARG;
  if (route < CG_MEANSHIFT_ROUTE_AUTO || route > CG_MEANSHIFT_ROUTE_STREAMED) return CG_ERR_ARG;
  const bool fits = n <= cg_meanshift_lds_max_points(pts_is_f64);
  if (route == CG_MEANSHIFT_ROUTE_LDS && !fits) return CG_ERR_ARG;
  if (n_seeds == 0) return CG_OK;
  const bool lds = route == CG_MEANSHIFT_ROUTE_AUTO ? fits : route == CG_MEANSHIFT_ROUTE_LDS;
  return pts_is_f64 ? launch_climb<double>(pts, n, seeds, n_seeds, bandwidth, max_iter, lds, means, counts, iters, (hipStream_t)stream)
                    : launch_climb<float>(pts, n, seeds, n_seeds, bandwidth, max_iter, lds, means, counts, iters, (hipStream_t)stream);
}

extern "C" int cg_meanshift_merge(const double* sorted_centers, int m, double bandwidth, unsigned char* keep, void* stream) {
  if (!sorted_centers || !keep || m <= 0) return CG_ERR_ARG;
  if (!(bandwidth > 0.0) || !isfinite(bandwidth)) return CG_ERR_ARG;
  hipLaunchKernelGGL(meanshift_merge_kernel, dim3(1), dim3(MS_MERGE_THREADS), 0, (hipStream_t)stream, sorted_centers, m,
                     bandwidth * bandwidth, keep);
  return cg_hip_status(hipGetLastError());
}
