// The grid index (include/catgrasp_amd_neighbors.h): radius-bounded neighbour queries over a cloud sorted by the keys of a uniform
// lattice, and on top of them the oriented normals of an unorganized cloud -- open3d's
// estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) + correct_pcd_normal_direction with the semantics of cg_organized_normals.
//
// The search: per axis the cells c(lo) .. c(hi) around q -+ radius (conservative, see cell_range), the cells along x being consecutive
// keys: one binary search in the sorted keys per (y, z) pair, then a walk to the end of the run.  Every candidate found is tested with
// the pinned d2 expression; the cells decide only WHERE to look, so nothing that comes out depends on them.  DESIGN 4.12 has the proof.
//
// Normals: one thread per point, in SORTED order (the lanes of a wave scan the same cells), one wave per workgroup.  The max_nn
// candidates that are smallest by (d2, original index) are kept as an unsorted list in LDS -- d2 bits and sorted position, 12 bytes an
// entry, entry e of thread t at [e * 64 + t] -- together with the list's worst entry in registers: a candidate below the worst replaces
// it and the list is read once for the new worst.  The list lives in LDS because it is indexed at run time; in registers it would go to
// scratch.  Afterwards the d2 slots take the original indices, and the moments are accumulated over the list in ascending original
// index by selection (max_nn^2 LDS reads), which is the order cg_organized_normals accumulates in.
//
// On the same tables (include/catgrasp_amd_kdtree.h): the unbounded exact nearest neighbour, by boxes of doubling radius with a linear
// pass as the bound on its work, and the index lists behind the counts.  DESIGN 4.12.1.
#include "cg_common.hpp"
#include "cg_normals.hpp"
#include "../../include/catgrasp_amd_neighbors.h"
#include "../../include/catgrasp_amd_kdtree.h"
#include <float.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int NB_THREADS = 64;                              // normals: one wave per workgroup, 12 * max_nn * 64 bytes of LDS
constexpr int NB_Q_THREADS = 256;                           // keys and the plain queries
constexpr size_t NB_ENTRY_BYTES = sizeof(long long) + sizeof(int);

struct Grid {
  const double* pts; const int* index; const long long* keys; long n;
  double ox, oy, oz, cell; long ex, ey, ez;
};

// floor((x - o) / cell), each operation rounded once: monotone (non-decreasing) in x
__device__ __forceinline__ double cell_coord(double x, double o, double cell) { return floor(__ddiv_rn(__dsub_rn(x, o), cell)); }

// into 0 .. ext - 1 (still monotone); NaN goes to 0
__device__ __forceinline__ long clamp_cell(double f, long ext) {
  if (!(f > 0.0)) return 0;
  if (f >= (double)ext) return ext - 1;
  const long c = (long)f;
  return c < ext ? c : ext - 1;
}

__device__ __forceinline__ long long cell_key(double x, double y, double z, const Grid& g) {
  const long cx = clamp_cell(cell_coord(x, g.ox, g.cell), g.ex), cy = clamp_cell(cell_coord(y, g.oy, g.cell), g.ey),
             cz = clamp_cell(cell_coord(z, g.oz, g.cell), g.ez);
  return ((long long)cz * g.ey + cy) * g.ex + cx;
}

// The cells of one axis that can hold a point in range of q.  In range means fl(d^2) <= fl(r^2) on this axis at least, so
// |p - q| <= r (1 + 2^-50) < reach = r (1 + 2^-40); the double below fl(q - reach) is <= q - reach and the double above fl(q + reach) is
// >= q + reach (round to nearest), so lo <= p <= hi and, c being monotone, c(lo) <= c(p) <= c(hi).  Every point has c >= 0 before the
// clamp (the origin is the minimum) and c <= ext - 1 after it, so a range wholly outside is empty.
struct Range { long lo, hi; };
__device__ __forceinline__ Range cell_range(double q, double reach, double o, double cell, long ext) {
  const double flo = cell_coord(nextafter(__dsub_rn(q, reach), -INFINITY), o, cell);
  const double fhi = cell_coord(nextafter(__dadd_rn(q, reach), INFINITY), o, cell);
  Range r = {0, -1};
  if (!(fhi >= 0.0) || !(flo < (double)ext)) return r;
  r.lo = clamp_cell(flo, ext); r.hi = clamp_cell(fhi, ext);
  return r;
}

// the first sorted position with key >= k0, in [0, n]
__device__ __forceinline__ long first_key_at_least(const Grid& g, long long k0) {
  long a = 0, b = g.n;
  while (a < b) {
    const long mid = a + ((b - a) >> 1);
    if (g.keys[mid] < k0) a = mid + 1; else b = mid;
  }
  return a;
}

// the pinned d2 of sorted point j, as bits: non-negative doubles order like their bits; NaN and infinity are above every finite one
__device__ __forceinline__ long long d2_bits(const Grid& g, long j, double qx, double qy, double qz) {
  const double dx = __dsub_rn(g.pts[j * 3], qx), dy = __dsub_rn(g.pts[j * 3 + 1], qy), dz = __dsub_rn(g.pts[j * 3 + 2], qz);
  return __double_as_longlong(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// f(j, d2 bits, dx, dy, dz) for every sorted position j whose point is in range of q: the query's own cell row, then the others;
// ascending j within a row
template <typename F>
__device__ __forceinline__ void for_each_in_range(const Grid& g, double qx, double qy, double qz, double reach, long long r2_bits, F&& f) {
  const Range rx = cell_range(qx, reach, g.ox, g.cell, g.ex), ry = cell_range(qy, reach, g.oy, g.cell, g.ey),
              rz = cell_range(qz, reach, g.oz, g.cell, g.ez);
  if (rx.lo > rx.hi || ry.lo > ry.hi || rz.lo > rz.hi) return;
  // the query's own row of cells first: its candidates are the near ones, and a list that starts with them is seldom overturned
  const long hy = clamp_cell(cell_coord(qy, g.oy, g.cell), g.ey), hz = clamp_cell(cell_coord(qz, g.oz, g.cell), g.ez);
  for (int pass = 0; pass < 2; ++pass)
    for (long cz = rz.lo; cz <= rz.hi; ++cz)
      for (long cy = ry.lo; cy <= ry.hi; ++cy) {
        if ((cz == hz && cy == hy) != (pass == 0)) continue;
        const long long row = ((long long)cz * g.ey + cy) * g.ex, k0 = row + rx.lo, k1 = row + rx.hi;
        for (long j = first_key_at_least(g, k0); j < g.n && g.keys[j] <= k1; ++j) {
          const double dx = __dsub_rn(g.pts[j * 3], qx), dy = __dsub_rn(g.pts[j * 3 + 1], qy), dz = __dsub_rn(g.pts[j * 3 + 2], qz);
          const long long bits = __double_as_longlong(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
          if (bits <= r2_bits) f(j, bits, dx, dy, dz);     // non-negative doubles order like their bits; NaN and infinity are above
        }
      }
}

template <typename T>
__global__ __launch_bounds__(NB_Q_THREADS) void cell_keys_kernel(const T* __restrict__ p, long n, Grid g, long long* __restrict__ keys) {
  const long i = (long)blockIdx.x * NB_Q_THREADS + threadIdx.x;
  if (i < n) keys[i] = cell_key((double)p[i * 3], (double)p[i * 3 + 1], (double)p[i * 3 + 2], g);
}

struct Moments { int n; long long d2max; double sx, sy, sz, sxx, sxy, sxz, syy, syz, szz; };

__global__ __launch_bounds__(NB_THREADS) void grid_normals_kernel(Grid g, double reach, long long r2_bits, int max_nn, double vx, double vy,
                                                                  double vz, double* __restrict__ normals, int* __restrict__ nb_count,
                                                                  double* __restrict__ nb_d2max) {
  extern __shared__ __align__(8) unsigned char nb_smem[];
  long long* l_d2 = (long long*)nb_smem;                    // d2 bits during the search, original indices after it
  int* l_j = (int*)(nb_smem + (size_t)max_nn * NB_THREADS * sizeof(long long));
  const int t = threadIdx.x;
  const long s = (long)blockIdx.x * NB_THREADS + t;
  if (s >= g.n) return;
  const double qx = g.pts[s * 3], qy = g.pts[s * 3 + 1], qz = g.pts[s * 3 + 2];

  int cnt = 0, worst_at = 0, worst_i = -1;                  // the list's largest (d2, original index) and where it is
  long long worst_b = -1;
  for_each_in_range(g, qx, qy, qz, reach, r2_bits, [&](long j, long long b, double, double, double) {
    if (cnt < max_nn) {
      const int i = g.index[j];
      l_d2[cnt * NB_THREADS + t] = b; l_j[cnt * NB_THREADS + t] = (int)j;
      if (b > worst_b || (b == worst_b && i > worst_i)) { worst_b = b; worst_i = i; worst_at = cnt; }
      ++cnt;
      return;
    }
    if (b > worst_b || (b == worst_b && g.index[j] > worst_i)) return;
    l_d2[worst_at * NB_THREADS + t] = b; l_j[worst_at * NB_THREADS + t] = (int)j;
    worst_b = -1; worst_i = -1; worst_at = 0;               // worst_i < 0: not read yet
#pragma unroll 4
    for (int e = 0; e < max_nn; ++e) {
      const long long eb = l_d2[e * NB_THREADS + t];
      if (eb > worst_b) { worst_b = eb; worst_at = e; worst_i = -1; continue; }
      if (eb < worst_b) continue;
      if (worst_i < 0) worst_i = g.index[l_j[worst_at * NB_THREADS + t]];
      const int ei = g.index[l_j[e * NB_THREADS + t]];
      if (ei > worst_i) { worst_i = ei; worst_at = e; }
    }
    if (worst_i < 0) worst_i = g.index[l_j[worst_at * NB_THREADS + t]];
  });

  for (int e = 0; e < cnt; ++e) l_d2[e * NB_THREADS + t] = (long long)g.index[l_j[e * NB_THREADS + t]];
  Moments m = {0, cnt > 0 ? worst_b : 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long last = -1;
  for (int k = 0; k < cnt; ++k) {
    long long next = LLONG_MAX;
    int j = 0;
    for (int e = 0; e < cnt; ++e) {
      const long long i = l_d2[e * NB_THREADS + t];
      if (i > last && i < next) { next = i; j = l_j[e * NB_THREADS + t]; }
    }
    last = next;
    const double dx = __dsub_rn(g.pts[(long)j * 3], qx), dy = __dsub_rn(g.pts[(long)j * 3 + 1], qy), dz = __dsub_rn(g.pts[(long)j * 3 + 2], qz);
    ++m.n;
    m.sx += dx; m.sy += dy; m.sz += dz;
    m.sxx += dx * dx; m.sxy += dx * dy; m.sxz += dx * dz; m.syy += dy * dy; m.syz += dy * dz; m.szz += dz * dz;
  }

  double nx, ny, nz;
  oriented_normal(m, qx, qy, qz, vx, vy, vz, nx, ny, nz);
  const long o = g.index[s];
  normals[o * 3] = nx; normals[o * 3 + 1] = ny; normals[o * 3 + 2] = nz;
  if (nb_count) nb_count[o] = m.n;
  if (nb_d2max) nb_d2max[o] = __longlong_as_double(m.d2max);
}

// NEAREST: nn_index / nn_d2 of the closest point in range; otherwise the number of points in range
template <typename T, bool NEAREST>
__global__ __launch_bounds__(NB_Q_THREADS) void grid_query_kernel(Grid g, const T* __restrict__ queries, const int* __restrict__ order, long m,
                                                                  double reach, long long r2_bits, int* __restrict__ out_i,
                                                                  double* __restrict__ out_d2) {
  const long t = (long)blockIdx.x * NB_Q_THREADS + threadIdx.x;
  if (t >= m) return;
  const long q = order ? (long)order[t] : t;
  const double qx = (double)queries[q * 3], qy = (double)queries[q * 3 + 1], qz = (double)queries[q * 3 + 2];
  int count = 0, best_i = -1;
  long long best_b = LLONG_MAX;
  for_each_in_range(g, qx, qy, qz, reach, r2_bits, [&](long j, long long b, double, double, double) {
    if (!NEAREST) { ++count; return; }
    if (b > best_b) return;
    const int i = g.index[j];
    if (b < best_b || i < best_i) { best_b = b; best_i = i; }
  });
  if (NEAREST) {
    out_i[q] = best_i;
    out_d2[q] = best_i < 0 ? INFINITY : __longlong_as_double(best_b);
  } else {
    out_i[q] = count;
  }
}

// the running minimum by (d2 bits, original index); whether the candidate took its place
struct Best { long long b; int i; };
__device__ __forceinline__ bool take_nearer(Best& best, const Grid& g, long j, long long b) {
  if (b > best.b) return false;
  const int i = g.index[j];
  if (!(b < best.b || i < best.i)) return false;
  best.b = b; best.i = i;
  return true;
}

struct Box { Range x, y, z; };
__device__ __forceinline__ Range meet(Range a, Range b) {
  const Range r = {a.lo > b.lo ? a.lo : b.lo, a.hi < b.hi ? a.hi : b.hi};
  return r;
}

// `box` without the cells that cannot hold a point with d2 <= best: rho = sqrt(max(best, 2^-900)) (1 + 2^-40) has fl(rho^2) >= best, a
// normal number, so by the lemma at cell_range such a point lies in cell_range(q, rho (1 + 2^-40)) on every axis.  A point outside has
// d2 > best and can neither beat nor tie it, now or later: the best only falls.  No pruning while best is infinite (nothing found yet).
__device__ __forceinline__ Box cells_within_best(const Grid& g, double qx, double qy, double qz, long long best_bits, Box box) {
  const double b = __longlong_as_double(best_bits);
  if (!(b <= 0x1p1000)) return box;
  const double rho = __dmul_rn(sqrt(b >= 0x1p-900 ? b : 0x1p-900), 1.0 + 0x1p-40), reach = __dmul_rn(rho, 1.0 + 0x1p-40);
  box.x = meet(box.x, cell_range(qx, reach, g.ox, g.cell, g.ex));
  box.y = meet(box.y, cell_range(qy, reach, g.oy, g.cell, g.ey));
  box.z = meet(box.z, cell_range(qz, reach, g.oz, g.cell, g.ez));
  return box;
}

// A lower bound, rounded down and >= 0, of |p - q| on one axis over the points p of cell c, h being the (clamped) cell of q; 0 where
// none is known.  c() is monotone, clamp included, so a double x with c(x) < c lies below every such p and one with c(x) > c above
// it: x is a guess at the cell's face, nudged 2^-30 of its offset towards q, and counts only if c(x) -- evaluated, not assumed --
// says so.
__device__ __forceinline__ double axis_gap(double q, long c, long h, double o, double cell, long ext) {
  double gap = 0.0;
  if (c > h) {
    const double x = __dadd_rn(o, __dmul_rn(__dmul_rn((double)c, cell), 1.0 - 0x1p-30));
    if (clamp_cell(cell_coord(x, o, cell), ext) < c) gap = nextafter(__dsub_rn(x, q), -INFINITY);
  } else if (c < h) {
    const double x = __dadd_rn(o, __dmul_rn(__dmul_rn((double)(c + 1), cell), 1.0 + 0x1p-30));
    if (clamp_cell(cell_coord(x, o, cell), ext) > c) gap = nextafter(__dsub_rn(q, x), -INFINITY);
  }
  return gap > 0.0 ? gap : 0.0;
}

// The cells along x of a row whose points lie at least gy and gz from q on the other axes that can hold a point with d2 <= best
// (empty: none).  fl(d2) <= best needs dy^2 + dz^2 <= best (1 + 2^-50) in real numbers (rounding is monotone and the terms are
// non-negative), so the row is out once (gy^2 + gz^2)(1 - 2^-40) > best, and otherwise dx^2 <= rem = best (1 + 2^-40) - (gy^2 + gz^2)
// (1 - 2^-40), whose rounding the two 2^-40 cover; the range is cell_range at sqrt(rem) (1 + 2^-40).  best is taken as at least
// 2^-900, so that rem is a normal number; above 2^1000 (nothing found yet) the row keeps the whole range.
__device__ __forceinline__ Range row_cells_within_best(const Grid& g, double qx, double gy, double gz, long long best_bits, Range x) {
  const double b = __longlong_as_double(best_bits);
  if (!(b <= 0x1p1000)) return x;
  const double bb = b >= 0x1p-900 ? b : 0x1p-900;
  const double low = __dmul_rn(__dadd_rn(__dmul_rn(gy, gy), __dmul_rn(gz, gz)), 1.0 - 0x1p-40);
  const Range none = {0, -1};
  if (low > bb) return none;
  const double rho = __dmul_rn(sqrt(__dsub_rn(__dmul_rn(bb, 1.0 + 0x1p-40), low)), 1.0 + 0x1p-40);
  return meet(x, cell_range(qx, __dmul_rn(rho, 1.0 + 0x1p-40), g.ox, g.cell, g.ex));
}

// The unbounded nearest neighbour (include/catgrasp_amd_kdtree.h): boxes of radius cell * 2^k around q until the best d2 is within
// the box's radius -- by the lemma at cell_range every point that could beat or tie it has then been seen -- or the box is the whole
// lattice; one linear pass over the table instead once a round would search more rows than there are points, or after
// CG_KD_MAX_ROUNDS rounds.  A box is scanned from the query's own row of cells outwards, and whenever a row lowers the best, the box
// shrinks to the cells that can still hold something as near (cells_within_best); a row of cells farther from q than the best is
// skipped and the others are searched only as far along x as the best allows (row_cells_within_best).  Every sorted position read
// is in [0, n).
template <typename T>
__global__ __launch_bounds__(NB_Q_THREADS) void grid_nearest_kernel(Grid g, const T* __restrict__ queries, const int* __restrict__ order, long m,
                                                                    int* __restrict__ nn_index, double* __restrict__ nn_d2,
                                                                    int* __restrict__ rounds) {
  const long t = (long)blockIdx.x * NB_Q_THREADS + threadIdx.x;
  if (t >= m) return;
  const long q = order ? (long)order[t] : t;
  const double qx = (double)queries[q * 3], qy = (double)queries[q * 3 + 1], qz = (double)queries[q * 3 + 2];
  // the query's own cell, clamped into the lattice: inside every non-empty cell_range around q
  const long hy = clamp_cell(cell_coord(qy, g.oy, g.cell), g.ey), hz = clamp_cell(cell_coord(qz, g.oz, g.cell), g.ez);
  Best best = {LLONG_MAX, INT_MAX};
  double r = g.cell;                                        // doubled every round: exact
  int k = 0;
  bool done = false;
  while (k < CG_KD_MAX_ROUNDS) {
    const double reach = __dmul_rn(r, 1.0 + 0x1p-40);
    const Box box = {cell_range(qx, reach, g.ox, g.cell, g.ex), cell_range(qy, reach, g.oy, g.cell, g.ey),
                     cell_range(qz, reach, g.oz, g.cell, g.ez)};
    Box live = cells_within_best(g, qx, qy, qz, best.b, box);
    if (live.x.lo <= live.x.hi && live.y.lo <= live.y.hi && live.z.lo <= live.z.hi) {
      if (k > 0 && (long long)(live.y.hi - live.y.lo + 1) * (live.z.hi - live.z.lo + 1) > (long long)g.n) break;   // the work bound
      for (long sz = 0; hz + sz <= live.z.hi || hz - sz >= live.z.lo; ++sz)
        for (int uz = 0; uz < (sz ? 2 : 1); ++uz) {
          const long cz = uz ? hz - sz : hz + sz;
          if (cz < live.z.lo || cz > live.z.hi) continue;
          const double gz = axis_gap(qz, cz, hz, g.oz, g.cell, g.ez);
          for (long sy = 0; hy + sy <= live.y.hi || hy - sy >= live.y.lo; ++sy)
            for (int uy = 0; uy < (sy ? 2 : 1); ++uy) {
              const long cy = uy ? hy - sy : hy + sy;
              if (cy < live.y.lo || cy > live.y.hi || cz < live.z.lo || cz > live.z.hi) continue;
              const Range x = row_cells_within_best(g, qx, axis_gap(qy, cy, hy, g.oy, g.cell, g.ey), gz, best.b, live.x);
              if (x.lo > x.hi) continue;
              const long long row = ((long long)cz * g.ey + cy) * g.ex, k1 = row + x.hi;
              bool nearer = false;
              for (long j = first_key_at_least(g, row + x.lo); j < g.n && g.keys[j] <= k1; ++j)
                nearer |= take_nearer(best, g, j, d2_bits(g, j, qx, qy, qz));
              if (nearer) live = cells_within_best(g, qx, qy, qz, best.b, live);
            }
        }
    }
    ++k;
    const double r2 = __dmul_rn(r, r);
    if (r2 >= DBL_MIN && r2 <= DBL_MAX && best.b <= __double_as_longlong(r2)) { done = true; break; }
    if (box.x.lo == 0 && box.x.hi == g.ex - 1 && box.y.lo == 0 && box.y.hi == g.ey - 1 && box.z.lo == 0 && box.z.hi == g.ez - 1) {
      done = true;                                          // the whole lattice: an empty range is {0, -1}, never this
      break;
    }
    r = __dmul_rn(r, 2.0);
  }
  if (!done)
    for (long j = 0; j < g.n; ++j) take_nearer(best, g, j, d2_bits(g, j, qx, qy, qz));
  nn_index[q] = best.i;
  nn_d2[q] = __longlong_as_double(best.b);
  if (rounds) rounds[q] = done ? k : -k;
}

// the original indices of the points in range, in scan order, into the query's segment [offsets[q], offsets[q + 1]) of `indices`
template <typename T>
__global__ __launch_bounds__(NB_Q_THREADS) void grid_ball_fill_kernel(Grid g, const T* __restrict__ queries, const int* __restrict__ order, long m,
                                                                      double reach, long long r2_bits, const long long* __restrict__ offsets,
                                                                      long total, int* __restrict__ indices) {
  const long t = (long)blockIdx.x * NB_Q_THREADS + threadIdx.x;
  if (t >= m) return;
  const long q = order ? (long)order[t] : t;
  const double qx = (double)queries[q * 3], qy = (double)queries[q * 3 + 1], qz = (double)queries[q * 3 + 2];
  long long at = offsets[q];
  const long long end = offsets[q + 1] < (long long)total ? offsets[q + 1] : (long long)total;
  if (at < 0) return;
  for_each_in_range(g, qx, qy, qz, reach, r2_bits, [&](long j, long long, double, double, double) {
    if (at < end) indices[at++] = g.index[j];
  });
}

int check_grid(const void* a, const void* b, const void* c, long n, double ox, double oy, double oz, double cell, long ex, long ey, long ez) {
  if (!a || !b || !c || n <= 0) return CG_ERR_ARG;
  if (n > (long)INT_MAX) return CG_ERR_UNSUPPORTED;         // original indices are i32
  if (!isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !(cell > 0.0) || !isfinite(cell)) return CG_ERR_ARG;
  if (ex < 1 || ey < 1 || ez < 1) return CG_ERR_ARG;
  const long long lim = 1LL << 62;
  if ((long long)ex > (lim - 1) / ey || (long long)ex * ey > (lim - 1) / ez) return CG_ERR_ARG;   // the keys need ex ey ez < 2^62
  return CG_OK;
}

int check_radius(double radius, double cell) {
  if (!(radius > 0.0) || !isfinite(radius) || radius > cell || !(radius * radius >= DBL_MIN)) return CG_ERR_ARG;
  return CG_OK;
}

long long bits_of(double x) {
  long long b;
  memcpy(&b, &x, sizeof b);
  return b;
}

double reach_of(double radius) { return radius * (1.0 + 0x1p-40); }

template <bool NEAREST>
int launch_query(const Grid& g, const void* queries, int queries_f64, const int* order, long m, double radius, int* out_i, double* out_d2,
                 void* stream) {
  const unsigned blocks = (unsigned)((m + NB_Q_THREADS - 1) / NB_Q_THREADS);
  if (queries_f64)
    hipLaunchKernelGGL((grid_query_kernel<double, NEAREST>), dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const double*)queries,
                       order, m, reach_of(radius), bits_of(radius * radius), out_i, out_d2);
  else
    hipLaunchKernelGGL((grid_query_kernel<float, NEAREST>), dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const float*)queries,
                       order, m, reach_of(radius), bits_of(radius * radius), out_i, out_d2);
  return cg_hip_status(hipGetLastError());
}

}  // namespace

extern "C" int cg_grid_cell_keys(const void* points, int points_f64, long n, double origin_x, double origin_y, double origin_z, double cell,
                                 long ext_x, long ext_y, long ext_z, long long* keys, void* stream) {
  const int st = check_grid(points, keys, keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st != CG_OK) return st;
  const Grid g = {nullptr, nullptr, nullptr, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  const unsigned blocks = (unsigned)((n + NB_Q_THREADS - 1) / NB_Q_THREADS);
  if (points_f64)
    hipLaunchKernelGGL(cell_keys_kernel<double>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, (const double*)points, n, g, keys);
  else
    hipLaunchKernelGGL(cell_keys_kernel<float>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, (const float*)points, n, g, keys);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_grid_normals(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                               double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, double radius, int max_nn,
                               double view_x, double view_y, double view_z, double* normals, int* nb_count, double* nb_d2max, void* stream) {
  if (max_nn > CG_NB_MAX_NN) return CG_ERR_UNSUPPORTED;
  if (max_nn < 1 || !normals) return CG_ERR_ARG;
  int st = check_grid(sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st == CG_OK) st = check_radius(radius, cell);
  if (st != CG_OK) return st;
  if (!isfinite(view_x) || !isfinite(view_y) || !isfinite(view_z)) return CG_ERR_ARG;
  const Grid g = {sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  const unsigned blocks = (unsigned)((n + NB_THREADS - 1) / NB_THREADS);
  hipLaunchKernelGGL(grid_normals_kernel, dim3(blocks), dim3(NB_THREADS), (size_t)max_nn * NB_THREADS * NB_ENTRY_BYTES, (hipStream_t)stream, g,
                     reach_of(radius), bits_of(radius * radius), max_nn, view_x, view_y, view_z, normals, nb_count, nb_d2max);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_grid_nearest_within(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n,
                                      double origin_x, double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z,
                                      const void* queries, int queries_f64, const int* query_order, long m, double radius, int* nn_index,
                                      double* nn_d2, void* stream) {
  if (!queries || !nn_index || !nn_d2 || m <= 0) return CG_ERR_ARG;
  if (m > (long)INT_MAX) return CG_ERR_UNSUPPORTED;
  int st = check_grid(sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st == CG_OK) st = check_radius(radius, cell);
  if (st != CG_OK) return st;
  const Grid g = {sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  return launch_query<true>(g, queries, queries_f64, query_order, m, radius, nn_index, nn_d2, stream);
}

extern "C" int cg_grid_count_within(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                                    double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                                    int queries_f64, const int* query_order, long m, double radius, int* count, void* stream) {
  if (!queries || !count || m <= 0) return CG_ERR_ARG;
  if (m > (long)INT_MAX) return CG_ERR_UNSUPPORTED;
  int st = check_grid(sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st == CG_OK) st = check_radius(radius, cell);
  if (st != CG_OK) return st;
  const Grid g = {sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  return launch_query<false>(g, queries, queries_f64, query_order, m, radius, count, nullptr, stream);
}

extern "C" int cg_grid_nearest(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                               double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                               int queries_f64, const int* query_order, long m, int* nn_index, double* nn_d2, int* rounds, void* stream) {
  if (!queries || !nn_index || !nn_d2 || m <= 0) return CG_ERR_ARG;
  if (m > (long)INT_MAX) return CG_ERR_UNSUPPORTED;
  const int st = check_grid(sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st != CG_OK) return st;
  const Grid g = {sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  const unsigned blocks = (unsigned)((m + NB_Q_THREADS - 1) / NB_Q_THREADS);
  if (queries_f64)
    hipLaunchKernelGGL(grid_nearest_kernel<double>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const double*)queries,
                       query_order, m, nn_index, nn_d2, rounds);
  else
    hipLaunchKernelGGL(grid_nearest_kernel<float>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const float*)queries,
                       query_order, m, nn_index, nn_d2, rounds);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_grid_ball_fill(const double* sorted_points, const int* sorted_index, const long long* sorted_keys, long n, double origin_x,
                                 double origin_y, double origin_z, double cell, long ext_x, long ext_y, long ext_z, const void* queries,
                                 int queries_f64, const int* query_order, long m, double radius, const long long* offsets, long total,
                                 int* indices, void* stream) {
  if (!queries || !offsets || m <= 0 || total < 0 || (!indices && total > 0)) return CG_ERR_ARG;
  if (m > (long)INT_MAX) return CG_ERR_UNSUPPORTED;
  int st = check_grid(sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z);
  if (st == CG_OK) st = check_radius(radius, cell);
  if (st != CG_OK) return st;
  if (total == 0) return CG_OK;
  const Grid g = {sorted_points, sorted_index, sorted_keys, n, origin_x, origin_y, origin_z, cell, ext_x, ext_y, ext_z};
  const unsigned blocks = (unsigned)((m + NB_Q_THREADS - 1) / NB_Q_THREADS);
  if (queries_f64)
    hipLaunchKernelGGL(grid_ball_fill_kernel<double>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const double*)queries,
                       query_order, m, reach_of(radius), bits_of(radius * radius), offsets, total, indices);
  else
    hipLaunchKernelGGL(grid_ball_fill_kernel<float>, dim3(blocks), dim3(NB_Q_THREADS), 0, (hipStream_t)stream, g, (const float*)queries,
                       query_order, m, reach_of(radius), bits_of(radius * radius), offsets, total, indices);
  return cg_hip_status(hipGetLastError());
}
