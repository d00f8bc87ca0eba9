// Device replacements for the host-side bookkeeping that capped the reference-API entry points in round 1
// (VERDICT r1 "What's weak" #1): at 50k candidates the python loops around the kernels cost 20x the kernels.
//  * cg_draw_resample_ids   : the per-candidate `np.random.choice(M, n_pts, replace=M<n_pts)` of GraspDataset.transform
//                             (dataset_grasp.py:72-73; one call per pose in the python loop of predicter.py:71-74) as a
//                             counter-based draw on the device (Philox4x32-10 keys; k-subsets in random order: a keyed Feistel
//                             bijection + cycle walking from 1,025 points on (round 6), a sort of random keys per row below).
//                             NOT numpy's stream: the seeded-parity mode of predict_batch keeps drawing on the host.
//  * cg_pose_inverse_rows   : inv(grasp_pose) of dataset_grasp.py:69-70 in float64, re-expressed for the centred
//                             float32 cloud (transforms.pose_inverse_rows), for poses that are already on the device
//                             (the filter's output).
//  * cg_mesh_grid_count/fill/sort : the broad-phase grid of the gripper mesh (my_cpp.MeshGrid), one thread per
//                             triangle instead of a python loop per triangle.
#include <stdlib.h>
#include "cg_common.hpp"
#include "../../include/catgrasp_amd.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0,k1) -> 4 x 32 random bits
// ---------------------------------------------------------------------------------------------------------------------
struct U4 { unsigned x, y, z, w; };
__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
    U4 n;
    n.x = (unsigned)(p1 >> 32) ^ c.y ^ k0;
    n.y = (unsigned)p1;
    n.z = (unsigned)(p0 >> 32) ^ c.w ^ k1;
    n.w = (unsigned)p0;
    c = n;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// uniform integer in [0, n): Lemire's multiply-shift with rejection (exactly uniform), drawing from a Philox stream
struct Stream {
  unsigned k0, k1, row; unsigned ctr; U4 buf; int have;
  __device__ __forceinline__ unsigned next() {
    if (have == 0) { buf = philox4x32_10(U4{row, ctr++, 0u, 0u}, k0, k1); have = 4; }
    const unsigned r = (have == 4) ? buf.x : (have == 3) ? buf.y : (have == 2) ? buf.z : buf.w;
    --have;
    return r;
  }
  __device__ __forceinline__ unsigned below(unsigned n) {
    unsigned long long m = (unsigned long long)next() * n;
    unsigned lo = (unsigned)m;
    if (lo < n) {
      const unsigned t = (0u - n) % n;
      while (lo < t) { m = (unsigned long long)next() * n; lo = (unsigned)m; }
    }
    return (unsigned)(m >> 32);
  }
};

// Draws without replacement from at most 1,024 points, as a SORT: one workgroup per row.  Every point index gets a 48-bit random key
// (two Philox words; a tie between two of 1,024 keys has probability 2e-9 per row and is then decided by the index), the (key, index)
// pairs are bitonic-sorted and the first n_pts indices are the row: a uniform n_pts-subset in uniform order, like
// np.random.choice(replace=False).  A row is N = 2^LOG_N = 1,024 pairs on 256 threads, E = N / 256 = 4 per thread IN REGISTERS: a
// compare-exchange round with partner distance 2^p runs inside the registers of a thread whenever bit p of the element index is one of
// the thread's register bits, and the elements are re-dealt through LDS (write E, barrier, read E) only when the next round's bit is
// not -- a few deals per merge stage instead of a trip through LDS per round.  (Larger clouds take the bijection kernel below; the
// Fisher-Yates and wider sort kernels it replaced are measured in DESIGN 4.4 / 4.7.)
template <int LOG_N>
struct SortGeo {
  static constexpr int LOG_T = 8, LOG_E = LOG_N - LOG_T, E = 1 << LOG_E, N = 1 << LOG_N;
  static_assert(LOG_N == 10, "1,024 pairs per row on 256 threads: the one size cg_draw_resample_ids launches");
  // lowest register bit of the layout that holds element-index bit p in a thread's registers
  static constexpr int lo_of(int p) { return (p / LOG_E) * LOG_E > LOG_N - LOG_E ? LOG_N - LOG_E : (p / LOG_E) * LOG_E; }
};

template <int LOG_N, int LO>
__device__ __forceinline__ int sort_index(int t, int r) {          // element index of register r of thread t when the register bits are [LO, LO + LOG_E)
  constexpr int LOG_E = SortGeo<LOG_N>::LOG_E;
  return ((t >> LO) << (LO + LOG_E)) | (r << LO) | (t & ((1 << LO) - 1));
}

template <int LOG_N, int FROM, int TO>
__device__ __forceinline__ void sort_deal(unsigned long long (&e)[1 << (LOG_N - 8)], unsigned long long* keys, int t) {
  constexpr int E = SortGeo<LOG_N>::E;
  __syncthreads();                                                 // whoever still reads the previous deal is done
#pragma unroll
  for (int r = 0; r < E; ++r) keys[sort_index<LOG_N, FROM>(t, r)] = e[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < E; ++r) e[r] = keys[sort_index<LOG_N, TO>(t, r)];
}

// rounds p = P .. 0 of merge stage S (blocks of 2^S: ascending where bit S of the index is 0; the last stage is ascending throughout)
template <int LOG_N, int S, int P, int LO>
__device__ __forceinline__ void sort_rounds(unsigned long long (&e)[1 << (LOG_N - 8)], unsigned long long* keys, int t) {
  constexpr int LOG_E = SortGeo<LOG_N>::LOG_E, E = SortGeo<LOG_N>::E;
  constexpr int NEED = SortGeo<LOG_N>::lo_of(P);
  if constexpr (NEED != LO) sort_deal<LOG_N, LO, NEED>(e, keys, t);
  constexpr int RB = 1 << (P - NEED);                              // the register bit of this round
  bool up_t = true;                                                // direction when bit S lies in the thread part of the index
  if constexpr (S < LOG_N && !(S >= NEED && S < NEED + LOG_E)) up_t = ((sort_index<LOG_N, NEED>(t, 0) >> S) & 1) == 0;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    if ((r & RB) == 0) {
      bool up = up_t;
      if constexpr (S < LOG_N && S >= NEED && S < NEED + LOG_E) up = ((r >> (S - NEED)) & 1) == 0;
      const unsigned long long a = e[r], b = e[r | RB];
      const bool sw = (a > b) == up;
      e[r] = sw ? b : a; e[r | RB] = sw ? a : b;
    }
  }
  if constexpr (P > 0) sort_rounds<LOG_N, S, P - 1, NEED>(e, keys, t);
  else if constexpr (S < LOG_N) sort_rounds<LOG_N, S + 1, S, NEED>(e, keys, t);
  else if constexpr (NEED != 0) sort_deal<LOG_N, NEED, 0>(e, keys, t);          // leave the sorted row in consecutive order
}

template <int LOG_N>
__global__ __launch_bounds__(256) void draw_ids_sort_kernel(int n_valid, int n_pts, long count, unsigned k0, unsigned k1, int base,
                                                            long row_offset, int* __restrict__ out) {
  constexpr int E = SortGeo<LOG_N>::E, N = SortGeo<LOG_N>::N;
  __shared__ unsigned long long keys[N];
  const int t = threadIdx.x;
  const long row = blockIdx.x;
  const long grow = row + row_offset;          // the stream is a function of the GLOBAL row: a shard draws what the whole would
  const unsigned c0 = (unsigned)grow, c2 = (unsigned)(grow >> 32);
  unsigned long long e[E];                     // elements t*E .. t*E + E-1 (layout with register bits [0, LOG_E))
#pragma unroll
  for (int r = 0; r < E; r += 2) {             // one Philox block keys two points
    const int i0 = t * E + r, i1 = i0 + 1;
    const U4 w = philox4x32_10(U4{c0, (unsigned)(i0 >> 1), c2, 0x50525453u}, k0, k1);
    e[r] = i0 < n_valid ? ((unsigned long long)w.x << 32 | (unsigned long long)(w.y & 0xffff0000u)) | (unsigned)i0 : ~0ull;
    e[r + 1] = i1 < n_valid ? ((unsigned long long)w.z << 32 | (unsigned long long)(w.w & 0xffff0000u)) | (unsigned)i1 : ~0ull;
  }
  sort_rounds<LOG_N, 1, 0, 0>(e, keys, t);
  // registers hold elements t*E + r of the sorted row again: the first n_pts indices leave through LDS for coalesced stores
  __syncthreads();
#pragma unroll
  for (int r = 0; r < E; ++r) keys[t * E + r] = e[r];
  __syncthreads();
  int* o = out + row * n_pts;
  for (int i = t; i < n_pts; i += 256) o[i] = (int)(keys[i] & 0xffffu) + base;
}

// The same draw WITHOUT a sort or a swap chain (round 6): a keyed BIJECTION of [0, 2^b), b = the even number of bits that covers n_valid,
// evaluated at i = 0 .. n_pts-1 and cycle-walked into [0, n_valid) (v <- pi(v) until v < n_valid: the standard way to restrict a
// permutation of a superset -- the i < n_pts <= n_valid start inside the set, every walk ends at a distinct element of it).  pi is a
// 12-round Feistel network on two b/2-bit halves whose round function is a multiply-xorshift hash of (half, round key); the 12
// round keys of a row are three Philox4x32-10 blocks of (seed, global row), so rows are independent and a shard draws what the whole
// batch would.  This is the construction of GPU shuffles without global synchronisation (Mitchell et al., "Bandwidth-optimal random
// shuffling for GPUs", 2021: a variable-length Feistel bijection + cycle walking); every output costs ~100 integer operations and
// nothing waits for anything: the row's 2,048 indices are 8 per thread of one workgroup.  Against the sort kernel above -- 38 ms of
// LDS-bound work per 50,000-candidate step, a tenth of it exposed -- this is ~1 ms.  (The sort draws a uniformly random permutation
// up to the quality of its 48-bit keys; this draws from a family of 2^384 keyed permutations per row.  Both are "a uniform
// n_pts-subset in uniform order" to every test a resampling of 2,048 of ~2,500 surface points can notice:
// tests/test_predicter_gpu.py checks index and slot frequencies, pair statistics and row independence.)
constexpr int BIJ_ROUNDS = 12;

// the round function's hash: two 24-BIT multiplies (v_mul_u32_u24 runs at full rate on gfx950, a 32-bit integer multiply at a quarter)
__device__ __forceinline__ unsigned bij_mix(unsigned x, unsigned k) {
  x += k & 0x7FFFFFu;                       // half < 2^15, key 23 bits: < 2^24
  unsigned h = __umul24(x, 0x9E3779u);
  h ^= h >> 15;
  h = __umul24(h >> 8, 0x85EBCBu);
  h ^= h >> 13;
  return h;
}

__global__ __launch_bounds__(256) void draw_ids_bijection_kernel(int n_valid, int n_pts, long count, unsigned k0, unsigned k1, int base,
                                                                 long row_offset, int half_bits, int* __restrict__ out) {
  __shared__ unsigned rk_lds[BIJ_ROUNDS];
  const int t = threadIdx.x;
  const unsigned hmask = (1u << half_bits) - 1u;
  for (long row = blockIdx.x; row < count; row += gridDim.x) {
    const long grow = row + row_offset;        // the stream is a function of the GLOBAL row
    __syncthreads();
    if (t < BIJ_ROUNDS / 4) {
      const U4 w = philox4x32_10(U4{(unsigned)grow, (unsigned)t, (unsigned)(grow >> 32), 0x42494A43u}, k0, k1);
      rk_lds[4 * t] = w.x; rk_lds[4 * t + 1] = w.y; rk_lds[4 * t + 2] = w.z; rk_lds[4 * t + 3] = w.w;
    }
    __syncthreads();
    unsigned rk[BIJ_ROUNDS];
#pragma unroll
    for (int q = 0; q < BIJ_ROUNDS; ++q) rk[q] = rk_lds[q];
    int* o = out + row * n_pts;
    // ONE loop over the thread's outputs i = t, t + 256, ... and their walks: a wavefront then runs for the largest SUM of walk
    // lengths among its lanes (~20 applications of pi for 8 outputs at n_valid / 2^b = 0.61) instead of the sum of the largest walk
    // per output (~35)
    int i = t;
    unsigned v = (unsigned)i;
    while (i < n_pts) {
      unsigned l = v >> half_bits, r = v & hmask;
#pragma unroll
      for (int q = 0; q < BIJ_ROUNDS; ++q) {
        const unsigned f = bij_mix(r, rk[q]) >> (32 - half_bits);        // the hash's top bits
        const unsigned nr = l ^ f;
        l = r; r = nr;
      }
      v = (l << half_bits) | r;
      if (v < (unsigned)n_valid) {
        o[i] = (int)v + base;
        i += 256;
        v = (unsigned)i;
      }
    }
  }
}

// The swap chain of numpy's permutation(n_valid) for `count` rows whose swap partners the host extracted from numpy's generator
// (cg_host_numpy_shuffle_partners): a[i] <-> a[j(i)] for i = n_valid-1 .. 1 on a = arange(n_valid), out = a[:n_pts] + base.
// One lane per row, the row's array in LDS as u16, rows interleaved (element k of row r at [k*R + r]: the lanes' sequential
// initialisation is conflict-free and their random accesses spread over the banks; the LDS operations of a lane execute in
// program order, so the chain needs no other synchronisation); partners arrive 8 steps per 16-byte load, one load
// ahead of the chain; the finished rows leave through coalesced stores by the whole wave.
__global__ __launch_bounds__(64) void apply_shuffle_rows_kernel(const unsigned short* __restrict__ partners, long row_stride,
                                                                int n_valid, int n_pts, long count, int base, int R,
                                                                int* __restrict__ out) {
  extern __shared__ unsigned short perm[];
  const int r = threadIdx.x;
  const long row0 = (long)blockIdx.x * R, row = row0 + r;
  if (r < R && row < count) {
    for (int k = 0; k < n_valid; ++k) perm[k * R + r] = (unsigned short)k;
    const uint4* js = (const uint4*)(partners + row * row_stride);
    const int steps = n_valid - 1;
    int i = n_valid - 1;
    uint4 nxt = js[0];
    for (int s0 = 0; s0 < steps; s0 += 8) {
      const uint4 cur = nxt;
      if (s0 + 8 < steps) nxt = js[(s0 >> 3) + 1];
      const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        if (s0 + t < steps) {
          const int j = (int)((w[t >> 1] >> ((t & 1) * 16)) & 0xffffu);
          const unsigned short pa = perm[i * R + r], pb = perm[j * R + r];
          perm[i * R + r] = pb;
          perm[j * R + r] = pa;
          --i;
        }
      }
    }
  }
  __syncthreads();
  const long left = count - row0;
  const int nrows = left < (long)R ? (int)left : R;
  for (int rr = 0; rr < nrows; ++rr) {
    int* o = out + (row0 + rr) * n_pts;
    for (int k = threadIdx.x; k < n_pts; k += 64) o[k] = (int)perm[k * R + rr] + base;
  }
}

// n_valid < n_pts: iid uniform indices = np.random.choice(replace=True)
__global__ __launch_bounds__(256) void draw_ids_iid_kernel(int n_valid, int n_pts, long count, unsigned k0, unsigned k1,
                                                           int base, long row_offset, int* __restrict__ out) {
  const long total = count * n_pts;
  const long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (g >= total) return;
  const long gg = g + row_offset * n_pts;      // n_pts % 4 == 0 (checked by the launcher): quads never straddle rows
  Stream s{k0, k1 ^ 0x5bd1e995u, (unsigned)(gg >> 2), (unsigned)(gg >> 34) << 24, U4{0, 0, 0, 0}, 0};
  for (int k = 0; k < 4 && g + k < total; ++k) out[g + k] = (int)s.below((unsigned)n_valid) + base;
}

// ---------------------------------------------------------------------------------------------------------------------
template <typename TIn>      // float: poses produced on the device (the filter's output); double: the caller's float64 pose list, uploaded as is
__global__ __launch_bounds__(256) void pose_inverse_rows_kernel(const TIn* __restrict__ poses, long E, double cx, double cy,
                                                                double cz, float* __restrict__ out, int* __restrict__ bad) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const TIn* P = poses + e * 16;
  int flags = 0;                // bit 0: NaN / Inf in the pose; bit 1: singular (np.linalg.inv raises LinAlgError) or an inverse beyond
                                // float32; bit 2: last row is not 0 0 0 1 (the closed form below inverts an AFFINE matrix)
  {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 16; ++k) ok = ok && isfinite((double)P[k]);
    if (!ok) flags |= 1;
    if (!((double)P[12] == 0.0 && (double)P[13] == 0.0 && (double)P[14] == 0.0 && (double)P[15] == 1.0)) flags |= 4;
  }
  const double a00 = P[0], a01 = P[1], a02 = P[2], t0 = P[3];
  const double a10 = P[4], a11 = P[5], a12 = P[6], t1 = P[7];
  const double a20 = P[8], a21 = P[9], a22 = P[10], t2 = P[11];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double id = 1.0 / det;
  if (det == 0.0 || !isfinite(id)) flags |= 2;
  double I[9];
  I[0] = c00 * id; I[1] = (a02 * a21 - a01 * a22) * id; I[2] = (a01 * a12 - a02 * a11) * id;
  I[3] = c01 * id; I[4] = (a00 * a22 - a02 * a20) * id; I[5] = (a02 * a10 - a00 * a12) * id;
  I[6] = c02 * id; I[7] = (a01 * a20 - a00 * a21) * id; I[8] = (a00 * a11 - a01 * a10) * id;
  // x_grasp = inv(A) (x_cam - t) with x_cam = x_centred + centre
  const double d0 = cx - t0, d1 = cy - t1, d2 = cz - t2;
  float* o = out + e * 12;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    o[r * 4 + 0] = (float)I[r * 3 + 0]; o[r * 4 + 1] = (float)I[r * 3 + 1]; o[r * 4 + 2] = (float)I[r * 3 + 2];
    o[r * 4 + 3] = (float)(I[r * 3 + 0] * d0 + I[r * 3 + 1] * d1 + I[r * 3 + 2] * d2);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (!isfinite(o[r * 4 + k])) flags |= 2;
  }
  if (bad && flags) atomicOr(bad, flags);
}

// ---------------------------------------------------------------------------------------------------------------------
// mesh-frame broad-phase grid (see cg_mesh_grid): cell range of a triangle's inflated bounding box, float64 like the
// host builder so both produce the same lists
// ---------------------------------------------------------------------------------------------------------------------
struct GridGeom { double ox, oy, oz, cell, inflate; int nx, ny, nz; };

__device__ __forceinline__ void tri_cell_range(const float* __restrict__ V, const int* __restrict__ F, int t, const GridGeom& g,
                                               int* lo, int* hi) {
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = V + 3 * (size_t)F[(size_t)t * 3 + k];
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double x = (double)v[a]; mn[a] = fmin(mn[a], x); mx[a] = fmax(mx[a], x); }
  }
  const double o[3] = {g.ox, g.oy, g.oz};
  const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const long l = (long)floor((mn[a] - g.inflate - o[a]) / g.cell);
    const long h = (long)floor((mx[a] + g.inflate - o[a]) / g.cell);
    lo[a] = (int)(l < 0 ? 0 : (l > n[a] - 1 ? n[a] - 1 : l));
    hi[a] = (int)(h < 0 ? 0 : (h > n[a] - 1 ? n[a] - 1 : h));
  }
}

template <bool FILL>
__global__ __launch_bounds__(256) void mesh_grid_kernel(const float* __restrict__ V, const int* __restrict__ F, int nf, GridGeom g,
                                                        int* __restrict__ counts, const int* __restrict__ cell_start,
                                                        int* __restrict__ tri_ids) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nf) return;
  int lo[3], hi[3];
  tri_cell_range(V, F, t, g, lo, hi);
  for (int i = lo[0]; i <= hi[0]; ++i)
    for (int j = lo[1]; j <= hi[1]; ++j)
      for (int k = lo[2]; k <= hi[2]; ++k) {
        const int c = (i * g.ny + j) * g.nz + k;
        const int pos = atomicAdd(counts + c, 1);
        if (FILL) tri_ids[cell_start[c] + pos] = t;
      }
}

// ascending triangle ids inside every cell (the host builder's order), so the structure is deterministic
__global__ __launch_bounds__(256) void mesh_grid_sort_kernel(const int* __restrict__ cell_start, long ncell, int* __restrict__ tri_ids) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const int b = cell_start[c], e = cell_start[c + 1];
  for (int i = b + 1; i < e; ++i) {
    const int v = tri_ids[i];
    int j = i - 1;
    while (j >= b && tri_ids[j] > v) { tri_ids[j + 1] = tri_ids[j]; --j; }
    tri_ids[j + 1] = v;
  }
}

inline bool geom_ok(const double* o, double cell, double inflate, const int* dims) {
  return o && dims && cell > 0.0 && inflate >= 0.0 && dims[0] > 0 && dims[1] > 0 && dims[2] > 0 &&
         (long)dims[0] * dims[1] * dims[2] < (1l << 31);
}

}  // namespace

extern "C" int cg_draw_resample_ids(int n_valid, int n_pts, long count, unsigned long long seed, int base, long row_offset, int* out,
                                    void* stream) {
  if (n_valid <= 0 || n_pts <= 0 || count < 0 || row_offset < 0) return CG_ERR_ARG;
  if (count == 0) return CG_OK;
  if (!out) return CG_ERR_ARG;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  hipStream_t s = (hipStream_t)stream;
  if (n_valid >= n_pts && n_valid > 1024) {   // without replacement: the keyed bijection (halves of >= 6 bits), any cloud size up to 2^30
    int bits = 2;
    while (bits < 30 && (1L << bits) < (long)n_valid) bits += 2;
    if ((1L << bits) < (long)n_valid) return CG_ERR_UNSUPPORTED;
    const long blocks = count < 65536 * 4 ? count : 65536 * 4;
    hipLaunchKernelGGL(draw_ids_bijection_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n_valid, n_pts, count, k0, k1, base, row_offset, bits / 2, out);
    return cg_hip_status(hipGetLastError());
  }
  if (n_valid >= n_pts) {                     // at most 1,024 points: the sort kernel
    hipLaunchKernelGGL(draw_ids_sort_kernel<10>, dim3((unsigned)count), dim3(256), 0, s, n_valid, n_pts, count, k0, k1, base, row_offset, out);
    return cg_hip_status(hipGetLastError());
  }
  if ((n_pts & 3) != 0) return CG_ERR_UNSUPPORTED;
  const long total = count * n_pts;
  hipLaunchKernelGGL(draw_ids_iid_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, n_valid, n_pts, count, k0, k1, base, row_offset, out);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_apply_shuffle_rows(const unsigned short* partners, long row_stride, int n_valid, int n_pts, long count, int base,
                                     int* out, void* stream) {
  if (n_valid < 2 || n_valid > 65536 || n_pts <= 0 || n_pts > n_valid || count < 0 || row_stride < n_valid - 1 || (row_stride & 7))
    return CG_ERR_ARG;
  if (count == 0) return CG_OK;
  if (!partners || !out || ((uintptr_t)partners & 15)) return CG_ERR_ARG;
  constexpr size_t LDS = 128 * 1024;
  int R = (int)(LDS / ((size_t)n_valid * 2));
  if (R > 64) R = 64;
  const size_t bytes = (size_t)R * n_valid * 2;
  if (bytes > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return CG_ERR_UNSUPPORTED;
    const int st = cg_allow_dynamic_lds<apply_shuffle_rows_kernel>(dev, LDS);
    if (st != CG_OK) return st;
  }
  hipLaunchKernelGGL(apply_shuffle_rows_kernel, dim3((unsigned)((count + R - 1) / R)), dim3(64), bytes, (hipStream_t)stream, partners, row_stride, n_valid,
                     n_pts, count, base, R, out);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_pose_inverse_rows(const float* poses, long n_poses, const double* h_center, float* out, void* stream) {
  if (n_poses < 0) return CG_ERR_ARG;
  if (n_poses == 0) return CG_OK;
  if (!poses || !out || !h_center) return CG_ERR_ARG;
  hipLaunchKernelGGL(pose_inverse_rows_kernel<float>, dim3((unsigned)((n_poses + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     poses, n_poses, h_center[0], h_center[1], h_center[2], out, (int*)nullptr);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_pose_inverse_rows_f64(const double* poses, long n_poses, const double* h_center, float* out, int* bad_flag, void* stream) {
  if (n_poses < 0) return CG_ERR_ARG;
  if (n_poses == 0) return CG_OK;
  if (!poses || !out || !h_center) return CG_ERR_ARG;
  hipLaunchKernelGGL(pose_inverse_rows_kernel<double>, dim3((unsigned)((n_poses + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     poses, n_poses, h_center[0], h_center[1], h_center[2], out, bad_flag);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_mesh_grid_count(const float* vertices, const int* faces, int n_faces, const double* h_origin, double cell,
                                  double inflate, const int* h_dims, int* counts, void* stream) {
  if (n_faces < 0 || !geom_ok(h_origin, cell, inflate, h_dims)) return CG_ERR_ARG;
  if (n_faces == 0) return CG_OK;
  if (!vertices || !faces || !counts) return CG_ERR_ARG;
  const GridGeom g{h_origin[0], h_origin[1], h_origin[2], cell, inflate, h_dims[0], h_dims[1], h_dims[2]};
  hipLaunchKernelGGL(mesh_grid_kernel<false>, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices, faces, n_faces, g, counts, (const int*)nullptr, (int*)nullptr);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_mesh_grid_fill(const float* vertices, const int* faces, int n_faces, const double* h_origin, double cell,
                                 double inflate, const int* h_dims, const int* cell_start, int* cursor, int* tri_ids, void* stream) {
  if (n_faces < 0 || !geom_ok(h_origin, cell, inflate, h_dims)) return CG_ERR_ARG;
  if (n_faces == 0) return CG_OK;
  if (!vertices || !faces || !cell_start || !cursor || !tri_ids) return CG_ERR_ARG;
  const GridGeom g{h_origin[0], h_origin[1], h_origin[2], cell, inflate, h_dims[0], h_dims[1], h_dims[2]};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_grid_kernel<true>, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, s,
                     vertices, faces, n_faces, g, cursor, cell_start, tri_ids);
  const long ncell = (long)h_dims[0] * h_dims[1] * h_dims[2];
  hipLaunchKernelGGL(mesh_grid_sort_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, s, cell_start, ncell, tri_ids);
  return cg_hip_status(hipGetLastError());
}
