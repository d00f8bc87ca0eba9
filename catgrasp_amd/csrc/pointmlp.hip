// Fused shared per-point MLP chain + max-pool over points ("PointNet set encoder" pass).
//
// Replaces, per network pass, the reference op sequence
//   Conv1d(k=1) -> BatchNorm1d -> ReLU  (x2 or x3)  ->  Conv1d(128->1024) -> BN [-> ReLU] -> max(dim=N)
// of STN3d.forward (pointnet2.py:172-176), STNkd.forward (:210-214) and
// PointNetEncoder.forward (:243-266), including the learned input transform `bmm(x, trans)` (:248)
// and feature transform `bmm(x, trans_feat)` (:257).  BatchNorm (eval) is folded into the conv
// weights on the host (catgrasp_amd/folding.py), so every layer here is  y = act(W' x + b').
//
// One workgroup (4 waves) owns one sample (or one slice of a sample's point tiles).  A tile of
// TP=64 points is carried through the whole chain inside LDS; only the 1024-wide max ever
// leaves the CU.  All contractions with K>=64 run on v_mfma_f32_32x32x2_f32 (exact f32):
// points are the MFMA M dimension (A operand, ds_read_b128 from LDS), channels the N dimension
// (B operand, pre-packed weight fragments streamed from L2 with global_load_dwordx4), so the
// max over points is a per-lane reduction over the 16 accumulator registers + one lane^32 swap.
#include <stdlib.h>
#include "cg_split.hpp"
#include "../../include/catgrasp_amd.h"
#include "../../include/catgrasp_amd_screen.h"
#include "l3_f32_asm.inc"

namespace {

constexpr int TP = 64;      // points per tile
constexpr int S64 = 68;     // LDS row stride (floats) of 64-wide activations (16B aligned, conflict-free b128)
constexpr int S128 = 132;   // LDS row stride of the 128-wide activation
constexpr int XS = 8;       // LDS row stride of the staged input points

struct Args {
  const float* x; int B; int N;
  const float* t3;                  // (B,9) or null
  const float* w1; const float* b1; // (64,6) row-major, (64)
  const float* wm; const float* bm; // packed 64->64 (MID==1)
  const float* t64;                 // (B,64,64) (MID==2), TRANSPOSED: t64[b][n][k] = T_b[k][n];  h' = h . T
  const float* w2; const float* b2; // packed 64->128
  const float* w3; const float* b3; // packed 128->1024
  int relu3;
  int nsplit;                       // workgroups per sample (point tiles are divided between them)
  int n_main; int tail_split;       // samples [n_main, B) use tail_split workgroups each (tail balancing, see the launcher)
  float* out;                       // (B,1024); pre-filled with -inf when nsplit>1
  float* pointfeat;                 // optional (B,N,64): output of the mid layer (MID==2 only)
  // SCR only (cg_pointmlp_max_screened): the bf16 hi / lo image of w3 (folding.pack_b_split), an upper bound of every row norm of w3
  // (+ their maximum at [1024]), the optional counters and the path selector (0 normal, 1 exact stream only, 2 screen first tiles too)
  const unsigned short* w3s; const float* wn; long long* stats; int force;
};

// LDS layout (floats): [h2 / hA region: TP*S128] [hB: TP*S64] [xs: TP*XS] [rmax: 1024]
constexpr int WM_FLOATS = 2 * 8 * 64 * 4;          // the 64 -> 64 layer's B fragments [nb 2][ks 8][lane 64][4]: 16 KB
constexpr int LDS_FLOATS = TP * S128 + TP * S64 + TP * XS + 1024 + WM_FLOATS;

// ---- the screened 128 -> 1024 layer (SCR; derivation of the bound: DESIGN.md §4.1c) ----
// Behind the front layers' LDS: [hn: TP floats][ctl: 4 ints][list: SCR_CAP x 16 bit][zt: SCR_CAP floats, only with stats]
constexpr int SCR_CAP = 3072;                         // (row << 10 | channel) entries a tile may hand to the exact verification
constexpr int SCR_LDS_BYTES = LDS_FLOATS * 4 + TP * 4 + 16 + SCR_CAP * 2;       // 80,144 B: two workgroups per CU as before
constexpr int SCR_LDS_BYTES_STATS = SCR_LDS_BYTES + SCR_CAP * 4;
// E_pc = SCR_KAPPA * wn_c * hn_p + SCR_FLOOR >= |screen value - fmaf chain value| while every wn_c, hn_p <= SCR_RANGE
constexpr float SCR_KAPPA = 7.f / 65536.f;            // 7 * 2^-16 = 1.068e-4 >= 1.05 * (3.03 * 2^-16 + 1.016 * 384 * 2^-23 + 128 * 2^-24)
constexpr float SCR_FLOOR = 0x1p-60f;                 // absolute part: pieces / products / sums that underflow
constexpr float SCR_RANGE = 0x1p30f;
constexpr float SCR_HN_UP = 1.f + 0x1p-16f;           // rounding of the f32 sum of squares and of the root
constexpr float SCR_HN_ABS = 0x1p-59f;                // squares below 2^-126 that the sum may have lost
enum { ST_SCREENED = 0, ST_OVERFLOW = 1, ST_RANGE = 2, ST_FIRST = 3, ST_PAIRS = 4, ST_RATIO = 5, ST_FORCED = 6 };

// max into an LDS float by sign bit, the total order v_max_f32 applies (-0 < +0): see atomic_max_f32
__device__ __forceinline__ void lds_max_f32(float* addr, float v) {
  if (!(__float_as_uint(v) >> 31)) atomicMax((int*)addr, __float_as_int(v));
  else atomicMin((unsigned int*)addr, __float_as_uint(v));
}

// 8 consecutive floats -> the 16-deep bf16 fragment pieces (hi, lo) of a 32x32x16 operand
__device__ __forceinline__ void scr_split8(f32x4 v0, f32x4 v1, frag& h, frag& l) {
  float unused = 0.f;
  unsigned hh[4], ll[4];
  split2<false>(v0[0], v0[1], hh[0], ll[0], unused); split2<false>(v0[2], v0[3], hh[1], ll[1], unused);
  split2<false>(v1[0], v1[1], hh[2], ll[2], unused); split2<false>(v1[2], v1[3], hh[3], ll[3], unused);
  h = frag{hh[0], hh[1], hh[2], hh[3]};
  l = frag{ll[0], ll[1], ll[2], ll[3]};
}

// the hi pieces alone: the first conversion of split2<false>, one v_cvt_pk_bf16_f32 per two elements
__device__ __forceinline__ frag scr_hi8(f32x4 v0, f32x4 v1) {
  const bf16x2 h0 = {(__bf16)v0[0], (__bf16)v0[1]}, h1 = {(__bf16)v0[2], (__bf16)v0[3]};
  const bf16x2 h2 = {(__bf16)v1[0], (__bf16)v1[1]}, h3 = {(__bf16)v1[2], (__bf16)v1[3]};
  return frag{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1), __builtin_bit_cast(unsigned, h2), __builtin_bit_cast(unsigned, h3)};
}

// CS: workgroups that share one (sample, tile slice) and divide the 1024 output channels of the 128 -> 1024 layer between them (each
// repeats the cheap front layers).  CS = 1 is the throughput kernel; CS = 2 / 4 / 8 serve calls of a few poses (predicter.py:67-94 scores
// a few hundred per object, a live caller one at a time): one pose is 32 tiles, i.e. 32 workgroups that each stream the whole 0.5 MB
// weight image through one MFMA chain per wave (38 us per pass) -- split 8 ways it is 256 workgroups with one 32-channel block per wave.
// Per output element the sequence of MFMAs is the one the CS = 1 stream issues (k ascending from a zero accumulator), so a
// candidate's bits do not depend on how many candidates it was scored with.
//
// SCR (CS == 1 only): the 128 -> 1024 layer of a tile is first SCREENED on bf16 MFMAs (three products per 16 channels, the bf16x3
// scheme), every (point, channel) pair whose screen value can still reach the channel's maximum is listed, and only the listed pairs
// are recomputed with the fmaf chain the f32 MFMA stream is defined to equal -- the running maxima, and so every output bit, are those
// of the exact stream.  A tile whose list overflows, whose activations leave the bound's range, or that is the workgroup's first
// (rmax still -inf) runs the exact stream instead; that decision is workgroup-uniform and precedes every rmax update of the tile.
template <int MID, int CS, bool SCR>
__device__ __forceinline__ void pointmlp_max_body(Args a) {
  static_assert(!SCR || CS == 1, "the screen serves the throughput path only");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* h2 = smem;                 // also hosts hA (first TP*S64 floats) while h2 is not live
  float* hA = smem;
  float* hB = smem + TP * S128;
  float* xs = hB + TP * S64;
  float* rmax = xs + TP * XS;
  f32x4* wms = (f32x4*)(rmax + 1024);      // MID != 0: tile-invariant mid-layer weight fragments, staged once per workgroup
  // SCR: the bf16 lo pieces of the h2 tile, [row][128] at hB's own row stride (S64 dwords = 272 B, conflict-free ds_read_b128 for the
  // same lane pattern as the f32 reads of hB).  It fills hB exactly (TP * S64 dwords) and leaves xs alone.  hB is dead while the image
  // lives: its last readers (the 64 -> 128 products) precede the barrier that completes h2, the image is written behind that barrier
  // and last read by the screen, which precedes the next tile's first barrier; hB's next writers (the 6 -> 64 layer for MID == 0, the
  // mid layer otherwise) follow that barrier.  pointfeat is written from registers, not from hB.
  unsigned* hlo = (unsigned*)hB;
  float* hn = smem + LDS_FLOATS;           // SCR: upper bounds of the tile's ||h2 row||
  int* ctl = (int*)(hn + TP);              // SCR: [0] list length, [1] the tile left the bound's range, [2] worst error / bound (stats)
  unsigned short* list = (unsigned short*)(ctl + 4);
  float* zt = (float*)(list + SCR_CAP);    // SCR with stats: the listed pairs' screen values

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = SCR ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;      // SCR: wave-uniform values in scalar registers
  int b, split, nsp;
  const int bid = CS == 1 ? (int)blockIdx.x : (int)blockIdx.x / CS;
  const int cs = CS == 1 ? 0 : (int)blockIdx.x % CS;           // this workgroup's share of the last layer's channels
  if (bid < a.n_main * a.nsplit) {
    nsp = a.nsplit; b = bid / nsp; split = bid - b * nsp;
  } else {
    const int r = bid - a.n_main * a.nsplit;
    nsp = a.tail_split; b = a.n_main + r / nsp; split = r - (r / nsp) * nsp;
  }
  const int ntiles = (a.N + TP - 1) / TP;
  const int t_begin = (int)(((long)ntiles * split) / nsp);
  const int t_end = (int)(((long)ntiles * (split + 1)) / nsp);

  for (int i = tid; i < 1024; i += 256) rmax[i] = -INFINITY;

  // per-thread first-layer weights: channel = tid&63
  float w1r[6], b1r;
  if constexpr (!SCR) {
    const int ch = tid & 63;
#pragma unroll
    for (int j = 0; j < 6; ++j) w1r[j] = a.w1[ch * 6 + j];
    b1r = a.b1[ch];
  }
  float t3r[9];
  if (a.t3) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      t3r[j] = a.t3[b * 9 + j];
      if constexpr (SCR) t3r[j] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(t3r[j])));      // scalar registers
    }
  }
  const float* xb = a.x + (size_t)b * a.N * 6;
  // Tile-invariant operands of the front layers, fetched ONCE per workgroup instead of once per tile with their L2 latency exposed
  // between two barriers: the 64 -> 128 weight fragments of this wave's channel block live in registers, the 64 -> 64 fragments
  // (shared weights, or this sample's feature transform) in LDS.
  // (SCR: the screen needs the registers -- these operands are re-read from L2 at the head of every tile instead, behind an offset
  // the compiler cannot see through, or it would hoist the loads and spill their results)
  f32x4 w2r[8];
  if constexpr (!SCR) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) w2r[ks] = ((const f32x4*)a.w2)[(w * 8 + ks) * 64 + lane];
  }
  if (MID == 1) {
    for (int i = tid; i < 2 * 8 * 64; i += 256) wms[i] = ((const f32x4*)a.wm)[i];
  }
  if (MID == 2) {      // t64 is stored TRANSPOSED (Tt[n][k] = T[k][n]): a lane's 4 consecutive k are one 16-byte load
    for (int i = tid; i < 2 * 8 * 64; i += 256) {
      const int ln = i & 63, ks = (i >> 6) & 7, nb = i >> 9;
      wms[i] = *(const f32x4*)(a.t64 + (size_t)b * 4096 + (nb * 32 + (ln & 31)) * 64 + ks * 8 + (ln >> 5) * 4);
    }
  }
  // the next tile's points travel from HBM during the current tile's 128 -> 1024 stream
  f32x2 xn0 = {0.f, 0.f}, xn1 = xn0, xn2 = xn0;
  auto fetch_points = [&](int tile) {
    if (tid < TP && tile < t_end) {
      int p = tile * TP + tid;
      if (p >= a.N) p = a.N - 1;        // replicate the last point: max-pool is idempotent
      const f32x2* src = (const f32x2*)(xb + (size_t)p * 6);
      xn0 = src[0]; xn1 = src[1]; xn2 = src[2];
    }
  };
  if constexpr (!SCR) fetch_points(t_begin);
  bool w_ok = true;
  if (SCR && tid == 0) ctl[2] = 0;        // with stats: bits of the worst |screen - exact| / bound this workgroup has seen
  if constexpr (SCR) w_ok = a.force != 1 && __float_as_uint(a.wn[1024]) <= __float_as_uint(SCR_RANGE);      // bit compare: NaN / inf / negative fail

  for (int tile = t_begin; tile < t_end; ++tile) {
    // SCR: every lane-dependent index and LDS address of the tile body is re-derived from an opaque copy of the thread id; hoisted out of
    // the tile loop (the exact kernels have the registers for that) they would be spilled to scratch beside the screen
    const int tid_outer = tid, lane_outer = lane;
    int opaque0 = 0;
    if constexpr (SCR) asm volatile("" : "+v"(opaque0));
    const int tid = tid_outer + opaque0, lane = lane_outer + opaque0, l31 = lane & 31, lhi = lane >> 5;
    __syncthreads();   // previous tile's L3 reads of h2 / our rmax init are complete
    if (SCR && tid == 0) { ctl[0] = opaque0; ctl[1] = opaque0; }      // (zero)
    if constexpr (SCR) {
      int opaque = 0;
      asm volatile("" : "+v"(opaque));
      const int ch = (tid & 63) + opaque;
#pragma unroll
      for (int j = 0; j < 6; ++j) w1r[j] = a.w1[ch * 6 + j];
      b1r = a.b1[ch];
      if (MID == 0) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w2r[ks] = ((const f32x4*)a.w2)[(w * 8 + ks) * 64 + lane + opaque];
      }
    }
    // ---- stage input points (apply the 3x3 input transform to xyz, leave normals) ----
    if constexpr (SCR) fetch_points(tile);     // no registers to carry them across the screen: read here, the partner workgroup covers the latency
    if (tid < TP) {
      const f32x2 v0 = xn0, v1 = xn1, v2 = xn2;
      float px = v0[0], py = v0[1], pz = v1[0];
      if (a.t3) {
        float qx = px * t3r[0] + py * t3r[3] + pz * t3r[6];
        float qy = px * t3r[1] + py * t3r[4] + pz * t3r[7];
        float qz = px * t3r[2] + py * t3r[5] + pz * t3r[8];
        px = qx; py = qy; pz = qz;
      }
      f32x4 o0 = {px, py, pz, v1[1]};
      f32x4 o1 = {v2[0], v2[1], 0.f, 0.f};
      *(f32x4*)(xs + tid * XS) = o0;
      *(f32x4*)(xs + tid * XS + 4) = o1;
    }
    if constexpr (!SCR) fetch_points(tile + 1);
    __syncthreads();
    // ---- L0: 6 -> 64 on VALU.  thread = (channel, 16-point group) ----
    {
      float* dst = (MID == 0) ? hB : hA;
      const int ch = tid & 63;
#pragma unroll 4
      for (int i = 0; i < 16; ++i) {
        const int p = w * 16 + i;
        f32x4 q0 = *(const f32x4*)(xs + p * XS);
        f32x2 q1 = *(const f32x2*)(xs + p * XS + 4);
        float v = b1r;
        v = fmaf(w1r[0], q0[0], v); v = fmaf(w1r[1], q0[1], v); v = fmaf(w1r[2], q0[2], v);
        v = fmaf(w1r[3], q0[3], v); v = fmaf(w1r[4], q1[0], v); v = fmaf(w1r[5], q1[1], v);
        dst[p * S64 + ch] = fmaxf(v, 0.f);
      }
    }
    __syncthreads();
    // ---- mid: 64 -> 64 (shared conv+BN+ReLU, or per-sample feature transform) ----
    if (MID != 0) {
      const int rt = w >> 1, nb = w & 1;
      f32x16 c = {0};
      const float* arow = hA + (rt * 32 + l31) * S64 + lhi * 4;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        f32x4 av = *(const f32x4*)(arow + ks * 8);
        const f32x4 bv = wms[(nb * 8 + ks) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) c = mfma32(av[j], bv[j], c);
      }
      if constexpr (SCR) {               // requested behind the mid layer's products, used behind its epilogue and a barrier
        int opaque = 0;
        asm volatile("" : "+v"(opaque));
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) w2r[ks] = ((const f32x4*)a.w2)[(w * 8 + ks) * 64 + lane + opaque];
      }
      const int col = nb * 32 + l31;
      const float bias = (MID == 1) ? a.bm[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rt * 32 + acc_row(r, lane);
        float v = c[r] + bias;
        if (MID == 1) v = fmaxf(v, 0.f);
        hB[row * S64 + col] = v;
        if (MID == 2 && a.pointfeat && cs == 0) {
          const int p = tile * TP + row;
          if (p < a.N) a.pointfeat[((size_t)b * a.N + p) * 64 + col] = v;
        }
      }
      __syncthreads();
    }
    // ---- L2: 64 -> 128.  wave w owns channel block w for both row tiles ----
    {
      f32x16 c0 = {0}, c1 = {0};
      const float* ar0 = hB + l31 * S64 + lhi * 4;
      const float* ar1 = ar0 + 32 * S64;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const f32x4 bv = w2r[ks];
        f32x4 a0 = *(const f32x4*)(ar0 + ks * 8);
        f32x4 a1 = *(const f32x4*)(ar1 + ks * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { c0 = mfma32(a0[j], bv[j], c0); c1 = mfma32(a1[j], bv[j], c1); }
      }
      // hA (aliasing h2) may still be read by other waves' mid layer only before the barrier above,
      // and hB reads of this layer do not alias h2 -> safe to write h2 now when MID!=0; for MID==0
      // nothing else lives in the h2 region.
      const int col = w * 32 + l31;
      const float bias = a.b2[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lane);
        h2[row * S128 + col] = fmaxf(c0[r] + bias, 0.f);
        h2[(row + 32) * S128 + col] = fmaxf(c1[r] + bias, 0.f);
      }
    }
    __syncthreads();
    // ---- L3: 128 -> 1024 + running max over points.  wave w owns channel blocks [8w, 8w+8), two at a time x both row tiles.
    // The 1024-MFMA stream of the tile is hand-scheduled assembly (gen_l3_f32_asm.py -> l3_f32_asm.inc): operands prefetched one
    // whole k-step ahead into a double buffer in accumulation registers; it returns the per-lane maxima of the 8 blocks.
    bool exact = true;
    if constexpr (SCR) {
      // upper bound of every row's norm; thread = (row, quarter of the 128 channels).  The same pass splits the tile ONCE: the bf16 lo
      // pieces of its 32 elements go to the hlo image (the screen forms the hi pieces from the f32 fragments it reads anyway).
      {
        const int row = tid >> 2, part = tid & 3;
        const float* hr = h2 + row * S128 + part * 32;
        frag* lr = (frag*)(hlo + row * S64 + part * 16);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 v = *(const f32x4*)(hr + i * 8), u = *(const f32x4*)(hr + i * 8 + 4);
          s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
          s = fmaf(u[0], u[0], s); s = fmaf(u[1], u[1], s); s = fmaf(u[2], u[2], s); s = fmaf(u[3], u[3], s);
          frag hi_unused, lo;
          scr_split8(v, u, hi_unused, lo);
          lr[i] = lo;
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        const float n = fmaf(sqrtf(s), SCR_HN_UP, SCR_HN_ABS);
        if (part == 0) {
          hn[row] = n;
          if ((__float_as_uint(n) & 0x7fffffffu) > __float_as_uint(SCR_RANGE)) atomicOr(&ctl[1], 1);      // also inf and NaN
        }
      }
      __syncthreads();
      // tile-invariant addresses and operands of the screen are re-derived per tile behind an offset the compiler cannot see through:
      // hoisted out of the tile loop they would be spilled
      int opq = 0;
      asm volatile("" : "+s"(opq));
      const unsigned short* w3s_t = a.w3s + opq;
      const float* wn_t = a.wn + opq;
      const float* w3_t = a.w3 + opq;
      const bool first = tile == t_begin && a.force != 2;
      const bool in_range = w_ok && ctl[1] == 0;
      exact = first || !in_range;
      if (!exact) {
        // ---- screen + select as a rolling pipeline over the wave's eight channel blocks: one block's products in flight (2 accumulators)
        // beside the previous, finished block (2 accumulators), ping-ponged; the finished block's select is cut into eight slices, one
        // behind each 16-channel step of the block in flight, so that its vector work runs between this wave's own MFMAs ----
        const float* ap = h2 + l31 * S128 + lhi * 8;
        const frag* lp = (const frag*)(hlo + l31 * S64 + lhi * 4);
        const float* hq = hn + lhi * 4;
        // The wave's 64 steps (8 blocks x 8 sixteen-channel steps) are one linear weight stream: the pair of step s = 8 blk + kc lies at
        // (2 s + h) * 64 fragments from bp.  Four rotating register pairs hold the steps s .. s + 3; a step's pair is requested for step
        // s + 4 as soon as its six products are issued (24 MFMAs ahead).  No request leaves the wave's 64 steps: the last block is peeled.
        const frag* bp = (const frag*)w3s_t + (size_t)(w * 8) * (8 * 2 * 64) + lane;       // [nb][kc][hi | lo][lane]
        frag bq[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) { bq[s][0] = bp[(2 * s) * 64]; bq[s][1] = bp[(2 * s + 1) * 64]; }
        // A operands, both row tiles.  They are the same for every block, so the hi fragments of all eight steps (the bf16 conversion of
        // the f32 image) are formed once per tile and stay in registers (64): read and converted per block they cost 384 instead of
        // 144 ds_read_b128 per wave and tile, and the step more than the rolling select gained.  The lo fragments of the hlo image are
        // requested behind a step's fourth product for the next step.
        frag ahr[8][2], fl[2];
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          const f32x4 f0 = *(const f32x4*)(ap + kc * 16), f1 = *(const f32x4*)(ap + kc * 16 + 4);
          const f32x4 f2 = *(const f32x4*)(ap + 32 * S128 + kc * 16), f3 = *(const f32x4*)(ap + 32 * S128 + kc * 16 + 4);
          ahr[kc][0] = scr_hi8(f0, f1); ahr[kc][1] = scr_hi8(f2, f3);
        }
        fl[0] = lp[0]; fl[1] = lp[32 * (S64 / 4)];
        // ---- select: lane = channel, registers = 32 points.  T = max(exact running max, the tile's own lower bound) ----
        // E = kw * hn + SCR_FLOOR.  Pass 1: lb = max(c - kw * hn) - SCR_FLOOR; pass 2: list c + kw * hn >= T - SCR_FLOOR.  Two elements
        // per packed fma; the compare's bit is shifted into the lane's mask through the carry (m = 2 m + bit), top register first.
        // Eight slices: the four quarters of pass 1 (T behind the fourth), then the four quarters of pass 2 from the top.  A slice is cut
        // again into four parts of one packed fma each: (row tile 0 | 1) x (register pair), in the order the masks fill.
        float wnn = 0.f, kw = 0.f, lb = -INFINITY, T = 0.f;     // wnn: the row-norm bound of the block in flight, requested a phase ahead
        unsigned m0 = 0, m1 = 0;
        f32x4 nn0 = *(const f32x4*)hq, nn1 = *(const f32x4*)(hq + 32);      // the next slice's hn, requested a step ahead
        auto part = [&](const f32x16* fin, int sl, int pt, f32x4 n0, f32x4 n1) __attribute__((always_inline)) {
          const int rt = pt >> 1;
          const f32x4 n = rt ? n1 : n0;
          if (sl < 4) {
            const int q = sl, j = (pt & 1) * 2;
            const f32x2 nkw = {-kw, -kw};
            const f32x2 t = __builtin_elementwise_fma(nkw, f32x2{n[j], n[j + 1]}, f32x2{fin[rt][q * 4 + j], fin[rt][q * 4 + j + 1]});
            lb = fmaxf(fmaxf(sl == 0 && pt == 0 ? -INFINITY : lb, t[0]), t[1]);
          } else {
            const int q = 7 - sl, j = 2 - (pt & 1) * 2;
            const f32x2 pkw = {kw, kw};
            const f32x2 u = __builtin_elementwise_fma(pkw, f32x2{n[j], n[j + 1]}, f32x2{fin[rt][q * 4 + j], fin[rt][q * 4 + j + 1]});
            if (rt == 0)
              asm("v_cmp_ge_f32 vcc, %1, %3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                  "v_cmp_ge_f32 vcc, %2, %3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(m0) : "v"(u[1]), "v"(u[0]), "v"(T) : "vcc");
            else
              asm("v_cmp_ge_f32 vcc, %1, %3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                  "v_cmp_ge_f32 vcc, %2, %3\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(m1) : "v"(u[1]), "v"(u[0]), "v"(T) : "vcc");
          }
        };
        // One 16-channel step of the block in flight (prod) with one slice of the finished block's select (sel), in issue order: every
        // product is followed by its share of the requests and of the slice, and the order is pinned product by product -- left to
        // itself the scheduler issues the six products first and the slice behind them, which is the serial form again.
        // Per accumulator element the three products of a step stay in the order hi-lo, lo-hi, hi-hi, kc ascending from zero.
        auto step = [&](f32x16* c, const f32x16* fin, const frag* bpb, int kc, int ch, bool prod, bool sel, bool last) __attribute__((always_inline)) {
          const frag ah0 = ahr[kc][0], ah1 = ahr[kc][1], al0 = fl[0], al1 = fl[1];
          const frag bh = bq[kc & 3][0], bl = bq[kc & 3][1];
          const bool next = prod && (!last || kc < 7);
          const int kn = (kc + 1) & 7;
          f32x4 n0 = {0}, n1 = {0};
          float rm = 0.f;
          if (prod) c[0] = mfma_x<false>(ah0, bl, c[0]);
          if (sel) {
            const int sn = (kc + 1) & 7, qn = sn < 4 ? sn : 7 - sn;      // quarter of the next slice (it wraps to the next block's first)
            n0 = nn0; n1 = nn1;
            nn0 = *(const f32x4*)(hq + qn * 8); nn1 = *(const f32x4*)(hq + 32 + qn * 8);
            if (kc == 3) rm = rmax[ch];
          }
          __builtin_amdgcn_sched_barrier(0);
          if (prod) c[1] = mfma_x<false>(ah1, bl, c[1]);
          __builtin_amdgcn_sched_barrier(0);
          if (prod) c[0] = mfma_x<false>(al0, bh, c[0]);
          if (sel) part(fin, kc, 0, n0, n1);
          __builtin_amdgcn_sched_barrier(0);
          if (prod) c[1] = mfma_x<false>(al1, bh, c[1]);
          if (sel) part(fin, kc, 1, n0, n1);
          if (next) { fl[0] = lp[kn * 2]; fl[1] = lp[32 * (S64 / 4) + kn * 2]; }
          __builtin_amdgcn_sched_barrier(0);
          if (prod) c[0] = mfma_x<false>(ah0, bh, c[0]);
          if (sel) part(fin, kc, 2, n0, n1);
          __builtin_amdgcn_sched_barrier(0);
          if (prod) c[1] = mfma_x<false>(ah1, bh, c[1]);
          if (prod && (!last || kc < 4)) {
            bq[kc & 3][0] = bpb[(2 * (kc + 4)) * 64];
            bq[kc & 3][1] = bpb[(2 * (kc + 4) + 1) * 64];
          }
          if (sel) part(fin, kc, 3, n0, n1);
          if (sel && kc == 3) {
            lb = fmaxf(lb - SCR_FLOOR, rm);
            T = fmaxf(lb, __shfl_xor(lb, 32)) - SCR_FLOOR;
            m0 = 0; m1 = 0;
          }
          __builtin_amdgcn_sched_barrier(0);
        };
        // the finished block's pairs join the tile's list (plain code behind the block's last slice: its accumulators are intact)
        auto append = [&](const f32x16* fin, int ch) __attribute__((always_inline)) {
          const int cnt = __popc(m0) + __popc(m1);
          if (cnt) {
            const int at0 = atomicAdd(&ctl[0], cnt);
            int at = at0;
            unsigned m = m0;
#pragma unroll 1
            for (int rt = 0; rt < 2; ++rt, m = m1) {
              while (m) {
                const int r = __ffs(m) - 1;
                m &= m - 1;
                if (at < SCR_CAP) list[at] = (unsigned short)(((rt * 32 + acc_row(r, lane)) << 10) | ch);
                ++at;
              }
            }
            if (a.stats) {               // the same slots, by static register index
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int i0 = at0 + __popc(m0 & ((1u << r) - 1)), i1 = at0 + __popc(m0) + __popc(m1 & ((1u << r) - 1));
                if (((m0 >> r) & 1) && i0 < SCR_CAP) zt[i0] = fin[0][r];
                if (((m1 >> r) & 1) && i1 < SCR_CAP) zt[i1] = fin[1][r];
              }
            }
          }
        };
        // one phase: the eight steps of block `pblk` into `cur` (prod), each followed by one slice of block `sblk`'s select on `fin` (sel)
        auto phase = [&](f32x16* cur, f32x16* fin, int pblk, int sblk, bool prod, bool sel, bool last) __attribute__((always_inline)) {
          const frag* bpb = bp + pblk * (16 * 64);
          const int ch = (w * 8 + sblk) * 32 + l31;
          if (sel) kw = SCR_KAPPA * wnn;
          if (prod) {
            wnn = wn_t[(w * 8 + pblk) * 32 + l31];
            cur[0] = f32x16{0}; cur[1] = f32x16{0};
          }
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            step(cur, fin, bpb, kc, ch, prod, sel, last);
          }
          if (sel) append(fin, ch);
        };
        f32x16 ca[2], cb[2];
        phase(ca, cb, 0, 0, true, false, false);               // fill
#pragma unroll 1
        for (int i = 0; i < 3; ++i) {
          phase(cb, ca, 2 * i + 1, 2 * i, true, true, false);
          phase(ca, cb, 2 * i + 2, 2 * i + 1, true, true, false);
        }
        phase(cb, ca, 7, 6, true, true, true);
        phase(ca, cb, 7, 7, false, true, true);                // drain
        __syncthreads();
        const int n = ctl[0];
        if (n > SCR_CAP) {
          exact = true;                    // nothing of this tile has touched rmax yet
          if (a.stats && tid == 0) atomicAdd((unsigned long long*)a.stats + ST_OVERFLOW, 1ull);
        } else {
          // ---- verify: one listed pair per thread, the operation sequence of the f32 MFMA stream (k-step order, zero accumulator) ----
          for (int i = tid; i < n; i += 256) {
            const int e = list[i], row = e >> 10, ch = e & 1023;
            const float* hr = h2 + row * S128;
            const f32x4* wp = (const f32x4*)w3_t + (size_t)(ch >> 5) * (16 * 64) + (ch & 31);
            float z = 0.f;
#pragma unroll 4
            for (int ks = 0; ks < 16; ++ks) {
              const f32x4 w0 = wp[ks * 64], w1 = wp[ks * 64 + 32];
              const f32x4 h0 = *(const f32x4*)(hr + ks * 8), h1 = *(const f32x4*)(hr + ks * 8 + 4);
#pragma unroll
              for (int j = 0; j < 4; ++j) { z = fmaf(h0[j], w0[j], z); z = fmaf(h1[j], w1[j], z); }
            }
            lds_max_f32(rmax + ch, z);
            if (a.stats) atomicMax((unsigned*)&ctl[2], __float_as_uint(fabsf(zt[i] - z) / fmaf(SCR_KAPPA * wn_t[ch], hn[row], SCR_FLOOR)));
          }
          if (a.stats && tid == 0) {
            atomicAdd((unsigned long long*)a.stats + ST_SCREENED, 1ull);
            atomicAdd((unsigned long long*)a.stats + ST_PAIRS, (unsigned long long)n);
          }
        }
      } else if (a.stats && tid == 0) {
        atomicAdd((unsigned long long*)a.stats + (a.force == 1 ? ST_FORCED : first ? ST_FIRST : ST_RANGE), 1ull);
      }
    }
    if constexpr (CS > 1) {
      constexpr int NBW = 8 / CS;                          // 32-channel blocks per wave
      const float* ar0 = h2 + l31 * S128 + lhi * 4;
      const float* ar1 = ar0 + 32 * S128;
#pragma unroll
      for (int p = 0; p < NBW; ++p) {
        const int nb = cs * (32 / CS) + w * NBW + p;
        f32x4 bv[16];                                      // the block's 16 weight fragments: all requested before the first product
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) bv[ks] = ((const f32x4*)a.w3)[(size_t)(nb * 16 + ks) * 64 + lane];
        f32x16 c0 = {0}, c1 = {0};
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const f32x4 a0 = *(const f32x4*)(ar0 + ks * 8);
          const f32x4 a1 = *(const f32x4*)(ar1 + ks * 8);
#pragma unroll
          for (int j = 0; j < 4; ++j) { c0 = mfma32(a0[j], bv[ks][j], c0); c1 = mfma32(a1[j], bv[ks][j], c1); }
        }
        float m = fmaxf(max16(c0), max16(c1));
        m = fmaxf(m, __shfl_xor(m, 32));
        if (lane < 32) rmax[nb * 32 + lane] = fmaxf(rmax[nb * 32 + lane], m);
      }
    } else if (exact) {
      const unsigned ar = (unsigned)(uintptr_t)(h2 + l31 * S128 + lhi * 4);      // generic -> LDS byte address = low 32 bits
      const unsigned voff = (unsigned)((w * 8 * 16) * 64 + lane) * 16u;          // this wave's first weight fragment
      float m00, m01, m10, m11, m20, m21, m30, m31, t0, t1;
      unsigned vo0, vo1;
      asm volatile(CG_L3_F32_ASM
                   : [m00] "=&v"(m00), [m01] "=&v"(m01), [m10] "=&v"(m10), [m11] "=&v"(m11), [m20] "=&v"(m20), [m21] "=&v"(m21),
                     [m30] "=&v"(m30), [m31] "=&v"(m31), [t0] "=&v"(t0), [t1] "=&v"(t1), [vo0] "=&v"(vo0), [vo1] "=&v"(vo1)
                   : [voff] "v"(voff), [ar] "v"(ar), [wb] "s"(a.w3)
                   : "memory", CG_L3_F32_CLOBBERS);
      const float mm[4][2] = {{m00, m01}, {m10, m11}, {m20, m21}, {m30, m31}};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float m0 = mm[p][0], m1 = mm[p][1];
        m0 = fmaxf(m0, __shfl_xor(m0, 32));
        m1 = fmaxf(m1, __shfl_xor(m1, 32));
        if (lane < 32) {
          const int ch0 = (w * 8 + p * 2) * 32 + lane;
          rmax[ch0] = fmaxf(rmax[ch0], m0);
          rmax[ch0 + 32] = fmaxf(rmax[ch0 + 32], m1);
        }
      }
    }
  }
  __syncthreads();
  if (SCR && a.stats && tid == 0) atomicMax((unsigned long long*)a.stats + ST_RATIO, (unsigned long long)(unsigned)ctl[2]);      // non-negative floats order as their bits
  if (t_end > t_begin) {
    int tid_e = tid;
    if constexpr (SCR) asm volatile("" : "+v"(tid_e));      // (the address of rmax[tid] from the prologue would be carried through the tile loop)
    for (int ch = tid_e; ch < 1024; ch += 256) {
      if (CS > 1 && ch / (1024 / CS) != cs) continue;
      float v = rmax[ch] + a.b3[ch];
      if (a.relu3) v = fmaxf(v, 0.f);
      if (nsp == 1) a.out[(size_t)b * 1024 + ch] = v;
      else atomic_max_f32(a.out + (size_t)b * 1024 + ch, v);
    }
  }
}

template <int MID, int CS, bool SCR = false>
__global__ __launch_bounds__(256) void pointmlp_max_kernel(Args a) { pointmlp_max_body<MID, CS, SCR>(a); }
// The screened kernels are held to two waves per SIMD (two workgroups per CU, as the exact kernels reach by themselves).
#define CG_SCREENED_KERNEL(MID)                                                                                          \
  template <> __global__ __launch_bounds__(256, 2) void pointmlp_max_kernel<MID, 1, true>(Args a) {                     \
    pointmlp_max_body<MID, 1, true>(a);                                                                                  \
  }
CG_SCREENED_KERNEL(0)
CG_SCREENED_KERNEL(1)
CG_SCREENED_KERNEL(2)
#undef CG_SCREENED_KERNEL

__global__ void fill_kernel(float* p, size_t n, float v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

// the launch plan of this file's and pointmlp_split.hip's entry points: see cg_common.hpp
CgPointMlpPlan cg_pointmlp_plan(int B, int ntiles, int nsplit, int slots_per_cu, int min_tiles, int tail_split, float* out, hipStream_t s) {
  CgPointMlpPlan p{CG_ERR_UNSUPPORTED, 0, nsplit < 1 ? 1 : nsplit > ntiles ? ntiles : nsplit, B, 1};
  if (hipGetDevice(&p.dev) != hipSuccess) return p;
  if (p.nsplit == 1 && ntiles >= min_tiles) {
    const int slots = slots_per_cu * cg_device_cu_count(p.dev);
    if (slots <= 0) return p;
    if (B >= slots && (B % slots) != 0) { p.n_main = B - B % slots; p.tail_split = tail_split; }
  }
  if (p.nsplit > 1 || p.tail_split > 1) {
    const int first = (p.nsplit > 1) ? 0 : p.n_main;
    const size_t n = (size_t)(B - first) * 1024;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out + (size_t)first * 1024, n, -INFINITY);
  }
  p.status = CG_OK;
  return p;
}

namespace {

// cg_pointmlp_max (w3s == nullptr) and cg_pointmlp_max_screened: one launcher.  The screen serves the throughput kernel (CS == 1);
// calls of a few poses take the channel-split exact kernels either way.
int pointmlp_launch(const float* x, int B, int N, const float* t3, const float* w1, const float* b1, int mid_mode, const float* wm_packed,
                    const float* bm, const float* t64, const float* w2_packed, const float* b2, const float* w3_packed, const float* b3,
                    int relu3, int nsplit, float* out, float* pointfeat, const unsigned short* w3s, const float* wn, long long* stats,
                    int force, void* stream) {
  if (!x || !w1 || !b1 || !w2_packed || !b2 || !w3_packed || !b3 || !out) return CG_ERR_ARG;
  if (B < 0 || N <= 0 || mid_mode < 0 || mid_mode > 2) return CG_ERR_ARG;
  if (mid_mode == 1 && (!wm_packed || !bm)) return CG_ERR_ARG;
  if (mid_mode == 2 && !t64) return CG_ERR_ARG;
  if (pointfeat && mid_mode != 2) return CG_ERR_ARG;
  if (B == 0) return CG_OK;
  hipStream_t s = (hipStream_t)stream;
  // two resident workgroups per CU (73,728 B of LDS each; 80,144 B screened); the tail is balanced from 8 tiles on, split 8 ways
  const CgPointMlpPlan plan = cg_pointmlp_plan(B, (N + TP - 1) / TP, nsplit, 2, 8, 8, out, s);
  if (plan.status != CG_OK) return plan.status;
  nsplit = plan.nsplit;
  const int n_main = plan.n_main, tail_split = plan.tail_split;
  Args a{x, B, N, t3, w1, b1, wm_packed, bm, t64, w2_packed, b2, w3_packed, b3, relu3, nsplit, n_main, tail_split, out, pointfeat,
         w3s, wn, stats, force};
  // few workgroups (a call of a few poses): divide the last layer's channels over 2 / 4 / 8 workgroups per (sample, slice)
  const long wgs = (long)n_main * nsplit + (long)(B - n_main) * tail_split;
  int csi = tail_split > 1 ? 0 : wgs <= 64 ? 3 : wgs <= 128 ? 2 : wgs <= 256 ? 1 : 0;
  static const char* cs_env = getenv("CATGRASP_AMD_POINTMLP_CSPLIT");     // dev knob: 1 / 2 / 4 / 8
  if (cs_env) { const int v = atoi(cs_env); csi = tail_split > 1 ? 0 : v == 8 ? 3 : v == 4 ? 2 : v == 2 ? 1 : 0; }
  if (w3s && csi == 0) csi = 4;           // the screened throughput kernel
  static bool lds_allowed[3][5][CG_MAX_DEVICES] = {};
  typedef void (*kern_t)(Args);
  static const kern_t kerns[3][5] = {
      {pointmlp_max_kernel<0, 1>, pointmlp_max_kernel<0, 2>, pointmlp_max_kernel<0, 4>, pointmlp_max_kernel<0, 8>, pointmlp_max_kernel<0, 1, true>},
      {pointmlp_max_kernel<1, 1>, pointmlp_max_kernel<1, 2>, pointmlp_max_kernel<1, 4>, pointmlp_max_kernel<1, 8>, pointmlp_max_kernel<1, 1, true>},
      {pointmlp_max_kernel<2, 1>, pointmlp_max_kernel<2, 2>, pointmlp_max_kernel<2, 4>, pointmlp_max_kernel<2, 8>, pointmlp_max_kernel<2, 1, true>}};
  const kern_t kern = kerns[mid_mode][csi];
  // 73,728 B and up: above the 64 KB default limit -> per-device function attribute (the screened kernel's larger size with counters
  // has a flag row of its own: the attribute is set to the largest size a row has asked for)
  const bool scr = csi == 4;
  const size_t lds = !scr ? LDS_FLOATS * sizeof(float) : stats ? SCR_LDS_BYTES_STATS : SCR_LDS_BYTES;
  const int st = cg_allow_dynamic_lds((const void*)kern, plan.dev, scr ? (size_t)SCR_LDS_BYTES_STATS : lds, lds_allowed[mid_mode][csi]);
  if (st != CG_OK) return st;
  dim3 grid((unsigned)(wgs << (scr ? 0 : csi))), block(256);
  hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  return cg_hip_status(hipGetLastError());
}

}  // namespace

extern "C" int cg_pointmlp_max(const float* x, int B, int N, const float* t3, const float* w1, const float* b1,
                               int mid_mode, const float* wm_packed, const float* bm, const float* t64,
                               const float* w2_packed, const float* b2, const float* w3_packed, const float* b3,
                               int relu3, int nsplit, float* out, float* pointfeat, void* stream) {
  return pointmlp_launch(x, B, N, t3, w1, b1, mid_mode, wm_packed, bm, t64, w2_packed, b2, w3_packed, b3, relu3, nsplit, out, pointfeat,
                         nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int cg_pointmlp_max_screened(const float* x, int B, int N, const float* t3, const float* w1, const float* b1,
                                        int mid_mode, const float* wm_packed, const float* bm, const float* t64,
                                        const float* w2_packed, const float* b2, const float* w3_packed, const float* b3,
                                        int relu3, int nsplit, float* out, float* pointfeat, const unsigned short* w3_split,
                                        const float* w3_norm, long long* stats, int force, void* stream) {
  if (!w3_split || !w3_norm || force < 0 || force > 2) return CG_ERR_ARG;
  if (((uintptr_t)w3_split & 15) != 0) return CG_ERR_ARG;
  return pointmlp_launch(x, B, N, t3, w1, b1, mid_mode, wm_packed, bm, t64, w2_packed, b2, w3_packed, b3, relu3, nsplit, out, pointfeat,
                         w3_split, w3_norm, stats, force, stream);
}
