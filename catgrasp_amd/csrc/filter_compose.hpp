// Pose composition of the grasp filter (my_cpp/common.cpp:184-216), shared by collision.hip (the filter) and iiwa_ik.hip (the fused
// compose + IK stage of cg_filter_grasp_pose_multi_ik).  Both are built with -ffp-contract=off: every product below is the float32
// expression written, in the order written, in either file.
#pragma once
#include <hip/hip_runtime.h>
#include "iiwa_ik.hpp"
#include "../../include/catgrasp_amd.h"

namespace cg_filter {

struct Mat4 { float m[16]; };

__device__ __forceinline__ void mat4_mul(const float* A, const float* B, float* C) {
  float t[16];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      t[r * 4 + c] = ((A[r * 4 + 0] * B[0 * 4 + c] + A[r * 4 + 1] * B[1 * 4 + c]) + A[r * 4 + 2] * B[2 * 4 + c]) + A[r * 4 + 3] * B[3 * 4 + c];
#pragma unroll
  for (int i = 0; i < 16; ++i) C[i] = t[i];
}

__device__ __forceinline__ void normalize_col(float* M, int col) {
  const float x = M[0 * 4 + col], y = M[1 * 4 + col], z = M[2 * 4 + col];
  const float s = (x * x + y * y) + z * z;
  if (s > 0.0f) { const float n = sqrtf(s); M[0 * 4 + col] = x / n; M[1 * 4 + col] = y / n; M[2 * 4 + col] = z / n; }
}

// The evaluations of SEVERAL filterGraspPose calls at once (cg_filter_grasp_pose_multi): evaluation e belongs to the segment whose
// [first, first + n_pose * n_sym) holds it (binary search in the device table), inside it e - first = i * n_sym + j.
struct ComposeMultiArgs {
  const cg_filter_segment* segs; int n_segs; long E;
  int filter_dir;
  const unsigned char* ik_ok;
  signed char* codes; float* poses_out; signed char* nudge;
};

// grasp_in_cam of evaluation e of the table and its approach-direction code (0 / 1): the first half of compose_grasp_pose_multi_kernel
__device__ __forceinline__ int compose_multi(const ComposeMultiArgs& a, long e, float* gic) {
  int lo = 0, hi = a.n_segs - 1;
  while (lo < hi) {                                        // the last segment whose first <= e
    const int mid = (lo + hi + 1) >> 1;
    if ((long)a.segs[mid].first <= e) lo = mid; else hi = mid - 1;
  }
  const cg_filter_segment& sg = a.segs[lo];
  const long le = e - (long)sg.first;
  const int i = (int)(le / sg.n_sym), j = (int)(le - (long)i * sg.n_sym);
  float P[16], S[16], C[16], tmp[16];
#pragma unroll
  for (int k = 0; k < 16; k += 4) {
    *(float4*)(P + k) = *(const float4*)(sg.grasp_poses + (size_t)i * 16 + k);
    *(float4*)(S + k) = *(const float4*)(sg.symmetry_tfs + (size_t)j * 16 + k);
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) C[k] = sg.c2c[k];
  mat4_mul(S, P, tmp);
  mat4_mul(C, tmp, gic);
  normalize_col(gic, 0); normalize_col(gic, 1); normalize_col(gic, 2);
  return (a.filter_dir && gic[2 * 4 + 0] < 0.0f) ? 1 : 0;
}

// The IK stage over the table (cg_filter_grasp_pose_multi_ik; kernel in iiwa_ik.hip).
struct MultiIkArgs {
  Mat4 cam_in_world, ee_in_grasp;
  cg_ik::IkLimits lim;
  float* ee_out;                              // ee_out mode only
};

// Launches the compose + IK kernel over the E evaluations of a.  ee_out = false: codes {0, 1, 2}, poses_out, nudge = -1 (what
// compose_grasp_pose_multi_kernel writes with an ik_ok); true (cg_filter_segments_ee_in_base): k.ee_out and codes {0, 1}.
int launch_compose_multi_ik(const ComposeMultiArgs& a, const MultiIkArgs& k, bool ee_out, hipStream_t stream);

}  // namespace cg_filter
