// get_ik_within_limits (my_cpp/common.cpp:9-72) on the device, one thread per end-effector pose: the closed-form iiwa14 IK of
// iiwa_ik.hpp over a stored (E,16) ee_in_base array, and fused into the pose composition of the multi-segment filter.
#include "cg_common.hpp"
#include "filter_compose.hpp"
#include "../../include/catgrasp_amd.h"

namespace {

__global__ __launch_bounds__(256) void iiwa_ik_kernel(const float* __restrict__ ee, long E, cg_ik::IkLimits lim, unsigned char* __restrict__ ok) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = ee[e * 16 + k];
  ok[e] = cg_ik::iiwa_ik_within_limits(T, lim) ? 1 : 0;
}

// The IK stage over a filter's segment table (filter_ik=True, common.cpp:214-226) without an (E,16) ee_in_base array in memory:
// ee = cam_in_world . grasp_in_cam . ee_in_grasp is formed in registers with the mat4_mul order of the single-call ee_out pass
// (collision.hip; -ffp-contract=off, so it is the float32 matrix that pass stores) and, where the approach test passed, goes through
// the IK -> code 2 when no solution lies inside the limits.  The grid and exhaustive kernels then skip every code != 0.
// EE_OUT (cg_filter_segments_ee_in_base, the pre-pass of a HOST solver): writes ee for every evaluation and codes {0, 1} instead.
// (Here and not in collision.hip: like iiwa_ik_kernel it spills scalar registers to VGPR lanes -- the float64 trig keeps its constants
// in SGPR pairs -- which the collision kernels are built never to do.  No scratch either way.)
template <bool EE_OUT>
__global__ __launch_bounds__(256) void compose_grasp_pose_multi_ik_kernel(cg_filter::ComposeMultiArgs a, cg_filter::MultiIkArgs k) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  float gic[16], t2[16], ee[16];
  int code = cg_filter::compose_multi(a, e, gic);
  if (EE_OUT || code == 0) {
    cg_filter::mat4_mul(k.cam_in_world.m, gic, t2);
    cg_filter::mat4_mul(t2, k.ee_in_grasp.m, ee);
  }
  if constexpr (EE_OUT) {
#pragma unroll
    for (int q = 0; q < 16; q += 4) *(float4*)(k.ee_out + e * 16 + q) = *(float4*)(ee + q);
    a.codes[e] = (signed char)code;
  } else {
    if (code == 0 && !cg_ik::iiwa_ik_within_limits(ee, k.lim)) code = 2;
#pragma unroll
    for (int q = 0; q < 16; q += 4) *(float4*)(a.poses_out + e * 16 + q) = *(float4*)(gic + q);
    a.codes[e] = (signed char)code;
    a.nudge[e] = (signed char)-1;
  }
}

}  // namespace

int cg_filter::launch_compose_multi_ik(const ComposeMultiArgs& a, const MultiIkArgs& k, bool ee_out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.E + 255) / 256));
  if (ee_out) hipLaunchKernelGGL(compose_grasp_pose_multi_ik_kernel<true>, grid, dim3(256), 0, stream, a, k);
  else hipLaunchKernelGGL(compose_grasp_pose_multi_ik_kernel<false>, grid, dim3(256), 0, stream, a, k);
  return cg_hip_status(hipGetLastError());
}

extern "C" int cg_iiwa_ik_within_limits(const float* ee_in_base, long E, const double* h_upper7, const double* h_lower7,
                                        unsigned char* ok, void* stream) {
  if (E < 0 || !h_upper7 || !h_lower7) return CG_ERR_ARG;
  if (E == 0) return CG_OK;
  if (!ee_in_base || !ok) return CG_ERR_ARG;
  cg_ik::IkLimits lim;
  for (int j = 0; j < 7; ++j) { lim.up[j] = h_upper7[j]; lim.lo[j] = h_lower7[j]; }
  hipLaunchKernelGGL(iiwa_ik_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ee_in_base, E, lim, ok);
  return cg_hip_status(hipGetLastError());
}
