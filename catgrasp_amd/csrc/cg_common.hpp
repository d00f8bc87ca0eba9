// Shared device helpers for the catgrasp_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define CG_OK 0
#define CG_ERR_ARG (-1)
#define CG_ERR_UNSUPPORTED (-2)

// v_mfma_f32_32x32x2_f32: exact-f32 matrix FMA (A: lane l -> A[i=l&31][k=l>>5], B: lane l -> B[k=l>>5][j=l&31],
// D: col j = l&31, row i = (reg&3) + 8*(reg>>2) + 4*(l>>5)).
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// row of accumulator register r for lane l in a 32x32 MFMA tile
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// max over the 16 accumulator registers of a lane.  Written as max(max(m, a), b) chains so that every pair folds into one
// v_max3_f32 (8 VALU ops per tile); the pointmlp files are compiled with -fno-honor-nans, which removes the per-operand
// canonicalisation (v_max x, x) the IEEE maxnum lowering would otherwise insert for MFMA results.
__device__ __forceinline__ float max16(const f32x16& c) {
  float m = fmaxf(fmaxf(c[0], c[1]), c[2]);
#pragma unroll
  for (int i = 3; i < 15; i += 2) m = fmaxf(fmaxf(m, c[i]), c[i + 1]);
  return fmaxf(m, c[15]);
}

// float atomic max valid for any sign (buffer pre-filled with -inf)
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  // by sign BIT: -0.0f must take the unsigned-min branch (its int pattern is INT_MIN and would lose every signed max)
  if (!(__float_as_uint(v) >> 31)) atomicMax((int*)addr, __float_as_int(v));
  else atomicMin((unsigned int*)addr, __float_as_uint(v));
}

static inline int cg_hip_status(hipError_t e) { return e == hipSuccess ? CG_OK : (int)e; }

// per-device launch state (function attributes, CU counts) is indexed by the HIP device ordinal
constexpr int CG_MAX_DEVICES = 64;
static inline int cg_device_cu_count(int dev) {
  static int n_cu[CG_MAX_DEVICES] = {};
  if (dev < 0 || dev >= CG_MAX_DEVICES) return -1;
  if (n_cu[dev] == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    n_cu[dev] = prop.multiProcessorCount;
  }
  return n_cu[dev];
}

// Allow `kernel` `bytes` of dynamic LDS on device `dev` (anything above the 64 KB default needs it).  The attribute is per device, so
// it is set once per (kernel, device): done[CG_MAX_DEVICES] is the caller's flag row for that kernel.
static inline int cg_allow_dynamic_lds(const void* kernel, int dev, size_t bytes, bool* done) {
  if (dev < 0 || dev >= CG_MAX_DEVICES) return CG_ERR_UNSUPPORTED;
  if (!done[dev]) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    done[dev] = true;
  }
  return CG_OK;
}
// the kernel known at compile time: its flag row lives here
template <auto Kernel>
int cg_allow_dynamic_lds(int dev, size_t bytes) {
  static bool done[CG_MAX_DEVICES] = {};
  return cg_allow_dynamic_lds((const void*)Kernel, dev, bytes, done);
}

// Launch plan of the fused per-point MLP + max-pool entry points (pointmlp.hip, which defines it, and pointmlp_split.hip), for B samples
// of ntiles point tiles each and the caller's nsplit workgroups per sample:
//  * nsplit is clamped to [1, ntiles];
//  * tail balancing: with one workgroup per sample (nsplit == 1) and B >= the resident workgroups (slots_per_cu per CU), the B % slots
//    samples of the last, partially filled scheduling round would occupy a few CUs for a whole sample's duration while the rest of the
//    chip idles; from min_tiles tiles on they are split tail_split ways instead (n_main = the samples before them), so that round is short;
//  * rows written by more than one workgroup (atomic max) are pre-filled with -inf: all of out (B, 1024) when nsplit > 1, the tail's rows
//    otherwise.
// status != CG_OK: nothing was launched.
struct CgPointMlpPlan { int status, dev, nsplit, n_main, tail_split; };
CgPointMlpPlan cg_pointmlp_plan(int B, int ntiles, int nsplit, int slots_per_cu, int min_tiles, int tail_split, float* out, hipStream_t s);

// Head of the dense-layer kernels' epilogue (gemm.hip, gemm_split.hip; A = their argument struct): the column's bias incl. the flattened
// identity (eye_k > 0: + I_k, col = i*k + i).  The rest of the epilogue -- per-group bias, ReLU, guarded store -- stays written out in
// each kernel: moved into a function (by reference, by value, per tile or per element) it changed the register allocation of all four.
template <typename A>
__device__ __forceinline__ float cg_gemm_col_bias(const A& a, int col) {
  float bias = a.bias ? a.bias[col] : 0.f;
  if (a.eye_k > 0 && (col % (a.eye_k + 1)) == 0) bias += 1.f;
  return bias;
}

// Argument check shared by the dense-layer entry points (K a multiple of k_mult: 8 for the f32 kernels' k-steps, 16 for the split ones')
static inline int cg_gemm_check_args(const float* x, int M, int K, int ldx, const void* w, int N, const float* row_bias, int rows_per_group,
                                     int ld_rb, const float* y, int ldy, int k_mult) {
  if (!x || !w || !y) return CG_ERR_ARG;
  if (M < 0 || N <= 0 || K <= 0 || (K % k_mult) != 0 || (ldx % 4) != 0 || ldx < K || ldy < N) return CG_ERR_ARG;
  if (((uintptr_t)x & 15) != 0) return CG_ERR_ARG;
  if (row_bias && (rows_per_group <= 0 || ld_rb < N)) return CG_ERR_ARG;
  return CG_OK;
}
