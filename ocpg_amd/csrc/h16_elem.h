// The 16-bit storage types of the own MFMA kernels of the ResNet body (csrc/conv3x3_mfma.hip, csrc/conv3x3_wgrad.hip,
// csrc/gemm_dgrad_bn.hip): storage type, MFMA opcode and the round-to-nearest-even narrowing -- what differs between a bf16 kernel and
// its fp16 twin.  The staging, the transposing LDS reads (ds_read_b64_tr_b16) and the "bits as a signed short > 0" ReLU-mask test are
// type-agnostic.  A file that needs more of a type (packing, an epilogue switch) derives its own trait from these.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace ocpg_h16 {

typedef short h16x8 __attribute__((ext_vector_type(8)));         // an MFMA operand fragment: 8 elements of either type, as bits
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Bf16 {
  using T = __hip_bfloat16;
  static __device__ __forceinline__ f32x16 mfma(h16x8 a, h16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ T narrow(float v) { return __float2bfloat16(v); }                          // RNE, NaN-preserving
  static __device__ __forceinline__ unsigned short bits(float v) { return __bfloat16_as_ushort(__float2bfloat16(v)); }
};

struct Fp16 {
  using T = __half;
  static __device__ __forceinline__ f32x16 mfma(h16x8 a, h16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ T narrow(float v) { return __float2half_rn(v); }                           // RNE; past 65504: inf, as in ATen
  static __device__ __forceinline__ unsigned short bits(float v) { return __half_as_ushort(__float2half_rn(v)); }
};

}  // namespace ocpg_h16
