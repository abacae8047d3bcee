// Device-side pieces shared by the SuperGlue units (sg_gemm.hip, sg_gnn.hip): MFMA operand types and wrappers.
#pragma once
#include <hip/hip_runtime.h>

namespace rspl {
namespace sg {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ floatx16 mfma32(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ floatx16 mfma16(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

}  // namespace sg
}  // namespace rspl
