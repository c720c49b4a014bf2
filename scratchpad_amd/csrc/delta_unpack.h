// The in-register unpack of this library's 4-bit 2:4 packed format (include/scratchpad_hip.h states the layout), shared by
// delta.hip (delta_mm_kernel) and quant_moe.hip (qmoe_gemm_kernel).  Unpacking is VALU: a code byte becomes two 16-bit
// floats through the exponent trick (0x6400 | c is 1024 + c in fp16, 0x4300 | c is 128 + c in bf16; subtracting 1032
// resp. 136 leaves the integer c - 8 exactly), and the pair is shifted to the 16-bit positions p0 and p1 of the group's
// four.
#pragma once
#include "sp_common.h"

namespace sp {

// one code byte -> (code_lo - 8) in the low and (code_hi - 8) in the high 16 bits, in the activation dtype, exactly
template <typename Tag>
__device__ __forceinline__ uint32_t delta_pair(uint32_t byte);
template <>
__device__ __forceinline__ uint32_t delta_pair<f16_tag>(uint32_t byte) {
  const uint32_t w = (byte & 0xfu) | ((byte & 0xf0u) << 12) | 0x64006400u;       // 1024 + c, twice
  const f16x2_t bias = {(_Float16)1032.0f, (_Float16)1032.0f};
  const f16x2_t v = as_f16x2(w) - bias;
  return __builtin_bit_cast(uint32_t, v);
}
template <>
__device__ __forceinline__ uint32_t delta_pair<bf16_tag>(uint32_t byte) {
  const uint32_t w = (byte & 0xfu) | ((byte & 0xf0u) << 12) | 0x43004300u;       // 128 + c, twice
  const float lo = as_f32(w << 16) - 136.0f, hi = as_f32(w & 0xffff0000u) - 136.0f;   // integers in [-8, 7]: the low
  return (as_u32(lo) >> 16) | (as_u32(hi) & 0xffff0000u);                             // 16 bits of both are zero
}

// the 8 dense 16-bit values of two groups: `codes16` = their two code bytes, `meta8` = their two meta nibbles
template <typename Tag>
__device__ __forceinline__ u32x4 delta_expand(uint32_t codes16, uint32_t meta8) {
  u32x4 o;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const uint32_t v = delta_pair<Tag>((codes16 >> (8 * g)) & 0xffu);
    const uint32_t m = meta8 >> (4 * g);
    const uint64_t z = ((uint64_t)(v & 0xffffu) << ((m & 3u) * 16)) | ((uint64_t)(v >> 16) << (((m >> 2) & 3u) * 16));
    o[2 * g] = (uint32_t)z;
    o[2 * g + 1] = (uint32_t)(z >> 32);
  }
  return o;
}

}  // namespace sp
