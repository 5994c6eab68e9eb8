// fp8_dev.h -- device helpers shared by the two OCP e4m3fn formats of the library: the drafter's weight bricks (weight_fp8.hip) and the KV-cache rows
// (kv_fp8.hip, tree_attention.hip).
#pragma once
#include "common.h"

namespace lantern {

// f32 -> e4m3fn, round to nearest even, saturating (|x| >= 464 would round past 448 -> 448; NaN -> 448 with its sign): the arithmetic of torch's
// float8_e4m3fn conversion on the range a scaled row can reach
__device__ __forceinline__ uint8_t f32_to_e4m3fn(float x) {
    const uint32_t u = __float_as_uint(x);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    const float a = __uint_as_float(u & 0x7fffffffu);
    if (!(a < 464.0f)) return sign | 0x7e;
    if (a < 0.015625f) return sign | (uint8_t)__float2int_rn(a * 512.0f);          // subnormal range: multiples of 2^-9 (8 = the smallest normal)
    uint32_t b = u & 0x7fffffffu;
    b += 0x7ffffu + ((b >> 20) & 1u);                                              // RNE to 3 mantissa bits (a carry moves into the exponent)
    return sign | (uint8_t)((((b >> 23) - 120u) << 3) | ((b >> 20) & 7u));
}

// ---- the KV-cache row format (include/lantern_hip.h, "FP8 KV cache"): d code bytes, the row's f32 scale 2^e, 12 zero bytes
constexpr int KV8_TAIL = 16;
constexpr int KV8_EMIN = -64, KV8_EMAX = 64;

// eight codes times the row's scale -> eight bf16 values (v_cvt_scalef32_pk_bf16_fp8 with the scale as its operand: code * 2^e is a bf16 value, so
// nothing is rounded)
typedef __bf16 kv8_bf16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ kv8_bf16x8_t kv8_expand8(uint2 c, float scale) {
    typedef __bf16 bf16x2v_t __attribute__((ext_vector_type(2)));
    const bf16x2v_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, scale, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, scale, true);
    const bf16x2v_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, scale, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, scale, true);
    return __builtin_bit_cast(kv8_bf16x8_t, make_uint4(__builtin_bit_cast(unsigned int, p0), __builtin_bit_cast(unsigned int, p1),
                                                       __builtin_bit_cast(unsigned int, p2), __builtin_bit_cast(unsigned int, p3)));
}

}  // namespace lantern
