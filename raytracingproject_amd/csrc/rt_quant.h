// rt_quant.h -- is a finished sample's quantised radiance (three channels on the
// 2^-FIX_SAMPLE_SHIFT grid) in [0, 1]?  One predicate, shared by render_coherent's finish in
// the fp32 sphere-grid kernels (r18) and the CPU driver that checks it over every bit pattern
// (tests/cpp/quant_range_driver.cpp).
//
// in01 compares the floats' bit patterns as unsigned integers: +0 .. 1.0 are 0 .. 0x3f800000 in
// ascending order, everything above 1.0, +inf and the positive NaNs lie above 0x3f800000, and
// every pattern with the sign bit set (negative values, -inf, negative NaNs, -0.0) above those.
// So max(bits) <= 0x3f800000 is "each channel >= 0 and <= 1" -- one v_max3_u32 and one compare
// for six float compares and five ANDs -- but for -0.0, which the float compares accept and
// this refuses.  A refused sample takes flush_sample's generic tail, where a channel of -0.0
// (v == 0.f) adds nothing, as it adds nothing to the item sums (q != 0.f); the other channels
// and the segment count arrive in the same sums either way.
#pragma once
#include <cstdint>
#include <cstring>

#include "rt_scene.h"   // RT_HD

namespace rtx {

constexpr uint32_t QUANT_ONE_BITS = 0x3f800000u;   // 1.0f

RT_HD inline uint32_t quant_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
#endif
}

RT_HD inline bool in01(float qx, float qy, float qz) {
    const uint32_t x = quant_bits(qx), y = quant_bits(qy), z = quant_bits(qz);
    const uint32_t m = x > y ? x : y;
    return (m > z ? m : z) <= QUANT_ONE_BITS;
}

}   // namespace rtx
