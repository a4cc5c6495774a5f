// f32_key.hpp — the order of the floats as unsigned integers: -inf < ... < -0 < +0 < ... < +inf.  Integer atomicMin / atomicMax on the keys give
// an order-free float minimum / maximum that holds for negative values too (pcr_label_aabb_f32, the PointNet chain's max over points).
#pragma once

#include <cstdint>
#include <cstring>

namespace pcr {

__host__ __device__ inline uint32_t f32_key(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float f32_from_key(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
constexpr uint32_t KEY_PINF = 0xFF800000u, KEY_NINF = 0x007FFFFFu;      // f32_key(+inf), f32_key(-inf)

}  // namespace pcr
