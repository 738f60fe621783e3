// The 8-bit luma that the integer rules on raw frames share (pips_corner_table, pips_cut_table; include/pips_hip.h): one helper,
// so the rules cannot drift apart.
#pragma once
#include "common.h"

namespace pips {

// A channel value as an integer 0..255: a uint8 as it is, a float by u = floor(min(max(v, 0), 255) + 0.5) (one fp32 add, no
// product: nothing for the compiler to contract).
template <typename T>
__device__ __forceinline__ int channel_u8(T v) {
    if constexpr (sizeof(T) == 1) {
        return (int)v;
    } else {
        return (int)floorf(fminf(fmaxf(v, 0.f), 255.f) + 0.5f);
    }
}

// The fixed-point BT.601 weights on quantised channels.
__device__ __forceinline__ int luma_of(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

// Luma of pixel (y, x) of a planar frame, `at` = y*w + x and `plane` = h*w.
template <typename T>
__device__ __forceinline__ int luma_at(const T* __restrict__ frame, size_t plane, size_t at) {
    int ch[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ch[k] = channel_u8(frame[k * plane + at]);
    return luma_of(ch[0], ch[1], ch[2]);
}

}  // namespace pips
