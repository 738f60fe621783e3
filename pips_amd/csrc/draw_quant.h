// The quantisation of a track position to eighths of a surface pixel (pips_tracks_draw's rule, include/pips_hip.h), shared by the
// kernels that place tracks on a surface -- draw.hip and masks.hip -- so that the rule exists once.
#pragma once
#include "common.h"
#include "fp_rn.h"

namespace pips {

constexpr int DRAW_ABSENT = INT_MIN;                            // x of a point that is not there

// a coordinate of the model's frame -> eighths of a surface pixel, DRAW_ABSENT for NaN, infinities and |u| > 32768
__device__ __forceinline__ int quantise(float x, bool scaled, float s) {
    const float u = scaled ? sub_rn(mul_rn(add_rn(x, 0.5f), s), 0.5f) : x;
    if (!(fabsf(u) <= 32768.0f)) return DRAW_ABSENT;
    return (int)floorf(add_rn(mul_rn(u, 8.0f), 0.5f));
}

}  // namespace pips
