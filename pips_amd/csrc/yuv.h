// The fixed-point YCbCr -> RGB rule of pips_frames_import (include/pips_hip.h): the constants and the one conversion that the
// kernels of frames_import.hip and their launcher share, so that the table exists once.
#pragma once
#include "common.h"

namespace pips {

// R = clamp((ky c + rv e + 32768) >> 16), G = clamp((ky c + gu d + gv e + 32768) >> 16), B = clamp((ky c + bu d + 32768) >> 16)
// with c = Y - y0, d = Cb - 128, e = Cr - 128; every constant is floor(65536 k + 0.5) of the standard coefficient (luma scaled by
// 255/219 and chroma by 255/224 in limited range).  Over all 2^24 triples every accumulator stays inside int32 (-1.9e7 .. 3.6e7).
struct YuvRule {
    int y0, ky, rv, gu, gv, bu;
};

// [matrix: PIPS_MATRIX_BT601, PIPS_MATRIX_BT709][range: PIPS_RANGE_LIMITED, PIPS_RANGE_FULL]
constexpr YuvRule YUV_RULES[2][2] = {
    {{16, 76309, 104597, -25675, -53279, 132201}, {0, 65536, 91881, -22553, -46802, 116130}},
    {{16, 76309, 117489, -13975, -34925, 138438}, {0, 65536, 103206, -12276, -30679, 121609}},
};

__host__ __device__ __forceinline__ int yuv_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One pixel; >> on a negative int is the arithmetic shift (floor) on every target this compiles for.
__host__ __device__ __forceinline__ void yuv_to_rgb(const YuvRule& k, int Y, int Cb, int Cr, int& r, int& g, int& b) {
    const int c = k.ky * (Y - k.y0) + 32768, d = Cb - 128, e = Cr - 128;
    r = yuv_clamp8((c + k.rv * e) >> 16);
    g = yuv_clamp8((c + k.gu * d + k.gv * e) >> 16);
    b = yuv_clamp8((c + k.bu * d) >> 16);
}

// The way back, for pips_tracks_draw's colours (include/pips_hip.h): Y = y0 + ((yr R + yg G + yb B + 32768) >> 16),
// Cb = clamp(128 + ((ur R + ug G + ub B + 32768) >> 16)), Cr = clamp(128 + ((vr R + vg G + vb B + 32768) >> 16)).  The constants are
// the standard coefficients scaled by 65536 (and by 219/255 for luma, 224/255 for chroma in limited range) and rounded so that each
// luma row sums to 65536 (56284 in limited range) and each chroma row to 0: a grey gives exactly (Y, 128, 128), white 235 / 255.
// Full-range chroma reaches 256 ahead of the clamp.  Every accumulator stays inside int32 (|sum| < 2^24).
struct RgbRule {
    int y0, yr, yg, yb, ur, ug, ub, vr, vg, vb;
};

// [matrix][range], as YUV_RULES
constexpr RgbRule RGB_RULES[2][2] = {
    {{16, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681}, {0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},
    {{16, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639}, {0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}},
};

__host__ __device__ __forceinline__ void rgb_to_yuv(const RgbRule& k, int r, int g, int b, int& Y, int& Cb, int& Cr) {
    Y = k.y0 + ((k.yr * r + k.yg * g + k.yb * b + 32768) >> 16);
    Cb = yuv_clamp8(128 + ((k.ur * r + k.ug * g + k.ub * b + 32768) >> 16));
    Cr = yuv_clamp8(128 + ((k.vr * r + k.vg * g + k.vb * b + 32768) >> 16));
}

// The 10-bit rule (PIPS_FMT_P010, PIPS_FMT_I010): samples 0..1023, c = Y - y0, d = Cb - 512, e = Cr - 512 and
// R = clamp((ky c + rv e + 2^17) >> 18), G and B likewise, to the same 8-bit levels; every constant is floor(2^18 k + 0.5) with luma
// scaled by 255/876 and chroma by 255/896 in limited range (the 8-bit constants: a sample of 4 v converts as the 8-bit v does) and
// both by 255/1023 in full range.  Over all 2^30 triples every accumulator stays inside int32 (-7.7e7 .. 1.5e8).
constexpr YuvRule YUV10_RULES[2][2] = {
    {{64, 76309, 104597, -25675, -53279, 132201}, {0, 65344, 91612, -22487, -46664, 115789}},
    {{64, 76309, 117489, -13975, -34925, 138438}, {0, 65344, 102903, -12240, -30589, 121252}},
};

__host__ __device__ __forceinline__ void yuv10_to_rgb(const YuvRule& k, int Y, int Cb, int Cr, int& r, int& g, int& b) {
    const int c = k.ky * (Y - k.y0) + 131072, d = Cb - 512, e = Cr - 512;
    r = yuv_clamp8((c + k.rv * e) >> 18);
    g = yuv_clamp8((c + k.gu * d + k.gv * e) >> 18);
    b = yuv_clamp8((c + k.bu * d) >> 18);
}

// The way back to 10 bits, for pips_tracks_draw_ex's colours on P010 and I010 (include/pips_hip.h): with h = 1 << (sh - 1),
// Y = y0 + ((yr R + yg G + yb B + h) >> sh), Cb = clamp(512 + ((ur R + ug G + ub B + h) >> sh)), Cr likewise, clamp to [0, 1023].
// Limited range is the 8-bit row with two more result bits (sh = 14): white 940, chroma 64..960.  Full range (sh = 16) has the
// standard coefficients scaled by 65536 x 1023 / 255 and rounded so that each luma row sums to 262915 and each chroma row to 0:
// black 0, white 1023, chroma reaches 1024 ahead of the clamp.  A grey gives exactly (Y, 512, 512) in both.  Every accumulator
// stays inside int32 (|sum| < 2^27).
struct Rgb10Rule {
    int y0, sh, yr, yg, yb, ur, ug, ub, vr, vg, vb;
};

// [matrix][range], as YUV_RULES
constexpr Rgb10Rule RGB10_RULES[2][2] = {
    {{64, 14, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681}, {0, 16, 78612, 154331, 29972, -44363, -87095, 131458, 131458, -110079, -21379}},
    {{64, 14, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639}, {0, 16, 55896, 188037, 18982, -30123, -101335, 131458, 131458, -119404, -12054}},
};

__host__ __device__ __forceinline__ int yuv_clamp10(int v) { return v < 0 ? 0 : (v > 1023 ? 1023 : v); }

__host__ __device__ __forceinline__ void rgb_to_yuv10(const Rgb10Rule& k, int r, int g, int b, int& Y, int& Cb, int& Cr) {
    const int half = 1 << (k.sh - 1);
    Y = k.y0 + ((k.yr * r + k.yg * g + k.yb * b + half) >> k.sh);
    Cb = yuv_clamp10(512 + ((k.ur * r + k.ug * g + k.ub * b + half) >> k.sh));
    Cr = yuv_clamp10(512 + ((k.vr * r + k.vg * g + k.vb * b + half) >> k.sh));
}

}  // namespace pips
