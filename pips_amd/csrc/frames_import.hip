// Decoder frames in (pips_frames_import, pips_frames_import_ex; drivers.import_frames): packed RGB / BGR / RGBA / BGRA, NV12, I420 and
// the 10-bit P010 and I010 frames with any base address, row pitch and frame step become the planar (F,3,H,W) frames, uint8 or
// float32, that every other entry point reads.  The rule (include/pips_hip.h; yuv.h for the YCbCr constants) is integer arithmetic
// up to the resize; the bilinear resize is resize_frames_kernel's (encoder.hip) single-rounded fp32 arithmetic and the triangle
// (antialiasing) filter is integer arithmetic to the end, so the output is bit for bit drivers.import_frames_torch's.
// Plain HIP, pure bandwidth: one launch, no atomics, no workspace; nothing outside dst is written.  Only the triangle filter uses LDS.
#include "common.h"
#include "fp_rn.h"
#include "yuv.h"

namespace pips {

namespace {

constexpr int IMPORT_THREADS = 256;
enum { LAYOUT_PACKED3 = 0, LAYOUT_PACKED4 = 1, LAYOUT_NV12 = 2, LAYOUT_I420 = 3, LAYOUT_P010 = 4, LAYOUT_I010 = 5 };
// 16-bit samples (P010, I010); one interleaved Cb Cr plane (NV12, P010)
template <int LAYOUT> constexpr bool WIDE16 = LAYOUT == LAYOUT_P010 || LAYOUT == LAYOUT_I010;
template <int LAYOUT> constexpr bool SEMI = LAYOUT == LAYOUT_NV12 || LAYOUT == LAYOUT_P010;

// frame f, row y of plane k starts at p[k] + f step[k] + y pitch[k]
struct ImportSrc {
    const unsigned char* p[3];
    size_t pitch[3], step[3];
};

__device__ __forceinline__ const unsigned char* src_row(const ImportSrc& s, int k, int f, int y) {
    return s.p[k] + (size_t)f * s.step[k] + (size_t)y * s.pitch[k];
}

// NW words of source bytes from p: UNIT-byte loads (UNIT = 16: NW a multiple of 4; UNIT = 4) when `wide` -- the caller has checked
// that p is UNIT-aligned and that all 4 NW bytes belong to the row -- and otherwise the first n bytes one by one, the rest 0.
template <int NW, int UNIT>
__device__ __forceinline__ void load_words(const unsigned char* __restrict__ p, bool wide, int n, unsigned (&wd)[NW]) {
    if (wide) {
        if constexpr (UNIT == 16) {
#pragma unroll
            for (int i = 0; i < NW / 4; ++i) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[i];
                wd[4 * i] = v.x, wd[4 * i + 1] = v.y, wd[4 * i + 2] = v.z, wd[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) wd[i] = reinterpret_cast<const unsigned*>(p)[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) wd[i] = 0;
#pragma unroll
        for (int i = 0; i < 4 * NW; ++i)
            if (i < n) wd[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
}

__device__ __forceinline__ int byte_of(const unsigned* wd, int i) { return (int)((wd[i >> 2] >> (8 * (i & 3))) & 255u); }

// the 10-bit value of a 16-bit little-endian word: the high ten bits of P010, the low ten of I010
template <int LAYOUT>
__device__ __forceinline__ int ten_bits(unsigned v) { return LAYOUT == LAYOUT_P010 ? (int)(v >> 6) : (int)(v & 1023u); }

// sample i of the words wd: a byte, or the 10-bit value of a 16-bit word
template <int LAYOUT>
__device__ __forceinline__ int sample_of(const unsigned* wd, int i) {
    if constexpr (WIDE16<LAYOUT>) return ten_bits<LAYOUT>((wd[i >> 1] >> (16 * (i & 1))) & 65535u);
    else return byte_of(wd, i);
}

// sample i of a row in memory (a 16-bit row starts on an even address: checked by the caller)
template <int LAYOUT>
__device__ __forceinline__ int sample_at(const unsigned char* __restrict__ row, size_t i) {
    if constexpr (WIDE16<LAYOUT>) return ten_bits<LAYOUT>(reinterpret_cast<const unsigned short*>(row)[i]);
    else return row[i];
}

template <int LAYOUT>
__device__ __forceinline__ void to_rgb(const YuvRule& k, int Y, int Cb, int Cr, int& r, int& g, int& b) {
    if constexpr (WIDE16<LAYOUT>) yuv10_to_rgb(k, Y, Cb, Cr, r, g, b);
    else yuv_to_rgb(k, Y, Cb, Cr, r, g, b);
}

// BYTES (2, 4, 8 or 16) bytes from a BYTES-aligned p as words, the rest of wd untouched
template <int BYTES>
__device__ __forceinline__ void load_chunk(const unsigned char* __restrict__ p, unsigned* wd) {
    if constexpr (BYTES == 2) {
        wd[0] = *reinterpret_cast<const unsigned short*>(p);
    } else if constexpr (BYTES == 4) {
        wd[0] = *reinterpret_cast<const unsigned*>(p);
    } else if constexpr (BYTES == 8) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        wd[0] = a.x, wd[1] = a.y;
    } else {
        const uint4 a = *reinterpret_cast<const uint4*>(p);
        wd[0] = a.x, wd[1] = a.y, wd[2] = a.z, wd[3] = a.w;
    }
}

// ---------------------------------------------------------------------------------------------------------------- no resize
// One thread per (frame, row, group).  A row is walked in GROUPS as cut_hist_kernel walks it, here by the DESTINATION's address:
// group 0 is the head [0, hd) that brings the row of dst to a 16-byte address, group g >= 1 the pixels [hd + (g-1) V, hd + g V)
// with V the pixels of 16 output bytes (16 uint8, 4 float).  A whole group is stored with one 16-byte store per plane; the head,
// the tail and every group of an output whose three planes do not share their alignment (plane bytes not a multiple of 16) with
// element stores.  The source bytes of a whole group are read with 16-byte (V = 16) or 4-byte (V = 4) loads where their address
// allows -- the chroma of a group only when the group starts on an even pixel, too -- and one by one otherwise: each byte once,
// the chroma of a pixel pair once for both pixels.  Neighbouring lanes take neighbouring groups of one row.  The 16-bit formats read
// twice the bytes by the same discipline: a group's Y is 32 (V = 16) or 8 (V = 4) bytes, two wide loads.
template <int LAYOUT, typename T>
__global__ __launch_bounds__(IMPORT_THREADS) void import_stream_kernel(ImportSrc s, int bgr, YuvRule rule, int h, int w, unsigned G,
                                                                       unsigned items, T* __restrict__ dst) {
    constexpr int V = 16 / (int)sizeof(T);                      // pixels of a group
    constexpr int UNIT = V == 16 ? 16 : 4;                      // bytes of a wide source load: V bytes of Y are one of them
    constexpr int BPP = LAYOUT == LAYOUT_PACKED3 ? 3 : LAYOUT == LAYOUT_PACKED4 ? 4 : 1;
    constexpr int SB = WIDE16<LAYOUT> ? 2 : 1;                  // bytes of a sample
    constexpr int NW = BPP * SB * V / 4;                        // words of plane 0 in a group
    const unsigned it = blockIdx.x * (unsigned)IMPORT_THREADS + threadIdx.x;
    if (it >= items) return;
    const unsigned g = it % G, row = it / G;
    const int y = (int)(row % (unsigned)h), f = (int)(row / (unsigned)h);
    const size_t plane = (size_t)h * w;
    T* d = dst + (size_t)f * 3 * plane + (size_t)y * w;
    const bool vec = (plane * sizeof(T)) % 16 == 0 && ((uintptr_t)dst % sizeof(T)) == 0;
    const int hd = vec ? min(w, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) / (unsigned)sizeof(T))) : 0;
    const int xa = g == 0 ? 0 : (int)min((long long)w, (long long)hd + (long long)(g - 1) * V);
    const int xb = g == 0 ? hd : (int)min((long long)w, (long long)xa + V);
    if (xa >= xb) return;
    const int n = xb - xa;
    const bool whole = n == V;

    int R[V], Gn[V], B[V];
    const unsigned char* p0 = src_row(s, 0, f, y) + (size_t)xa * BPP * SB;
    unsigned wd[NW];
    load_words<NW, UNIT>(p0, whole && ((uintptr_t)p0 & (UNIT - 1)) == 0, n * BPP * SB, wd);
    if constexpr (LAYOUT == LAYOUT_PACKED3 || LAYOUT == LAYOUT_PACKED4) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c0 = byte_of(wd, k * BPP), c2 = byte_of(wd, k * BPP + 2);
            R[k] = bgr ? c2 : c0, Gn[k] = byte_of(wd, k * BPP + 1), B[k] = bgr ? c0 : c2;
        }
    } else {
        // the chroma samples xa/2 .. (xb-1)/2: V/2 of them, one more when the group starts on an odd pixel
        constexpr int NC = V / 2 + 1;
        int cb[NC], cr[NC];
        const int c0 = xa >> 1, cn = ((xb - 1) >> 1) - c0 + 1, odd = xa & 1;
        if constexpr (SEMI<LAYOUT>) {
            constexpr int PB = 2 * SB;                           // bytes of a Cb Cr pair
            constexpr int CWN = (NC * PB + 3) / 4, CWW = V / 2 * PB / 4;          // words of V/2 + 1 pairs; of the V/2 of a wide load
            const unsigned char* pc = src_row(s, 1, f, y >> 1) + PB * (size_t)c0;
            unsigned cw[CWN];
            if (whole && !odd && ((uintptr_t)pc & (UNIT - 1)) == 0) {
                unsigned a[CWW];
                load_words<CWW, UNIT>(pc, true, 0, a);
#pragma unroll
                for (int i = 0; i < CWN; ++i) cw[i] = 0;
#pragma unroll
                for (int i = 0; i < CWW; ++i) cw[i] = a[i];
            } else {
                load_words<CWN, 4>(pc, false, PB * cn, cw);
            }
#pragma unroll
            for (int j = 0; j < NC; ++j) cb[j] = sample_of<LAYOUT>(cw, 2 * j), cr[j] = sample_of<LAYOUT>(cw, 2 * j + 1);
        } else {
            const unsigned char* pu = src_row(s, 1, f, y >> 1) + SB * (size_t)c0;
            const unsigned char* pv = src_row(s, 2, f, y >> 1) + SB * (size_t)c0;
            constexpr int CW = (NC * SB + 3) / 4;                // V/2 + 1 samples
            constexpr int WB = V / 2 * SB;                       // bytes of the V/2 samples of a wide load
            unsigned uw[CW], vw[CW];
            if (whole && !odd && (((uintptr_t)pu | (uintptr_t)pv) & (WB - 1)) == 0) {
#pragma unroll
                for (int i = 0; i < CW; ++i) uw[i] = vw[i] = 0;
                load_chunk<WB>(pu, uw);
                load_chunk<WB>(pv, vw);
            } else {
                load_words<CW, 4>(pu, false, SB * cn, uw);
                load_words<CW, 4>(pv, false, SB * cn, vw);
            }
#pragma unroll
            for (int j = 0; j < NC; ++j) cb[j] = sample_of<LAYOUT>(uw, j), cr[j] = sample_of<LAYOUT>(vw, j);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int j0 = k >> 1, j1 = (k + 1) >> 1;             // pixel xa + k reads sample (xa + k)/2 - xa/2
            to_rgb<LAYOUT>(rule, sample_of<LAYOUT>(wd, k), odd ? cb[j1] : cb[j0], odd ? cr[j1] : cr[j0], R[k], Gn[k], B[k]);
        }
    }

    if (vec && g > 0 && whole) {
        if constexpr (sizeof(T) == 1) {
            unsigned ow[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) ow[i] = 0;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                ow[k >> 2] |= (unsigned)R[k] << (8 * (k & 3));
                ow[4 + (k >> 2)] |= (unsigned)Gn[k] << (8 * (k & 3));
                ow[8 + (k >> 2)] |= (unsigned)B[k] << (8 * (k & 3));
            }
            *reinterpret_cast<uint4*>(d + xa) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            *reinterpret_cast<uint4*>(d + plane + xa) = make_uint4(ow[4], ow[5], ow[6], ow[7]);
            *reinterpret_cast<uint4*>(d + 2 * plane + xa) = make_uint4(ow[8], ow[9], ow[10], ow[11]);
        } else {
            *reinterpret_cast<float4*>(d + xa) = make_float4((float)R[0], (float)R[1], (float)R[2], (float)R[3]);
            *reinterpret_cast<float4*>(d + plane + xa) = make_float4((float)Gn[0], (float)Gn[1], (float)Gn[2], (float)Gn[3]);
            *reinterpret_cast<float4*>(d + 2 * plane + xa) = make_float4((float)B[0], (float)B[1], (float)B[2], (float)B[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (k < n) {
                d[xa + k] = (T)R[k];
                d[plane + xa + k] = (T)Gn[k];
                d[2 * plane + xa + k] = (T)B[k];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- resize
// One thread per output pixel, all three channels; neighbouring lanes take neighbouring x.  The four neighbours of
// resize_frames_kernel are converted once each, and a chroma sample is fetched once for the neighbours that fall into it; the blend
// is that kernel's: the source index one fused multiply-add, then four single-rounded products and three sums per channel in its
// order (fp_rn.h: nothing else is fused).  uint8 output: floor(v + 0.5), the
// quantisation of luma.h (v lies in [0, 255]).
template <int LAYOUT>
__device__ __forceinline__ void packed_px(const unsigned char* __restrict__ p, int bgr, int (&c)[3]) {
    const int a = p[0], b = p[2];
    c[0] = bgr ? b : a, c[1] = p[1], c[2] = bgr ? a : b;
}

template <int LAYOUT, typename T>
__global__ __launch_bounds__(IMPORT_THREADS) void import_resize_kernel(ImportSrc s, int bgr, YuvRule rule, int h, int w,
                                                                       T* __restrict__ dst, int H, int W, float sh, float sw,
                                                                       unsigned total) {
    constexpr int BPP = LAYOUT == LAYOUT_PACKED3 ? 3 : LAYOUT == LAYOUT_PACKED4 ? 4 : 1;
    const unsigned i = blockIdx.x * (unsigned)IMPORT_THREADS + threadIdx.x;
    if (i >= total) return;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const int x = (int)(i % (unsigned)W), y = (int)((i / (unsigned)W) % (unsigned)H), f = (int)(i / HW);
    const float fy = fmaxf(fmaf(sh, (float)y + 0.5f, -0.5f), 0.f);
    const float fx = fmaxf(fmaf(sw, (float)x + 0.5f, -0.5f), 0.f);
    // (the min guards the addresses alone: fy <= h - 0.5 up to rounding, so y0 <= h - 1 already)
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;

    int p00[3], p01[3], p10[3], p11[3];
    const unsigned char* r0 = src_row(s, 0, f, y0);
    const unsigned char* r1 = src_row(s, 0, f, y1);
    if constexpr (LAYOUT == LAYOUT_PACKED3 || LAYOUT == LAYOUT_PACKED4) {
        packed_px<LAYOUT>(r0 + (size_t)x0 * BPP, bgr, p00);
        packed_px<LAYOUT>(r0 + (size_t)x1 * BPP, bgr, p01);
        packed_px<LAYOUT>(r1 + (size_t)x0 * BPP, bgr, p10);
        packed_px<LAYOUT>(r1 + (size_t)x1 * BPP, bgr, p11);
    } else {
        const int cx0 = x0 >> 1, cx1 = x1 >> 1, cy0 = y0 >> 1, cy1 = y1 >> 1;
        int cb00, cr00, cb01, cr01, cb10, cr10, cb11, cr11;
        auto chroma = [&](int cy, int cx, int& cb, int& cr) {
            if constexpr (SEMI<LAYOUT>) {
                const unsigned char* q = src_row(s, 1, f, cy);
                cb = sample_at<LAYOUT>(q, 2 * (size_t)cx), cr = sample_at<LAYOUT>(q, 2 * (size_t)cx + 1);
            } else {
                cb = sample_at<LAYOUT>(src_row(s, 1, f, cy), cx), cr = sample_at<LAYOUT>(src_row(s, 2, f, cy), cx);
            }
        };
        chroma(cy0, cx0, cb00, cr00);
        if (cx1 != cx0) chroma(cy0, cx1, cb01, cr01); else cb01 = cb00, cr01 = cr00;
        if (cy1 != cy0) {
            chroma(cy1, cx0, cb10, cr10);
            if (cx1 != cx0) chroma(cy1, cx1, cb11, cr11); else cb11 = cb10, cr11 = cr10;
        } else {
            cb10 = cb00, cr10 = cr00, cb11 = cb01, cr11 = cr01;
        }
        to_rgb<LAYOUT>(rule, sample_at<LAYOUT>(r0, x0), cb00, cr00, p00[0], p00[1], p00[2]);
        to_rgb<LAYOUT>(rule, sample_at<LAYOUT>(r0, x1), cb01, cr01, p01[0], p01[1], p01[2]);
        to_rgb<LAYOUT>(rule, sample_at<LAYOUT>(r1, x0), cb10, cr10, p10[0], p10[1], p10[2]);
        to_rgb<LAYOUT>(rule, sample_at<LAYOUT>(r1, x1), cb11, cr11, p11[0], p11[1], p11[2]);
    }
    T* o = dst + (size_t)f * 3 * HW + (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = add_rn(mul_rn(lx0, (float)p00[c]), mul_rn(lx1, (float)p01[c]));
        const float bot = add_rn(mul_rn(lx0, (float)p10[c]), mul_rn(lx1, (float)p11[c]));
        const float v = add_rn(mul_rn(ly0, top), mul_rn(ly1, bot));
        if constexpr (sizeof(T) == 1) {
            o[(size_t)c * HW] = (unsigned char)(int)floorf(add_rn(v, 0.5f));
        } else {
            o[(size_t)c * HW] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- triangle filter
// PIPS_FILTER_TRIANGLE (include/pips_hip.h): along an axis of n source and N output samples the raw weight of source j for output
// i is max(0, m2 - |(2 j + 1) N - (2 i + 1) n|) with m2 = 2 max(n, N).  It is positive exactly for tri_lo <= j <= tri_hi (clipped
// to the source), at least one and at most 2 max(n / N, 1) + 1 samples; both bounds do not decrease with i.  Everything fits int32:
// (2 j + 1) N and (2 i + 1) n stay below 2^28 under PIPS_FILTER_DIM_MAX.
__host__ __device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// the first j with (2 j + 1) N > (2 i + 1) n - m2
__host__ __device__ __forceinline__ int tri_lo(int i, int n, int N, int m2) {
    const int j = floor_div((2 * i + 1) * n - m2 - N, 2 * N) + 1;
    return j < 0 ? 0 : j;
}
// the last j with (2 j + 1) N < (2 i + 1) n + m2
__host__ __device__ __forceinline__ int tri_hi(int i, int n, int N, int m2) {
    const int j = floor_div((2 * i + 1) * n + m2 - N - 1, 2 * N);
    return j > n - 1 ? n - 1 : j;
}
__host__ __device__ __forceinline__ int tri_weight(int i, int j, int n, int N, int m2) {
    const int d = (2 * j + 1) * N - (2 * i + 1) * n;
    return m2 - (d < 0 ? -d : d);
}

constexpr int TRI_TW = 32, TRI_TH = 8;                          // output pixels of a tile: x on the lanes of half a wave, <= 8 rows
constexpr int TRI_LDS_MAX = 64 * 1024;

// pixel (y, x) of frame f, converted, as R | G << 8 | B << 16
template <int LAYOUT>
__device__ __forceinline__ unsigned packed_rgb_at(const ImportSrc& s, int bgr, const YuvRule& rule, int f, int y, int x) {
    int r, g, b;
    if constexpr (LAYOUT == LAYOUT_PACKED3 || LAYOUT == LAYOUT_PACKED4) {
        constexpr int BPP = LAYOUT == LAYOUT_PACKED3 ? 3 : 4;
        int c[3];
        packed_px<LAYOUT>(src_row(s, 0, f, y) + (size_t)x * BPP, bgr, c);
        r = c[0], g = c[1], b = c[2];
    } else {
        const int Y = sample_at<LAYOUT>(src_row(s, 0, f, y), x);
        int cb, cr;
        if constexpr (SEMI<LAYOUT>) {
            const unsigned char* q = src_row(s, 1, f, y >> 1);
            cb = sample_at<LAYOUT>(q, 2 * (size_t)(x >> 1)), cr = sample_at<LAYOUT>(q, 2 * (size_t)(x >> 1) + 1);
        } else {
            cb = sample_at<LAYOUT>(src_row(s, 1, f, y >> 1), x >> 1), cr = sample_at<LAYOUT>(src_row(s, 2, f, y >> 1), x >> 1);
        }
        to_rgb<LAYOUT>(rule, Y, cb, cr, r, g, b);
    }
    return (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
}

// One block per tile of TRI_TW x TH output pixels of one frame (TH <= TRI_TH, chosen by the launcher from the ratio).  The tile's
// footprint -- source rows r0..r1, columns c0..c1 -- is walked eight rows at a time: the block stages those rows in LDS, row-major,
// neighbouring lanes reading neighbouring source pixels and converting each once (stage: [8][CW] packed RGB); then thread (row,
// x) sums its taps of that row into hs: [3][R][TRI_TW] int32, one plane per channel so that the lanes of a store or a load are 32
// consecutive words (no bank is hit twice).  Pass 2: thread (y, x) sums its rows of hs with ry in int64 and divides.
// R and CW: the most rows and columns of any tile's footprint, from the launcher.  The reads of stage run with a lane stride of
// about w / W words: free of conflicts at odd strides, two-way on average at a typical ratio.
template <int LAYOUT, typename T>
__global__ __launch_bounds__(IMPORT_THREADS) void import_triangle_kernel(ImportSrc s, int bgr, YuvRule rule, int h, int w,
                                                                         T* __restrict__ dst, int H, int W, int TH, unsigned tiles_x,
                                                                         unsigned tiles_y, int R, int CW) {
    extern __shared__ int tri_lds[];
    int* hs = tri_lds;
    unsigned* stage = reinterpret_cast<unsigned*>(tri_lds + 3 * R * TRI_TW);
    const unsigned tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const int f = (int)(blockIdx.x / (tiles_x * tiles_y));
    const int X0 = (int)tx * TRI_TW, Y0 = (int)ty * TH, X1 = min(X0 + TRI_TW, W), Y1 = min(Y0 + TH, H);
    const int my2 = 2 * max(h, H), mx2 = 2 * max(w, W);
    const int r0 = tri_lo(Y0, h, H, my2), rows = tri_hi(Y1 - 1, h, H, my2) - r0 + 1;
    const int c0 = tri_lo(X0, w, W, mx2), cols = tri_hi(X1 - 1, w, W, mx2) - c0 + 1;
    const int lane = threadIdx.x & (TRI_TW - 1), slot = threadIdx.x / TRI_TW;
    const int x = X0 + lane;
    const bool xin = x < X1;
    const int jlo = xin ? tri_lo(x, w, W, mx2) : 0, jhi = xin ? tri_hi(x, w, W, mx2) : -1;

    for (int rb = 0; rb < rows; rb += IMPORT_THREADS / TRI_TW) {
        const int r = rb + slot;                                 // this thread's row of the footprint
        if (r < rows)
            for (int c = lane; c < cols; c += TRI_TW) stage[slot * CW + c] = packed_rgb_at<LAYOUT>(s, bgr, rule, f, r0 + r, c0 + c);
        __syncthreads();
        if (r < rows && xin) {
            int ar = 0, ag = 0, ab = 0;
            for (int j = jlo; j <= jhi; ++j) {
                const int wt = tri_weight(x, j, w, W, mx2);
                const unsigned px = stage[slot * CW + (j - c0)];
                ar += wt * (int)(px & 255u), ag += wt * (int)((px >> 8) & 255u), ab += wt * (int)(px >> 16);
            }
            hs[(0 * R + r) * TRI_TW + lane] = ar;
            hs[(1 * R + r) * TRI_TW + lane] = ag;
            hs[(2 * R + r) * TRI_TW + lane] = ab;
        }
        __syncthreads();
    }

    const int y = Y0 + slot;
    if (slot >= TH || y >= Y1 || !xin) return;
    long long sx = 0, sy = 0, num[3] = {0, 0, 0};
    for (int j = jlo; j <= jhi; ++j) sx += tri_weight(x, j, w, W, mx2);
    const int klo = tri_lo(y, h, H, my2), khi = tri_hi(y, h, H, my2);
    for (int k = klo; k <= khi; ++k) {
        const long long wt = tri_weight(y, k, h, H, my2);
        sy += wt;
#pragma unroll
        for (int c = 0; c < 3; ++c) num[c] += wt * (long long)hs[(c * R + (k - r0)) * TRI_TW + lane];
    }
    const long long den = sx * sy;                               // < 2^38; 512 num < 2^55
    const size_t HW = (size_t)H * W;
    T* o = dst + (size_t)f * 3 * HW + (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int q = (int)((512 * num[c] + den) / (2 * den));   // 8.8 fixed point, round half up: 0..65280
        if constexpr (sizeof(T) == 1) o[(size_t)c * HW] = (unsigned char)((q + 128) >> 8);
        else o[(size_t)c * HW] = (float)q * (1.0f / 256.0f);
    }
}

// the most source samples under any tile of `tile` outputs along one axis
int tri_extent(int n, int N, int tile) {
    const int m2 = 2 * std::max(n, N);
    int most = 0;
    for (int i0 = 0; i0 < N; i0 += tile)
        most = std::max(most, tri_hi(std::min(i0 + tile, N) - 1, n, N, m2) - tri_lo(i0, n, N, m2) + 1);
    return most;
}

template <int LAYOUT, typename T>
void import_launch(const ImportSrc& s, int bgr, const YuvRule& rule, int filter, int F, int h, int w, T* dst, int H, int W,
                   hipStream_t st) {
    if (H == h && W == w) {
        constexpr int V = 16 / (int)sizeof(T);
        const unsigned G = (unsigned)((w + V - 1) / V + 1);                        // the head and at most ceil(w / V) groups behind it
        const unsigned items = (unsigned)((size_t)F * h * G);                      // <= 2 F h w <= 2^31: checked by the caller
        hipLaunchKernelGGL((import_stream_kernel<LAYOUT, T>), dim3((items + IMPORT_THREADS - 1) / IMPORT_THREADS), dim3(IMPORT_THREADS),
                           0, st, s, bgr, rule, h, w, G, items, dst);
    } else if (filter == PIPS_FILTER_TRIANGLE) {
        // the tallest tile whose row sums and staged rows fit TRI_LDS_MAX: 8 rows up to a ratio of about 12, 6 at 16 x 16
        const int CW = tri_extent(w, W, TRI_TW);
        int TH = TRI_TH, R = 0;
        size_t lds = 0;
        for (; TH >= 1; --TH) {
            R = tri_extent(h, H, TH);
            lds = ((size_t)3 * R * TRI_TW + (size_t)(IMPORT_THREADS / TRI_TW) * CW) * sizeof(int);
            if (lds <= (size_t)TRI_LDS_MAX) break;
        }
        const unsigned tiles_x = (unsigned)((W + TRI_TW - 1) / TRI_TW), tiles_y = (unsigned)((H + TH - 1) / TH);
        hipLaunchKernelGGL((import_triangle_kernel<LAYOUT, T>), dim3((unsigned)F * tiles_x * tiles_y), dim3(IMPORT_THREADS), lds, st, s,
                           bgr, rule, h, w, dst, H, W, TH, tiles_x, tiles_y, R, CW);
    } else {
        const unsigned total = (unsigned)((size_t)F * H * W);
        const float sh = (float)h / (float)H, sw = (float)w / (float)W;
        hipLaunchKernelGGL((import_resize_kernel<LAYOUT, T>), dim3((total + IMPORT_THREADS - 1) / IMPORT_THREADS), dim3(IMPORT_THREADS),
                           0, st, s, bgr, rule, h, w, dst, H, W, sh, sw, total);
    }
}

}  // namespace

int launch_frames_import(int format, int matrix, int range, int filter, int F, int h, int w, const void* const* p, const size_t* pitch,
                         const size_t* step, void* dst, int dst_u8, int H, int W, hipStream_t st) {
    ImportSrc s;
    for (int k = 0; k < 3; ++k) s.p[k] = (const unsigned char*)p[k], s.pitch[k] = pitch[k], s.step[k] = step[k];
    const bool yuv8 = format == PIPS_FMT_NV12 || format == PIPS_FMT_I420, yuv10 = format == PIPS_FMT_P010 || format == PIPS_FMT_I010;
    const YuvRule rule = yuv8 ? YUV_RULES[matrix][range] : yuv10 ? YUV10_RULES[matrix][range] : YuvRule{0, 0, 0, 0, 0, 0};
    const int bgr = format == PIPS_FMT_BGR24 || format == PIPS_FMT_BGRA32;
    const int layout = format == PIPS_FMT_NV12 ? LAYOUT_NV12 : format == PIPS_FMT_I420 ? LAYOUT_I420
                     : format == PIPS_FMT_P010 ? LAYOUT_P010 : format == PIPS_FMT_I010 ? LAYOUT_I010
                     : (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? LAYOUT_PACKED4 : LAYOUT_PACKED3;
#define PIPS_IMPORT_CASE(L)                                                                                        \
    case L:                                                                                                        \
        if (dst_u8) import_launch<L, unsigned char>(s, bgr, rule, filter, F, h, w, (unsigned char*)dst, H, W, st); \
        else import_launch<L, float>(s, bgr, rule, filter, F, h, w, (float*)dst, H, W, st);                        \
        break;
    switch (layout) {
        PIPS_IMPORT_CASE(LAYOUT_PACKED3)
        PIPS_IMPORT_CASE(LAYOUT_PACKED4)
        PIPS_IMPORT_CASE(LAYOUT_NV12)
        PIPS_IMPORT_CASE(LAYOUT_I420)
        PIPS_IMPORT_CASE(LAYOUT_P010)
        default:
        PIPS_IMPORT_CASE(LAYOUT_I010)
    }
#undef PIPS_IMPORT_CASE
    PIPS_CHECK_LAUNCH("frames_import");
    return PIPS_OK;
}

}  // namespace pips
