// Object masks (pips_object_masks, pips_masks_tint; drivers.object_masks, drivers.tint_masks): a label per pixel from a label per
// track -- every pixel takes the label that the nearest tracks within a radius vote for -- and that label plane shown on
// caller-owned surfaces, a colour and an opacity per (frame, label) blended in place.
// Both rules (include/pips_hip.h) are integer arithmetic behind draw's quantisation of the positions (draw_quant.h), so the bytes
// are drivers.object_masks_torch's and drivers.tint_masks_torch's.  Plain HIP.  Masks: mask_prepare_kernel writes one 8-byte record
// per (frame, column) into the workspace, mask_raster_kernel owns a 32 x 32 tile of one frame, compacts the records within reach of
// the tile in column order (draw_raster_kernel's ballot and prefix) and keeps the `vote` smallest keys of its four pixels in
// registers.  Tint: one launch per TINT_ALPHAS / C frames, a block per 64 x 32 tile; the (opacity, colour) table of the frame is
// converted into LDS by the block.  No atomics; a sample is owned by one thread.  Nothing outside the w x h image is written.
#include "common.h"
#include "draw_quant.h"
#include "yuv.h"

namespace pips {

namespace {

constexpr int MASK_THREADS = 256;
constexpr int MASK_TILE = 32;                                   // pixels a side; a thread owns four neighbours of a row: one dword
enum { TINT_PACKED3 = 0, TINT_PACKED4 = 1, TINT_NV12 = 2, TINT_I420 = 3, TINT_PLANAR8 = 4 };
constexpr int TINT_TILE_W = 64, TINT_TILE_H = 32;               // a thread owns 4 x 2 pixels and their two chroma samples

// ------------------------------------------------------------------------------------------------------------------ prepare
// One thread per (frame, column): the record (Qx, Qy * 256 + label) of a column that takes part, (DRAW_ABSENT, 0) of one that
// does not -- an absent point or the label PIPS_MASK_NONE.  |Q| < 2^19, so Qy * 256 + label stays inside int32.
__global__ __launch_bounds__(MASK_THREADS) void mask_prepare_kernel(const float* __restrict__ trajs, const unsigned char* __restrict__ labels,
                                                                    int n, int first, int f_base, int scale_x, int scale_y, float sx,
                                                                    float sy, int2* __restrict__ recs) {
    const int i = (int)(blockIdx.x * (unsigned)MASK_THREADS + threadIdx.x);
    if (i >= n) return;
    const int f = f_base + (int)blockIdx.y;
    const size_t at = (size_t)(first + f) * n + i;
    int qx = quantise(trajs[2 * at], scale_x != 0, sx);
    int qy = quantise(trajs[2 * at + 1], scale_y != 0, sy);
    const int label = labels[at];
    if (qy == DRAW_ABSENT || label == PIPS_MASK_NONE) qx = DRAW_ABSENT;
    recs[(size_t)f * n + i] = qx == DRAW_ABSENT ? make_int2(DRAW_ABSENT, 0) : make_int2(qx, qy * 256 + label);
}

// ------------------------------------------------------------------------------------------------------------------- raster
// the label that the keys k[0] <= k[1] <= ... vote for (a free slot holds LLONG_MAX): the most frequent low byte, among equals the
// one met first, PIPS_MASK_NONE when no slot is taken
template <int VOTE>
__device__ __forceinline__ int mask_vote(const long long (&k)[VOTE]) {
    int best = PIPS_MASK_NONE, most = 0;
#pragma unroll
    for (int j = 0; j < VOTE; ++j) {
        const int lj = (int)(k[j] & 255);
        int c = 0;
#pragma unroll
        for (int i = 0; i < VOTE; ++i) c += (k[i] != LLONG_MAX && (int)(k[i] & 255) == lj) ? 1 : 0;
        if (k[j] != LLONG_MAX && c > most) best = lj, most = c;
    }
    return best;
}

// One block per 32 x 32 tile of one frame; thread t owns the pixels x .. x + 3 of row Y0 + t / 8, x = X0 + 4 (t % 8).  The records
// are walked 256 at a time: thread j tests record j against the tile grown by the radius (a record that takes no part fails it),
// a ballot per wave and a prefix over the four waves compact the hits, in column order, into an LDS list of (Qx, Qy, column * 256 +
// label), and every thread walks that list -- every lane reads the same entry, one broadcast -- for its four pixels.  VOTE == 1
// keeps the smallest d2 and its label (the list is in column order: a strict comparison keeps the lower column); otherwise the
// VOTE smallest keys d2 << 24 | column << 8 | label stay sorted in registers.  The record of the next chunk is loaded ahead of the
// barriers of this one.
template <int VOTE>
__global__ __launch_bounds__(MASK_THREADS) void mask_raster_kernel(const int2* __restrict__ recs, int n, int h, int w, int radius8,
                                                                   unsigned char* __restrict__ mask, size_t pitch, size_t step,
                                                                   int tiles_x, int f_base) {
    __shared__ int4 list[MASK_THREADS];
    __shared__ int wave_hits[MASK_THREADS / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = f_base + (int)blockIdx.y;
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * MASK_TILE, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * MASK_TILE;
    const int x = X0 + 4 * (tid & 7), y = Y0 + (tid >> 3);
    // the positions within reach of a pixel of the tile that lies inside the image
    const int lox = 8 * X0 - radius8, hix = 8 * min(X0 + MASK_TILE - 1, w - 1) + radius8;
    const int loy = 8 * Y0 - radius8, hiy = 8 * min(Y0 + MASK_TILE - 1, h - 1) + radius8;
    const int r2 = radius8 * radius8;
    const int2* rec_f = recs + (size_t)f * n;

    long long key[4][VOTE];                                     // VOTE == 1: the smallest d2 in the high half, its label in the low byte
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int j = 0; j < VOTE; ++j) key[p][j] = LLONG_MAX;

    int2 next = tid < n ? rec_f[tid] : make_int2(DRAW_ABSENT, 0);
    for (int base = 0; base < n; base += MASK_THREADS) {
        const int2 cur = next;
        const int mine = base + tid, ahead = mine + MASK_THREADS;
        next = ahead < n ? rec_f[ahead] : make_int2(DRAW_ABSENT, 0);
        const int qy = cur.y >> 8;                              // (the arithmetic shift: floor)
        const bool hit = cur.x >= lox && cur.x <= hix && qy >= loy && qy <= hiy;
        const unsigned long long votes = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < MASK_THREADS / 64; ++v) {
            const int cnt = wave_hits[v];
            before += v < wave ? cnt : 0, total += cnt;
        }
        if (hit) list[before + __popcll(votes & ((1ull << lane) - 1ull))] = make_int4(cur.x, qy, mine * 256 + (cur.y & 255), 0);
        __syncthreads();
        for (int e = 0; e < total; ++e) {
            const int4 c = list[e];
            const int dy = 8 * y - c.y;
            if (abs(dy) > radius8) continue;
            const int dy2 = dy * dy;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int dx = 8 * (x + p) - c.x;               // |dx|, |dy| <= 8 * 31 + 2048: the sum of squares stays below 2^24
                const int d2 = dx * dx + dy2;
                if (d2 > r2) continue;
                if constexpr (VOTE == 1) {
                    if (d2 < (int)(key[p][0] >> 32)) key[p][0] = (long long)d2 << 32 | (c.z & 255);
                } else {
                    long long k = (long long)d2 << 24 | c.z;
#pragma unroll
                    for (int j = 0; j < VOTE; ++j) {
                        const long long lo = min(k, key[p][j]);
                        k = max(k, key[p][j]), key[p][j] = lo;
                    }
                }
            }
        }
    }
    if (y >= h || x >= w) return;
    unsigned out = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) out |= (unsigned)mask_vote<VOTE>(key[p]) << (8 * p);
    unsigned char* q = mask + (size_t)f * step + (size_t)y * pitch + x;
    if (x + 3 < w && ((uintptr_t)q & 3) == 0) {
        *(unsigned*)q = out;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (x + p < w) q[p] = (unsigned char)(out >> (8 * p));
    }
}

// --------------------------------------------------------------------------------------------------------------------- tint
// frame f, row y of plane k starts at p[k] + f step[k] + y pitch[k]
struct TintDst {
    unsigned char* p[3];
    size_t pitch[3], step[3];
};

// the opacities of the frames of one launch by value: entry k C + l is alpha[f_base + k][l]
struct TintAlpha {
    unsigned short a[TINT_ALPHAS];
};

__device__ __forceinline__ unsigned char* tint_row(const TintDst& d, int k, int f, int y) {
    return d.p[k] + (size_t)f * d.step[k] + (size_t)y * d.pitch[k];
}

// the first nb <= 4 bytes at p, little-endian, the others zero: one dword where p allows it
__device__ __forceinline__ unsigned load_n(const unsigned char* p, int nb) {
    if (nb == 4 && ((uintptr_t)p & 3) == 0) return *(const unsigned*)p;
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < nb) v |= (unsigned)p[b] << (8 * b);
    return v;
}

// v over old = load_n(p, nb): nothing when they are equal, one dword where p allows it, the bytes that differ otherwise
__device__ __forceinline__ void store_n(unsigned char* p, unsigned v, unsigned old, int nb) {
    if (v == old) return;
    if (nb == 4 && ((uintptr_t)p & 3) == 0) {
        *(unsigned*)p = v;
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < nb && ((v ^ old) >> (8 * b) & 255u) != 0) p[b] = (unsigned char)(v >> (8 * b));
}

__device__ __forceinline__ int tint_blend(int p, int c, int A) { return (p * (256 - A) + c * A + 128) >> 8; }

// byte b of `old` blended towards component (col >> shift) with opacity A, back in its place
__device__ __forceinline__ unsigned tint_byte(unsigned old, int b, int col, int shift, int A) {
    const int p = (int)(old >> (8 * b) & 255u);
    return (unsigned)(A != 0 ? tint_blend(p, (col >> shift) & 255, A) : p) << (8 * b);
}

// One block per 64 x 32 tile of one frame; thread t owns the pixels x .. x + 3 of the rows y and y + 1, x = X0 + 4 (t % 16),
// y = Y0 + 2 (t / 16), and the two 4:2:0 chroma samples above them.  Thread l < 256 first writes entry l of the frame's table into
// LDS: the opacity alpha[f][l] and the colour in the surface's components for l < C, opacity 0 otherwise (PIPS_MASK_NONE is such a
// label).  A thread whose eight pixels all have opacity 0 reads and writes no surface byte; a group of four bytes that the blend
// leaves as it was is not written.
template <int LAYOUT>
__global__ __launch_bounds__(MASK_THREADS) void masks_tint_kernel(TintDst d, int bgr, int h, int w, const unsigned char* __restrict__ mask,
                                                                  size_t mpitch, size_t mstep, const unsigned char* __restrict__ colors,
                                                                  int C, RgbRule rule, int tiles_x, int f_base, TintAlpha alphas) {
    constexpr bool YUV = LAYOUT == TINT_NV12 || LAYOUT == TINT_I420;
    __shared__ int tab_a[256], tab_c[256];
    const int tid = (int)threadIdx.x;
    const int f = f_base + (int)blockIdx.y;
    {
        int A = 0, col = 0;
        if (tid < C) {
            A = alphas.a[(int)blockIdx.y * C + tid];
            const unsigned char* rgb = colors + ((size_t)f * C + tid) * 3;
            int c0 = rgb[0], c1 = rgb[1], c2 = rgb[2];
            if constexpr (YUV) rgb_to_yuv(rule, rgb[0], rgb[1], rgb[2], c0, c1, c2);
            col = c0 | c1 << 8 | c2 << 16;
        }
        tab_a[tid] = A, tab_c[tid] = col;
    }
    __syncthreads();
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * TINT_TILE_W, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * TINT_TILE_H;
    const int x = X0 + 4 * (tid & 15), y = Y0 + 2 * (tid >> 4);
    if (x >= w || y >= h) return;
    const int nx = min(4, w - x), ny = min(2, h - y);
    int A[2][4], col[2][4], any = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned m = j < ny ? load_n(mask + (size_t)f * mstep + (size_t)(y + j) * mpitch + x, nx) : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = (int)(m >> (8 * i) & 255u);
            A[j][i] = (j < ny && i < nx) ? tab_a[l] : 0;
            col[j][i] = tab_c[l];
            any |= A[j][i];
        }
    }
    if (any == 0) return;

    if constexpr (LAYOUT == TINT_PACKED4) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (A[j][i] == 0) continue;
                unsigned char* q = tint_row(d, 0, f, y + j) + 4 * (size_t)(x + i);
                const unsigned old = load_n(q, 3);
                const unsigned v = tint_byte(old, bgr ? 2 : 0, col[j][i], 0, A[j][i]) | tint_byte(old, 1, col[j][i], 8, A[j][i]) |
                                   tint_byte(old, bgr ? 0 : 2, col[j][i], 16, A[j][i]);
                store_n(q, v, old, 3);                          // (three bytes: the alpha byte is never written)
            }
    } else if constexpr (LAYOUT == TINT_PACKED3) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j >= ny) continue;
            unsigned char* q = tint_row(d, 0, f, y + j) + 3 * (size_t)x;
            unsigned old[3], v[3] = {0u, 0u, 0u};
#pragma unroll
            for (int g = 0; g < 3; ++g) old[g] = load_n(q + 4 * g, min(max(3 * nx - 4 * g, 0), 4));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {                   // byte k of pixel i: component k of R G B, or of B G R
                    const int at = 3 * i + k;
                    v[at >> 2] |= tint_byte(old[at >> 2], at & 3, col[j][i], 8 * (bgr ? 2 - k : k), A[j][i]);
                }
#pragma unroll
            for (int g = 0; g < 3; ++g) store_n(q + 4 * g, v[g], old[g], min(max(3 * nx - 4 * g, 0), 4));
        }
    } else {
        // full-resolution planes: Y alone, or R, G and B
#pragma unroll
        for (int k = 0; k < (YUV ? 1 : 3); ++k)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= ny) continue;
                unsigned char* q = tint_row(d, k, f, y + j) + x;
                const unsigned old = load_n(q, nx);
                unsigned v = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) v |= tint_byte(old, i, col[j][i], 8 * k, A[j][i]);
                store_n(q, v, old, nx);
            }
    }
    if constexpr (YUV) {
        // sample s of the thread covers the pixels 2 s and 2 s + 1 of both rows; those outside the image have opacity 0
        const int ns = (nx + 1) >> 1;
        int SA[2], Sb[2], Sr[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            SA[s] = Sb[s] = Sr[s] = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 2 * s; i < 2 * s + 2; ++i)
                    SA[s] += A[j][i], Sb[s] += ((col[j][i] >> 8) & 255) * A[j][i], Sr[s] += ((col[j][i] >> 16) & 255) * A[j][i];
        }
        const auto blend = [](unsigned old, int b, int SAs, int Ss) -> unsigned {
            const int p = (int)(old >> (8 * b) & 255u);
            return (unsigned)(SAs != 0 ? (p * (1024 - SAs) + Ss + 512) >> 10 : p) << (8 * b);
        };
        if constexpr (LAYOUT == TINT_NV12) {
            unsigned char* q = tint_row(d, 1, f, y >> 1) + 2 * (size_t)(x >> 1);
            const unsigned old = load_n(q, 2 * ns);
            unsigned v = blend(old, 0, SA[0], Sb[0]) | blend(old, 1, SA[0], Sr[0]);
            if (ns > 1) v |= blend(old, 2, SA[1], Sb[1]) | blend(old, 3, SA[1], Sr[1]);
            store_n(q, v, old, 2 * ns);
        } else {
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                unsigned char* q = tint_row(d, k, f, y >> 1) + (x >> 1);
                const unsigned old = load_n(q, ns);
                unsigned v = blend(old, 0, SA[0], k == 1 ? Sb[0] : Sr[0]);
                if (ns > 1) v |= blend(old, 1, SA[1], k == 1 ? Sb[1] : Sr[1]);
                store_n(q, v, old, ns);
            }
        }
    }
}

}  // namespace

int launch_object_masks(const float* trajs, const unsigned char* labels, int n, int first, int F, int src_h, int src_w, int h, int w,
                        int radius8, int vote, unsigned char* mask, size_t pitch, size_t step, void* workspace, hipStream_t st) {
    const float sx = (float)w / (float)src_w, sy = (float)h / (float)src_h;
    const int tiles_x = (w + MASK_TILE - 1) / MASK_TILE, tiles_y = (h + MASK_TILE - 1) / MASK_TILE;     // <= 256 each
    int2* recs = (int2*)workspace;
    constexpr int FRAMES_A_LAUNCH = 65535;                     // the grid's y
    for (int f0 = 0; f0 < F; f0 += FRAMES_A_LAUNCH) {
        const unsigned fc = (unsigned)std::min(F - f0, FRAMES_A_LAUNCH);
        if (n > 0)
            hipLaunchKernelGGL(mask_prepare_kernel, dim3((unsigned)((n + MASK_THREADS - 1) / MASK_THREADS), fc), dim3(MASK_THREADS), 0, st,
                               trajs, labels, n, first, f0, src_w != w, src_h != h, sx, sy, recs);
        const dim3 grid((unsigned)(tiles_x * tiles_y), fc);
#define PIPS_MASK_CASE(V)                                                                                                                \
    case V:                                                                                                                              \
        hipLaunchKernelGGL(mask_raster_kernel<V>, grid, dim3(MASK_THREADS), 0, st, (const int2*)recs, n, h, w, radius8, mask, pitch,     \
                           step, tiles_x, f0);                                                                                           \
        break
        switch (vote) {
            PIPS_MASK_CASE(1);
            PIPS_MASK_CASE(2);
            PIPS_MASK_CASE(3);
            PIPS_MASK_CASE(4);
            default:
                PIPS_MASK_CASE(5);
        }
#undef PIPS_MASK_CASE
    }
    PIPS_CHECK_LAUNCH("object_masks");
    return PIPS_OK;
}

int launch_masks_tint(int format, int matrix, int range, int F, int h, int w, void* const* p, const size_t* pitch, const size_t* step,
                      const unsigned char* mask, size_t mpitch, size_t mstep, const unsigned char* colors, const int* alpha, int C,
                      hipStream_t st) {
    TintDst d;
    for (int k = 0; k < 3; ++k) d.p[k] = (unsigned char*)p[k], d.pitch[k] = pitch[k], d.step[k] = step[k];
    const bool yuv = format == PIPS_FMT_NV12 || format == PIPS_FMT_I420;
    const RgbRule rule = yuv ? RGB_RULES[matrix][range] : RgbRule{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int bgr = format == PIPS_FMT_BGR24 || format == PIPS_FMT_BGRA32;
    const int tiles_x = (w + TINT_TILE_W - 1) / TINT_TILE_W, tiles_y = (h + TINT_TILE_H - 1) / TINT_TILE_H;
    const int frames_a_launch = TINT_ALPHAS / C;               // >= 4: C <= 255
    TintAlpha table;
    for (int f0 = 0; f0 < F; f0 += frames_a_launch) {
        const int fc = std::min(F - f0, frames_a_launch);
        for (int k = 0; k < fc * C; ++k) table.a[k] = (unsigned short)alpha[(size_t)f0 * C + k];
        for (int k = fc * C; k < TINT_ALPHAS; ++k) table.a[k] = 0;
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)fc);
#define PIPS_TINT_CASE(L)                                                                                                                \
    hipLaunchKernelGGL(masks_tint_kernel<L>, grid, dim3(MASK_THREADS), 0, st, d, bgr, h, w, mask, mpitch, mstep, colors, C, rule,        \
                       tiles_x, f0, table)
        switch (format) {
            case PIPS_FMT_RGB24:
            case PIPS_FMT_BGR24: PIPS_TINT_CASE(TINT_PACKED3); break;
            case PIPS_FMT_RGBA32:
            case PIPS_FMT_BGRA32: PIPS_TINT_CASE(TINT_PACKED4); break;
            case PIPS_FMT_NV12: PIPS_TINT_CASE(TINT_NV12); break;
            case PIPS_FMT_I420: PIPS_TINT_CASE(TINT_I420); break;
            default: PIPS_TINT_CASE(TINT_PLANAR8); break;
        }
#undef PIPS_TINT_CASE
    }
    PIPS_CHECK_LAUNCH("masks_tint");
    return PIPS_OK;
}

}  // namespace pips
