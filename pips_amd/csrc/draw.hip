// Tracks out (pips_tracks_draw, pips_tracks_draw_ex; drivers.draw_tracks, drivers.TrackPainter): the trails of n tracks drawn into F
// caller-owned surfaces in place -- packed RGB / BGR / RGBA / BGRA, NV12, I420 or planar RGB, and through the _ex entry the 16-bit
// P010 and I010, with any base address, row pitch and frame step.
// The rule (include/pips_hip.h; yuv.h for the RGB -> YCbCr constants) is integer arithmetic behind the quantisation of the
// positions, so the bytes are drivers.draw_tracks_torch's.  Plain HIP, two launches: draw_prepare_kernel writes one record per
// (frame, track) into the workspace, draw_raster_kernel blends the records into the tiles they touch (its DrawFade form when the
// _ex entry has a fade table: the same body with a factor per subsample in place of the coverage mask).  No atomics: a pixel is
// owned by one thread, which applies the tracks in column order.  Nothing outside the w x h image of a plane is written.
#include "common.h"
#include "draw_quant.h"
#include "fp_rn.h"
#include "yuv.h"

namespace pips {

namespace {

constexpr int DRAW_THREADS = 256;
constexpr int DRAW_TILE = 16;                                   // pixels a side: 256 pixels, 8 x 8 chroma samples
enum { DRAW_PACKED3 = 0, DRAW_PACKED4 = 1, DRAW_NV12 = 2, DRAW_I420 = 3, DRAW_PLANAR8 = 4, DRAW_P010 = 5, DRAW_I010 = 6 };
// The workspace: first the boxes, one int4 per (frame, track) = x0, y0, x1, y1 of the pixels it can touch (inclusive; x0 > x1:
// none) -- every tile of a frame reads all of them, 16 bytes a lane -- then the records of DRAW_REC_INTS + 2 (trail + 1) ints:
// [0] the opacity A, [1] the colour c0 | c1 << 8 | c2 << 16 (R G B, or Y Cb Cr for the YCbCr surfaces; three 10-bit fields
// c0 | c1 << 10 | c2 << 20 for P010 and I010), [2] bit j - 1 set when the segment from point j - 1 to point j is drawn, [3] 1 when
// the head's disc is drawn; then the points (x, y) in eighths, point `trail` the head
constexpr int DRAW_REC_INTS = DRAW_HEAD_INTS - 4;
enum { DH_ALPHA = 0, DH_COLOR = 1, DH_SEGS = 2, DH_HEAD = 3 };
__host__ __device__ __forceinline__ size_t draw_rec_ints(int trail) { return draw_track_ints(trail) - 4; }

// frame f, row y of plane k starts at p[k] + f step[k] + y pitch[k]
struct DrawDst {
    unsigned char* p[3];
    size_t pitch[3], step[3];
};

// pips_tracks_draw_ex's table by value: f[a] the factor 0..256 of the capsule of age a
struct DrawFade {
    unsigned short f[PIPS_DRAW_TRAIL_MAX];
};

__device__ __forceinline__ unsigned char* dst_row(const DrawDst& d, int k, int f, int y) {
    return d.p[k] + (size_t)f * d.step[k] + (size_t)y * d.pitch[k];
}

// the same row of a 16-bit plane (pointer, pitch and step are even)
__device__ __forceinline__ unsigned short* dst_row16(const DrawDst& d, int k, int f, int y) {
    return (unsigned short*)dst_row(d, k, f, y);
}

// (quantise and DRAW_ABSENT: draw_quant.h)
// ------------------------------------------------------------------------------------------------------------------ prepare
// One thread per (frame, track): the trail + 1 points of rows r - trail .. r quantised, the segments that are drawn, the box of
// pixels with a subsample within the larger radius of a drawn end (clipped to the image), the opacity and the converted colour.
// yuv: 0 the colour stays R G B, 1 the 8-bit rule, 2 rule10.  dead: bit a set when the fade factor of age a is 0 -- such a capsule
// draws nothing, so it is not among the record's segments and not in the box.
__global__ __launch_bounds__(DRAW_THREADS) void draw_prepare_kernel(const float* __restrict__ trajs, const float* __restrict__ vis, int n,
                                                                    int first, int f_base, int h, int w, int scale_x, int scale_y,
                                                                    float sx, float sy, const unsigned char* __restrict__ colors,
                                                                    int yuv, RgbRule rule, Rgb10Rule rule10, unsigned dead, DrawStyle st,
                                                                    int4* __restrict__ boxes, int* __restrict__ recs) {
    const int i = (int)(blockIdx.x * (unsigned)DRAW_THREADS + threadIdx.x);
    if (i >= n) return;
    const int f = f_base + (int)blockIdx.y, r = first + f;
    int* rec = recs + ((size_t)f * n + i) * draw_rec_ints(st.trail);
    int* pts = rec + DRAW_REC_INTS;
    int px = DRAW_ABSENT, py = 0;                               // the point before
    int lox = INT_MAX, loy = INT_MAX, hix = INT_MIN, hiy = INT_MIN;
    unsigned segs = 0;
    for (int j = 0; j <= st.trail; ++j) {
        const int g = r - st.trail + j;
        int qx = DRAW_ABSENT, qy = 0;
        if (g >= 0) {
            const float* xy = trajs + ((size_t)g * n + i) * 2;
            qx = quantise(xy[0], scale_x != 0, sx);
            qy = quantise(xy[1], scale_y != 0, sy);
            if (qy == DRAW_ABSENT) qx = DRAW_ABSENT;
            if (qx == DRAW_ABSENT) qy = 0;
        }
        pts[2 * j] = qx, pts[2 * j + 1] = qy;
        // (the segment that ends on point j has age trail - j)
        if (j > 0 && st.line8 >= 0 && qx != DRAW_ABSENT && px != DRAW_ABSENT && abs(qx - px) <= PIPS_DRAW_JUMP8_MAX &&
            abs(qy - py) <= PIPS_DRAW_JUMP8_MAX && !((dead >> (st.trail - j)) & 1u)) {
            segs |= 1u << (j - 1);
            lox = min(lox, min(px, qx)), hix = max(hix, max(px, qx));
            loy = min(loy, min(py, qy)), hiy = max(hiy, max(py, qy));
        }
        px = qx, py = qy;
    }
    const bool head = px != DRAW_ABSENT;                        // (px, py) is the head now
    const int alpha = (vis == nullptr || vis[(size_t)r * n + i] > st.vis_logit) ? st.alpha_vis : st.alpha_occ;
    const bool disc = head && st.dot8 >= 0;
    if (!head) segs = 0;
    if (disc) lox = min(lox, px), hix = max(hix, px), loy = min(loy, py), hiy = max(hiy, py);
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    if ((disc || segs != 0) && alpha != 0) {
        // pixel x has subsamples at 8 x - 2 and 8 x + 2; >> is the arithmetic shift (floor)
        const int grow = max(st.line8, st.dot8) + 2;
        x0 = max(0, (lox - grow + 7) >> 3), x1 = min(w - 1, (hix + grow) >> 3);
        y0 = max(0, (loy - grow + 7) >> 3), y1 = min(h - 1, (hiy + grow) >> 3);
    }
    const int R = colors[3 * (size_t)i], G = colors[3 * (size_t)i + 1], B = colors[3 * (size_t)i + 2];
    int c0 = R, c1 = G, c2 = B;
    if (yuv == 1) rgb_to_yuv(rule, R, G, B, c0, c1, c2);
    if (yuv == 2) rgb_to_yuv10(rule10, R, G, B, c0, c1, c2);
    boxes[(size_t)f * n + i] = make_int4(x0, y0, x1, y1);
    rec[DH_ALPHA] = alpha, rec[DH_COLOR] = yuv == 2 ? (c0 | c1 << 10 | c2 << 20) : (c0 | c1 << 8 | c2 << 16), rec[DH_SEGS] = (int)segs,
    rec[DH_HEAD] = disc ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- raster
// The subsamples of the pixel centred at (cx, cy) (eighths) that lie inside the capsule of radius R around P0 P1 (a disc when P0 ==
// P1), as a 4-bit mask.  A pixel with no subsample in the ends' box grown by R is skipped; for the others |c - P0| <= 2047 + R + 4 a
// component (PIPS_DRAW_JUMP8_MAX, PIPS_DRAW_RADIUS8_MAX), so a . b, b . b and the cross product stay below 2^24 in int32; only the
// cross product's square (< 2^47) against R^2 L is taken in int64.
__device__ __forceinline__ unsigned capsule_mask(int p0x, int p0y, int p1x, int p1y, int R, int cx, int cy) {
    const int grow = R + 2;
    if (cx < min(p0x, p1x) - grow || cx > max(p0x, p1x) + grow || cy < min(p0y, p1y) - grow || cy > max(p0y, p1y) + grow) return 0u;
    const int ax = p1x - p0x, ay = p1y - p0y, L = ax * ax + ay * ay, R2 = R * R;
    const long long R2L = (long long)R2 * (long long)L;
    unsigned mask = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int qx = cx + ((s & 1) ? 2 : -2), qy = cy + ((s & 2) ? 2 : -2);
        const int bx = qx - p0x, by = qy - p0y, t = ax * bx + ay * by;
        bool in;
        if (L == 0 || t <= 0) {
            in = bx * bx + by * by <= R2;
        } else if (t >= L) {
            const int dx = qx - p1x, dy = qy - p1y;
            in = dx * dx + dy * dy <= R2;
        } else {
            const long long cr = (long long)(ax * by - ay * bx);
            in = cr * cr <= R2L;
        }
        mask |= in ? 1u << s : 0u;
    }
    return mask;
}

// One block per 16 x 16 tile of one frame; a 2 x 2 pixel quad is four neighbouring lanes, lane 0 of a quad owns its chroma sample.
// The tracks are walked 256 at a time: thread j tests the box of track j against the tile, a ballot per wave and a prefix over
// the four waves compact the hits, in column order, into an LDS list, and every thread walks that list for its pixel -- the union
// of the track's primitives on four subsamples, the sum over the quad by two lane exchanges, the blend in registers.  The pixel is
// loaded when the first list is not empty and stored when a track changed it.
// FADE: the pixel keeps a factor 0..256 per subsample, the largest among the primitives that hold it (the head's disc: 256), in
// place of the mask; the segments are walked youngest first, so that a table that does not grow with age ends the walk as soon as
// all four stand at 256.  The table is the one trailing argument `fade` (a DrawFade; the form without it is the plain kernel, with
// pips_tracks_draw's arguments and instructions); the block stages it in LDS ahead of its first barrier.
// The 16-bit layouts: a sample is a word whose 10-bit value lies in the high (P010) or low (I010) bits; a touched word is written
// back with the other six bits zero, every other word is not written.
template <int LAYOUT, typename... Fade>
__global__ __launch_bounds__(DRAW_THREADS) void draw_raster_kernel(DrawDst d, int bgr, int h, int w, int n, int trail, int line8, int dot8,
                                                                   const int4* __restrict__ boxes, const int* __restrict__ recs,
                                                                   int tiles_x, int f_base, Fade... fade) {
    constexpr bool FADE = sizeof...(Fade) != 0;
    constexpr bool WIDE = LAYOUT == DRAW_P010 || LAYOUT == DRAW_I010;
    constexpr bool YUV = LAYOUT == DRAW_NV12 || LAYOUT == DRAW_I420 || WIDE;
    constexpr int BPP = LAYOUT == DRAW_PACKED3 ? 3 : 4;
    constexpr int CBITS = WIDE ? 10 : 8, CMASK = (1 << CBITS) - 1;  // a field of the record's colour word
    constexpr int VSHIFT = LAYOUT == DRAW_P010 ? 6 : 0;            // where the value lies in a 16-bit word
    __shared__ int list[DRAW_THREADS];
    __shared__ int wave_hits[DRAW_THREADS / 64];
    __shared__ int fade_s[FADE ? PIPS_DRAW_TRAIL_MAX : 1];
    if constexpr (FADE) {                                       // (static indices only: the argument stays in scalar registers)
        const DrawFade& table = (fade, ...);
        if (threadIdx.x < PIPS_DRAW_TRAIL_MAX) {
            int v = 0;
#pragma unroll
            for (int a = 0; a < PIPS_DRAW_TRAIL_MAX; ++a) v = (int)threadIdx.x == a ? (int)table.f[a] : v;
            fade_s[threadIdx.x] = v;
        }
    }
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = f_base + (int)blockIdx.y;
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * DRAW_TILE, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * DRAW_TILE;
    const int quad = tid >> 2, sub = tid & 3;
    const int x = X0 + 2 * (quad & 7) + (sub & 1), y = Y0 + 2 * (quad >> 3) + (sub >> 1);
    const bool inimg = x < w && y < h;
    const bool chroma = YUV && sub == 0 && inimg;               // the quad's sample exists when its first pixel does
    const int TX0 = 8 * X0 - 2, TY0 = 8 * Y0 - 2;                // the tile's first subsample; its last lies TSPAN further
    constexpr int TSPAN = 8 * (DRAW_TILE - 1) + 4;
    const size_t RI = draw_rec_ints(trail);
    const int4* box_f = boxes + (size_t)f * n;
    const int* rec_f = recs + (size_t)f * n * RI;

    int c[3] = {0, 0, 0}, cb = 0, cr = 0;
    bool loaded = false, touched = false, ctouched = false;
    for (int base = 0; base < n; base += DRAW_THREADS) {
        const int mine = base + tid;
        bool hit = false;
        if (mine < n) {
            const int4 b = box_f[mine];
            hit = b.z >= X0 && b.x < X0 + DRAW_TILE && b.w >= Y0 && b.y < Y0 + DRAW_TILE;
        }
        const unsigned long long votes = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < DRAW_THREADS / 64; ++v) {
            const int cnt = wave_hits[v];
            before += v < wave ? cnt : 0, total += cnt;
        }
        if (hit) list[before + __popcll(votes & ((1ull << lane) - 1ull))] = mine;
        __syncthreads();
        if (total == 0) continue;                               // (the same for every thread of the block)
        if (!loaded) {
            loaded = true;
            if (inimg) {
                if constexpr (LAYOUT == DRAW_PACKED3 || LAYOUT == DRAW_PACKED4) {
                    const unsigned char* q = dst_row(d, 0, f, y) + (size_t)x * BPP;
                    c[0] = q[bgr ? 2 : 0], c[1] = q[1], c[2] = q[bgr ? 0 : 2];
                } else if constexpr (LAYOUT == DRAW_PLANAR8) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] = dst_row(d, k, f, y)[x];
                } else if constexpr (WIDE) {
                    c[0] = (dst_row16(d, 0, f, y)[x] >> VSHIFT) & 1023;
                } else {
                    c[0] = dst_row(d, 0, f, y)[x];
                }
            }
            if (chroma) {
                if constexpr (LAYOUT == DRAW_NV12) {
                    const unsigned char* q = dst_row(d, 1, f, y >> 1) + 2 * (size_t)(x >> 1);
                    cb = q[0], cr = q[1];
                } else if constexpr (LAYOUT == DRAW_I420) {
                    cb = dst_row(d, 1, f, y >> 1)[x >> 1], cr = dst_row(d, 2, f, y >> 1)[x >> 1];
                } else if constexpr (LAYOUT == DRAW_P010) {
                    const unsigned short* q = dst_row16(d, 1, f, y >> 1) + 2 * (size_t)(x >> 1);
                    cb = q[0] >> 6, cr = q[1] >> 6;
                } else if constexpr (LAYOUT == DRAW_I010) {
                    cb = dst_row16(d, 1, f, y >> 1)[x >> 1] & 1023, cr = dst_row16(d, 2, f, y >> 1)[x >> 1] & 1023;
                }
            }
        }
        for (int e = 0; e < total; ++e) {
            const int ti = __builtin_amdgcn_readfirstlane(list[e]);
            const int* rec = rec_f + (size_t)ti * RI;
            const int4 b = box_f[ti];
            int k = 0;                                          // the pixel's coverage: 0..4 subsamples, 0..1024 with FADE
            if (inimg && x >= b.x && x <= b.z && y >= b.y && y <= b.w) {
                const int* pts = rec + DRAW_REC_INTS;
                unsigned mask = 0;
                if (rec[DH_HEAD]) mask = capsule_mask(pts[2 * trail], pts[2 * trail + 1], pts[2 * trail], pts[2 * trail + 1], dot8, 8 * x, 8 * y);
                if constexpr (!FADE) {
                    for (unsigned m = (unsigned)rec[DH_SEGS]; m != 0 && mask != 15u; m &= m - 1) {
                        const int j = __builtin_ctz(m);         // the segment from point j to point j + 1
                        const int p0x = pts[2 * j], p0y = pts[2 * j + 1], p1x = pts[2 * j + 2], p1y = pts[2 * j + 3];
                        // a segment that reaches no subsample of the tile (the same for every thread: decided once for the block)
                        if (max(p0x, p1x) + line8 < TX0 || min(p0x, p1x) - line8 > TX0 + TSPAN || max(p0y, p1y) + line8 < TY0 ||
                            min(p0y, p1y) - line8 > TY0 + TSPAN)
                            continue;
                        mask |= capsule_mask(p0x, p0y, p1x, p1y, line8, 8 * x, 8 * y);
                    }
                    k = __popc(mask);
                } else {
                    int phi[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) phi[s] = ((mask >> s) & 1u) ? 256 : 0;
                    // (a factor is at most 256: the four together have bit 8 set when all stand there)
                    for (unsigned m = (unsigned)rec[DH_SEGS]; m != 0 && ((phi[0] & phi[1] & phi[2] & phi[3]) & 256) == 0;) {
                        const int j = 31 - __builtin_clz(m);    // the youngest left: from point j to point j + 1, age trail - 1 - j
                        m &= ~(1u << j);
                        const int p0x = pts[2 * j], p0y = pts[2 * j + 1], p1x = pts[2 * j + 2], p1y = pts[2 * j + 3];
                        if (max(p0x, p1x) + line8 < TX0 || min(p0x, p1x) - line8 > TX0 + TSPAN || max(p0y, p1y) + line8 < TY0 ||
                            min(p0y, p1y) - line8 > TY0 + TSPAN)
                            continue;
                        const int fa = fade_s[trail - 1 - j];
                        const unsigned in = capsule_mask(p0x, p0y, p1x, p1y, line8, 8 * x, 8 * y);
#pragma unroll
                        for (int s = 0; s < 4; ++s) phi[s] = max(phi[s], ((in >> s) & 1u) ? fa : 0);
                    }
                    k = phi[0] + phi[1] + phi[2] + phi[3];
                }
            }
            const int A = rec[DH_ALPHA], col = rec[DH_COLOR];
            if constexpr (YUV) {
                int K = k + __shfl_xor(k, 1);
                K += __shfl_xor(K, 2);
                const int W = FADE ? (K * A + 128) >> 8 : K * A;
                if (chroma && W != 0) {
                    cb = (cb * (4096 - W) + ((col >> CBITS) & CMASK) * W + 2048) >> 12;
                    cr = (cr * (4096 - W) + ((col >> (2 * CBITS)) & CMASK) * W + 2048) >> 12;
                    ctouched = true;
                }
            }
            const int wgt = FADE ? (k * A + 128) >> 8 : k * A;
            if (wgt != 0) {
#pragma unroll
                for (int q = 0; q < (YUV ? 1 : 3); ++q) c[q] = (c[q] * (1024 - wgt) + ((col >> (CBITS * q)) & CMASK) * wgt + 512) >> 10;
                touched = true;
            }
        }
    }
    if (touched) {
        if constexpr (LAYOUT == DRAW_PACKED3 || LAYOUT == DRAW_PACKED4) {
            unsigned char* q = dst_row(d, 0, f, y) + (size_t)x * BPP;
            q[bgr ? 2 : 0] = (unsigned char)c[0], q[1] = (unsigned char)c[1], q[bgr ? 0 : 2] = (unsigned char)c[2];
        } else if constexpr (LAYOUT == DRAW_PLANAR8) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dst_row(d, k, f, y)[x] = (unsigned char)c[k];
        } else if constexpr (WIDE) {
            dst_row16(d, 0, f, y)[x] = (unsigned short)(c[0] << VSHIFT);
        } else {
            dst_row(d, 0, f, y)[x] = (unsigned char)c[0];
        }
    }
    if (ctouched) {
        if constexpr (LAYOUT == DRAW_NV12) {
            unsigned char* q = dst_row(d, 1, f, y >> 1) + 2 * (size_t)(x >> 1);
            q[0] = (unsigned char)cb, q[1] = (unsigned char)cr;
        } else if constexpr (LAYOUT == DRAW_I420) {
            dst_row(d, 1, f, y >> 1)[x >> 1] = (unsigned char)cb, dst_row(d, 2, f, y >> 1)[x >> 1] = (unsigned char)cr;
        } else if constexpr (LAYOUT == DRAW_P010) {
            unsigned short* q = dst_row16(d, 1, f, y >> 1) + 2 * (size_t)(x >> 1);
            q[0] = (unsigned short)(cb << 6), q[1] = (unsigned short)(cr << 6);
        } else if constexpr (LAYOUT == DRAW_I010) {
            dst_row16(d, 1, f, y >> 1)[x >> 1] = (unsigned short)cb, dst_row16(d, 2, f, y >> 1)[x >> 1] = (unsigned short)cr;
        }
    }
}

}  // namespace

int launch_tracks_draw(int format, int matrix, int range, int F, int h, int w, void* const* p, const size_t* pitch, const size_t* step,
                       const float* trajs, const float* vis, int n, int first, int src_h, int src_w, const unsigned char* colors,
                       const DrawStyle& style, const int* fade, int* workspace, hipStream_t st) {
    DrawDst d;
    for (int k = 0; k < 3; ++k) d.p[k] = (unsigned char*)p[k], d.pitch[k] = pitch[k], d.step[k] = step[k];
    const bool yuv8 = format == PIPS_FMT_NV12 || format == PIPS_FMT_I420, yuv10 = format == PIPS_FMT_P010 || format == PIPS_FMT_I010;
    const RgbRule rule = yuv8 ? RGB_RULES[matrix][range] : RgbRule{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const Rgb10Rule rule10 = yuv10 ? RGB10_RULES[matrix][range] : Rgb10Rule{0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int bgr = format == PIPS_FMT_BGR24 || format == PIPS_FMT_BGRA32;
    const float sx = (float)w / (float)src_w, sy = (float)h / (float)src_h;
    const int tiles_x = (w + DRAW_TILE - 1) / DRAW_TILE, tiles_y = (h + DRAW_TILE - 1) / DRAW_TILE;     // <= 512 each
    int4* boxes = (int4*)workspace;
    int* recs = workspace + 4 * (size_t)F * n;
    DrawFade table;
    unsigned dead = 0;
    for (int a = 0; a < PIPS_DRAW_TRAIL_MAX; ++a) {
        table.f[a] = (unsigned short)((fade != nullptr && a < style.trail) ? fade[a] : 256);
        if (table.f[a] == 0) dead |= 1u << a;
    }
    constexpr int FRAMES_A_LAUNCH = 65535;                     // the grid's y
    for (int f0 = 0; f0 < F; f0 += FRAMES_A_LAUNCH) {
        const unsigned fc = (unsigned)std::min(F - f0, FRAMES_A_LAUNCH);
        hipLaunchKernelGGL(draw_prepare_kernel, dim3((unsigned)((n + DRAW_THREADS - 1) / DRAW_THREADS), fc), dim3(DRAW_THREADS), 0, st,
                           trajs, vis, n, first, f0, h, w, src_w != w, src_h != h, sx, sy, colors, yuv8 ? 1 : yuv10 ? 2 : 0, rule, rule10,
                           dead, style, boxes, recs);
        const dim3 grid((unsigned)(tiles_x * tiles_y), fc);
#define PIPS_DRAW_CASE(L)                                                                                                                \
    do {                                                                                                                                 \
        if (fade == nullptr)                                                                                                             \
            hipLaunchKernelGGL(draw_raster_kernel<L>, grid, dim3(DRAW_THREADS), 0, st, d, bgr, h, w, n, style.trail, style.line8,        \
                               style.dot8, (const int4*)boxes, (const int*)recs, tiles_x, f0);                                           \
        else                                                                                                                             \
            hipLaunchKernelGGL((draw_raster_kernel<L, DrawFade>), grid, dim3(DRAW_THREADS), 0, st, d, bgr, h, w, n, style.trail, style.line8,   \
                               style.dot8, (const int4*)boxes, (const int*)recs, tiles_x, f0, table);                                    \
    } while (0)
        switch (format) {
            case PIPS_FMT_RGB24:
            case PIPS_FMT_BGR24: PIPS_DRAW_CASE(DRAW_PACKED3); break;
            case PIPS_FMT_RGBA32:
            case PIPS_FMT_BGRA32: PIPS_DRAW_CASE(DRAW_PACKED4); break;
            case PIPS_FMT_NV12: PIPS_DRAW_CASE(DRAW_NV12); break;
            case PIPS_FMT_I420: PIPS_DRAW_CASE(DRAW_I420); break;
            case PIPS_FMT_P010: PIPS_DRAW_CASE(DRAW_P010); break;
            case PIPS_FMT_I010: PIPS_DRAW_CASE(DRAW_I010); break;
            default: PIPS_DRAW_CASE(DRAW_PLANAR8); break;
        }
#undef PIPS_DRAW_CASE
    }
    PIPS_CHECK_LAUNCH("tracks_draw");
    return PIPS_OK;
}

}  // namespace pips
