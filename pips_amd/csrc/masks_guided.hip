// Object masks that follow image edges (pips_object_masks_guided, pips_guide_plane; drivers.object_masks_guided, drivers.guide_plane):
// a pixel takes the label of the track that is nearest along a path over the 8-neighbour grid whose steps cost the 5-7 chamfer plus
// `edge` times the step's difference of an 8-bit guide plane -- a geodesic distance that is expensive across luma edges.  The rule
// (include/pips_hip.h) is integer arithmetic behind draw's quantisation of the positions (draw_quant.h): one 32-bit key
// cost << 16 | column per pixel and the fixed point of a min-relaxation, so the bytes are drivers.object_masks_guided_torch's.
// Plain HIP.  guided_prepare_kernel writes one 8-byte record per (frame, column) into the workspace: the seed pixel Y << 16 | X (-1 for
// a column that seeds nothing) and the label.  guided_relax_kernel owns a GUIDED_TILE x GUIDED_TILE tile of one frame: it holds the
// keys and the guide of the tile grown by GUIDED_HALO pixels a side in LDS, relaxes them there and stores the tile alone.  A sweep
// updates the four classes (x & 1, y & 1) of pixels one after the other, in place, with a barrier between two classes: the eight
// neighbours of a pixel lie in the other three classes, so no thread reads a key that another writes in the same phase -- the
// result of a launch is a pure function of its input, and a sweep does at least what a Jacobi step does.  After s sweeps the keys
// at least s pixels from the patch border are no larger than s Jacobi steps of the whole image would leave them and never smaller
// than the fixed point; GUIDED_HALO sweeps make the tile good for GUIDED_HALO steps.  A block stops as soon as a sweep changes
// nothing (its patch is at its own fixed point: a tile with no key in reach takes one sweep).  ceil(floor(reach / 5) / GUIDED_HALO)
// launches, at least one, decided on the host; launch 1 builds its seeds from the records (atomicMin in LDS: the lowest column of
// a pixel), launches hand the keys on through two planes of the workspace in turn, the last gathers labels[column] and stores
// bytes, a dword where the address allows.  guide_plane_kernel: the luma (luma.h) of packed or planar RGB as such a guide plane.
// No atomics but that integer min; nothing outside the w x h image is written.
#include "common.h"
#include "draw_quant.h"
#include "luma.h"

namespace pips {

namespace {

constexpr int GUIDED_THREADS = 256;
constexpr int GUIDED_TILE = 64;                                 // pixels a side that a block stores
constexpr int GUIDED_HALO = 16;                                 // pixels around them that it relaxes along: the steps a launch is good for
constexpr int GUIDED_PATCH = GUIDED_TILE + 2 * GUIDED_HALO;
constexpr int KEY_PITCH = GUIDED_PATCH + 2;                     // a ring of KEY_NONE around the patch: no bounds test in the sweep
constexpr int GUIDE_PITCH = GUIDED_PATCH + 8;                   // bytes; patch column i at byte i + 4, so that groups of four are dwords
constexpr unsigned KEY_NONE = 0xFFFFFFFFu;
constexpr int GUIDE_FRAMES_Y = 65535;                           // the grid's y of guide_plane_kernel; it strides over the frames beyond
static_assert(GUIDED_TILE % 4 == 0 && GUIDED_HALO % 4 == 0 && GUIDED_PATCH % 2 == 0, "dword groups and the four pixel classes");
static_assert(KEY_PITCH * KEY_PITCH * 4 + KEY_PITCH * GUIDE_PITCH <= 65536, "the patch fits the static LDS of a block");

// ------------------------------------------------------------------------------------------------------------------ prepare
// One thread per (frame, column): the record (Y << 16 | X, label) of a column that takes part and whose seed pixel X = (Qx + 4) >> 3,
// Y = (Qy + 4) >> 3 lies inside the image, (-1, label) of any other.  h, w <= 8192: X and Y take 13 bits each.
__global__ __launch_bounds__(GUIDED_THREADS) void guided_prepare_kernel(const float* __restrict__ trajs, const unsigned char* __restrict__ labels,
                                                                      int n, int first, int f_base, int scale_x, int scale_y, float sx,
                                                                      float sy, int h, int w, int2* __restrict__ recs) {
    const int i = (int)(blockIdx.x * (unsigned)GUIDED_THREADS + threadIdx.x);
    if (i >= n) return;
    const int f = f_base + (int)blockIdx.y;
    const size_t at = (size_t)(first + f) * n + i;
    const int qx = quantise(trajs[2 * at], scale_x != 0, sx);
    const int qy = quantise(trajs[2 * at + 1], scale_y != 0, sy);
    const int label = labels[at];
    int seed = -1;
    if (qx != DRAW_ABSENT && qy != DRAW_ABSENT && label != PIPS_MASK_NONE) {
        const int X = (qx + 4) >> 3, Y = (qy + 4) >> 3;         // (the arithmetic shift: floor)
        if (X >= 0 && X < w && Y >= 0 && Y < h) seed = Y << 16 | X;
    }
    recs[(size_t)f * n + i] = make_int2(seed, label);
}

// -------------------------------------------------------------------------------------------------------------------- relax
// One block per tile and frame.  FIRST: the keys start from the records, otherwise from keys_in; LAST: labels go to the mask,
// otherwise the tile's keys to keys_out.  Patch pixel (px, py) is image pixel (X0 - GUIDED_HALO + px, Y0 - GUIDED_HALO + py); one
// outside the image holds KEY_NONE and is never updated -- it is absent, not a pixel of guide 0.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(GUIDED_THREADS) void guided_relax_kernel(const int2* __restrict__ recs, int n, int h, int w, int edge, int reach,
                                                                    const unsigned char* __restrict__ guide, size_t gpitch, size_t gstep,
                                                                    const unsigned* __restrict__ keys_in, unsigned* __restrict__ keys_out,
                                                                    unsigned char* __restrict__ mask, size_t pitch, size_t step,
                                                                    int tiles_x, int f_base) {
    __shared__ unsigned key[KEY_PITCH * KEY_PITCH];
    __shared__ unsigned guide_dw[KEY_PITCH * GUIDE_PITCH / 4];
    const unsigned char* gd = reinterpret_cast<const unsigned char*>(guide_dw);
    const int tid = (int)threadIdx.x;
    const int f = f_base + (int)blockIdx.y;
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * GUIDED_TILE, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * GUIDED_TILE;
    const int PX0 = X0 - GUIDED_HALO, PY0 = Y0 - GUIDED_HALO;
    const size_t plane_f = (size_t)f * h * w;

    // the keys: KEY_NONE on the ring, outside the image and, FIRST, everywhere
    for (int k = tid; k < KEY_PITCH * KEY_PITCH; k += GUIDED_THREADS) {
        unsigned v = KEY_NONE;
        if constexpr (!FIRST) {
            const int px = k % KEY_PITCH - 1, py = k / KEY_PITCH - 1;
            const int gx = PX0 + px, gy = PY0 + py;
            if (px >= 0 && px < GUIDED_PATCH && py >= 0 && py < GUIDED_PATCH && gx >= 0 && gx < w && gy >= 0 && gy < h)
                v = keys_in[plane_f + (size_t)gy * w + gx];
        }
        key[k] = v;
    }
    // the guide, four pixels a thread: a dword where the four lie inside the image and the address allows, 0 where there is no pixel
    for (int k = tid; k < KEY_PITCH * (GUIDE_PITCH / 4); k += GUIDED_THREADS) {
        const int py = k / (GUIDE_PITCH / 4) - 1, px = 4 * (k % (GUIDE_PITCH / 4)) - 4;
        const int gx = PX0 + px, gy = PY0 + py;
        unsigned v = 0;
        if (guide != nullptr && px >= 0 && px < GUIDED_PATCH && py >= 0 && py < GUIDED_PATCH && gy >= 0 && gy < h && gx + 3 >= 0 && gx < w) {
            const unsigned char* p = guide + (size_t)f * gstep + (size_t)gy * gpitch + gx;      // (gx >= 0: PX0 is a multiple of four)
            if (gx + 3 < w && ((uintptr_t)p & 3) == 0) {
                v = *(const unsigned*)p;
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (gx + b < w) v |= (unsigned)p[b] << (8 * b);
            }
        }
        guide_dw[k] = v;
    }
    __syncthreads();
    if constexpr (FIRST) {
        const int2* rec_f = recs + (size_t)f * n;
        for (int i = tid; i < n; i += GUIDED_THREADS) {
            const int seed = rec_f[i].x;
            if (seed < 0) continue;
            const int px = (seed & 0xFFFF) - PX0, py = (seed >> 16) - PY0;
            if (px >= 0 && px < GUIDED_PATCH && py >= 0 && py < GUIDED_PATCH)
                atomicMin(&key[(py + 1) * KEY_PITCH + px + 1], (unsigned)i);                     // cost 0: the key is the column
        }
        __syncthreads();
    }

    constexpr int HALF = GUIDED_PATCH / 2;
    for (int s = 0; s < GUIDED_HALO; ++s) {
        int changed = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            for (int k = tid; k < HALF * HALF; k += GUIDED_THREADS) {
                const int px = 2 * (k % HALF) + (c & 1), py = 2 * (k / HALF) + (c >> 1);
                const int gx = PX0 + px, gy = PY0 + py;
                if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;
                const int at = (py + 1) * KEY_PITCH + px + 1, gat = (py + 1) * GUIDE_PITCH + px + 4;
                const unsigned old = key[at];
                const int g = gd[gat];
                unsigned best = old;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dx == 0 && dy == 0) continue;
                        const unsigned kq = key[at + dy * KEY_PITCH + dx];
                        const int diff = g - (int)gd[gat + dy * GUIDE_PITCH + dx];
                        // cost(q) <= reach <= 32767 and c <= 7 + 64 * 255: the sum stays below 2^16
                        const unsigned cand = kq + ((unsigned)(((dx != 0 && dy != 0) ? 7 : 5) + edge * abs(diff)) << 16);
                        if (kq != KEY_NONE && (int)(cand >> 16) <= reach) best = min(best, cand);
                    }
                if (best != old) key[at] = best, changed = 1;
            }
            if (c < 3) __syncthreads();
        }
        if (__syncthreads_or(changed) == 0) break;
    }

    if constexpr (!LAST) {
        for (int k = tid; k < GUIDED_TILE * GUIDED_TILE; k += GUIDED_THREADS) {
            const int tx = k % GUIDED_TILE, ty = k / GUIDED_TILE;
            const int gx = X0 + tx, gy = Y0 + ty;
            if (gx < w && gy < h) keys_out[plane_f + (size_t)gy * w + gx] = key[(ty + GUIDED_HALO + 1) * KEY_PITCH + tx + GUIDED_HALO + 1];
        }
    } else {
        const int2* rec_f = recs + (size_t)f * n;
        for (int k = tid; k < GUIDED_TILE * GUIDED_TILE / 4; k += GUIDED_THREADS) {
            const int tx = 4 * (k % (GUIDED_TILE / 4)), ty = k / (GUIDED_TILE / 4);
            const int x = X0 + tx, y = Y0 + ty;
            if (x >= w || y >= h) continue;
            unsigned out = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const unsigned kq = key[(ty + GUIDED_HALO + 1) * KEY_PITCH + tx + p + GUIDED_HALO + 1];
                out |= (kq == KEY_NONE ? (unsigned)PIPS_MASK_NONE : (unsigned)(rec_f[kq & 0xFFFFu].y & 255)) << (8 * p);
            }
            unsigned char* q = mask + (size_t)f * step + (size_t)y * pitch + x;
            if (x + 3 < w && ((uintptr_t)q & 3) == 0) {
                *(unsigned*)q = out;
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (x + p < w) q[p] = (unsigned char)(out >> (8 * p));
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- guide
// frame f, row y of plane k starts at p[k] + f step[k] + y pitch[k]
struct GuideSrc {
    const unsigned char* p[3];
    size_t pitch[3], step[3];
};

// One thread per four neighbouring pixels of a row, the same four of every frame blockIdx.y, blockIdx.y + gridDim.y, ...: the luma
// of R G B bytes, BPP == 3 or 4 bytes a pixel of plane 0 (`bgr`: B first), or BPP == 1: a byte of each of three planes.
template <int BPP>
__global__ __launch_bounds__(GUIDED_THREADS) void guide_plane_kernel(GuideSrc s, int bgr, int F, int h, int w, unsigned char* __restrict__ guide,
                                                                   size_t gpitch, size_t gstep, int quads_x) {
    const int q = (int)(blockIdx.x * (unsigned)GUIDED_THREADS + threadIdx.x);
    if (q >= quads_x * h) return;
    const int y = q / quads_x, x = 4 * (q % quads_x);
    const int nx = min(4, w - x);
    for (int f = (int)blockIdx.y; f < F; f += (int)gridDim.y) {
        unsigned out = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p >= nx) continue;
            int r, g, b;
            if constexpr (BPP == 1) {
                r = s.p[0][(size_t)f * s.step[0] + (size_t)y * s.pitch[0] + x + p];
                g = s.p[1][(size_t)f * s.step[1] + (size_t)y * s.pitch[1] + x + p];
                b = s.p[2][(size_t)f * s.step[2] + (size_t)y * s.pitch[2] + x + p];
            } else {
                const unsigned char* px = s.p[0] + (size_t)f * s.step[0] + (size_t)y * s.pitch[0] + (size_t)BPP * (x + p);
                r = px[bgr ? 2 : 0], g = px[1], b = px[bgr ? 0 : 2];
            }
            out |= (unsigned)luma_of(r, g, b) << (8 * p);
        }
        unsigned char* o = guide + (size_t)f * gstep + (size_t)y * gpitch + x;
        if (nx == 4 && ((uintptr_t)o & 3) == 0) {
            *(unsigned*)o = out;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (p < nx) o[p] = (unsigned char)(out >> (8 * p));
        }
    }
}

}  // namespace

int guided_launches(int reach) { return std::max(1, (reach / 5 + GUIDED_HALO - 1) / GUIDED_HALO); }

int launch_object_masks_guided(const float* trajs, const unsigned char* labels, int n, int first, int F, int src_h, int src_w, int h, int w,
                               int edge, int reach, const unsigned char* guide, size_t gpitch, size_t gstep, unsigned char* mask,
                               size_t pitch, size_t step, void* workspace, hipStream_t st) {
    const float sx = (float)w / (float)src_w, sy = (float)h / (float)src_h;
    const int tiles_x = (w + GUIDED_TILE - 1) / GUIDED_TILE, tiles_y = (h + GUIDED_TILE - 1) / GUIDED_TILE;   // <= 128 each
    int2* recs = (int2*)workspace;
    unsigned* keys[2] = {nullptr, nullptr};
    if (n > 0) {
        keys[0] = (unsigned*)((char*)workspace + align_up((size_t)F * (size_t)n * MASK_REC_BYTES, 16));
        keys[1] = keys[0] + (size_t)F * h * w;
    }
    const int launches = n > 0 ? guided_launches(reach) : 1;   // no column: no key, one launch writes PIPS_MASK_NONE
    constexpr int FRAMES_A_LAUNCH = 65535;                     // the grid's y
    for (int f0 = 0; f0 < F; f0 += FRAMES_A_LAUNCH) {
        const unsigned fc = (unsigned)std::min(F - f0, FRAMES_A_LAUNCH);
        if (n > 0)
            hipLaunchKernelGGL(guided_prepare_kernel, dim3((unsigned)((n + GUIDED_THREADS - 1) / GUIDED_THREADS), fc), dim3(GUIDED_THREADS), 0,
                               st, trajs, labels, n, first, f0, src_w != w, src_h != h, sx, sy, h, w, recs);
        const dim3 grid((unsigned)(tiles_x * tiles_y), fc);
#define PIPS_GUIDED_CASE(A, B)                                                                                                           \
    hipLaunchKernelGGL((guided_relax_kernel<A, B>), grid, dim3(GUIDED_THREADS), 0, st, (const int2*)recs, n, h, w, edge, reach, guide,   \
                       gpitch, gstep, (const unsigned*)keys[(j + 1) & 1], keys[j & 1], mask, pitch, step, tiles_x, f0)
        for (int j = 0; j < launches; ++j) {                   // launch j writes plane j & 1 and reads the other
            const bool head = j == 0, tail = j == launches - 1;
            if (head && tail) PIPS_GUIDED_CASE(true, true);
            else if (head) PIPS_GUIDED_CASE(true, false);
            else if (tail) PIPS_GUIDED_CASE(false, true);
            else PIPS_GUIDED_CASE(false, false);
        }
#undef PIPS_GUIDED_CASE
    }
    PIPS_CHECK_LAUNCH("object_masks_guided");
    return PIPS_OK;
}

int launch_guide_plane(int format, int F, int h, int w, const void* const* p, const size_t* pitch, const size_t* step, unsigned char* guide,
                       size_t gpitch, size_t gstep, hipStream_t st) {
    GuideSrc s;
    for (int k = 0; k < 3; ++k) s.p[k] = (const unsigned char*)p[k], s.pitch[k] = pitch[k], s.step[k] = step[k];
    const int bgr = format == PIPS_FMT_BGR24 || format == PIPS_FMT_BGRA32;
    const int quads_x = (w + 3) / 4;
    const dim3 grid((unsigned)(((size_t)quads_x * h + GUIDED_THREADS - 1) / GUIDED_THREADS), (unsigned)std::min(F, GUIDE_FRAMES_Y));
#define PIPS_GUIDE_CASE(BPP) \
    hipLaunchKernelGGL(guide_plane_kernel<BPP>, grid, dim3(GUIDED_THREADS), 0, st, s, bgr, F, h, w, guide, gpitch, gstep, quads_x)
    switch (format) {
        case PIPS_FMT_RGB24:
        case PIPS_FMT_BGR24: PIPS_GUIDE_CASE(3); break;
        case PIPS_FMT_RGBA32:
        case PIPS_FMT_BGRA32: PIPS_GUIDE_CASE(4); break;
        default: PIPS_GUIDE_CASE(1); break;
    }
#undef PIPS_GUIDE_CASE
    PIPS_CHECK_LAUNCH("guide_plane");
    return PIPS_OK;
}

}  // namespace pips
