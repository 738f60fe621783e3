// Seeding on corners (drivers.Cover(seed="corners"), pips_corner_table / pips_cover_place): corner_table_kernel scores every pixel
// of every frame and keeps the best corner of each cover cell; cover_place_kernel moves the seeds of a cover step onto them.  The
// rule (include/pips_hip.h) is integer arithmetic up to the argmax -- 8-bit luma, central differences, the 7x7 structure tensor
// (a, b, c) in int32, S = a + c - ceil(sqrt((a-c)^2 + 4b^2)) with the root made exact by an integer correction -- so the table
// is bit for bit drivers.corner_table_torch's.  Plain HIP, the default floating-point flags (cover.hip's): `/` in the placing is
// the correctly rounded fp32 quotient, as in cover_flag_kernel.  No atomics and no global scratch: one block owns one cell.
#include "common.h"
#include "luma.h"

namespace pips {

namespace {

constexpr int CRN_THREADS = 256;
constexpr int CRN_WAVES = CRN_THREADS / 64;
constexpr int CRN_TILE = 32;                   // a block walks its cell in tiles of at most 32 x 32 candidates
constexpr int CRN_HALO = 4;                    // 3 for the window and 1 for the central difference
constexpr int CRN_LW = CRN_TILE + 2 * CRN_HALO;            // 40: the luma tile's side, and the row stride of luma and gradients
constexpr int CRN_GW = CRN_TILE + 6;                       // 38: the side of the gradient tile

// (luma_at, the luma of pixel (y, x) of a planar frame, is luma.h's: pips_cut_table quantises the same way)

// One block per (frame, cell).  The candidates of the cell -- its pixels with 4 <= x <= w-5 and 4 <= y <= h-5 -- are walked in
// tiles; every pass below maps consecutive lanes to consecutive dwords of one LDS row (luma and gradients share the stride 40 and
// are indexed by the loop counter itself, the 32-wide sums give a 32-lane half its own row), so no pass has a bank conflict.
//   A  luma of the tile and its 4-pixel halo, from the three planes                           lum  (th+8) x (tw+8)
//   B  central differences, gx and gy packed as two int16 in one dword                        grad (th+6) x (tw+6)
//   C  the three products summed over 7 columns                                               row  (th+6) x tw, three planes
//   D  summed over 7 rows, the score, and the running best as one 64-bit key per thread
// The key holds S in its high half and ~(y*w + x) in its low half: one max picks the largest S, then the lowest y, then the lowest
// x; 0 is no key of a candidate (its low half would need y*w + x = 2^32 - 1).
template <typename T>
__global__ __launch_bounds__(CRN_THREADS) void corner_table_kernel(const T* __restrict__ frames, int h, int w, int cell, int gh, int gw,
                                                                   float* __restrict__ table) {
    __shared__ int lum[CRN_LW * CRN_LW];
    __shared__ int grad[CRN_GW * CRN_LW];
    __shared__ int row[3][CRN_GW * CRN_TILE];
    __shared__ unsigned long long wave_best[CRN_WAVES];
    const int tid = threadIdx.x;
    const int cells = gh * gw;
    const int f = blockIdx.x / cells, ij = blockIdx.x % cells, ci = ij / gw, cj = ij % gw;
    const size_t plane = (size_t)h * w;
    const T* frame = frames + (size_t)f * 3 * plane;
    // the candidates of this cell: rows [cy0, cy1), columns [cx0, cx1); the products stay in range for any cell and frame size
    const int cy0 = max(ci * cell, CRN_HALO), cy1 = (int)min((long long)(ci + 1) * cell, (long long)h - CRN_HALO);
    const int cx0 = max(cj * cell, CRN_HALO), cx1 = (int)min((long long)(cj + 1) * cell, (long long)w - CRN_HALO);
    unsigned long long best = 0ull;
    for (int y0 = cy0; y0 < cy1; y0 += CRN_TILE) {
        const int th = min(CRN_TILE, cy1 - y0);
        for (int x0 = cx0; x0 < cx1; x0 += CRN_TILE) {
            const int tw = min(CRN_TILE, cx1 - x0);
            // A: lum[r][c] is pixel (y0 - 4 + r, x0 - 4 + c); a candidate's halo lies inside the frame
            for (int idx = tid; idx < (th + 2 * CRN_HALO) * CRN_LW; idx += CRN_THREADS) {
                const int r = idx / CRN_LW, c = idx % CRN_LW;
                if (c < tw + 2 * CRN_HALO) lum[idx] = luma_at(frame, plane, (size_t)(y0 - CRN_HALO + r) * w + (x0 - CRN_HALO + c));
            }
            __syncthreads();
            // B: grad[r][c] is pixel (y0 - 3 + r, x0 - 3 + c), which is lum[r + 1][c + 1]
            for (int idx = tid; idx < (th + 6) * CRN_LW; idx += CRN_THREADS) {
                if (idx % CRN_LW < tw + 6) {
                    const int gx = lum[idx + CRN_LW + 2] - lum[idx + CRN_LW];
                    const int gy = lum[idx + 2 * CRN_LW + 1] - lum[idx + 1];
                    grad[idx] = (int)(((unsigned)gx & 0xffffu) | ((unsigned)gy << 16));
                }
            }
            __syncthreads();
            // C: row[.][r][c] sums the products of grad[r][c .. c + 6]: the window columns of pixel column x0 + c
            for (int idx = tid; idx < (th + 6) * CRN_TILE; idx += CRN_THREADS) {
                const int r = idx / CRN_TILE, c = idx % CRN_TILE;
                if (c < tw) {
                    int sa = 0, sb = 0, sc = 0;
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        const int p = grad[r * CRN_LW + c + k];
                        const int gx = (int)(short)(p & 0xffff), gy = p >> 16;
                        sa += gx * gx;
                        sb += gx * gy;
                        sc += gy * gy;
                    }
                    row[0][idx] = sa;
                    row[1][idx] = sb;
                    row[2][idx] = sc;
                }
            }
            __syncthreads();
            // D: rows r .. r + 6 of the sums are the window rows of pixel row y0 + r
            for (int idx = tid; idx < th * CRN_TILE; idx += CRN_THREADS) {
                const int r = idx / CRN_TILE, c = idx % CRN_TILE;
                if (c < tw) {
                    int sa = 0, sb = 0, sc = 0;
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        sa += row[0][idx + k * CRN_TILE];
                        sb += row[1][idx + k * CRN_TILE];
                        sc += row[2][idx + k * CRN_TILE];
                    }
                    const long long dac = (long long)sa - sc;
                    const long long d = dac * dac + 4ll * sb * sb;                    // < 2^53: exact as a double
                    long long root = (long long)sqrt((double)d);                      // floor(sqrt(d)) after the correction
                    if (root * root > d) --root;
                    if ((root + 1) * (root + 1) <= d) ++root;
                    const int score = sa + sc - (int)(root + (root * root < d ? 1 : 0));
                    const unsigned at = (unsigned)(y0 + r) * (unsigned)w + (unsigned)(x0 + c);
                    const unsigned long long key = ((unsigned long long)(unsigned)score << 32) | (unsigned long long)(0xffffffffu - at);
                    best = key > best ? key : best;
                }
            }
            // (the next tile's pass A writes lum only, which nobody reads after B; its barrier orders everything else)
        }
    }
    // the block's best: shuffles inside a wave, the four waves through LDS
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(best >> 32), off, 64), lo = __shfl_xor((unsigned)best, off, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < CRN_WAVES; ++k) best = wave_best[k] > best ? wave_best[k] : best;
        float* out = table + (size_t)blockIdx.x * 3;
        if (best == 0ull) {                     // no candidate: the centre as cover_list_kernel computes it
            const float fc = (float)cell;
            out[0] = fminf(((float)cj + 0.5f) * fc, (float)(w - 1));
            out[1] = fminf(((float)ci + 0.5f) * fc, (float)(h - 1));
            out[2] = -1.f;
        } else {
            const unsigned at = 0xffffffffu - (unsigned)best;
            out[0] = (float)(at % (unsigned)w);
            out[1] = (float)(at / (unsigned)w);
            out[2] = (float)(unsigned)(best >> 32);
        }
    }
}

// A thread per seed: the cell of the centre the cover step wrote (cover_flag_kernel's quotient; a value that is no position,
// which the cover step never writes, counts as cell 0), and the table's corner in its place when that scores above min_corner.
__global__ __launch_bounds__(CRN_THREADS) void cover_place_kernel(float* __restrict__ seeds, int k, const float* __restrict__ table,
                                                                  int gh, int gw, int cell, int min_corner) {
    const int s = blockIdx.x * CRN_THREADS + threadIdx.x;
    if (s >= k) return;
    const float fc = (float)cell;
    const float qi = floorf(seeds[3 * (size_t)s + 2] / fc), qj = floorf(seeds[3 * (size_t)s + 1] / fc);
    const int i = qi >= 0.f ? (qi < (float)gh ? (int)qi : gh - 1) : 0;
    const int j = qj >= 0.f ? (qj < (float)gw ? (int)qj : gw - 1) : 0;
    const float* e = table + ((size_t)i * gw + j) * 3;
    if (e[2] > (float)min_corner) {
        seeds[3 * (size_t)s + 1] = e[0];
        seeds[3 * (size_t)s + 2] = e[1];
    }
}

}  // namespace

int launch_corner_table(const void* frames, int src_u8, int F, int h, int w, int cell, int gh, int gw, float* table, hipStream_t st) {
    const dim3 grid((unsigned)((long long)F * gh * gw)), block(CRN_THREADS);
    if (src_u8) {
        hipLaunchKernelGGL(corner_table_kernel<unsigned char>, grid, block, 0, st, (const unsigned char*)frames, h, w, cell, gh, gw, table);
    } else {
        hipLaunchKernelGGL(corner_table_kernel<float>, grid, block, 0, st, (const float*)frames, h, w, cell, gh, gw, table);
    }
    PIPS_CHECK_LAUNCH("corner_table");
    return PIPS_OK;
}

int launch_cover_place(float* seeds, int k, const float* table, int gh, int gw, int cell, int min_corner, hipStream_t st) {
    hipLaunchKernelGGL(cover_place_kernel, dim3((k + CRN_THREADS - 1) / CRN_THREADS), dim3(CRN_THREADS), 0, st, seeds, k, table, gh, gw,
                       cell, min_corner);
    PIPS_CHECK_LAUNCH("cover_place");
    return PIPS_OK;
}

}  // namespace pips
