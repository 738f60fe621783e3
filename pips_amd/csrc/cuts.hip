// Scene cuts (drivers.Cover(cut_thr=), drivers.find_cuts, pips_cut_table): cut_hist_kernel counts the 8-bit luma of every frame
// into 32 bins in each region of a 4 x 4 grid, cut_dist_kernel sums the absolute differences of the counts of neighbouring frames.
// The rule (include/pips_hip.h) is integer arithmetic on corner_table_kernel's luma (luma.h), and sums of counts do not depend on
// their order, so hist and dist are bit for bit drivers.cut_table_torch's.  Plain HIP.  No global atomics and no hand-off between
// blocks: a block stores its partial histogram with plain stores, and the second launch sums the partials in a fixed order.
#include "common.h"
#include "luma.h"

namespace pips {

namespace {

constexpr int CUT_THREADS = 256;
constexpr int CUT_WAVES = CUT_THREADS / 64;
constexpr int CUT_BINS = 32;                   // Y >> 3
constexpr int CUT_KEYS = 4 * CUT_BINS;         // a block counts the 4 regions of one region row
constexpr int CUT_HIST = 16 * CUT_BINS;        // the counts of a frame
// A flat frame sends every pixel of a region to one counter.  The block keeps 32 copies of its counters, lane l of either half of
// a wave adding into copy l % 32: an LDS add instruction is served a 32-lane half at a time, and with the odd stride the 32 copies
// of one counter lie in 32 different banks -- such a frame costs what any other costs.  Runs of equal keys inside a thread's
// group of pixels are merged in registers first.
constexpr int CUT_COPIES = 32;
constexpr int CUT_STRIDE = CUT_KEYS + 1;

// One block per (frame, region row, strip): the pixel rows [y0, y1) of region row rr, all columns.  A row is walked in GROUPS:
// group 0 is the head [0, hd) that brings the row to a 16-byte address, group g >= 1 the pixels [hd + (g-1) V, hd + g V) with V
// the pixels of 16 bytes.  A whole group at an aligned address is read with one 16-byte load per plane; the head, the tail and
// every group of a frame whose planes do not share their alignment (plane bytes not a multiple of 16) with element loads.
template <typename T>
__global__ __launch_bounds__(CUT_THREADS) void cut_hist_kernel(const T* __restrict__ frames, int h, int w, int strips,
                                                               int* __restrict__ partial) {
    constexpr int V = 16 / (int)sizeof(T);
    __shared__ int counts[CUT_COPIES * CUT_STRIDE];
    const int tid = threadIdx.x;
    const int s = blockIdx.x % strips, rr = (blockIdx.x / strips) % 4, f = blockIdx.x / (4 * strips);
    for (int i = tid; i < CUT_COPIES * CUT_STRIDE; i += CUT_THREADS) counts[i] = 0;
    __syncthreads();
    // (4y)/h == rr  <=>  ceil(rr h / 4) <= y < ceil((rr+1) h / 4); the same for the columns
    const int ry0 = (int)(((long long)rr * h + 3) / 4), ry1 = (int)(((long long)(rr + 1) * h + 3) / 4);
    const int y0 = ry0 + (int)((long long)(ry1 - ry0) * s / strips), y1 = ry0 + (int)((long long)(ry1 - ry0) * (s + 1) / strips);
    const int cx1 = (int)(((long long)w + 3) / 4), cx2 = (int)((2ll * w + 3) / 4), cx3 = (int)((3ll * w + 3) / 4);
    const size_t plane = (size_t)h * w;
    const T* frame = frames + (size_t)f * 3 * plane;
    const bool vec = (plane * sizeof(T)) % 16 == 0 && ((uintptr_t)frames % sizeof(T)) == 0;
    const int G = (w + V - 1) / V + 1;                                             // the head and at most ceil(w / V) groups behind it
    int* mine = counts + (tid & (CUT_COPIES - 1)) * CUT_STRIDE;
    const int items = (y1 - y0) * G;                                               // < 2^31: (h/4 + 1)(w/4 + 2) with h w <= 2^30
    for (int it = tid; it < items; it += CUT_THREADS) {
        const int y = y0 + it / G, g = it % G;
        const T* p = frame + (size_t)y * w;
        const int hd = vec ? min(w, (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / (unsigned)sizeof(T))) : 0;
        const int xa = g == 0 ? 0 : (int)min((long long)w, (long long)hd + (long long)(g - 1) * V);
        const int xb = g == 0 ? hd : (int)min((long long)w, (long long)xa + V);
        if (xa >= xb) continue;
        int lum[V];
        if (vec && g > 0 && xb - xa == V) {
            if constexpr (sizeof(T) == 1) {
                const uint4 r4 = *reinterpret_cast<const uint4*>(p + xa);
                const uint4 g4 = *reinterpret_cast<const uint4*>(p + plane + xa);
                const uint4 b4 = *reinterpret_cast<const uint4*>(p + 2 * plane + xa);
                const unsigned rw[4] = {r4.x, r4.y, r4.z, r4.w}, gw[4] = {g4.x, g4.y, g4.z, g4.w}, bw[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int sh = 8 * (k & 3);
                    lum[k] = luma_of((int)((rw[k >> 2] >> sh) & 255u), (int)((gw[k >> 2] >> sh) & 255u), (int)((bw[k >> 2] >> sh) & 255u));
                }
            } else {
                const float4 r4 = *reinterpret_cast<const float4*>(p + xa);
                const float4 g4 = *reinterpret_cast<const float4*>(p + plane + xa);
                const float4 b4 = *reinterpret_cast<const float4*>(p + 2 * plane + xa);
                lum[0] = luma_of(channel_u8(r4.x), channel_u8(g4.x), channel_u8(b4.x));
                lum[1] = luma_of(channel_u8(r4.y), channel_u8(g4.y), channel_u8(b4.y));
                lum[2] = luma_of(channel_u8(r4.z), channel_u8(g4.z), channel_u8(b4.z));
                lum[3] = luma_of(channel_u8(r4.w), channel_u8(g4.w), channel_u8(b4.w));
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) lum[k] = xa + k < xb ? luma_at(frame, plane, (size_t)y * w + xa + k) : 0;
        }
        int run_key = -1, run = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (xa + k < xb) {
                const int x = xa + k;
                const int key = ((x >= cx1) + (x >= cx2) + (x >= cx3)) * CUT_BINS + (lum[k] >> 3);
                if (key == run_key) {
                    ++run;
                } else {
                    if (run > 0) atomicAdd(&mine[run_key], run);
                    run_key = key;
                    run = 1;
                }
            }
        }
        if (run > 0) atomicAdd(&mine[run_key], run);
    }
    __syncthreads();
    // every block writes its whole partial, an empty strip its zeros: the second launch reads them all
    if (tid < CUT_KEYS) {
        int sum = 0;
#pragma unroll
        for (int c = 0; c < CUT_COPIES; ++c) sum += counts[c * CUT_STRIDE + tid];
        partial[(size_t)blockIdx.x * CUT_KEYS + tid] = sum;
    }
}

// One block per frame: entry e = region * 32 + bin of the frame's histogram is the sum of the strips' partials, the one of the
// frame before it likewise (prev_hist for frame 0; without it frame 0 has distance 0), and dist the sum of |difference| --
// shuffles inside a wave, the four waves through LDS.
__global__ __launch_bounds__(CUT_THREADS) void cut_dist_kernel(const int* __restrict__ partial, const int* __restrict__ prev_hist,
                                                               int strips, int* __restrict__ hist, int* __restrict__ dist) {
    __shared__ unsigned wave_sum[CUT_WAVES];
    const int tid = threadIdx.x, f = blockIdx.x;
    unsigned d = 0;
    for (int e = tid; e < CUT_HIST; e += CUT_THREADS) {
        const int rr = e / CUT_KEYS, k = e % CUT_KEYS;                           // region = 4 rr + rc, k = 32 rc + bin
        const int* p = partial + ((size_t)f * 4 + rr) * strips * CUT_KEYS + k;
        int cur = 0, old = 0;
        for (int s = 0; s < strips; ++s) cur += p[(size_t)s * CUT_KEYS];
        if (f > 0) {
            const int* q = p - (size_t)4 * strips * CUT_KEYS;
            for (int s = 0; s < strips; ++s) old += q[(size_t)s * CUT_KEYS];
        } else {
            old = prev_hist != nullptr ? prev_hist[e] : cur;
        }
        hist[(size_t)f * CUT_HIST + e] = cur;
        d += (unsigned)(cur > old ? cur - old : old - cur);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < CUT_WAVES; ++k) d += wave_sum[k];
        dist[f] = (int)d;
    }
}

}  // namespace

int launch_cut_table(const void* frames, int src_u8, int F, int h, int w, const int* prev_hist, int* hist, int* dist, int* partial,
                     hipStream_t st) {
    const int strips = cut_strips(h);
    const dim3 grid((unsigned)(F * 4 * strips)), block(CUT_THREADS);
    if (src_u8) {
        hipLaunchKernelGGL(cut_hist_kernel<unsigned char>, grid, block, 0, st, (const unsigned char*)frames, h, w, strips, partial);
    } else {
        hipLaunchKernelGGL(cut_hist_kernel<float>, grid, block, 0, st, (const float*)frames, h, w, strips, partial);
    }
    PIPS_CHECK_LAUNCH("cut_hist");
    hipLaunchKernelGGL(cut_dist_kernel, dim3((unsigned)F), block, 0, st, (const int*)partial, prev_hist, strips, hist, dist);
    PIPS_CHECK_LAUNCH("cut_dist");
    return PIPS_OK;
}

}  // namespace pips
