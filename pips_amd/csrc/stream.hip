// Streamed chaining (drivers.StreamTracker) as device-side bookkeeping around the tracker and pips_chain_hop: which queries of a
// caller-owned state are ready for a window, which of them join with this round, the lowest window start still pending
// (stream_select_kernel), the staging and the scatter of a joining query's first-window features (stream_join_*_kernel) and the
// move of the frames that became final out of the row ring (stream_emit_kernel; stream_emit_cols_kernel for the columns of one
// stream of several), and the copy of the kept columns of a state into narrower arrays when queries leave the stream
// (stream_keep_state_kernel, stream_keep_rows_kernel).  Plain HIP; built with the default floating-point flags, as chain.hip is.  No atomics on the lists: their
// order is part of the contract.
#include <climits>

#include "common.h"

namespace pips {

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int STREAM_S = PIPS_S;
constexpr unsigned STREAM_NAN = 0x7fc00000u;      // the fp32 quiet NaN of torch's float("nan") fill

// row of logical frame f in a ring of L rows (base 0; Python's modulo: never negative)
__device__ __forceinline__ int stream_row(int f, int L) {
    const int r = f % L;
    return r < 0 ? r + L : r;
}

struct SelectArgs {
    const int* tq; const float* xy; const int* cur;
    int* status; float* trajs; int* active; int* new_list; int* counts;
    int T, final_, n, L;
    // CLIPS: V streams in one state -- the stream of each query, the frames appended to each stream and whether it has ended
    const int* clip; const int* clip_frames; const int* clip_final; int V;
};

// ONE block walks the n queries in chunks of SEL_THREADS, a thread per query.  The ready queries of a chunk get consecutive
// slots of `active`, the ready ones that were still waiting consecutive slots of `new_list`, by a block scan each (ballot inside a
// wave, the waves' counts through LDS) on top of the offsets carried from the chunks before: both lists ascend.  The lowest
// window start of the queries that are not done is a wave reduction plus LDS at the end of the same walk.
// CLIPS: a query is judged by the frames and the end of its own stream, and counts[4 + v] receives the lowest window start of
// stream v -- an integer minimum through LDS (order-independent).  A template parameter, so that the one-stream instantiation is
// the code it was.
template <bool CLIPS>
__global__ __launch_bounds__(SEL_THREADS) void stream_select_kernel(const SelectArgs a) {
    __shared__ int wave_act[SEL_WAVES];
    __shared__ int wave_new[SEL_WAVES];
    __shared__ int wave_low[SEL_WAVES];
    __shared__ int clip_low[CLIPS ? STREAM_V_MAX : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carried_act = 0, carried_new = 0, low = INT_MAX;
    if (CLIPS) {
        if (tid < STREAM_V_MAX) clip_low[tid] = INT_MAX;
        __syncthreads();
    }
    for (int q0 = 0; q0 < a.n; q0 += SEL_THREADS) {
        const int q = q0 + tid;
        bool ready = false, fresh = false;
        if (q < a.n) {
            int s = a.status[q];
            const int c = a.cur[q];
            int T = a.T, v = 0;
            bool final_ = a.final_ != 0;
            if (CLIPS) {
                v = min(max(a.clip[q], 0), a.V - 1);
                T = a.clip_frames[v];
                final_ = a.clip_final[v] != 0;
            }
            if (final_ && s == 1 && c >= T) {          // its last window ran past the end of the video
                s = 2;
                a.status[q] = 2;
            }
            if (s != 2) {
                low = min(low, c);
                if (CLIPS) atomicMin(&clip_low[v], c);                  // (LDS)
                ready = final_ ? c < T : c <= T - STREAM_S;      // all 8 frames of its window have arrived
                fresh = ready && s == 0;
            }
        }
        const unsigned long long ma = __ballot(ready), mn = __ballot(fresh);
        if (lane == 0) {
            wave_act[wave] = __popcll(ma);
            wave_new[wave] = __popcll(mn);
        }
        __syncthreads();
        int off_act = carried_act, off_new = carried_new, tot_act = 0, tot_new = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) {
            const int ca = wave_act[w], cn = wave_new[w];
            if (w < wave) { off_act += ca; off_new += cn; }
            tot_act += ca;
            tot_new += cn;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        if (ready) a.active[off_act + __popcll(ma & below)] = q;
        if (fresh) {       // first window: the start is the query itself, at its own frame
            a.new_list[off_new + __popcll(mn & below)] = q;
            const size_t o = ((size_t)stream_row(a.tq[q], a.L) * a.n + q) * 2;
            a.trajs[o] = a.xy[2 * q];
            a.trajs[o + 1] = a.xy[2 * q + 1];
            a.status[q] = 1;
        }
        carried_act += tot_act;
        carried_new += tot_new;
        __syncthreads();                // the wave counts are rewritten by the next chunk
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) low = min(low, __shfl_xor(low, d));
    if (lane == 0) wave_low[wave] = low;
    __syncthreads();
    if (tid == 0) {
        int m = wave_low[0];
#pragma unroll
        for (int w = 1; w < SEL_WAVES; ++w) m = min(m, wave_low[w]);
        a.counts[0] = carried_act;
        a.counts[1] = carried_new;
        a.counts[2] = m;
        a.counts[3] = 0;
    }
    if (CLIPS && tid < a.V) a.counts[4 + tid] = clip_low[tid];      // (the barrier above orders the LDS minima)
}

// the start positions and query frames of the joining queries new_list[0..n_new): the xys / win_start of their point sample.  A
// member outside [0, n) is never dereferenced: zeros are staged for it and the scatter ignores it.
__global__ __launch_bounds__(SEL_THREADS) void stream_join_gather_kernel(const int* __restrict__ new_list, int n_new, int n,
                                                                         const float* __restrict__ xy, const int* __restrict__ tq,
                                                                         float* __restrict__ sxy, int* __restrict__ stq,
                                                                         const int* __restrict__ clip, int* __restrict__ sclip) {
    const int j = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (j >= n_new) return;
    const int q = new_list[j];
    const bool ok = (unsigned)q < (unsigned)n;
    sxy[2 * j] = ok ? xy[2 * q] : 0.f;
    sxy[2 * j + 1] = ok ? xy[2 * q + 1] : 0.f;
    stq[j] = ok ? tq[q] : 0;
    if (clip != nullptr) sclip[j] = ok ? clip[q] : 0;         // (several streams: the stream of the query, its win_clip)
}

// one block per joining query: feat[q] = the features its point sample returned
__global__ __launch_bounds__(PIPS_C) void stream_join_scatter_kernel(const int* __restrict__ new_list, int n_new, int n,
                                                                     const float* __restrict__ sfeat, float* __restrict__ feat) {
    const int j = blockIdx.x;
    if (j >= n_new) return;
    const int q = new_list[j];
    if ((unsigned)q >= (unsigned)n) return;
    feat[(size_t)q * PIPS_C + threadIdx.x] = sfeat[(size_t)j * PIPS_C + threadIdx.x];
}

// `len` 32-bit words of one ring row to its dense output row, the ring row reset to NaN; bit patterns, not floats.  vec: the row
// length is a multiple of 4 words and both buffers are 16-byte aligned, so every row starts on a 16-byte boundary and moves as
// 16-byte pieces; any other row moves word by word (the scalar tail is then the whole row).
__device__ __forceinline__ void emit_row(unsigned* __restrict__ src, unsigned* __restrict__ dst, int len, bool vec, int t, int nt) {
    const int nv = vec ? len / 4 : 0;
    const uint4 nan4 = make_uint4(STREAM_NAN, STREAM_NAN, STREAM_NAN, STREAM_NAN);
    uint4* s4 = reinterpret_cast<uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (int i = t; i < nv; i += nt) {
        d4[i] = s4[i];
        s4[i] = nan4;
    }
    for (int i = 4 * nv + t; i < len; i += nt) {
        dst[i] = src[i];
        src[i] = STREAM_NAN;
    }
}

// blockIdx.y = frame f0 + y of the emitted range; the blocks of one frame share its two rows
__global__ __launch_bounds__(SEL_THREADS) void stream_emit_kernel(unsigned* __restrict__ trajs, unsigned* __restrict__ vis, int L, int n,
                                                                  int f0, int m, unsigned* __restrict__ out_trajs,
                                                                  unsigned* __restrict__ out_vis, int vec_trajs, int vec_vis) {
    const int i = blockIdx.y;
    if (i >= m) return;
    const int r = stream_row(f0 + i, L);
    const int t = blockIdx.x * SEL_THREADS + threadIdx.x, nt = gridDim.x * SEL_THREADS;
    emit_row(trajs + (size_t)r * n * 2, out_trajs + (size_t)i * n * 2, n * 2, vec_trajs != 0, t, nt);
    emit_row(vis + (size_t)r * n, out_vis + (size_t)i * n, n, vec_vis != 0, t, nt);
}

// the same for the columns cols[0..m) of the state: thread j of a frame's blocks moves column cols[j] -- two words of trajs (as one
// 8-byte piece where both buffers allow it) and one of vis.  A column outside [0, n) is not touched; its outputs get the NaN.
__global__ __launch_bounds__(SEL_THREADS) void stream_emit_cols_kernel(unsigned* __restrict__ trajs, unsigned* __restrict__ vis, int L,
                                                                       int n, int f0, int nf, const int* __restrict__ cols, int m,
                                                                       unsigned* __restrict__ out_trajs, unsigned* __restrict__ out_vis,
                                                                       int vec) {
    const int i = blockIdx.y, j = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i >= nf || j >= m) return;
    const int c = cols[j];
    const size_t o = (size_t)i * m + j;
    if ((unsigned)c >= (unsigned)n) {
        out_trajs[2 * o] = out_trajs[2 * o + 1] = out_vis[o] = STREAM_NAN;
        return;
    }
    const size_t e = (size_t)stream_row(f0 + i, L) * n + c;
    if (vec) {
        uint2* s2 = reinterpret_cast<uint2*>(trajs);
        reinterpret_cast<uint2*>(out_trajs)[o] = s2[e];
        s2[e] = make_uint2(STREAM_NAN, STREAM_NAN);
    } else {
        out_trajs[2 * o] = trajs[2 * e];
        out_trajs[2 * o + 1] = trajs[2 * e + 1];
        trajs[2 * e] = trajs[2 * e + 1] = STREAM_NAN;
    }
    out_vis[o] = vis[e];
    vis[e] = STREAM_NAN;
}

struct KeepArgs {
    StreamState in; StreamStateOut out;
    const int* keep; int* counts;
    int n, m, V;
};

// Queries leave the state.  ONE block walks keep[0..m) in chunks of SEL_THREADS, a thread per kept query: the per-query scalars of
// column keep[j] go to column j of the narrower arrays (xy as bit patterns), and the lowest window start of the kept queries that
// are not done is reduced the way stream_select_kernel does it -- a wave reduction plus LDS at the end of the walk, an LDS integer
// minimum per stream (CLIPS) -- so counts is what a select over the kept set would report.  A member outside [0, n) is never
// dereferenced: a done, empty query stands in its column and enters no minimum.  m == 0: counts alone.
template <bool CLIPS>
__global__ __launch_bounds__(SEL_THREADS) void stream_keep_state_kernel(const KeepArgs a) {
    __shared__ int wave_low[SEL_WAVES];
    __shared__ int clip_low[CLIPS ? STREAM_V_MAX : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned* xy = reinterpret_cast<const unsigned*>(a.in.xy);
    unsigned* xy_out = reinterpret_cast<unsigned*>(a.out.xy);
    int low = INT_MAX;
    if (CLIPS) {
        if (tid < STREAM_V_MAX) clip_low[tid] = INT_MAX;
        __syncthreads();
    }
    for (int j0 = 0; j0 < a.m; j0 += SEL_THREADS) {
        const int j = j0 + tid;
        if (j >= a.m) continue;
        const int c = a.keep[j];
        const bool ok = (unsigned)c < (unsigned)a.n;
        const int s = ok ? a.in.status[c] : 2;
        const int cu = ok ? a.in.cur[c] : 0;
        a.out.tq[j] = ok ? a.in.tq[c] : 0;
        a.out.cur[j] = cu;
        a.out.status[j] = s;
        xy_out[2 * j] = ok ? xy[2 * c] : 0u;
        xy_out[2 * j + 1] = ok ? xy[2 * c + 1] : 0u;
        int v = 0;
        if (CLIPS) {
            const int cl = ok ? a.in.clip[c] : 0;
            a.out.clip[j] = cl;
            v = min(max(cl, 0), a.V - 1);
        }
        if (s != 2) {
            low = min(low, cu);
            if (CLIPS) atomicMin(&clip_low[v], cu);                  // (LDS)
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) low = min(low, __shfl_xor(low, d));
    if (lane == 0) wave_low[wave] = low;
    __syncthreads();
    if (tid == 0) {
        int lo = wave_low[0];
#pragma unroll
        for (int w = 1; w < SEL_WAVES; ++w) lo = min(lo, wave_low[w]);
        a.counts[0] = 0;
        a.counts[1] = 0;
        a.counts[2] = lo;
        a.counts[3] = 0;
    }
    if (CLIPS && tid < a.V) a.counts[4 + tid] = clip_low[tid];      // (the barrier above orders the LDS minima)
}

constexpr int KEEP_FEAT_Y = 4;       // rows of blocks that move feat, behind the rows of blocks that move the row ring
constexpr int KEEP_ROWS_Y = 4096;    // ... of which a launch has at most this many (a longer ring: several rows per block)

// The first min(L, KEEP_ROWS_Y) rows of blocks move the ring: blockIdx.y takes rows y, y + their number, ...  Thread j of a row's
// blocks moves column keep[j] -- two words of trajs (one 8-byte piece where both buffers allow it) and one of vis -- to column j:
// keep ascends, so neighbouring lanes read neighbouring kept columns of one row (every fetched line is used as far as it holds
// kept columns) and write a dense run.  A gathered row has no 16-byte pieces: its columns are not neighbours in the source.
// The last KEEP_FEAT_Y rows of blocks move the feature rows, 512 contiguous bytes each: in 16-byte pieces where both buffers are
// 16-byte aligned, word by word otherwise; 32 (128) neighbouring lanes share a row.  Bit patterns throughout.  A column outside
// [0, n) is not read: its rows get the NaN and its features zero.
__global__ __launch_bounds__(SEL_THREADS) void stream_keep_rows_kernel(const unsigned* __restrict__ trajs, const unsigned* __restrict__ vis,
                                                                       const unsigned* __restrict__ feat, int L, int n,
                                                                       const int* __restrict__ keep, int m, unsigned* __restrict__ trajs_out,
                                                                       unsigned* __restrict__ vis_out, unsigned* __restrict__ feat_out,
                                                                       int vec_trajs, int vec_feat) {
    const int ry = gridDim.y - KEEP_FEAT_Y;                          // rows of blocks on the ring: min(L, KEEP_ROWS_Y)
    if ((int)blockIdx.y < ry) {
        for (int j = blockIdx.x * SEL_THREADS + threadIdx.x; j < m; j += gridDim.x * SEL_THREADS) {
            const int c = keep[j];
            const bool ok = (unsigned)c < (unsigned)n;
            for (int y = blockIdx.y; y < L; y += ry) {
                const size_t o = (size_t)y * m + j, e = (size_t)y * n + (ok ? c : 0);
                if (!ok) {
                    trajs_out[2 * o] = trajs_out[2 * o + 1] = vis_out[o] = STREAM_NAN;
                } else if (vec_trajs) {
                    reinterpret_cast<uint2*>(trajs_out)[o] = reinterpret_cast<const uint2*>(trajs)[e];
                    vis_out[o] = vis[e];
                } else {
                    trajs_out[2 * o] = trajs[2 * e];
                    trajs_out[2 * o + 1] = trajs[2 * e + 1];
                    vis_out[o] = vis[e];
                }
            }
        }
        return;
    }
    const int per = vec_feat ? PIPS_C / 4 : PIPS_C;                  // pieces of one feature row
    const size_t total = (size_t)m * per, stride = (size_t)gridDim.x * SEL_THREADS * KEEP_FEAT_Y;
    for (size_t p = ((size_t)(blockIdx.y - ry) * gridDim.x + blockIdx.x) * SEL_THREADS + threadIdx.x; p < total; p += stride) {
        const int j = (int)(p / per), i = (int)(p % per);
        const int c = keep[j];
        const bool ok = (unsigned)c < (unsigned)n;
        if (vec_feat) {
            reinterpret_cast<uint4*>(feat_out)[p] = ok ? reinterpret_cast<const uint4*>(feat)[(size_t)c * per + i] : make_uint4(0u, 0u, 0u, 0u);
        } else {
            feat_out[p] = ok ? feat[(size_t)c * per + i] : 0u;
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int launch_stream_select(int T, int final_, int n, const int* tq, const float* xy, const int* cur, int* status, float* trajs, int L,
                         int* active, int* new_list, int* counts, hipStream_t st, const StreamClips* clips) {
    SelectArgs a;
    a.tq = tq; a.xy = xy; a.cur = cur; a.status = status; a.trajs = trajs; a.active = active; a.new_list = new_list; a.counts = counts;
    a.T = T; a.final_ = final_ != 0; a.n = n; a.L = L;
    a.clip = a.clip_frames = a.clip_final = nullptr; a.V = 0;
    if (clips != nullptr) {
        a.clip = clips->clip; a.clip_frames = clips->frames; a.clip_final = clips->final_; a.V = clips->V;
        hipLaunchKernelGGL(stream_select_kernel<true>, dim3(1), dim3(SEL_THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL(stream_select_kernel<false>, dim3(1), dim3(SEL_THREADS), 0, st, a);
    }
    PIPS_CHECK_LAUNCH("stream_select");
    return PIPS_OK;
}

int launch_stream_join_gather(const int* new_list, int n_new, int n, const float* xy, const int* tq, float* sxy, int* stq,
                              hipStream_t st, const int* clip, int* sclip) {
    hipLaunchKernelGGL(stream_join_gather_kernel, dim3((n_new + SEL_THREADS - 1) / SEL_THREADS), dim3(SEL_THREADS), 0, st, new_list,
                       n_new, n, xy, tq, sxy, stq, clip, sclip);
    PIPS_CHECK_LAUNCH("stream_join_gather");
    return PIPS_OK;
}

int launch_stream_join_scatter(const int* new_list, int n_new, int n, const float* sfeat, float* feat, hipStream_t st) {
    hipLaunchKernelGGL(stream_join_scatter_kernel, dim3(n_new), dim3(PIPS_C), 0, st, new_list, n_new, n, sfeat, feat);
    PIPS_CHECK_LAUNCH("stream_join_scatter");
    return PIPS_OK;
}

int launch_stream_emit(float* trajs, float* vis, int L, int n, int f0, int f1, float* out_trajs, float* out_vis, hipStream_t st) {
    const int m = f1 - f0;
    const int vec_trajs = (2 * n) % 4 == 0 && aligned16(trajs) && aligned16(out_trajs);
    const int vec_vis = n % 4 == 0 && aligned16(vis) && aligned16(out_vis);
    // a thread moves one 16-byte piece (or one word) of the longer row per pass; 64 blocks per frame at the most
    const int per_row = vec_trajs ? (2 * n) / 4 : 2 * n;
    const int bx = min(max((per_row + SEL_THREADS - 1) / SEL_THREADS, 1), 64);
    hipLaunchKernelGGL(stream_emit_kernel, dim3(bx, m), dim3(SEL_THREADS), 0, st, reinterpret_cast<unsigned*>(trajs),
                       reinterpret_cast<unsigned*>(vis), L, n, f0, m, reinterpret_cast<unsigned*>(out_trajs),
                       reinterpret_cast<unsigned*>(out_vis), vec_trajs, vec_vis);
    PIPS_CHECK_LAUNCH("stream_emit");
    return PIPS_OK;
}

int launch_stream_emit_cols(float* trajs, float* vis, int L, int n, int f0, int f1, const int* cols, int m, float* out_trajs,
                            float* out_vis, hipStream_t st) {
    const int vec = ((reinterpret_cast<uintptr_t>(trajs) | reinterpret_cast<uintptr_t>(out_trajs)) & 7u) == 0;
    hipLaunchKernelGGL(stream_emit_cols_kernel, dim3((m + SEL_THREADS - 1) / SEL_THREADS, f1 - f0), dim3(SEL_THREADS), 0, st,
                       reinterpret_cast<unsigned*>(trajs), reinterpret_cast<unsigned*>(vis), L, n, f0, f1 - f0, cols, m,
                       reinterpret_cast<unsigned*>(out_trajs), reinterpret_cast<unsigned*>(out_vis), vec);
    PIPS_CHECK_LAUNCH("stream_emit_cols");
    return PIPS_OK;
}

int launch_stream_keep(int n, const int* keep, int m, const StreamState& in, const StreamStateOut& out, int L, int V, int* counts,
                       hipStream_t st) {
    KeepArgs a;
    a.in = in; a.out = out; a.keep = keep; a.counts = counts; a.n = n; a.m = m; a.V = V;
    if (in.clip != nullptr)
        hipLaunchKernelGGL(stream_keep_state_kernel<true>, dim3(1), dim3(SEL_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(stream_keep_state_kernel<false>, dim3(1), dim3(SEL_THREADS), 0, st, a);
    PIPS_CHECK_LAUNCH("stream_keep_state");
    if (m == 0) return PIPS_OK;
    const auto aligned8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; };
    const int vec_trajs = aligned8(in.trajs) && aligned8(out.trajs);
    const int vec_feat = aligned16(in.feat) && aligned16(out.feat);
    // a thread moves one kept column of a row per pass; 64 blocks per row at the most
    const int bx = min((m + SEL_THREADS - 1) / SEL_THREADS, 64);
    hipLaunchKernelGGL(stream_keep_rows_kernel, dim3(bx, min(L, KEEP_ROWS_Y) + KEEP_FEAT_Y), dim3(SEL_THREADS), 0, st,
                       reinterpret_cast<const unsigned*>(in.trajs), reinterpret_cast<const unsigned*>(in.vis),
                       reinterpret_cast<const unsigned*>(in.feat), L, n, keep, m, reinterpret_cast<unsigned*>(out.trajs),
                       reinterpret_cast<unsigned*>(out.vis), reinterpret_cast<unsigned*>(out.feat), vec_trajs, vec_feat);
    PIPS_CHECK_LAUNCH("stream_keep_rows");
    return PIPS_OK;
}

}  // namespace pips
