// The cover step of a streamed tracker (drivers.CoverTracker, pips_cover_step): on the frames a push has just returned, which
// queries are retired -- outside the frame, or below the visibility threshold for lost_after frames in a row -- which are kept,
// which cells of a gh x gw grid over the frame hold no kept or pending query, and one seed per empty cell.  cover_flag_kernel
// judges the queries (a thread each) and marks the occupied cells; cover_list_kernel writes the lists.  Plain HIP; built with
// the default floating-point flags, as chain.hip and stream.hip are, so `/` is the correctly rounded fp32 quotient.  No atomics:
// every writer of the occupancy table stores the same 1, and the lists are scanned by ONE block because their order is the
// contract.  `lost` is an input and is left untouched: the runs of the kept queries come back in lost_out.
// The thin step (pips_cover_step_thin) adds a cap of per_cell tracks per cell: on every returned frame a query that counts -- started
// on that frame, inside on it, not retired as outside or lost in this step -- is SURPLUS when at least per_cell counting queries of
// lower column stand in its cell (lower columns are older identities), and a query that stayed surplus for crowd_after returned
// frames in a row is retired as crowded.  The rule is not greedy: an elder counts on a row even when it is itself retired as
// crowded in this step, so the rank by age needs no sequential pass.  cover_flag_kernel runs without its occupancy store,
// cover_crowd_kernel ranks every (frame, query) against the elder queries through LDS, cover_settle_kernel walks the second run,
// retires the crowded and marks the cells, and cover_list_kernel also writes crowd_out, gone and reason.
#include <climits>

#include "common.h"

namespace pips {

namespace {

constexpr int COV_THREADS = 256;
constexpr int COV_WAVES = COV_THREADS / 64;
constexpr int COV_KEEP = 0, COV_OUTSIDE = 1, COV_LOST = 2, COV_CROWDED = 3;      // (the retired ones: the values of `reason`)
constexpr int COV_ROWS_MAX = 65535;                                               // blocks along y of one launch

struct CoverArgs {
    int n, m, f1;
    const float* trajs; const float* vis; const int* tq; const float* xy; const int* lost;
    int H, W, cell, gh, gw;
    float vis_logit;
    int lost_after, max_queries;
    int* keep; int* lost_out; float* seeds; int* counts;
    int* flag; int* run; int* occ;            // workspace: (n), (n), (gh*gw)
    // the thin step alone
    const int* crowd; int per_cell, crowd_after;
    int* crowd_out; int* gone; int* reason;
    int* crun; int* over;                     // workspace behind occ: (n), (m*n)
};

__device__ __forceinline__ bool cover_inside(const CoverArgs& a, float x, float y) {
    return x >= 0.f && x <= (float)(a.W - 1) && y >= 0.f && y <= (float)(a.H - 1);
}
// the cell of a position that passed cover_inside
__device__ __forceinline__ int cover_cell(const CoverArgs& a, float x, float y) {
    const float fc = (float)a.cell;
    return min((int)floorf(y / fc), a.gh - 1) * a.gw + min((int)floorf(x / fc), a.gw - 1);
}

// A thread per query.  A pending query (t_q beyond the last returned frame; every query of a step without rows) is kept with a
// run of 0 and stands on its query position; a started one walks the m returned rows (row g is frame f1 - m + g; neighbouring
// threads read neighbouring columns of a row), updates its run on the frames from t_q on, and stands on its position in the last
// row.  The inside test is written so that NaN and +-inf fail it.  OCC = false (the thin step): the cells are marked by
// cover_settle_kernel, once the crowded are known.
template <bool OCC>
__global__ __launch_bounds__(COV_THREADS) void cover_flag_kernel(const CoverArgs a) {
    const int c = blockIdx.x * COV_THREADS + threadIdx.x;
    if (c >= a.n) return;
    const int t = a.tq[c];
    const bool pending = a.m == 0 || t > a.f1 - 1;
    unsigned run = 0u;
    float x, y;
    if (pending) {
        x = a.xy[2 * c];
        y = a.xy[2 * c + 1];
    } else {
        run = (unsigned)a.lost[c];
        const int f0 = a.f1 - a.m;
        for (int g = 0; g < a.m; ++g) {
            if (f0 + g < t) continue;
            const float v = a.vis[(size_t)g * a.n + c];
            run = v < a.vis_logit ? run + 1u : 0u;       // (a NaN compares false and resets the run)
        }
        const size_t o = ((size_t)(a.m - 1) * a.n + c) * 2;
        x = a.trajs[o];
        y = a.trajs[o + 1];
    }
    const bool inside = x >= 0.f && x <= (float)(a.W - 1) && y >= 0.f && y <= (float)(a.H - 1);
    int flag = COV_KEEP;
    if (!pending) flag = !inside ? COV_OUTSIDE : ((int)run >= a.lost_after ? COV_LOST : COV_KEEP);
    a.flag[c] = flag;
    a.run[c] = (int)run;
    if (OCC && flag == COV_KEEP && inside) {             // (a pending query outside the frame occupies no cell)
        const float fc = (float)a.cell;
        const int i = min((int)floorf(y / fc), a.gh - 1), j = min((int)floorf(x / fc), a.gw - 1);
        a.occ[i * a.gw + j] = 1;
    }
}

// exclusive position of this thread among the threads of the block whose `on` is set, and the block's total: ballot inside a
// wave, the waves' counts through LDS (stream_select_kernel's scan).  Every thread of the block calls it.
__device__ __forceinline__ int block_scan(bool on, int* wave_cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(on);
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < COV_WAVES; ++w) {
        const int k = wave_cnt[w];
        if (w < wave) off += k;
        total += k;
    }
    __syncthreads();                // the wave counts are rewritten by the next scan
    return off + __popcll(mask & ((1ull << lane) - 1ull));
}

// The thin step: which (frame, query) pairs are surplus.  Grid (ceil(n / COV_THREADS), rows): a block owns COV_THREADS queries j
// on row g (frame f1 - m + g) and walks the queries i from 0 up to its own last one in tiles of COV_THREADS.  Thread t puts the cell
// of query i0 + t on row g into LDS (-1: it does not count there; the row read is coalesced); behind the barrier every thread
// counts the entries equal to its own cell -- all lanes read the same LDS word, a broadcast -- among i < j: every entry of the
// tiles before the block's own, the entries below its own in the last.  over[g * n + j] = 1 where the count reaches per_cell.
__global__ __launch_bounds__(COV_THREADS) void cover_crowd_kernel(const CoverArgs a) {
    __shared__ int cells[COV_THREADS];
    const int tid = threadIdx.x, j0 = blockIdx.x * COV_THREADS;
    const int f0 = a.f1 - a.m;
    for (int g = blockIdx.y; g < a.m; g += gridDim.y) {
        const float* row = a.trajs + (size_t)g * a.n * 2;
        auto cell_of = [&](int i) {         // the cell of query i on row g, -1 where it does not count
            if (i >= a.n || a.tq[i] > f0 + g || a.flag[i] != COV_KEEP) return -1;      // (a pending query has tq > f1 - 1 >= f0 + g)
            const float x = row[2 * (size_t)i], y = row[2 * (size_t)i + 1];
            return cover_inside(a, x, y) ? cover_cell(a, x, y) : -1;
        };
        const int mine = cell_of(j0 + tid);
        int older = 0;
        for (int i0 = 0; i0 <= j0; i0 += COV_THREADS) {
            const bool own = i0 == j0;      // the last tile: the block's own queries, of which only those below the thread's count
            __syncthreads();                // (the tile before this one has been counted)
            cells[tid] = own ? mine : cell_of(i0 + tid);
            __syncthreads();
            const int end = own ? tid : COV_THREADS;
            for (int k = 0; k < end; ++k) older += cells[k] == mine ? 1 : 0;
        }
        if (j0 + tid < a.n) a.over[(size_t)g * a.n + j0 + tid] = (mine >= 0 && older >= a.per_cell) ? 1 : 0;
    }
}

// The thin step, a thread per query: the second run over the returned frames from t_q on, crowd = surplus ? crowd + 1 : 0 starting
// from crowd[c] (0 for a pending query); a started query that cover_flag_kernel kept is retired as crowded when that run reaches
// crowd_after; a query that is still kept and stands inside the frame marks its cell (every writer stores the same 1).
__global__ __launch_bounds__(COV_THREADS) void cover_settle_kernel(const CoverArgs a) {
    const int c = blockIdx.x * COV_THREADS + threadIdx.x;
    if (c >= a.n) return;
    const int t = a.tq[c];
    const bool pending = a.m == 0 || t > a.f1 - 1;
    unsigned run = 0u;
    float x, y;
    if (pending) {
        x = a.xy[2 * c];
        y = a.xy[2 * c + 1];
    } else {
        run = (unsigned)a.crowd[c];
        const int f0 = a.f1 - a.m;
        for (int g = 0; g < a.m; ++g) {
            if (f0 + g < t) continue;
            run = a.over[(size_t)g * a.n + c] != 0 ? run + 1u : 0u;
        }
        const size_t o = ((size_t)(a.m - 1) * a.n + c) * 2;
        x = a.trajs[o];
        y = a.trajs[o + 1];
    }
    int flag = a.flag[c];
    if (flag == COV_KEEP && !pending && (int)run >= a.crowd_after) a.flag[c] = flag = COV_CROWDED;
    a.crun[c] = (int)run;
    if (flag == COV_KEEP && cover_inside(a, x, y)) a.occ[cover_cell(a, x, y)] = 1;
}

// ONE block.  First the n flags in chunks of COV_THREADS: the kept queries of a chunk get consecutive slots of keep / lost_out on
// top of the offset carried from the chunks before, so both ascend.  Then the gh*gw cells the same way: the k-th empty cell in
// row-major order becomes seed k while k < max(0, max_queries - n_keep).  The four counts are written last.
// THIN: the kept also leave their second run in crowd_out; a retired query c, with `at` kept ones below it, is entry c - at of
// gone / reason, so both ascend with the columns; the crowded are scanned into a fifth count.
template <bool THIN>
__global__ __launch_bounds__(COV_THREADS) void cover_list_kernel(const CoverArgs a) {
    __shared__ int wave_cnt[COV_WAVES];
    const int tid = threadIdx.x;
    int n_keep = 0, n_out = 0, n_lost = 0, n_crowded = 0, tot;
    for (int c0 = 0; c0 < a.n; c0 += COV_THREADS) {
        const int c = c0 + tid;
        const int flag = c < a.n ? a.flag[c] : -1;
        const int at = n_keep + block_scan(flag == COV_KEEP, wave_cnt, tot);
        if (flag == COV_KEEP) {
            a.keep[at] = c;
            a.lost_out[at] = a.run[c];
            if (THIN) a.crowd_out[at] = a.crun[c];
        } else if (THIN && flag > COV_KEEP) {
            a.gone[c - at] = c;
            a.reason[c - at] = flag;
        }
        n_keep += tot;
        block_scan(flag == COV_OUTSIDE, wave_cnt, tot);
        n_out += tot;
        block_scan(flag == COV_LOST, wave_cnt, tot);
        n_lost += tot;
        if (THIN) {
            block_scan(flag == COV_CROWDED, wave_cnt, tot);
            n_crowded += tot;
        }
    }
    const int cap = max(a.max_queries - n_keep, 0), cells = a.gh * a.gw;
    const float t = (float)a.f1, fc = (float)a.cell;
    int n_empty = 0;
    for (int k0 = 0; k0 < cells && n_empty < cap; k0 += COV_THREADS) {      // (n_empty is the same in every thread)
        const int k = k0 + tid;
        const bool empty = k < cells && a.occ[k] == 0;
        const int at = n_empty + block_scan(empty, wave_cnt, tot);
        if (empty && at < cap) {
            const int i = k / a.gw, j = k % a.gw;
            a.seeds[3 * (size_t)at] = t;
            a.seeds[3 * (size_t)at + 1] = fminf(((float)j + 0.5f) * fc, (float)(a.W - 1));
            a.seeds[3 * (size_t)at + 2] = fminf(((float)i + 0.5f) * fc, (float)(a.H - 1));
        }
        n_empty += tot;
    }
    if (tid == 0) {
        a.counts[0] = n_keep;
        a.counts[1] = min(n_empty, cap);
        a.counts[2] = n_out;
        a.counts[3] = n_lost;
        if (THIN) a.counts[4] = n_crowded;
    }
}

CoverArgs cover_args(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy, const int* lost, int H,
                     int W, int cell, int gh, int gw, float vis_logit, int lost_after, int max_queries, int* keep, int* lost_out,
                     float* seeds, int* counts, int* workspace) {
    CoverArgs a = {};
    a.n = n; a.m = m; a.f1 = f1; a.trajs = trajs; a.vis = vis; a.tq = tq; a.xy = xy; a.lost = lost;
    a.H = H; a.W = W; a.cell = cell; a.gh = gh; a.gw = gw; a.vis_logit = vis_logit; a.lost_after = lost_after;
    a.max_queries = max_queries; a.keep = keep; a.lost_out = lost_out; a.seeds = seeds; a.counts = counts;
    a.flag = workspace; a.run = workspace + n; a.occ = workspace + 2 * (size_t)n;
    return a;
}

}  // namespace

size_t cover_workspace_ints(int n, int gh, int gw) { return 2 * (size_t)n + (size_t)gh * (size_t)gw; }
size_t cover_thin_workspace_ints(int n, int m, int gh, int gw) { return cover_workspace_ints(n, gh, gw) + (size_t)n + (size_t)m * (size_t)n; }

int launch_cover_step(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy, const int* lost,
                      int H, int W, int cell, int gh, int gw, float vis_logit, int lost_after, int max_queries, int* keep,
                      int* lost_out, float* seeds, int* counts, int* workspace, hipStream_t st) {
    const CoverArgs a = cover_args(n, m, f1, trajs, vis, tq, xy, lost, H, W, cell, gh, gw, vis_logit, lost_after, max_queries, keep,
                                   lost_out, seeds, counts, workspace);
    if (hipMemsetAsync(a.occ, 0, (size_t)gh * gw * sizeof(int), st) != hipSuccess) {
        set_error("cover_step: clearing the occupancy table failed");
        return PIPS_E_LAUNCH;
    }
    if (n > 0) {
        hipLaunchKernelGGL(cover_flag_kernel<true>, dim3((n + COV_THREADS - 1) / COV_THREADS), dim3(COV_THREADS), 0, st, a);
        PIPS_CHECK_LAUNCH("cover_flag");
    }
    hipLaunchKernelGGL(cover_list_kernel<false>, dim3(1), dim3(COV_THREADS), 0, st, a);
    PIPS_CHECK_LAUNCH("cover_list");
    return PIPS_OK;
}

int launch_cover_step_thin(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy, const int* lost,
                           const int* crowd, int H, int W, int cell, int gh, int gw, float vis_logit, int lost_after, int max_queries,
                           int per_cell, int crowd_after, int* keep, int* lost_out, int* crowd_out, float* seeds, int* gone,
                           int* reason, int* counts, int* workspace, hipStream_t st) {
    CoverArgs a = cover_args(n, m, f1, trajs, vis, tq, xy, lost, H, W, cell, gh, gw, vis_logit, lost_after, max_queries, keep, lost_out,
                             seeds, counts, workspace);
    a.crowd = crowd; a.per_cell = per_cell; a.crowd_after = crowd_after; a.crowd_out = crowd_out; a.gone = gone; a.reason = reason;
    a.crun = a.occ + (size_t)gh * gw; a.over = a.crun + n;
    if (hipMemsetAsync(a.occ, 0, (size_t)gh * gw * sizeof(int), st) != hipSuccess) {
        set_error("cover_step_thin: clearing the occupancy table failed");
        return PIPS_E_LAUNCH;
    }
    if (n > 0) {
        const int blocks = (n + COV_THREADS - 1) / COV_THREADS;
        hipLaunchKernelGGL(cover_flag_kernel<false>, dim3(blocks), dim3(COV_THREADS), 0, st, a);
        PIPS_CHECK_LAUNCH("cover_flag");
        if (m > 0) {
            hipLaunchKernelGGL(cover_crowd_kernel, dim3(blocks, m < COV_ROWS_MAX ? m : COV_ROWS_MAX), dim3(COV_THREADS), 0, st, a);
            PIPS_CHECK_LAUNCH("cover_crowd");
        }
        hipLaunchKernelGGL(cover_settle_kernel, dim3(blocks), dim3(COV_THREADS), 0, st, a);
        PIPS_CHECK_LAUNCH("cover_settle");
    }
    hipLaunchKernelGGL(cover_list_kernel<true>, dim3(1), dim3(COV_THREADS), 0, st, a);
    PIPS_CHECK_LAUNCH("cover_list");
    return PIPS_OK;
}

}  // namespace pips
