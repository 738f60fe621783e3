// Visibility-aware chaining (chain_demo.py:40-83) as device-side bookkeeping around pips_track_ring: the staging of one hop's
// windows (chain_gather_kernel) and the write-back, skip scan, window-start update and stable compaction of the particles that
// stay live (chain_step_kernel).  Window length 8 only: the reference's scan is written for frames 7..2 of an 8-frame window.
// Plain HIP; built with the default floating-point flags (NaN logits must stay NaN: a NaN row admits no frame and steps by 7).
#include "common.h"

namespace pips {

namespace {

constexpr int CHAIN_S = PIPS_S;
constexpr int CHAIN_THR = 64;        // thresholds 0.9, 0.88, ...: the scan of a non-NaN window ends at the 46th (thr < 0)
constexpr int STEP_THREADS = 256;
constexpr int STEP_WAVES = STEP_THREADS / 64;

struct ThrTable { float v[CHAIN_THR]; };

// chain_demo.py:64,75: thr = 0.9, then thr -= 0.02 in Python doubles; the tensor comparison rounds it to fp32
ThrTable build_thresholds() {
    ThrTable t;
    double thr = 0.9;
    for (int k = 0; k < CHAIN_THR; ++k) {
        t.v[k] = (float)thr;
        thr -= 0.02;
    }
    return t;
}
const ThrTable& thresholds() {
    static const ThrTable t = build_thresholds();
    return t;
}

// row of logical frame f in a buffer of L rows whose row 0 holds frame -base (Python's modulo: never negative)
__device__ __forceinline__ int chain_row(int f, int base, int L) {
    const int r = (f + base) % L;
    return r < 0 ? r + L : r;
}

// One block per active particle j (q = active[j]): its start position, window start, direction and carried features -- and, in a
// state that holds several videos (clip != null), the video it belongs to.
__global__ __launch_bounds__(PIPS_C) void chain_gather_kernel(const float* __restrict__ trajs, int L, int base, int n,
                                                              const int* __restrict__ cur, const int* __restrict__ dir,
                                                              const float* __restrict__ feat, const int* __restrict__ active,
                                                              int n_act, int sample_feat, float* __restrict__ xy,
                                                              int* __restrict__ ws, int* __restrict__ wd, float* __restrict__ fi,
                                                              const int* __restrict__ clip, int* __restrict__ wc) {
    const int j = blockIdx.x;
    if (j >= n_act) return;
    const int q = active[j];
    const bool ok = (unsigned)q < (unsigned)n;           // an index outside [0, n) is never dereferenced: zeros are staged for it
                                                         // and chain_step_kernel ignores it (include/pips_hip.h)
    const int t = threadIdx.x;
    if (t == 0) {
        const int c = ok ? cur[q] : 0;
        const size_t src = ((size_t)chain_row(c, base, L) * n + (ok ? q : 0)) * 2;
        xy[2 * j] = ok ? trajs[src] : 0.f;
        xy[2 * j + 1] = ok ? trajs[src + 1] : 0.f;
        ws[j] = c;
        wd[j] = (ok && dir != nullptr) ? dir[q] : 1;
        if (clip != nullptr) wc[j] = ok ? clip[q] : 0;
    }
    if (!sample_feat) fi[(size_t)j * PIPS_C + t] = ok ? feat[(size_t)q * PIPS_C + t] : 0.f;
}

struct StepArgs {
    const float* win_trajs;      // (8, n_act, 2)
    const float* win_vis;        // (8, n_act) logits
    const float* win_ffeat0;     // (n_act, 128), read with sample_feat
    const int* active;
    const int* dir;
    const int* clip;             // (n) video of each particle, or null: one video of T frames
    const int* clip_frames;      // (V) frames of each video
    float* trajs; float* vis; float* feat;
    int* cur; int* next_active; int* next_count; int* steps;
    int n, n_act, sample_feat, L, base, T, V;
    ThrTable thr;
};

// ONE block walks the active list in chunks of STEP_THREADS particles, a thread per particle: write-back of the window's rows,
// skip scan, new window start.  The live particles of a chunk get consecutive slots of next_active by a block scan (ballot
// inside a wave, the waves' counts through LDS) on top of the offset carried from the chunks before -- the order of `active`
// is kept, whatever the chunking.
__global__ __launch_bounds__(STEP_THREADS) void chain_step_kernel(const StepArgs a) {
    __shared__ int wave_cnt[STEP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carried = 0;
    for (int j0 = 0; j0 < a.n_act; j0 += STEP_THREADS) {
        const int j = j0 + tid;
        bool live = false;
        int q = 0;
        if (j < a.n_act) {
            q = a.active[j];
            if ((unsigned)q < (unsigned)a.n) {
                const int c = a.cur[q];
                const int d = (a.dir != nullptr && a.dir[q] < 0) ? -1 : 1;
                float p[CHAIN_S];
#pragma unroll
                for (int s = 0; s < CHAIN_S; ++s) {
                    const size_t w = (size_t)s * a.n_act + j;
                    const size_t o = (size_t)chain_row(c + d * s, a.base, a.L) * a.n + q;
                    const float lg = a.win_vis[w];
                    a.trajs[2 * o] = a.win_trajs[2 * w];                      // traj_e[cur:cur+8] = xys (chain_demo.py:59)
                    a.trajs[2 * o + 1] = a.win_trajs[2 * w + 1];
                    if (a.vis != nullptr) a.vis[o] = lg;
                    p[s] = 1.0f / (1.0f + expf(-lg));
                }
                // chain_demo.py:63-77: frames 7..2 against thr, lowered whenever the scan reaches frame 1; the latest admitted
                // frame of the first threshold that admits one.  NaN admits nothing: si stays 7 (argmax of all-false rows)
                int si = CHAIN_S - 1;
                bool found = false;
                for (int k = 0; k < CHAIN_THR && !found; ++k) {
                    const float thr = a.thr.v[k];
#pragma unroll
                    for (int s = CHAIN_S - 1; s >= 2; --s)
                        if (!found && p[s] > thr) { si = s; found = true; }
                }
                const int nc = c + d * si;
                a.cur[q] = nc;
                if (a.steps != nullptr) a.steps[j] = si;
                // inside the particle's own video (a video index outside the table is clamped into it, as the gather kernels do)
                const int Tq = a.clip != nullptr ? a.clip_frames[min(max(a.clip[q], 0), a.V - 1)] : a.T;
                live = nc >= 0 && nc < Tq;
            }
        }
        if (a.sample_feat) {           // the features of a particle's first window are carried from here on (chain_demo.py:57)
            const int cnt = min(STEP_THREADS, a.n_act - j0);
            for (int i = tid; i < cnt * PIPS_C; i += STEP_THREADS) {
                const int jj = j0 + i / PIPS_C, ch = i % PIPS_C;
                const int qq = a.active[jj];
                if ((unsigned)qq < (unsigned)a.n) a.feat[(size_t)qq * PIPS_C + ch] = a.win_ffeat0[(size_t)jj * PIPS_C + ch];
            }
        }
        const unsigned long long m = __ballot(live);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = carried, total = 0;
#pragma unroll
        for (int w = 0; w < STEP_WAVES; ++w) {
            const int cw = wave_cnt[w];
            if (w < wave) off += cw;
            total += cw;
        }
        if (live) a.next_active[off + __popcll(m & ((1ull << lane) - 1ull))] = q;
        carried += total;
        __syncthreads();                // wave_cnt is rewritten by the next chunk
    }
    if (tid == 0) *a.next_count = carried;
}

}  // namespace

float chain_threshold(int k) { return (k < 0 || k >= CHAIN_THR) ? 0.f : thresholds().v[k]; }

int launch_chain_gather(const float* trajs, int L, int base, int n, const int* cur, const int* dir, const float* feat,
                        const int* active, int n_act, int sample_feat, float* xy, int* ws, int* wd, float* fi, hipStream_t st,
                        const int* clip, int* wc) {
    hipLaunchKernelGGL(chain_gather_kernel, dim3(n_act), dim3(PIPS_C), 0, st, trajs, L, base, n, cur, dir, feat, active, n_act,
                       sample_feat, xy, ws, wd, fi, clip, wc);
    PIPS_CHECK_LAUNCH("chain_gather");
    return PIPS_OK;
}

int launch_chain_step(const float* win_trajs, const float* win_vis, const float* win_ffeat0, int n, const int* active, int n_act,
                      int sample_feat, float* trajs, float* vis, int L, int base, int T, int* cur, const int* dir, float* feat,
                      int* next_active, int* next_count, int* steps, hipStream_t st, const int* clip, const int* clip_frames, int V) {
    StepArgs a;
    a.win_trajs = win_trajs; a.win_vis = win_vis; a.win_ffeat0 = win_ffeat0; a.active = active; a.dir = dir;
    a.trajs = trajs; a.vis = vis; a.feat = feat; a.cur = cur; a.next_active = next_active; a.next_count = next_count; a.steps = steps;
    a.clip = clip; a.clip_frames = clip_frames; a.V = V;
    a.n = n; a.n_act = n_act; a.sample_feat = sample_feat; a.L = L; a.base = base; a.T = T;
    a.thr = thresholds();
    hipLaunchKernelGGL(chain_step_kernel, dim3(1), dim3(STEP_THREADS), 0, st, a);
    PIPS_CHECK_LAUNCH("chain_step");
    return PIPS_OK;
}

}  // namespace pips
