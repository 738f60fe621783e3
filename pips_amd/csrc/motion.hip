// Global motion from tracks (drivers.motion_fit, drivers.MotionEstimator, pips_motion_fit): a consensus similarity q = a p + t between
// consecutive rows of a trajectory tensor.  The rule (include/pips_hip.h) decides the consensus in integers on quarter-pixel
// positions, so flags, counts and sums are bit for bit drivers.motion_table_torch's, and the least-squares model on the inliers is
// formed from those integer sums by fp64 operations that are rounded once each (fp_rn.h), so it is too.  Plain HIP, three launches:
//   motion_compact_kernel   a block per pair quantises the valid columns and stores them in column order (a wave ballot and a prefix
//                           over the four waves in LDS: stable, no atomics), four int16 a column;
//   motion_score_kernel     a block per (pair, MOTION_HYPS hypotheses): a lane owns a hypothesis, the points go through LDS in tiles
//                           of MOTION_TILE, each wave walks a quarter of a tile -- every lane of a wave reads the same point, a
//                           broadcast -- and the block stores its best (score, hypothesis) key with a plain store.  A push returns
//                           a handful of rows: splitting a pair's hypotheses over blocks is what fills more of the GPU;
//   motion_select_kernel    a block per pair takes the largest key, tests every column against the winner, writes flags, the inlier
//                           sums, head and model.
// No atomics and no hand-off between the blocks of a launch.
// Motion layers (drivers.motion_layers, drivers.MotionLayers, pips_motion_layers): the same consensus peeled L times.  1 + 2 L + 1
// launches:
//   motion_compact_kernel<true>    the compact kernel, which also stores each entry's column and writes layer = 255 / 254;
//   motion_score_kernel            as it stands, per layer, on the layer's list with the layer's seed;
//   motion_layers_select_kernel    a block per pair takes the largest key, tests the LIST's entries against the winner, writes
//                                  layer[col] = l, the (pair, layer) rows with the box, and compacts the entries that stay into the
//                                  other of two ping-pong lists (the same ballot and prefix: stable);
//   motion_overlap_kernel          a block per pair counts the (layer now, layer before) codes with one ballot a code.
#include "common.h"
#include "fp_rn.h"

namespace pips {

namespace {

constexpr int MOTION_THREADS = 256;
constexpr int MOTION_WAVES = MOTION_THREADS / 64;
static_assert(MOTION_HYPS == 64, "a lane of wave 0 reduces one hypothesis");
static_assert(PIPS_MOTION_HYPS_MAX <= 1024 && PIPS_MOTION_N_MAX <= (1 << 16), "a key is score * 1024 + (1023 - h) in an int");
static_assert((long long)(PIPS_MOTION_ROWS_MAX - 1) * (PIPS_MOTION_HYPS_MAX / MOTION_HYPS) <= INT_MAX, "the score launch's grid fits an int");

typedef unsigned long long u64;

// quarter pixels: s = 4 v is exact in fp32; usable iff finite and |s| <= 8191 (a NaN compares false); rint is round-half-even
__device__ __forceinline__ bool motion_quarter(float x, float y, int& qx, int& qy) {
    const float sx = x * 4.0f, sy = y * 4.0f;
    const bool ok = fabsf(sx) <= (float)PIPS_MOTION_QUARTER_MAX && fabsf(sy) <= (float)PIPS_MOTION_QUARTER_MAX;
    qx = ok ? (int)rintf(sx) : 0;
    qy = ok ? (int)rintf(sy) : 0;
    return ok;
}

// column k of the pair that ends on row f: valid iff usable in rows f - 1 and f and, with vis, above the threshold in both
__device__ __forceinline__ bool motion_column(const float* __restrict__ trajs, const float* __restrict__ vis, int n, int f, int k,
                                              float vis_logit, int4& v) {
    const size_t a = ((size_t)(f - 1) * n + k), b = ((size_t)f * n + k);
    bool ok = motion_quarter(trajs[2 * a], trajs[2 * a + 1], v.x, v.y);
    ok = motion_quarter(trajs[2 * b], trajs[2 * b + 1], v.z, v.w) && ok;
    if (vis != nullptr) ok = ok && vis[a] > vis_logit && vis[b] > vis_logit;
    return ok;
}

__device__ __forceinline__ int2 motion_pack(const int4& v) {
    return make_int2((v.x & 0xffff) | (int)((unsigned)v.y << 16), (v.z & 0xffff) | (int)((unsigned)v.w << 16));
}
__device__ __forceinline__ int4 motion_unpack(const int2& w) {
    return make_int4((int)((unsigned)w.x << 16) >> 16, w.x >> 16, (int)((unsigned)w.y << 16) >> 16, w.y >> 16);
}

__device__ __forceinline__ unsigned motion_mix(unsigned seed, unsigned g, unsigned k) {
    unsigned u = seed + 0x9E3779B9u * (g + 1u) + 0x85EBCA6Bu * (k + 1u);
    u ^= u >> 16;
    u *= 0x85EBCA6Bu;
    u ^= u >> 13;
    u *= 0xC2B2AE35u;
    u ^= u >> 16;
    return u;
}

// Hypothesis h of frame g on the m valid points P: d = p_j - p_i, e = q_j - q_i, and r(k) = e (p_k - p_i) - d (q_k - q_i) as
// e p_k - d q_k - c with c = e p_i - d q_i.  |d|, |e| <= 16382 and |p|, |q| <= 8191 a component: every product fits 24 x 24 -> 32
// bits (v_mul_i32_i24, full rate), e p_k - d q_k and c stay below 2^30, r below 2^31.  rhs = thr4^2 |d|^2 < 2^50.
struct MotionHyp {
    int ex, ey, dx, dy, cre, cim;
    u64 rhs;
    bool ok;                                                                       // d != 0
};
__device__ __forceinline__ MotionHyp motion_hypothesis(const int2* __restrict__ P, int m, int g, int h, unsigned seed, int thr4) {
    const int i = (int)__umulhi(motion_mix(seed, (unsigned)g, 2u * (unsigned)h), (unsigned)m);
    int j = (int)__umulhi(motion_mix(seed, (unsigned)g, 2u * (unsigned)h + 1u), (unsigned)(m - 1));
    j += j >= i;
    const int4 a = motion_unpack(P[i]), b = motion_unpack(P[j]);
    MotionHyp H;
    H.dx = b.x - a.x, H.dy = b.y - a.y, H.ex = b.z - a.z, H.ey = b.w - a.w;
    H.cre = (__mul24(H.ex, a.x) - __mul24(H.ey, a.y)) - (__mul24(H.dx, a.z) - __mul24(H.dy, a.w));
    H.cim = (__mul24(H.ex, a.y) + __mul24(H.ey, a.x)) - (__mul24(H.dx, a.w) + __mul24(H.dy, a.z));
    H.rhs = (u64)(unsigned)(thr4 * thr4) * (u64)(unsigned)(__mul24(H.dx, H.dx) + __mul24(H.dy, H.dy));
    H.ok = (H.dx | H.dy) != 0;
    return H;
}
// |r|^2 <= rhs for the point v = (p, q); the caller looks at H.ok
__device__ __forceinline__ bool motion_inlier(const MotionHyp& H, const int4& v) {
    const int rre = __mul24(H.ex, v.x) - __mul24(H.ey, v.y) - __mul24(H.dx, v.z) + __mul24(H.dy, v.w) - H.cre;
    const int rim = __mul24(H.ex, v.y) + __mul24(H.ey, v.x) - __mul24(H.dx, v.w) - __mul24(H.dy, v.z) - H.cim;
    const unsigned ar = (unsigned)abs(rre), ai = (unsigned)abs(rim);
    return (u64)ar * ar + (u64)ai * ai <= H.rhs;                                   // two 32 x 32 -> 64 products, each < 2^62
}

// The least-squares similarity on the inliers from their sums S, (1, 0, 0, 0) without a model.  D > 0: the winner's two points are
// inliers with different p.  Everything below 2^61; an int64 -> fp64 conversion, a product, a difference and a quotient are each
// rounded once
__device__ __forceinline__ void motion_model(const long long* S, bool have, double& are, double& aim, double& tx, double& ty) {
    are = 1.0, aim = 0.0, tx = 0.0, ty = 0.0;
    if (have) {
        const long long N = S[0];
        const long long D = N * S[5] - (S[1] * S[1] + S[2] * S[2]);
        const long long A = N * S[6] - (S[1] * S[3] + S[2] * S[4]);
        const long long B = N * S[7] - (S[1] * S[4] - S[2] * S[3]);
        const double spx = (double)S[1], spy = (double)S[2], sqx = (double)S[3], sqy = (double)S[4], n4 = (double)(4 * N);
        are = (double)A / (double)D;
        aim = (double)B / (double)D;
        tx = sub_rn(sqx, sub_rn(mul_rn(are, spx), mul_rn(aim, spy))) / n4;
        ty = sub_rn(sqy, add_rn(mul_rn(aim, spx), mul_rn(are, spy))) / n4;
    }
}

// One block per pair: pts[pair][0..m) = the valid columns in column order, cnt[pair] = m.  LAYERS (pips_motion_layers): the column
// of each entry beside it in col[pair][0..m), and layer[pair][k] = 254 for a valid column, 255 for any other.
template <bool LAYERS>
__global__ __launch_bounds__(MOTION_THREADS) void motion_compact_kernel(const float* __restrict__ trajs, const float* __restrict__ vis,
                                                                        int n, float vis_logit, int2* __restrict__ pts,
                                                                        int* __restrict__ cnt, int* __restrict__ col,
                                                                        unsigned char* __restrict__ layer) {
    __shared__ int wave_n[MOTION_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    int2* out = pts + (size_t)pair * n;
    int run = 0;
    for (int base = 0; base < n; base += MOTION_THREADS) {
        const int k = base + tid;
        int4 v = make_int4(0, 0, 0, 0);
        const bool ok = k < n && motion_column(trajs, vis, n, pair + 1, k, vis_logit, v);
        const u64 mask = __ballot(ok);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < MOTION_WAVES; ++w) {
            const int c = wave_n[w];
            before += w < wave ? c : 0;
            total += c;
        }
        const int at = run + before + __popcll(mask & ((1ull << lane) - 1ull));    // < m <= n where ok
        if (ok) out[at] = motion_pack(v);
        if (LAYERS) {
            if (ok) col[(size_t)pair * n + at] = k;
            if (k < n) layer[(size_t)pair * n + k] = ok ? 254 : 255;
        }
        run += total;
        __syncthreads();
    }
    if (tid == 0) cnt[pair] = run;
}

// One block per (pair, 256 / SPLIT hypotheses): part[pair][b] = max over the block's hypotheses h < K of score * 1024 + (1023 - h)
// -- the highest score, ties to the lowest h -- or 0 when the pair has fewer than two valid points.  SPLIT waves share a group of
// 64 hypotheses and walk a part of each tile each.  SPLIT = 4 (MOTION_HYPS hypotheses a block) is the product; SPLIT = 1, every wave
// with hypotheses of its own -- one block per pair at K = 256 --, exists in a tuning build only (tools/motion_bench.py times both).
template <int SPLIT>
__global__ __launch_bounds__(MOTION_THREADS) void motion_score_kernel(const int2* __restrict__ pts, const int* __restrict__ cnt, int n,
                                                                      int K, int NB, int frame0, int thr4, unsigned seed,
                                                                      int* __restrict__ part) {
    constexpr int GROUPS = MOTION_WAVES / SPLIT;
    __shared__ int4 tile[MOTION_TILE];
    __shared__ int wave_score[MOTION_WAVES][MOTION_HYPS];
    const int pair = blockIdx.x / NB, b = blockIdx.x % NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = cnt[pair];
    const int2* P = pts + (size_t)pair * n;
    const int h = (b * GROUPS + wave / SPLIT) * MOTION_HYPS + lane;
    int key = 0;
    if (m >= 2) {                                                                  // (the same in every thread of the block)
        const MotionHyp H = motion_hypothesis(P, m, frame0 + pair + 1, h < K ? h : 0, seed, thr4);
        int score = 0;
        for (int t0 = 0; t0 < m; t0 += MOTION_TILE) {
            const int tn = min(MOTION_TILE, m - t0);
            __syncthreads();
            for (int i = tid; i < tn; i += MOTION_THREADS) tile[i] = motion_unpack(P[t0 + i]);
            __syncthreads();
            const int per = (tn + SPLIT - 1) / SPLIT, k0 = (wave % SPLIT) * per, k1 = min(tn, k0 + per);
#pragma unroll 4
            for (int k = k0; k < k1; ++k) score += motion_inlier(H, tile[k]) ? 1 : 0;
        }
        wave_score[wave][lane] = H.ok ? score : 0;
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                const int hg = (b * GROUPS + g) * MOTION_HYPS + lane;
                score = 0;
#pragma unroll
                for (int w = 0; w < SPLIT; ++w) score += wave_score[g * SPLIT + w][lane];
                key = max(key, hg < K ? score * 1024 + (1023 - hg) : 0);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) key = max(key, __shfl_xor(key, off, 64));
        }
    }
    if (tid == 0) part[(size_t)pair * NB + b] = key;
}

// One block per pair: the winner of the pair's keys, every column against it, flags, the sums over the inliers, head and model.
// cnt == NULL (n == 0): a pair without points.
__global__ __launch_bounds__(MOTION_THREADS) void motion_select_kernel(const float* __restrict__ trajs, const float* __restrict__ vis,
                                                                       int n, int NB, int frame0, float vis_logit, int thr4,
                                                                       unsigned seed, const int2* __restrict__ pts,
                                                                       const int* __restrict__ cnt, const int* __restrict__ part,
                                                                       int* __restrict__ head, long long* __restrict__ sums,
                                                                       double* __restrict__ model, unsigned char* __restrict__ flags) {
    __shared__ long long wave_sum[MOTION_WAVES][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    const int m = cnt != nullptr ? cnt[pair] : 0;
    int key = 0;
    if (m >= 2)
        for (int b = 0; b < NB; ++b) key = max(key, part[(size_t)pair * NB + b]);
    const int h_best = 1023 - (key & 1023);
    const bool have = m >= 2 && (key >> 10) >= 2;
    MotionHyp H = {};
    if (have) H = motion_hypothesis(pts + (size_t)pair * n, m, frame0 + pair + 1, h_best, seed, thr4);
    long long S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += MOTION_THREADS) {
        int4 v;
        const bool ok = motion_column(trajs, vis, n, pair + 1, k, vis_logit, v);
        const bool in = have && ok && motion_inlier(H, v);                         // (have: the winner has d != 0)
        if (in) {
            S[0] += 1, S[1] += v.x, S[2] += v.y, S[3] += v.z, S[4] += v.w;
            S[5] += __mul24(v.x, v.x) + __mul24(v.y, v.y);
            S[6] += __mul24(v.x, v.z) + __mul24(v.y, v.w);
            S[7] += __mul24(v.x, v.w) - __mul24(v.y, v.z);
        }
        flags[(size_t)pair * n + k] = in ? 2 : ok ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) S[e] += __shfl_xor(S[e], off, 64);
        if (lane == 0) wave_sum[wave][e] = S[e];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            S[e] = 0;
#pragma unroll
            for (int w = 0; w < MOTION_WAVES; ++w) S[e] += wave_sum[w][e];
            sums[(size_t)pair * 8 + e] = S[e];
        }
        head[4 * pair] = m, head[4 * pair + 1] = (int)S[0], head[4 * pair + 2] = have ? h_best : -1, head[4 * pair + 3] = 0;
        double are, aim, tx, ty;
        motion_model(S, have, are, aim, tx, ty);
        model[4 * pair] = are, model[4 * pair + 1] = aim, model[4 * pair + 2] = tx, model[4 * pair + 3] = ty;
    }
}

// ---- motion layers
// One block per pair, layer l: the winner of the pair's keys, the m entries of the layer's list against it.  An inlier's column gets
// layer = l and goes into the sums and the box; every other entry goes to the `next` list in its order (with no model that is every
// entry), whose length replaces cnt[pair].  Row pair * L + l of head, sums, model and box.  cnt == NULL (n == 0): a pair without points.
__global__ __launch_bounds__(MOTION_THREADS) void motion_layers_select_kernel(int n, int NB, int frame0, int thr4, unsigned seed, int l,
                                                                              int L, int need, const int2* __restrict__ pts,
                                                                              const int* __restrict__ col, int2* __restrict__ next_pts,
                                                                              int* __restrict__ next_col, int* __restrict__ cnt,
                                                                              const int* __restrict__ part, int* __restrict__ head,
                                                                              long long* __restrict__ sums, double* __restrict__ model,
                                                                              int* __restrict__ box, unsigned char* __restrict__ layer) {
    __shared__ long long wave_sum[MOTION_WAVES][8];
    __shared__ int wave_box[MOTION_WAVES][4];
    __shared__ int wave_n[MOTION_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    const int m = cnt != nullptr ? cnt[pair] : 0;
    int key = 0;
    if (m >= 2)
        for (int b = 0; b < NB; ++b) key = max(key, part[(size_t)pair * NB + b]);
    const int h_best = 1023 - (key & 1023);
    const bool have = m >= 2 && (key >> 10) >= need;                               // (need >= 2)
    const int2* P = pts + (size_t)pair * n;
    MotionHyp H = {};
    if (have) H = motion_hypothesis(P, m, frame0 + pair + 1, h_best, seed, thr4);
    long long S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = INT_MIN, hi_y = INT_MIN;
    int run = 0;
    for (int base = 0; base < m; base += MOTION_THREADS) {                         // (m is the same in every thread)
        const int i = base + tid;
        int2 w = make_int2(0, 0);
        int c = 0;
        if (i < m) w = P[i], c = col[(size_t)pair * n + i];
        const int4 v = motion_unpack(w);
        const bool in = have && i < m && motion_inlier(H, v);                      // (have: the winner has d != 0)
        const bool stay = i < m && !in;
        if (in) {
            S[0] += 1, S[1] += v.x, S[2] += v.y, S[3] += v.z, S[4] += v.w;
            S[5] += __mul24(v.x, v.x) + __mul24(v.y, v.y);
            S[6] += __mul24(v.x, v.z) + __mul24(v.y, v.w);
            S[7] += __mul24(v.x, v.w) - __mul24(v.y, v.z);
            lo_x = min(lo_x, v.z), lo_y = min(lo_y, v.w), hi_x = max(hi_x, v.z), hi_y = max(hi_y, v.w);
            layer[(size_t)pair * n + c] = (unsigned char)l;                        // c < n: a column the compact kernel stored
        }
        const u64 mask = __ballot(stay);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < MOTION_WAVES; ++k) {
            const int t = wave_n[k];
            before += k < wave ? t : 0;
            total += t;
        }
        if (stay) {
            const size_t at = (size_t)pair * n + run + before + __popcll(mask & ((1ull << lane) - 1ull));   // run + .. < m <= n
            next_pts[at] = w, next_col[at] = c;
        }
        run += total;
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) S[e] += __shfl_xor(S[e], off, 64);
        if (lane == 0) wave_sum[wave][e] = S[e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo_x = min(lo_x, __shfl_xor(lo_x, off, 64)), lo_y = min(lo_y, __shfl_xor(lo_y, off, 64));
        hi_x = max(hi_x, __shfl_xor(hi_x, off, 64)), hi_y = max(hi_y, __shfl_xor(hi_y, off, 64));
    }
    if (lane == 0) wave_box[wave][0] = lo_x, wave_box[wave][1] = lo_y, wave_box[wave][2] = hi_x, wave_box[wave][3] = hi_y;
    __syncthreads();
    if (tid == 0) {
        const size_t row = (size_t)pair * L + l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            S[e] = 0;
#pragma unroll
            for (int w = 0; w < MOTION_WAVES; ++w) S[e] += wave_sum[w][e];
            sums[row * 8 + e] = S[e];
        }
#pragma unroll
        for (int w = 1; w < MOTION_WAVES; ++w) {
            lo_x = min(lo_x, wave_box[w][0]), lo_y = min(lo_y, wave_box[w][1]);
            hi_x = max(hi_x, wave_box[w][2]), hi_y = max(hi_y, wave_box[w][3]);
        }
        head[4 * row] = m, head[4 * row + 1] = (int)S[0], head[4 * row + 2] = have ? h_best : -1, head[4 * row + 3] = 0;
        box[4 * row] = have ? lo_x : 0, box[4 * row + 1] = have ? lo_y : 0, box[4 * row + 2] = have ? hi_x : 0;
        box[4 * row + 3] = have ? hi_y : 0;
        double are, aim, tx, ty;
        motion_model(S, have, are, aim, tx, ty);
        model[4 * row] = are, model[4 * row + 1] = aim, model[4 * row + 2] = tx, model[4 * row + 3] = ty;
        if (cnt != nullptr) cnt[pair] = run;
    }
}

// One block per pair: overlap[pair][a][b] = the columns with layer a in this pair and layer b in the pair before -- the row above,
// or `prev_layer` for the first pair of the call (NULL: zeros).  Lane c of a wave keeps the count of the code c = a L + b, from one
// ballot a code; the waves meet in LDS.  Labels of L and above (254, 255) count nowhere.
__global__ __launch_bounds__(MOTION_THREADS) void motion_overlap_kernel(const unsigned char* __restrict__ layer,
                                                                        const unsigned char* __restrict__ prev_layer, int n, int L,
                                                                        int* __restrict__ overlap) {
    __shared__ int wave_count[MOTION_WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    const unsigned char* now = layer + (size_t)pair * n;
    const unsigned char* before = pair > 0 ? now - n : prev_layer;
    const int codes = L * L;                                                        // <= 64
    int count = 0;
    if (before != nullptr)
        for (int base = 0; base < n; base += MOTION_THREADS) {
            const int k = base + tid;
            int code = -1;
            if (k < n) {
                const int a = now[k], b = before[k];
                code = a < L && b < L ? a * L + b : -1;
            }
            if (__ballot(code >= 0) == 0ull) continue;                             // (the same in every lane of the wave)
            for (int c = 0; c < codes; ++c) {
                const int t = __popcll(__ballot(code == c));
                count += lane == c ? t : 0;
            }
        }
    wave_count[wave][lane] = count;
    __syncthreads();
    if (tid < codes) {
        count = 0;
#pragma unroll
        for (int w = 0; w < MOTION_WAVES; ++w) count += wave_count[w][tid];
        overlap[(size_t)pair * codes + tid] = count;
    }
}

}  // namespace

int launch_motion_fit(const float* trajs, const float* vis, int F, int n, int frame0, float vis_logit, int K, int thr4, unsigned seed,
                      int* head, long long* sums, double* model, unsigned char* flags, void* workspace, hipStream_t st) {
    const int pairs = F - 1;
    int NB = motion_blocks(K);
    const dim3 block(MOTION_THREADS);
    int2* pts = (int2*)workspace;
    int* cnt = n > 0 ? (int*)((char*)workspace + (size_t)pairs * n * 8) : nullptr;
    int* part = n > 0 ? cnt + pairs : nullptr;
    if (n > 0) {
        hipLaunchKernelGGL(motion_compact_kernel<false>, dim3((unsigned)pairs), block, 0, st, trajs, vis, n, vis_logit, pts, cnt,
                           (int*)nullptr, (unsigned char*)nullptr);
        PIPS_CHECK_LAUNCH("motion_compact");
#ifdef PIPS_TUNING
        if (PIPS_TUNE("PIPS_MOTION_ONE_BLOCK", 0)) {                               // 256 hypotheses a block: fewer keys, the same workspace
            NB = (K + MOTION_THREADS - 1) / MOTION_THREADS;
            hipLaunchKernelGGL(motion_score_kernel<1>, dim3((unsigned)(pairs * NB)), block, 0, st, (const int2*)pts, (const int*)cnt, n, K,
                               NB, frame0, thr4, seed, part);
        } else
#endif
            hipLaunchKernelGGL(motion_score_kernel<MOTION_WAVES>, dim3((unsigned)(pairs * NB)), block, 0, st, (const int2*)pts,
                               (const int*)cnt, n, K, NB, frame0, thr4, seed, part);
        PIPS_CHECK_LAUNCH("motion_score");
    }
    hipLaunchKernelGGL(motion_select_kernel, dim3((unsigned)pairs), block, 0, st, trajs, vis, n, NB, frame0, vis_logit, thr4, seed,
                       (const int2*)pts, (const int*)cnt, (const int*)part, head, sums, model, flags);
    PIPS_CHECK_LAUNCH("motion_select");
    return PIPS_OK;
}

int launch_motion_layers(const float* trajs, const float* vis, const unsigned char* prev_layer, int F, int n, int frame0,
                         float vis_logit, int K, int thr4, unsigned seed, int L, int min_in, int* head, long long* sums, double* model,
                         int* box, unsigned char* layer, int* overlap, void* workspace, hipStream_t st) {
    const int pairs = F - 1, NB = motion_blocks(K);
    const dim3 block(MOTION_THREADS), grid((unsigned)pairs);
    const size_t slots = (size_t)pairs * n;
    int2* pts[2] = {(int2*)workspace, (int2*)workspace + slots};
    int* col[2] = {(int*)((char*)workspace + slots * 16), (int*)((char*)workspace + slots * 20)};
    int* cnt = n > 0 ? (int*)((char*)workspace + slots * 24) : nullptr;
    int* part = n > 0 ? cnt + pairs : nullptr;
    if (n > 0) {
        hipLaunchKernelGGL(motion_compact_kernel<true>, grid, block, 0, st, trajs, vis, n, vis_logit, pts[0], cnt, col[0], layer);
        PIPS_CHECK_LAUNCH("motion_layers_compact");
    }
    for (int l = 0; l < L; ++l) {
        const unsigned seed_l = seed + (unsigned)l * 0x632BE5ABu;
        const int from = l & 1, to = from ^ 1;
        if (n > 0) {
            hipLaunchKernelGGL(motion_score_kernel<MOTION_WAVES>, dim3((unsigned)(pairs * NB)), block, 0, st, (const int2*)pts[from],
                               (const int*)cnt, n, K, NB, frame0, thr4, seed_l, part);
            PIPS_CHECK_LAUNCH("motion_layers_score");
        }
        hipLaunchKernelGGL(motion_layers_select_kernel, grid, block, 0, st, n, NB, frame0, thr4, seed_l, l, L, l == 0 ? 2 : min_in,
                           (const int2*)pts[from], (const int*)col[from], pts[to], col[to], cnt, (const int*)part, head, sums, model,
                           box, layer);
        PIPS_CHECK_LAUNCH("motion_layers_select");
    }
    hipLaunchKernelGGL(motion_overlap_kernel, grid, block, 0, st, (const unsigned char*)layer, prev_layer, n, L, overlap);
    PIPS_CHECK_LAUNCH("motion_overlap");
    return PIPS_OK;
}

}  // namespace pips
