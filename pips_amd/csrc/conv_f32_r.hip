// The 64 -> 64, 3x3 / stride 1 / pad 1 convolutions of the fp32 encoder's layer 1 (nets/pips.py:135-136,173-181) with BOTH operands
// resident in LDS -- the exact-fp32 counterpart of conv3x3_c64_bf16_kernel (conv_bf16_c64.hip).
//
// conv3x3_f32_t4_kernel<0> stages the pixel operand once per filter tap: every input value goes global -> registers -> LDS nine
// times, with a barrier per stage.  Here a persistent block keeps the weights of ALL nine taps of its 32 output channels in LDS
// (9 x 32 rows) and the input patch of a 4-row x 32-column output tile with its one-pixel halo (6 x 34 pixels), staged ONCE per tile:
// the K loop holds fragment reads at static offsets and MFMAs only -- no global load, no LDS write, no barrier.  The fragment of tap
// (kh, kw) is the patch base + (kh PW + kw) rows.  Rows (a pixel's / an output channel's 64 input channels = 256 B) are padded to
// 272 B: the lanes of a ds_read_b128 group fall on different 16-byte bank groups.  LDS: 78 336 + 55 488 = 133 824 B, one block per
// compute unit.  One wave per image row of the tile: 32 pixels x 32 channels = ONE v_mfma_f32_32x32x2_f32 accumulator, 288 MFMAs a
// tile in one chain.  The grid covers the output channels in two halves; the two blocks of a patch run side by side on one XCD.
//
// The next tile's patch is fetched into registers (13 x 16 B per thread) at the start of the current tile and written to LDS between
// the two barriers of the tile switch -- the only barriers of a tile.  in_norm (optional): {mean, rstd} per (frame, input channel)
// of the PRODUCING layer; every staged value becomes fmaxf((x - mean) * rstd, 0) -- the three operations of inorm_apply_kernel<0>
// (encoder.hip) in its order, so the staged value is bitwise that kernel's output and the normalised map never goes to memory.
// Pieces outside the image are fetched out of the frame's buffer range (zeros) and are NOT normalised: the padding stays zero.
//
// K order: igemm_f32_kernel<..., CONV>'s and conv3x3_f32_t4_kernel's -- tap-major, 32 channels per stage, lane halves on the K values
// (k, k + 4), one chain per output value, + bias at the end: the output map is BITWISE theirs.  The InstanceNorm partials
// {sum(x - p), sum((x - p)^2), p, n} come one per (wave, channel): 4 ceil(H / 4) ceil(W / 32) parts per frame.
#include "common.h"

namespace pips {

constexpr int CR_ROWS = 4, CR_COLS = 32, CR_TN = 32, CR_PITCH = 272;
constexpr int CR_PW = CR_COLS + 2, CR_PH = CR_ROWS + 2;
constexpr int CR_WBYTES = 9 * CR_TN * CR_PITCH, CR_PBYTES = CR_PH * CR_PW * CR_PITCH;
constexpr int CR_LDS = CR_WBYTES + CR_PBYTES;
constexpr int CR_NCH = CR_PH * CR_PW * 16, CR_NIT = (CR_NCH + 255) / 256;       // 16-byte pieces of a patch; pieces per thread (13)
constexpr unsigned CR_OOB = 0x80000000u;                                         // an offset outside every buffer range

struct ConvRArgs {
    const float* in; const float* wgt; const float* bias; float* out; float* stats; const float* in_norm;
    int H, W, tiles_x, tiles, bph;      // tiles: 4 x 32 tiles of a frame; bph: blocks per frame and channel half
    int by_xcd;                         // frames % 8 == 0: all blocks of a frame run on ONE XCD (block & 7 = frame & 7)
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// grid = frames x 2 channel halves x bph blocks; block (f, hc, b) walks tiles b, b + bph, ... of frame f
__global__ __launch_bounds__(256) void conv3x3_c64_f32_r_kernel(ConvRArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Wl = smem;
    char* Pl = smem + CR_WBYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int H = p.H, W = p.W;
    int f, rem;
    if (p.by_xcd) {
        const int per = 16 * p.bph, grp = blockIdx.x / per, j = blockIdx.x - grp * per;
        f = 8 * grp + (j & 7); rem = j >> 3;
    } else {
        f = blockIdx.x / (2 * p.bph); rem = blockIdx.x - f * (2 * p.bph);
    }
    const int hc = rem & 1, b = rem >> 1;                   // the two halves of a patch are neighbours in the launch order

    // weights [cout][kh][kw][cin] -> LDS [tap][cout of this half][cin]: all 18 pieces of a thread in flight before the first is written
    {
        constexpr int NW = 9 * CR_TN * 16 / 256;
        float4 wv[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int i = tid + 256 * k, row = i >> 4, tap = row >> 5, co = row & 31;
            wv[k] = *reinterpret_cast<const float4*>(p.wgt + ((size_t)(hc * CR_TN + co) * 9 + tap) * 64 + (i & 15) * 4);
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int i = tid + 256 * k;
            *reinterpret_cast<float4*>(Wl + (i >> 4) * CR_PITCH + (i & 15) * 16) = wv[k];
        }
    }

    // the frame's map as a buffer: offsets above and below the image lie outside its range and read as zero
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in + (size_t)f * H * W * 64), (short)0, (int)((unsigned)(H * W) * 256u), 0x00020000);
    // piece i = tid + 256 it of a patch = (patch pixel i >> 4, 16-byte chunk c = tid & 15 -- the same for every piece of a thread)
    const int chunk = tid & 15;
    unsigned goff[CR_NIT], pyx[CR_NIT];                      // byte offset from the patch's first pixel (y0 - 1, x0 - 1); py | px << 8
#pragma unroll
    for (int it = 0; it < CR_NIT; ++it) {
        const int pix = (tid >> 4) + it * 16;
        const int py = pix / CR_PW, px = pix - py * CR_PW;
        goff[it] = (unsigned)((py * W + px) * 256 + chunk * 16);
        pyx[it] = (unsigned)(py | px << 8);
    }
    const bool last_ok = tid + (CR_NIT - 1) * 256 < CR_NCH;
    char* lds_dst = Pl + (tid >> 4) * CR_PITCH + chunk * 16;                     // + it * 16 rows
    float4 nrm[2] = {make_float4(0.f, 1.f, 0.f, 1.f), make_float4(0.f, 1.f, 0.f, 1.f)};     // {mean, rstd} of this thread's 4 channels
    if (p.in_norm != nullptr) {
        const float4* np = reinterpret_cast<const float4*>(p.in_norm + ((size_t)f * 64 + chunk * 4) * 2);
        nrm[0] = np[0]; nrm[1] = np[1];
    }

    u32x4 fr[CR_NIT];                                       // the fetched patch
    unsigned inside = 0;                                    // which pieces of it lie inside the image (bit per piece)
    // (every vector-memory instruction of the tile loop is issued unconditionally, masked lanes and the fetch behind the last tile with
    // an out-of-range offset: the compiler then counts the loads and stores in flight exactly, and the wait for the patch in stage()
    // leaves the stores of the tile before in flight -- under a branch it waits for them as well, 2-3 us per tile)
    auto fetch = [&](int t, bool live) __attribute__((always_inline)) {
        const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
        const int y0 = ty * CR_ROWS, x0 = tx * CR_COLS;
        const unsigned base = (unsigned)(((y0 - 1) * W + (x0 - 1)) * 256);        // wraps below zero on the first row: out of range
        const bool interior = y0 >= 1 && y0 + CR_ROWS + 1 <= H && x0 >= 1 && x0 + CR_COLS + 1 <= W;
        if (interior) {
            inside = last_ok ? (1u << CR_NIT) - 1 : (1u << (CR_NIT - 1)) - 1;
#pragma unroll
            for (int it = 0; it < CR_NIT; ++it) {
                const unsigned off = (live && (it + 1 < CR_NIT || last_ok)) ? base + goff[it] : CR_OOB;
                fr[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0);
            }
        } else {
            inside = 0;
#pragma unroll
            for (int it = 0; it < CR_NIT; ++it) {
                const int gy = y0 - 1 + (int)(pyx[it] & 0xff), gx = x0 - 1 + (int)(pyx[it] >> 8);
                const bool ok = live && (it + 1 < CR_NIT || last_ok) && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
                inside |= ok ? 1u << it : 0u;
                fr[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(ok ? base + goff[it] : CR_OOB), 0, 0);
            }
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < CR_NIT; ++it) {
            if (it + 1 < CR_NIT || last_ok) {
                float4 v = make_float4(__uint_as_float(fr[it].x), __uint_as_float(fr[it].y), __uint_as_float(fr[it].z),
                                       __uint_as_float(fr[it].w));
                if (p.in_norm != nullptr) {                                       // (uniform) pieces outside the image stay zero: a select
                    const bool in = inside >> it & 1;
                    const float nx = fmaxf((v.x - nrm[0].x) * nrm[0].y, 0.f), ny = fmaxf((v.y - nrm[0].z) * nrm[0].w, 0.f);
                    const float nz = fmaxf((v.z - nrm[1].x) * nrm[1].y, 0.f), nw = fmaxf((v.w - nrm[1].z) * nrm[1].w, 0.f);
                    v = make_float4(in ? nx : 0.f, in ? ny : 0.f, in ? nz : 0.f, in ? nw : 0.f);
                }
                *reinterpret_cast<float4*>(lds_dst + it * (16 * CR_PITCH)) = v;
            }
        }
    };

    const int col = hc * CR_TN + l31;
    const float bv = p.bias[col];
    const char* pa = Pl + (wave * CR_PW + l31) * CR_PITCH + half * 16;           // patch pixel (wave + kh, l31 + kw), K values 4 half ..
    const char* pb = Wl + l31 * CR_PITCH + half * 16;                            // weight row (tap, l31)
    // output map and partials of the frame as buffers: a masked lane stores to an out-of-range offset (dropped)
    const int parts = p.tiles * 4;
    const __amdgpu_buffer_rsrc_t rsrc_out = __builtin_amdgcn_make_buffer_rsrc(
        p.out + (size_t)f * H * W * 64, (short)0, (int)((unsigned)(H * W) * 256u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_st = __builtin_amdgcn_make_buffer_rsrc(
        p.stats + (size_t)f * parts * 256, (short)0, (int)((unsigned)parts * 1024u), 0x00020000);

    // bias, statistics and weights have landed before the loop: a load still pending at the loop head is waited for inside the loop
    // with a count that also drains the patch prefetch
    float bvs = bv;
    asm volatile("" : "+v"(bvs), "+v"(nrm[0].x), "+v"(nrm[0].y), "+v"(nrm[0].z), "+v"(nrm[0].w), "+v"(nrm[1].x), "+v"(nrm[1].y),
                 "+v"(nrm[1].z), "+v"(nrm[1].w));
    fetch(b, true);
    // 17 stores to nowhere: the loop head then sees the same vector-memory queue from the prologue as from the loop's back edge (a
    // patch prefetch followed by a tile's 16 + 1 stores), and the compiler's wait for the patch leaves the stores in flight on both
    // paths; with an empty queue from the prologue it assumes the shorter one and waits for the stores of every tile
#pragma unroll
    for (int r = 0; r < 16; ++r) __builtin_amdgcn_raw_buffer_store_b32((unsigned)r, rsrc_out, (int)(CR_OOB + 256u * r), 0, 0);   // (distinct: not merged)
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsrc_st, (int)CR_OOB, 0, 0);
    for (int t = b; t < p.tiles; t += p.bph) {
        lds_barrier();                                      // the previous tile's fragment reads are done (first tile: Wl is written)
        stage();
        lds_barrier();
        fetch(t + p.bph < p.tiles ? t + p.bph : t, t + p.bph < p.tiles);
        __builtin_amdgcn_sched_barrier(0);

        // ---- 72 groups (tap, 32-channel block, 8 K values) of 2 fragment reads + 4 MFMAs, fragments requested CR_AHEAD groups ahead
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        constexpr int CR_AHEAD = 2, CR_NBUF = 3;
        float4 fa[CR_NBUF], fb[CR_NBUF];
#define PIPS_CR_LOAD(g_)                                                                                                \
        {                                                                                                               \
            constexpr int tap_ = (g_) / 8, kb_ = (g_) % 8, kh_ = tap_ / 3, kw_ = tap_ % 3, buf_ = (g_) % CR_NBUF;         \
            fa[buf_] = *reinterpret_cast<const float4*>(pa + (kh_ * CR_PW + kw_) * CR_PITCH + kb_ * 32);                 \
            fb[buf_] = *reinterpret_cast<const float4*>(pb + tap_ * (CR_TN * CR_PITCH) + kb_ * 32);                      \
        }
#define PIPS_CR_STEP(g_)                                                                                                \
        if constexpr ((g_) + CR_AHEAD < 72) PIPS_CR_LOAD((g_) + CR_AHEAD)                                               \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[(g_) % CR_NBUF].x, fb[(g_) % CR_NBUF].x, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[(g_) % CR_NBUF].y, fb[(g_) % CR_NBUF].y, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[(g_) % CR_NBUF].z, fb[(g_) % CR_NBUF].z, acc, 0, 0, 0);            \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[(g_) % CR_NBUF].w, fb[(g_) % CR_NBUF].w, acc, 0, 0, 0);            \
        __builtin_amdgcn_sched_barrier(0);
#define PIPS_CR_STEP8(g_)                                                                                               \
        PIPS_CR_STEP(g_) PIPS_CR_STEP((g_) + 1) PIPS_CR_STEP((g_) + 2) PIPS_CR_STEP((g_) + 3) PIPS_CR_STEP((g_) + 4)      \
        PIPS_CR_STEP((g_) + 5) PIPS_CR_STEP((g_) + 6) PIPS_CR_STEP((g_) + 7)
        PIPS_CR_LOAD(0) PIPS_CR_LOAD(1)
        __builtin_amdgcn_sched_barrier(0);
        PIPS_CR_STEP8(0) PIPS_CR_STEP8(8) PIPS_CR_STEP8(16) PIPS_CR_STEP8(24) PIPS_CR_STEP8(32) PIPS_CR_STEP8(40) PIPS_CR_STEP8(48)
        PIPS_CR_STEP8(56) PIPS_CR_STEP8(64)
#undef PIPS_CR_STEP8
#undef PIPS_CR_STEP
#undef PIPS_CR_LOAD

        // ---- epilogue: C orientation -- lane = output channel col, register r = pixel (r & 3) + 8 (r >> 2) + 4 half of the wave's row
        const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
        const int y = ty * CR_ROWS + wave, x0 = tx * CR_COLS;
        const int nvalid = y < H ? min(CR_COLS, W - x0) : 0;                     // rows and columns beyond the image: not stored, not counted
        const unsigned obase = (unsigned)(((y * W + x0) * 64 + col) * 4);
        // the pivot: the wave's second pixel, its first where the row segment has one pixel (lanes of half 0, r = 1 / 0) -- the first pixel of
        // the first column tile is image column 0, whose value sits apart from the row's where the input's mean is not zero
        const float piv1 = __shfl(acc[1] + bvs, l31), piv0 = __shfl(acc[0] + bvs, l31);
        const float pivot = nvalid > 1 ? piv1 : piv0;
        float cs = 0.f, cq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int px = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float v = acc[r] + bvs;
            const bool ok = px < nvalid;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc_out, (int)(ok ? obase + (unsigned)px * 256u : CR_OOB), 0, 0);
            const float d = ok ? v - pivot : 0.f;
            cs += d;
            cq += d * d;
        }
        // one float4 per (wave, channel): the lane halves' sums meet, the lower half stores {s1, s2, p, n}
        const float s1 = cs + __shfl_xor(cs, 32), s2 = cq + __shfl_xor(cq, 32);
        const u32x4 sv = {__float_as_uint(s1), __float_as_uint(s2), __float_as_uint(pivot), __float_as_uint((float)nvalid)};
        __builtin_amdgcn_raw_buffer_store_b128(sv, rsrc_st, (int)(half == 0 ? (unsigned)(((t * 4 + wave) * 64 + col) * 16) : CR_OOB), 0, 0);
    }
}

// Can the kernel run this layer at all: 3x3, stride 1, pad 1, 64 -> 64, bias and statistics, every buffer offset below 2^31 (the
// out-of-range offset), and room for its 4 ceil(H / 4) ceil(W / 32) partials per frame?
bool conv_f32_r_admits(const GemmArgs& a) {
    if (a.KH != 3 || a.KW != 3 || a.cstride != 1 || a.pad != 1 || a.Cin != 64 || a.N != 64 || a.ldc != 64 || a.Ho != a.H ||
        a.Wo != a.Win || a.bias == nullptr || a.stats == nullptr)
        return false;
    if ((unsigned long long)(a.H + 2) * (a.Win + 2) * 256ull >= (1ull << 31)) return false;
    const long parts = 4l * cdiv(a.H, CR_ROWS) * cdiv(a.Win, CR_COLS);
    const long cap = a.stats_parts_cap > 0 ? a.stats_parts_cap : 2 * cdiv(a.M, 64) + 4;
    return parts <= cap && parts * 64 * 16 < (1l << 31);
}

// Does the encoder send the layer here (enc_front_f32): at least `min` tiles (4 x 32 pixels x 32 channels) per compute unit (hook
// PIPS_CONV_F32_R_MINPCT, in percent; PIPS_CONV_F32_R=0: never).  Per-layer A/B of inorm_apply<0> + the shape-selected convolution
// against this kernel normalising on stage, three runs each (profiles/conv_r_layers_ab.txt): this kernel wins at every size measured,
// by more than the spread -- 8-10 us at 3 tiles per compute unit (8 frames of 128 x 160), 26-37 us at the headline's 23, 176-260 us
// at config 4's 112.  Below 3 nothing was measured: those maps stay on the staged sequence.
bool conv_f32_r_takes(const GemmArgs& a, int frames) {
    if (!PIPS_TUNE("PIPS_CONV_F32_R", 1) || !conv_f32_r_admits(a)) return false;
    const int cus = device_cus();
    const long tiles = 2l * cdiv(a.H, CR_ROWS) * cdiv(a.Win, CR_COLS) * frames;
    return cus > 0 && tiles * 100 >= (long)cus * PIPS_TUNE("PIPS_CONV_F32_R_MINPCT", 300);
}

int launch_conv_f32_r(const GemmArgs& a, int frames, int* parts_out, hipStream_t st) {
    const int cus = device_cus();
    if (cus <= 0) {
        set_error("conv3x3_c64_f32_r: cannot query the device");
        return PIPS_E_LAUNCH;
    }
    static std::atomic<unsigned long long> raised{0};
    const int rc = ensure_dynamic_lds(raised, (const void*)conv3x3_c64_f32_r_kernel, CR_LDS);
    if (rc != PIPS_OK) return rc;
    ConvRArgs p;
    p.in = a.A; p.wgt = a.W; p.bias = a.bias; p.out = a.C; p.stats = a.stats; p.in_norm = a.in_norm;
    p.H = a.H; p.W = a.Win; p.tiles_x = cdiv(a.Win, CR_COLS); p.tiles = p.tiles_x * cdiv(a.H, CR_ROWS);
    p.bph = max(1, min(p.tiles, cdiv(cus, 2 * frames)));                  // about one block per compute unit
    p.by_xcd = (frames % 8 == 0) && PIPS_TUNE("PIPS_CONV_F32_R_XCD", 1);
    hipLaunchKernelGGL(conv3x3_c64_f32_r_kernel, dim3(frames * 2 * p.bph), dim3(256), CR_LDS, st, p);
    PIPS_CHECK_LAUNCH("conv3x3_c64_f32_r_kernel");
    if (parts_out) *parts_out = p.tiles * 4;
    return PIPS_OK;
}

}  // namespace pips
