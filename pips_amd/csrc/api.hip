// C ABI of libpips_hip.so (include/pips_hip.h): weight arena, stage entry points and the
// whole-forward driver that replaces Pips.forward (nets/pips.py:428-611).  Everything here
// is host-side launch logic; no allocation, no synchronisation, no global mutable state.
#include "common.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace pips {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#ifdef PIPS_TUNING
int tune_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
#endif

int device_cus() {
    static std::atomic<int> cache[64];                 // zero-initialised; one slot per device ordinal
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::atomic<int>& slot = cache[dev & 63];
    int v = slot.load(std::memory_order_relaxed);
    if (v > 0) return v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 0;
    slot.store(v, std::memory_order_relaxed);
    return v;
}

// ------------------------------------------------------------------ arena layout
// conv geometry in execution (= state-dict) order: nets/pips.py:206-223, 135-136, 169-170
static ArenaLayout build_layout(int S) {
    ArenaLayout A;
    memset(&A, 0, sizeof(A));
    A.S = S; A.nout = S * (PIPS_C + 2); A.nout_pad = (A.nout + 3) & ~3;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };   // 256-B aligned
    int ci = 0, idx = 0;
    auto add_conv = [&](int cout, int cin, int k, int s, int p) {
        ConvW& c = A.conv[idx++];
        c.cout = cout; c.cin = cin; c.k = k; c.stride = s; c.pad = p;
        c.w = take((size_t)cout * cin * k * k);
        c.b = take(cout);
    };
    add_conv(64, 3, 7, 2, 3);
    ci = 64;
    const int dims[4] = {64, 96, 128, 128}, strides[4] = {1, 2, 2, 2};
    for (int l = 0; l < 4; ++l)
        for (int b = 0; b < 2; ++b) {
            const int s = b == 0 ? strides[l] : 1;
            add_conv(dims[l], ci, 3, s, 1);
            add_conv(dims[l], dims[l], 3, 1, 1);
            if (s != 1) add_conv(dims[l], ci, 1, s, 0);
            ci = dims[l];
        }
    add_conv(256, 416, 3, 1, 1);
    add_conv(128, 256, 1, 1, 0);
    A.w_in = take((size_t)PIPS_DMIX * PIPS_KIN_PAD);
    A.b_in = take(PIPS_DMIX);
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        MixLayerW& L = A.mix[d];
        L.ln1g = take(PIPS_DMIX); L.ln1b = take(PIPS_DMIX);
        L.w1 = take((size_t)4 * PIPS_DMIX * PIPS_DMIX); L.b1 = take(4 * PIPS_DMIX);
        L.w2 = take((size_t)4 * PIPS_DMIX * PIPS_DMIX); L.b2 = take(PIPS_DMIX);
        L.ln2g = take(PIPS_DMIX); L.ln2b = take(PIPS_DMIX);
    }
    A.lnf_g = take(PIPS_DMIX); A.lnf_b = take(PIPS_DMIX);
    A.norm_g = take(PIPS_C); A.norm_b = take(PIPS_C);
    A.w_upd_t = take(PIPS_C * PIPS_C); A.b_upd = take(PIPS_C);
    A.w_vis = take(PIPS_C); A.b_vis = take(1);
    A.total = off;
    size_t hoff = 0;
    auto take_h = [&](size_t n) { size_t o = hoff; hoff += (n + 127) / 128 * 128; return o; };   // 256-B aligned
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        A.h_w1[d] = take_h((size_t)4 * PIPS_DMIX * PIPS_DMIX);
        A.h_w2[d] = take_h((size_t)4 * PIPS_DMIX * PIPS_DMIX);
    }
    A.h_conv[0] = 0;                                   // the 7x7 stem stays fp32 (VALU kernel)
    for (int i = 1; i < 22; ++i) A.h_conv[i] = take_h((size_t)A.conv[i].cout * A.conv[i].cin * A.conv[i].k * A.conv[i].k);
    A.h_in = take_h((size_t)PIPS_DMIX * PIPS_KIN_PAD);
    A.total_h = hoff;
    size_t toff = 0;
    auto take_t = [&](size_t n) { size_t o = toff; toff += (3 * n + 127) / 128 * 128; return o; };
    A.t_in = take_t((size_t)PIPS_DMIX * PIPS_KIN_PAD);
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        A.t_w1[d] = take_t((size_t)4 * PIPS_DMIX * PIPS_DMIX);
        A.t_w2[d] = take_t((size_t)4 * PIPS_DMIX * PIPS_DMIX);
    }
    A.t_conv[0] = 0;
    for (int i = 1; i < 22; ++i) A.t_conv[i] = take_t((size_t)A.conv[i].cout * A.conv[i].cin * A.conv[i].k * A.conv[i].k);
    A.total_t = toff;
    // ---- the S-dependent block, behind the three sections (offsets in floats from the arena base)
    off = A.total + (A.total_h + A.total_t + 1) / 2;
    off = (off + 63) / 64 * 64;
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        MixLayerW& L = A.mix[d];
        L.tw0 = take((size_t)4 * S * S); L.tb0 = take(4 * S); L.tw3 = take((size_t)S * 4 * S); L.tb3 = take(S);
    }
    A.w_head = take((size_t)A.nout_pad * PIPS_DMIX); A.b_head = take(A.nout_pad);
    // bf16 copy / split planes of the head: addressed like the members of their sections, i.e. in ushorts from
    // (arena + total) and from (arena + total) + total_h
    const size_t hh = take(((size_t)A.nout_pad * PIPS_DMIX + 1) / 2);
    const size_t th = take((3 * (size_t)A.nout_pad * PIPS_DMIX + 1) / 2);
    A.h_head = 2 * (hh - A.total);
    A.t_head = 2 * (th - A.total) - A.total_h;
    A.total_all = off;
    return A;
}

const ArenaLayout& arena_layout(int S) {
    static ArenaLayout table[PIPS_S_MAX + 1];
    static std::once_flag once[PIPS_S_MAX + 1];
    if (S < 1 || S > PIPS_S_MAX) S = PIPS_S;          // (callers validate S; the S-independent members are the same anyway)
    std::call_once(once[S], [S]() { table[S] = build_layout(S); });
    return table[S];
}

// ------------------------------------------------------------------ repack kernels
// OIHW -> O(HW)I   (implicit-GEMM K order = kh, kw, ci)
__global__ void repack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int I, int T) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)O * I * T) return;
    const int ci = (int)(i % I);
    const int t = (int)((i / I) % T);
    const int o = (int)(i / ((size_t)I * T));
    dst[i] = src[((size_t)o * I + ci) * T + t];
}
// [R][Cc] -> [Cc][R]
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int Cc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * Cc) return;
    const int r = (int)(i % R), c = (int)(i / R);
    dst[i] = src[(size_t)r * Cc + c];
}
// [R][Kin] -> [R][Kpad] zero padded
__global__ void pad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int Kin, int Kpad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * Kpad) return;
    const int k = (int)(i % Kpad), r = (int)(i / Kpad);
    dst[i] = k < Kin ? src[(size_t)r * Kin + k] : 0.f;
}

// fp32 -> bf16 (round to nearest even, hardware v_cvt_pk_bf16_f32)
__global__ void cvt_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (__bf16)src[i];
}

static inline unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }

// pips_repack_weights*: the sections of the arena for window length S, from the reference state dict
static int repack_weights(const void* const* params, int nparams, void* arena_v, int S, int sections, void* stream) {
    PIPS_CHECK_ARG(arena_v != nullptr, "repack: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "repack: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(sections != 0 && (sections & ~(PIPS_PACK_FP32 | PIPS_PACK_BF16 | PIPS_PACK_SPLIT)) == 0, "repack: bad section mask %d", sections);
    hipStream_t st = (hipStream_t)stream;
    const ArenaLayout& A = arena_layout(S);
    float* arena = (float*)arena_v;
    int pi = 0;
  if (sections & PIPS_PACK_FP32) {
    PIPS_CHECK_ARG(params != nullptr, "repack: null pointer");
    PIPS_CHECK_ARG(nparams == PIPS_NPARAMS, "repack: expected %d tensors, got %d", PIPS_NPARAMS, nparams);
    for (int i = 0; i < nparams; ++i) PIPS_CHECK_ARG(params[i] != nullptr, "repack: tensor %d is null", i);
    auto src = [&]() { return (const float*)params[pi++]; };
    auto copy = [&](size_t dst_off, size_t n) {
        (void)hipMemcpyAsync(arena + dst_off, src(), n * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    // stem: [64][3*49] -> [147][64]
    {
        const ConvW& c = A.conv[0];
        hipLaunchKernelGGL(transpose_kernel, dim3(nblk(64 * 147)), dim3(256), 0, st, src(), arena + c.w, 64, 147);
        copy(c.b, 64);
    }
    for (int i = 1; i < 22; ++i) {
        const ConvW& c = A.conv[i];
        const size_t n = (size_t)c.cout * c.cin * c.k * c.k;
        hipLaunchKernelGGL(repack_conv_kernel, dim3(nblk(n)), dim3(256), 0, st, src(), arena + c.w, c.cout,
                           c.cin, c.k * c.k);
        copy(c.b, c.cout);
    }
    hipLaunchKernelGGL(pad_rows_kernel, dim3(nblk((size_t)PIPS_DMIX * PIPS_KIN_PAD)), dim3(256), 0, st, src(),
                       arena + A.w_in, PIPS_DMIX, PIPS_KIN, PIPS_KIN_PAD);
    copy(A.b_in, PIPS_DMIX);
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        const MixLayerW& L = A.mix[d];
        copy(L.tw0, (size_t)4 * S * S); copy(L.tb0, 4 * S); copy(L.tw3, (size_t)S * 4 * S); copy(L.tb3, S);     // nets/pips.py:102-109 over S tokens
        copy(L.ln1g, PIPS_DMIX); copy(L.ln1b, PIPS_DMIX);
        copy(L.w1, (size_t)4 * PIPS_DMIX * PIPS_DMIX); copy(L.b1, 4 * PIPS_DMIX);
        copy(L.w2, (size_t)4 * PIPS_DMIX * PIPS_DMIX); copy(L.b2, PIPS_DMIX);
        copy(L.ln2g, PIPS_DMIX); copy(L.ln2b, PIPS_DMIX);
    }
    copy(A.lnf_g, PIPS_DMIX); copy(A.lnf_b, PIPS_DMIX);
    if (A.nout_pad != A.nout) {                          // odd S: zero rows up to a multiple of 4
        (void)hipMemsetAsync(arena + A.w_head, 0, (size_t)A.nout_pad * PIPS_DMIX * sizeof(float), st);
        (void)hipMemsetAsync(arena + A.b_head, 0, (size_t)A.nout_pad * sizeof(float), st);
    }
    copy(A.w_head, (size_t)A.nout * PIPS_DMIX); copy(A.b_head, A.nout);
    copy(A.norm_g, PIPS_C); copy(A.norm_b, PIPS_C);
    hipLaunchKernelGGL(transpose_kernel, dim3(nblk(PIPS_C * PIPS_C)), dim3(256), 0, st, src(), arena + A.w_upd_t,
                       PIPS_C, PIPS_C);
    copy(A.b_upd, PIPS_C);
    copy(A.w_vis, PIPS_C); copy(A.b_vis, 1);
    if (pi != PIPS_NPARAMS) return PIPS_E_ARG;
  }
  if (sections & PIPS_PACK_BF16) {
    // bf16 copies of the channel-mix / head / conv weights (bf16-operand modes), from the fp32 section
    __bf16* hb = reinterpret_cast<__bf16*>(arena + A.total);
    auto to_h = [&](size_t src_off, size_t dst_off, size_t n) {
        hipLaunchKernelGGL(cvt_bf16_kernel, dim3(nblk(n)), dim3(256), 0, st, arena + src_off, hb + dst_off, n);
    };
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        to_h(A.mix[d].w1, A.h_w1[d], (size_t)4 * PIPS_DMIX * PIPS_DMIX);
        to_h(A.mix[d].w2, A.h_w2[d], (size_t)4 * PIPS_DMIX * PIPS_DMIX);
    }
    to_h(A.w_head, A.h_head, (size_t)A.nout_pad * PIPS_DMIX);
    to_h(A.w_in, A.h_in, (size_t)PIPS_DMIX * PIPS_KIN_PAD);

    for (int i = 1; i < 22; ++i)
        to_h(A.conv[i].w, A.h_conv[i], (size_t)A.conv[i].cout * A.conv[i].cin * A.conv[i].k * A.conv[i].k);
  }
  if (sections & PIPS_PACK_SPLIT) {
    // split-bf16 planes of the same weights (fp32-grade matrix path on the bf16 cores), from the fp32 section
    unsigned short* tb = reinterpret_cast<unsigned short*>(arena + A.total) + A.total_h;
    auto to_t = [&](size_t src_off, size_t dst_off, size_t n) {
        (void)launch_split_bf16x3(arena + src_off, n, tb + dst_off, st);
    };
    to_t(A.w_in, A.t_in, (size_t)PIPS_DMIX * PIPS_KIN_PAD);
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        to_t(A.mix[d].w1, A.t_w1[d], (size_t)4 * PIPS_DMIX * PIPS_DMIX);
        to_t(A.mix[d].w2, A.t_w2[d], (size_t)4 * PIPS_DMIX * PIPS_DMIX);
    }
    to_t(A.w_head, A.t_head, (size_t)A.nout_pad * PIPS_DMIX);
    for (int i = 1; i < 22; ++i)
        to_t(A.conv[i].w, A.t_conv[i], (size_t)A.conv[i].cout * A.conv[i].cin * A.conv[i].k * A.conv[i].k);
  }
    PIPS_CHECK_LAUNCH("pips_repack_weights");
    return PIPS_OK;
}

}  // namespace pips

using namespace pips;

// ------------------------------------------------------------------ host-side plumbing
// Everything down to the extern "C" block at the end of the file is internal: ONE implementation per stage, taking a
// zero-initialised call descriptor the exported wrappers fill field by field.
namespace {

#define RUN(x) do { int rc__ = (x); if (rc__ != PIPS_OK) return rc__; } while (0)

struct Bump {
    size_t off = 0;
    size_t take(size_t floats) { size_t o = off; off += (floats + 63) / 64 * 64; return o; }
};

// How the matrix products of a stage run: exact-fp32 MFMA, bf16 operands (RNE), or split-bf16 (fp32-grade, three bf16 planes)
enum MatMode { EXACT, BF16, SPLIT };
// the encoder's convolutions; BF16 also means bf16 activation maps (the rounding points of the reference under
// torch.autocast(bfloat16)); SPLIT wins over BF16
MatMode encoder_mode(int flags) {
    if (flags & PIPS_FLAG_SPLIT_BF16) return SPLIT;
    return (flags & PIPS_FLAG_BF16_ENCODER) ? BF16 : EXACT;
}
// the mixer's Linears.  bf16_stream (BF16 only, honoured at S = 8 only): the residual stream x is stored as bf16 -- written by
// the input projection, read and rewritten by token mixing and the down-projection (whose fp32 sums take the bf16 residual and are
// rounded once), read by the final LayerNorm; what PreNormResidual holds under autocast (nets/pips.py:93-100)
struct MixerMode { MatMode mode; bool bf16_stream; };
MixerMode mixer_mode(int flags) {
    MixerMode m = {EXACT, false};
    if (flags & PIPS_FLAG_SPLIT_BF16) m.mode = SPLIT;
    else if (flags & PIPS_FLAG_BF16_MIXER) { m.mode = BF16; m.bf16_stream = (flags & PIPS_FLAG_BF16_STREAM) != 0; }
    return m;
}

// HIP events of a timed entry point: created together, destroyed with the scope whatever happens in between
struct Events {
    static constexpr int CAP = 2 * (2 * PIPS_DEPTH + 2);
    hipEvent_t ev[CAP];
    int want, made = 0;
    explicit Events(int n) : want(n) { while (made < want && hipEventCreate(&ev[made]) == hipSuccess) ++made; }
    ~Events() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]); }
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    bool ok() const { if (made != want) set_error("hipEventCreate failed"); return made == want; }
    void record(int i, hipStream_t st) { (void)hipEventRecord(ev[i], st); }
    bool wait(int i) { return hipEventSynchronize(ev[i]) == hipSuccess; }
    float elapsed(int i, int j) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[i], ev[j]); return ms; }
};

// ------------------------------------------------------------------ building blocks
bool epi_ok(int epi, const float* R) { return (epi & 0xff) <= 2 && ((epi & 0xff) != EPI_RESIDUAL || R != nullptr); }

// C[M][ldc] = epi(A[M][lda] W[N][K]^T + bias (+ R[M][ldr])): the argument order of the pips_gemm_* entry points
GemmArgs gemm_args(const void* A, int lda, const void* W, const float* bias, void* C, int ldc, int M, int N, int K, int epi,
                   const float* R, int ldr) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = (const float*)A; g.W = (const float*)W; g.bias = bias; g.C = (float*)C; g.R = R;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.ldr = ldr; g.epi = epi;
    return g;
}
// the dense problem the *_route queries describe: bias and residual present (only their null-ness is inspected)
GemmArgs route_args(int M, int N, int K, int epi) {
    static const float dummy = 0.f;
    return gemm_args(nullptr, K, nullptr, &dummy, nullptr, N, M, N, K, epi, &dummy, N);
}

// One NHWC convolution.  wgt points at the weight form of `mode` (fp32, bf16 copy, split planes), handed over as float*.
// in_bf16 / out_bf16 / in_norm / parts_cap (BF16 only): the maps themselves are bf16; see GemmArgs for the last two.
struct ConvCall {
    const float* in; int F, H, W, Cin;
    const float* wgt; const float* bias; int Cout, k, stride, pad;
    float* out; float* stats; int* tiles;
    MatMode mode; bool in_bf16, out_bf16; const float* in_norm; int parts_cap;
    int route;               // EXACT only: GemmArgs::conv_route
};
// the geometry part, in the argument order of the pips_conv_nhwc_* entry points; mode and map types are left EXACT / fp32
ConvCall conv_call(const void* in, int F, int H, int W, int Cin, const void* wgt, const float* bias, int Cout, int k, int stride,
                   int pad, void* out, float* stats, int* tiles) {
    ConvCall c;
    memset(&c, 0, sizeof(c));
    c.in = (const float*)in; c.F = F; c.H = H; c.W = W; c.Cin = Cin;
    c.wgt = (const float*)wgt; c.bias = bias; c.Cout = Cout; c.k = k; c.stride = stride; c.pad = pad;
    c.out = (float*)out; c.stats = stats; c.tiles = tiles;
    return c;
}
int conv_nhwc(const ConvCall& c, hipStream_t st) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = c.in; g.W = c.wgt; g.bias = c.bias; g.C = c.out; g.stats = c.stats; g.in_norm = c.in_norm; g.stats_parts_cap = c.parts_cap;
    g.conv_route = c.route;
    g.H = c.H; g.Win = c.W; g.Cin = c.Cin; g.KH = g.KW = c.k; g.cstride = c.stride; g.pad = c.pad;
    g.Ho = conv_out(c.H, c.k, c.stride, c.pad); g.Wo = conv_out(c.W, c.k, c.stride, c.pad);
    g.M = g.Ho * g.Wo; g.N = c.Cout; g.K = c.k * c.k * c.Cin; g.ldc = c.Cout; g.epi = EPI_BIAS;
    PIPS_CHECK_ARG(g.Ho > 0 && g.Wo > 0, "conv: empty output");
    if (c.mode == SPLIT) return launch_conv_x3(g, c.F, c.tiles, st);
    PIPS_CHECK_ARG(c.mode == BF16 || (!c.in_bf16 && !c.out_bf16), "conv: bf16 maps need the bf16-operand kernels");
    PIPS_CHECK_ARG(c.mode == BF16 || !c.in_norm || c.route == PIPS_CONV_ROUTE_R, "conv: an fp32 map is normalised while staged by the LDS-resident 64 -> 64 kernel only");
    return c.mode == BF16 ? launch_conv_bf16(g, c.F, c.tiles, st, c.in_bf16, c.out_bf16) : launch_conv(g, c.F, c.tiles, st);
}

// ------------------------------------------------------------------ pyramid layout
// THE level table of a packed pyramid of `frames` frames with H8 x W8 level-0 pixels, in floats: the fp32 levels at off[l]
// (lh[l] x lw[l] pixels, 256-byte aligned), their bf16 mirror (same element offsets, half the bytes) behind all of them at
// `levels` -- written by the bf16 encoder, pips_pyramid_mirror or pips_pyramid_append, read by the gather under
// PIPS_FLAG_BF16_MAPS -- and a slack of a few map rows of the coarsest level (+ a pixel block) behind the mirror:
// gather_mfma_kernel fetches whole 8 x 4 pixel blocks; the slots of a border block that hang over the last level's last frame must
// still lie inside the buffer (their values are never used)
struct PyramidView {
    size_t off[PIPS_LEVELS];
    int lh[PIPS_LEVELS], lw[PIPS_LEVELS];
    size_t levels, mirror, slack;        // floats: the fp32 levels (= where the mirror starts), the mirror, the slack
    size_t total() const { return levels + mirror + slack; }
    bool empty() const { return lh[PIPS_LEVELS - 1] < 1 || lw[PIPS_LEVELS - 1] < 1; }     // too small for four levels
};
PyramidView pyramid_view(int frames, int H8, int W8) {
    PyramidView v;
    v.levels = 0;
    for (int l = 0; l < PIPS_LEVELS; ++l) {
        v.lh[l] = l ? v.lh[l - 1] / 2 : H8; v.lw[l] = l ? v.lw[l - 1] / 2 : W8;
        v.off[l] = v.levels;
        v.levels += ((size_t)frames * v.lh[l] * v.lw[l] * PIPS_C + 63) / 64 * 64;
    }
    v.mirror = (v.levels / 2 + 63) / 64 * 64;
    v.slack = (((size_t)4 * v.lw[PIPS_LEVELS - 1] + 16) * PIPS_C / 2 + 63) / 64 * 64;      // (4 rows + 16 pixels) of bf16 channels
    return v;
}

// THE size rule of every entry point that samples correlation windows (the gathers, the tracker, the hop, the stream round).  The
// sampler normalises a level's coordinates with 2 x / (W - 1) - 1 (nets/pips.py:318-319; level_sample_geometry, corr_window): a
// level one pixel wide or high divides by zero and all 49 of its taps are NaN, which the model turns into NaN positions.  So every
// one of the PIPS_LEVELS levels must be at least 2 x 2 pixels: H8, W8 >= 16.  Encoding, the pyramid copies and the score maps divide
// by no size - 1 and keep the weaker limit of PyramidView::empty().
int check_sampled_map(int H8, int W8, const char* who) {
    const int least = 2 << (PIPS_LEVELS - 1);
    PIPS_CHECK_ARG(H8 >= least && W8 >= least,
                   "%s: map %dx%d too small, need at least %dx%d: its coarsest pyramid level would be %dx%d, and a level one pixel "
                   "wide or high cannot be sampled (the reference normalises with 2x/(W-1)-1, a division by zero: NaN)",
                   who, H8, W8, least, least, H8 > 0 ? H8 >> (PIPS_LEVELS - 1) : 0, W8 > 0 ? W8 >> (PIPS_LEVELS - 1) : 0);
    return PIPS_OK;
}

// ------------------------------------------------------------------ encoder
struct EncPlan {
    int F, H, W, stride;
    int Hs[5], Ws[5];         // stem/layer1, layer2, layer3, layer4 resolutions; [4] = target H8,W8
    size_t raw, mid, xa, xb, ds, outs[4], cat, partial, partial2, st_a, st_b;
    size_t total;             // floats
};

// room for InstanceNorm partials per frame of a layer with H x W output pixels: the documented bound of the conv entry
// points, or one partial per wave of the 4 x 32-pixel tiles of the ping-pong 64 -> 64 kernel (conv_bf16_c64.hip)
int enc_parts_cap(int H, int W) {
    const int a = 2 * cdiv(H * W, 64) + 4, b = cdiv(W, 32) * cdiv(H, 4) * 4;
    return a > b ? a : b;
}

EncPlan plan_encoder(int F, int H, int W, int stride) {
    EncPlan P;
    P.F = F; P.H = H; P.W = W; P.stride = stride;
    P.Hs[0] = conv_out(H, 7, 2, 3); P.Ws[0] = conv_out(W, 7, 2, 3);
    for (int l = 1; l < 4; ++l) { P.Hs[l] = conv_out(P.Hs[l - 1], 3, 2, 1); P.Ws[l] = conv_out(P.Ws[l - 1], 3, 2, 1); }
    P.Hs[4] = H / stride; P.Ws[4] = W / stride;
    const int ch[4] = {64, 96, 128, 128};
    size_t big = 0;
    for (int l = 0; l < 4; ++l) big = big > (size_t)F * P.Hs[l] * P.Ws[l] * ch[l] ? big : (size_t)F * P.Hs[l] * P.Ws[l] * ch[l];
    const size_t tgt = (size_t)F * P.Hs[4] * P.Ws[4];
    if (big < tgt * 256) big = tgt * 256;
    Bump b;
    P.raw = b.take(big); P.mid = b.take(big); P.xa = b.take(big); P.xb = b.take(big); P.ds = b.take(big);
    for (int l = 0; l < 4; ++l) P.outs[l] = b.take((size_t)F * P.Hs[l] * P.Ws[l] * ch[l]);
    P.cat = b.take(tgt * 416);
    // partial statistics: float4 [F][parts][C]; parts <= 2 wave rows x (rows/64 + 1) m tiles
    size_t pmax = 0;
    for (int l = 0; l < 4; ++l) {
        size_t t = (size_t)F * enc_parts_cap(P.Hs[l], P.Ws[l]) * ch[l] * 4;
        pmax = pmax > t ? pmax : t;
    }
    {
        const size_t ts = (size_t)F * stem_tiles_m(P.Hs[0], P.Ws[0]) * 64 * 4;        // the stem's partials are float4
        pmax = pmax > ts ? pmax : ts;
    }
    size_t t2 = (size_t)F * (2 * cdiv(P.Hs[4] * P.Ws[4], 64) + 4) * 256 * 4;
    pmax = pmax > t2 ? pmax : t2;
    P.partial = b.take(pmax); P.partial2 = b.take(pmax);
    P.st_a = b.take((size_t)F * 256 * 2); P.st_b = b.take((size_t)F * 256 * 2);
    P.total = b.off;
    return P;
}

int check_geometry(int F, int H, int W, int stride) {
    PIPS_CHECK_ARG(F > 0 && H > 0 && W > 0 && stride >= 1, "bad geometry F=%d H=%d W=%d stride=%d", F, H, W, stride);
    PIPS_CHECK_ARG(!pyramid_view(F, H / stride, W / stride).empty(), "input %dx%d too small for a 4-level pyramid at stride %d", H, W,
                   stride);
    return PIPS_OK;
}

// Matrix mode of one convolution.  The split path is used where it measured faster than the exact kernel
// (tools/x3_check.py): every layer with >= 8000 output pixels over the batch (at config 2: all but the 23x31 maps).
MatMode layer_mm(const ConvW& c, int F, int H, int W, MatMode mode) {
    if (mode != SPLIT) return mode;
    const long rows = (long)F * conv_out(H, c.k, c.stride, c.pad) * conv_out(W, c.k, c.stride, c.pad);
    return rows >= 8000 ? SPLIT : EXACT;
}
// weight pointer for that mode, handed over as float* (bf16 copy / split planes live behind the fp32 arena)
const float* conv_w(const float* arena, const ArenaLayout& A, int ci, MatMode mode) {
    if (mode == EXACT) return arena + A.conv[ci].w;
    const unsigned short* hb = reinterpret_cast<const unsigned short*>(arena + A.total);
    return reinterpret_cast<const float*>(mode == BF16 ? hb + A.h_conv[ci] : hb + A.total_h + A.t_conv[ci]);
}

// One encoder pass.  mode == BF16 (PIPS_FLAG_BF16_ENCODER; kernels: encoder_bf16.hip, conv_bf16_c64.hip, gemm_bf16.hip): every
// activation map is bf16 -- the buffers are the fp32 plan's, used as bf16, hence the void* maps below; statistics, normalisation,
// adds and resizes are fp32 arithmetic and the pyramid is fp32 in every mode.
struct Enc {
    const float* arena; const ArenaLayout& A;
    int F; float* ws; const EncPlan& P; hipStream_t st; MatMode mode;
};

// layer ci of the arena on a map of H x W pixels, in the mode layer_mm() picks for it; bf16 maps in (and out, if out_bf16)
ConvCall enc_conv(const Enc& e, int ci, const void* in, int H, int W, void* out, bool out_bf16) {
    const ConvW& c = e.A.conv[ci];
    const MatMode lm = layer_mm(c, e.F, H, W, e.mode);
    ConvCall cc = conv_call(in, e.F, H, W, c.cin, conv_w(e.arena, e.A, ci, lm), e.arena + c.b, c.cout, c.k, c.stride, c.pad, out,
                            nullptr, nullptr);
    cc.mode = lm;
    cc.in_bf16 = e.mode == BF16;
    cc.out_bf16 = out_bf16;
    return cc;
}

// conv (optional normalise-on-load of the input map by in_norm: BF16, or EXACT on `route` PIPS_CONV_ROUTE_R) -> raw map + partial
// stats -> {mean, rstd}
int conv_stats(const Enc& e, int ci, const void* in, const float* in_norm, int H, int W, void* out, float* partial,
               float* mean_rstd, int route = PIPS_CONV_ROUTE_AUTO) {
    const ConvW& c = e.A.conv[ci];
    int tiles = 0;
    ConvCall cc = enc_conv(e, ci, in, H, W, out, e.mode == BF16);
    cc.stats = partial; cc.tiles = &tiles; cc.in_norm = in_norm; cc.route = route;
    if (e.mode == BF16 || route == PIPS_CONV_ROUTE_R)
        cc.parts_cap = enc_parts_cap(conv_out(H, c.k, c.stride, c.pad), conv_out(W, c.k, c.stride, c.pad));
    RUN(conv_nhwc(cc, e.st));
    return launch_inorm_finalize_pivot(partial, e.F, tiles, c.cout, mean_rstd, e.st);
}

// y = relu(n(x))  |  relu(res + relu(n(x)))  |  relu(n2(res) + relu(n(x))), by the null-ness of res / res_stats
int inorm_apply(const Enc& e, const void* x, const float* stats, const void* res, const float* res_stats, void* y, int HW, int C) {
    if (e.mode == BF16)
        return launch_inorm_apply_bf16(x, stats, res, res_stats, res == nullptr ? 0 : res_stats == nullptr ? 1 : 2, y, e.F, HW, C, e.st);
    return launch_inorm_apply((const float*)x, stats, (const float*)res, res_stats, (float*)y, e.F, HW, C, e.st);
}

// ResidualBlock.forward, nets/pips.py:173-181
int res_block(const Enc& e, int& ci, bool down, const void* x, int H, int W, void* out) {
    const int i1 = ci++, i2 = ci++;
    const ConvW& c1 = e.A.conv[i1];
    const ConvW& c2 = e.A.conv[i2];
    const int Ho = conv_out(H, 3, c1.stride, 1), Wo = conv_out(W, 3, c1.stride, 1);
    float* ws = e.ws; const EncPlan& P = e.P;
    void* raw = ws + P.raw; void* mid = ws + P.mid;
    RUN(conv_stats(e, i1, x, nullptr, H, W, raw, ws + P.partial, ws + P.st_a));
    RUN(inorm_apply(e, raw, ws + P.st_a, nullptr, nullptr, mid, Ho * Wo, c1.cout));
    RUN(conv_stats(e, i2, mid, nullptr, Ho, Wo, raw, ws + P.partial, ws + P.st_a));
    if (down) {
        const int id = ci++;
        RUN(conv_stats(e, id, x, nullptr, H, W, ws + P.ds, ws + P.partial2, ws + P.st_b));
        return inorm_apply(e, raw, ws + P.st_a, ws + P.ds, ws + P.st_b, out, Ho * Wo, c2.cout);
    }
    return inorm_apply(e, raw, ws + P.st_a, x, nullptr, out, Ho * Wo, c2.cout);
}

// Does the exact-fp32 encoder run layer 1 of F maps of H0 x W0 pixels on the LDS-resident kernel (conv_f32_r.hip)?  The geometry
// of the layer's four convolutions, with the room plan_encoder() gives their partials.
bool enc_l1_fused(int F, int H0, int W0) {
    static const float dummy = 0.f;
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.bias = &dummy; g.stats = const_cast<float*>(&dummy);      // only their null-ness is inspected
    g.H = g.Ho = H0; g.Win = g.Wo = W0; g.Cin = g.N = g.ldc = 64; g.KH = g.KW = 3; g.cstride = 1; g.pad = 1;
    g.M = H0 * W0; g.K = 9 * 64; g.stats_parts_cap = enc_parts_cap(H0, W0);
    return conv_f32_r_takes(g, F);
}

// stem + layer1 with fp32 maps (nets/pips.py:251-253, 265) -> ws + P.outs[0]
int enc_front_f32(const Enc& e, const void* rgbs, int rgb_u8, int H, int W, int& ci) {
    float* ws = e.ws; const EncPlan& P = e.P;
    const int H0 = P.Hs[0], W0 = P.Ws[0];
    int tiles = 0;
    RUN(launch_stem(rgbs, rgb_u8, e.arena + e.A.conv[0].w, e.arena + e.A.conv[0].b, ws + P.raw, ws + P.partial, e.F, H, W, H0, W0,
                    &tiles, e.st));
    RUN(launch_inorm_finalize_pivot(ws + P.partial, e.F, tiles, 64, ws + P.st_a, e.st));
    if (e.mode == EXACT && enc_l1_fused(e.F, H0, W0)) {
        // layer 1 on the LDS-resident 64 -> 64 kernel, the sequence of enc_front_bf16: a convolution normalises its input while
        // staging it, so relu(norm(.)) of the stem and of each block's first convolution never goes to memory
        const int R = PIPS_CONV_ROUTE_R;
        float* raw = ws + P.raw; float* mid = ws + P.mid; float* xa = ws + P.xa; float* xb = ws + P.xb;
        float* st_a = ws + P.st_a; float* st_b = ws + P.st_b;
        RUN(conv_stats(e, ci++, raw, st_a, H0, W0, mid, ws + P.partial, st_b, R));       // block 1 conv1 on the raw stem map
        RUN(conv_stats(e, ci++, mid, st_b, H0, W0, xa, ws + P.partial, st_b, R));        // block 1 conv2
        // relu(x + y), x = relu(norm1(stem)) recomputed from the raw stem map, y = relu(norm2(conv2)) (:176-181)
        RUN(launch_inorm_apply(xa, st_b, raw, st_a, xb, e.F, H0 * W0, 64, e.st, true));
        RUN(conv_stats(e, ci++, xb, nullptr, H0, W0, raw, ws + P.partial, st_a, R));     // block 2 conv1
        RUN(conv_stats(e, ci++, raw, st_a, H0, W0, mid, ws + P.partial, st_b, R));       // block 2 conv2
        return launch_inorm_apply(mid, st_b, xb, nullptr, ws + P.outs[0], e.F, H0 * W0, 64, e.st);
    }
    RUN(launch_inorm_apply(ws + P.raw, ws + P.st_a, nullptr, nullptr, ws + P.xa, e.F, H0 * W0, 64, e.st));
    RUN(res_block(e, ci, false, ws + P.xa, H0, W0, ws + P.xb));
    return res_block(e, ci, false, ws + P.xb, H0, W0, ws + P.outs[0]);
}

// the same with bf16 maps -> ws + P.outs[0]
int enc_front_bf16(const Enc& e, const void* rgbs, int rgb_u8, int H, int W, int& ci) {
    float* ws = e.ws; const EncPlan& P = e.P; const ArenaLayout& A = e.A; hipStream_t st = e.st;
    const int F = e.F, H0 = P.Hs[0], W0 = P.Ws[0];
    int tiles = 0;
    void* xa = ws + P.xa; void* xb = ws + P.xb; void* raw = ws + P.raw; void* mid = ws + P.mid;
    float* st_a = ws + P.st_a; float* st_b = ws + P.st_b;
    // stem: conv1 (:251); its norm1 + relu (:252-253) is applied by the consumers
    RUN(launch_stem_bf16(rgbs, rgb_u8, e.arena + A.conv[0].w, e.arena + A.conv[0].b, xa, ws + P.partial, F, H, W, H0, W0, &tiles, st));
    RUN(launch_inorm_finalize_pivot(ws + P.partial, F, tiles, 64, st_a, st));
    if (conv3x3_c64_takes(H0, W0, F)) {
        // layer1 on the LDS-resident 64 -> 64 kernel: a convolution normalises its input while staging it, so relu(norm(.))
        // of the stem and of each block's first convolution never goes to HBM.  xa = raw stem map (statistics st_a).
        RUN(conv_stats(e, ci++, xa, st_a, H0, W0, raw, ws + P.partial, st_b));          // block 1 conv1
        RUN(conv_stats(e, ci++, raw, st_b, H0, W0, mid, ws + P.partial, st_b));         // block 1 conv2
        // relu(x + y), x = relu(norm1(stem)) recomputed from the raw stem map, y = relu(norm2(conv2)) (:176-181)
        RUN(launch_inorm_apply_bf16(mid, st_b, xa, st_a, 3, xb, F, H0 * W0, 64, st));
        RUN(conv_stats(e, ci++, xb, nullptr, H0, W0, raw, ws + P.partial, st_a));       // block 2 conv1
        RUN(conv_stats(e, ci++, raw, st_a, H0, W0, mid, ws + P.partial, st_b));         // block 2 conv2
        return launch_inorm_apply_bf16(mid, st_b, xb, nullptr, 1, ws + P.outs[0], F, H0 * W0, 64, st);
    }
    RUN(launch_inorm_apply_bf16(xa, st_a, nullptr, nullptr, 0, xb, F, H0 * W0, 64, st));
    RUN(res_block(e, ci, false, xb, H0, W0, xa));
    return res_block(e, ci, false, xa, H0, W0, ws + P.outs[0]);
}

// flags: PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_SPLIT_BF16 (encoder_mode) and PIPS_FLAG_RGB_U8: rgbs is uint8 (B,S,3,H,W) instead of float
int encoder_impl(const void* arena_v, const void* rgbs, int F, int H, int W, int stride, int flags, float* pyramid, void* workspace,
                 size_t workspace_bytes, hipStream_t st) {
    PIPS_CHECK_ARG(arena_v && rgbs && pyramid && workspace, "encoder: null pointer");
    RUN(check_geometry(F, H, W, stride));
    const EncPlan P = plan_encoder(F, H, W, stride);
    if (workspace_bytes < P.total * sizeof(float)) {
        set_error("encoder: workspace %zu < %zu bytes", workspace_bytes, P.total * sizeof(float));
        return PIPS_E_WORKSPACE;
    }
    float* ws = (float*)workspace;
    const Enc e = {(const float*)arena_v, arena_layout(), F, ws, P, st, encoder_mode(flags)};
    const bool h = e.mode == BF16;
    const int rgb_u8 = (flags & PIPS_FLAG_RGB_U8) ? 1 : 0;

    // stem + layer1 (nets/pips.py:251-253, 265)
    int ci = 1;
    RUN(h ? enc_front_bf16(e, rgbs, rgb_u8, H, W, ci) : enc_front_f32(e, rgbs, rgb_u8, H, W, ci));
    // layer2..4 (:266-268)
    const void* x = ws + P.outs[0];
    int Hc = P.Hs[0], Wc = P.Ws[0];
    for (int l = 1; l < 4; ++l) {
        RUN(res_block(e, ci, true, x, Hc, Wc, ws + P.xb));
        Hc = P.Hs[l]; Wc = P.Ws[l];
        RUN(res_block(e, ci, false, ws + P.xb, Hc, Wc, ws + P.outs[l]));
        x = ws + P.outs[l];
    }
    // resize a,b,c,d to (H//stride, W//stride) and concatenate (:269-273)
    const int ch[4] = {64, 96, 128, 128};
    const int H8 = P.Hs[4], W8 = P.Ws[4];
    for (int l = 0, coff = 0; l < 4; coff += ch[l], ++l)
        RUN(h ? launch_resize_into_bf16(ws + P.outs[l], F, P.Hs[l], P.Ws[l], ch[l], ws + P.cat, H8, W8, 416, coff, st)
              : launch_resize_into(ws + P.outs[l], F, P.Hs[l], P.Ws[l], ch[l], ws + P.cat, H8, W8, 416, coff, st));
    // conv2 + norm2 + relu + conv3 (:273-276); conv3 writes the fp32 level-0 map of the correlation pyramid
    const int i2 = ci++, i3 = ci++;
    RUN(conv_stats(e, i2, ws + P.cat, nullptr, H8, W8, ws + P.raw, ws + P.partial, ws + P.st_a));
    RUN(inorm_apply(e, ws + P.raw, ws + P.st_a, nullptr, nullptr, ws + P.mid, H8 * W8, 256));
    RUN(conv_nhwc(enc_conv(e, i3, ws + P.mid, H8, W8, pyramid, false), st));
    // CorrBlock.__init__ pyramid (:346-352)
    const PyramidView v = pyramid_view(F, H8, W8);
    for (int l = 1; l < PIPS_LEVELS; ++l)
        RUN(launch_avgpool2(pyramid + v.off[l - 1], F, v.lh[l - 1], v.lw[l - 1], PIPS_C, pyramid + v.off[l], st));
    // the bf16 mirror the gather of the bf16 mode reads (PIPS_FLAG_BF16_MAPS)
    if (h) RUN(launch_pyramid_mirror(pyramid, v.levels, pyramid + v.levels, st));
    return PIPS_OK;
}

// ------------------------------------------------------------------ windows of several videos
// The checks every clip form shares, ahead of any launch, and the table the kernels take.  win_clip == null: no table, no check.
// ring == 0: the videos lie one after the other on a linear cache (R = T).  ring > 0 (the _rings forms; a table is then required):
// every video is a ring of `ring` slots on a buffer of R = T = F flat slots.
int clip_table(const int* win_clip, const int* clip_first, const int* clip_frames, int V, const int* win_start, int B, int T, int R,
               int ring, const char* who, ClipTable& ct) {
    ct = ClipTable{win_clip, clip_first, clip_frames, V, ring > 0 ? ring : R};
    if (ring == 0 && win_clip == nullptr) return PIPS_OK;
    PIPS_CHECK_ARG(ring >= 0, "%s: a ring needs R >= 1 slots (R=%d)", who, ring);
    PIPS_CHECK_ARG(V >= 1, "%s: a clip table needs V >= 1 videos (V=%d)", who, V);
    PIPS_CHECK_ARG(win_clip && clip_first && clip_frames, "%s: win_clip needs clip_first and clip_frames", who);
    PIPS_CHECK_ARG(win_start != nullptr, "%s: win_clip needs win_start", who);
    PIPS_CHECK_ARG(B == 1, "%s: the videos of a clip table share ONE flat cache, B = 1 (B=%d)", who, B);
    PIPS_CHECK_ARG(R == T, "%s: a clip table needs a linear cache, R = T (R=%d, T=%d)", who, R, T);
    PIPS_CHECK_ARG(ring == 0 || (long long)V * ring <= T, "%s: %d rings of %d slots need a buffer of %lld slots (F=%d)", who, V, ring,
                   (long long)V * ring, T);
    return PIPS_OK;
}
// the slots-per-video argument of a _rings entry point as the `ring` of the descriptors: a value < 1 stays invalid
int ring_arg(int R) { return R >= 1 ? R : -1; }

// ------------------------------------------------------------------ correlation gather
enum GatherRoute { GATHER_AUTO, GATHER_DIRECT, GATHER_TILED };   // AUTO: tiled for a dense query set if the call allows it

// pyramid: B clips x R frame slots holding T logical frames (frame f in slot f mod R; T is the clamp bound; a linear cache
// has R = T); S = window length = mixer rows per particle.  win_dir (per-particle time direction, sign) is read with win_start only.
// bf16_maps: the gather reads the bf16 mirror behind the fp32 levels.  The tiled kernels need scratch, a dense un-windowed
// query set and R = T = S = PIPS_S; ev != null (tiled only): 4 events around their three launches.
// win_clip (per-particle video index) + clip_first / clip_frames (V videos): the windows of several videos on one flat linear
// cache, B = 1 and R = T = all frames (ClipTable, common.h); read with win_start only.  ring > 0: the videos are rings of `ring`
// slots each on that buffer (R = T = its flat slots).
struct GatherCall {
    const float* pyramid; int B, T, R, S, H8, W8;
    const float* ffeats; const float* coords; const float* times; int N;
    const int* win_start; const int* win_dir;
    const int* win_clip; const int* clip_first; const int* clip_frames; int V, ring;
    float* X;
    bool bf16_maps; GatherRoute route;
    void* scratch; size_t scratch_bytes; hipEvent_t* ev;
    hipStream_t st;
};

int mixer_input(const GatherCall& g) {
    PIPS_CHECK_ARG(g.pyramid && g.ffeats && g.coords && g.times && g.X, "mixer_input: null pointer");
    PIPS_CHECK_ARG(g.T >= 1 && g.R >= 1 && g.B > 0 && g.N > 0, "mixer_input: need T, R, B, N >= 1");
    PIPS_CHECK_ARG(g.S >= 1 && g.S <= PIPS_S_MAX, "mixer_input: window length S=%d outside 1..%d", g.S, PIPS_S_MAX);
    RUN(check_sampled_map(g.H8, g.W8, "mixer_input"));
    const PyramidView v = pyramid_view(g.B * g.R, g.H8, g.W8);
    ClipTable ct;
    RUN(clip_table(g.win_clip, g.clip_first, g.clip_frames, g.V, g.win_start, g.B, g.T, g.R, g.ring, "mixer_input", ct));
    const ClipTable* clips = g.win_clip != nullptr ? &ct : nullptr;
    const float* mirror = g.pyramid + v.levels;
    const bool can_tile = g.scratch != nullptr && g.win_start == nullptr && g.win_dir == nullptr && g.R == PIPS_S && g.T == g.R &&
                          g.S == PIPS_S && g.scratch_bytes >= tiled_gather_scratch_bytes(g.B, g.N, g.H8, g.W8);
    const bool tiled = g.route == GATHER_AUTO ? tiled_gather_wanted(g.B, g.N, g.H8, g.W8, g.bf16_maps) : g.route == GATHER_TILED;
    if (tiled && can_tile)      // (bf16 mode: the same work items on the matrix cores, reading the bf16 mirror)
        return launch_mixer_input_tiled(g.pyramid, v.off, v.lh, v.lw, g.B, g.R, g.ffeats, g.coords, g.times, g.N, g.X, g.scratch,
                                        g.scratch_bytes, g.st, g.ev,
                                        g.bf16_maps ? reinterpret_cast<const unsigned short*>(mirror) : nullptr);
    PIPS_CHECK_ARG(g.route != GATHER_TILED, "tiled gather needs scratch of %zu bytes, no win_start and 8 frames per clip",
                   tiled_gather_scratch_bytes(g.B, g.N, g.H8, g.W8));
    PIPS_CHECK_ARG(g.win_dir == nullptr || g.win_start != nullptr, "mixer_input: win_dir needs win_start");
    if (g.bf16_maps)
        return launch_mixer_input_bf16maps(mirror, v.off, v.lh, v.lw, g.B, g.R, g.T, g.ffeats, g.coords, g.times, g.N, g.win_start,
                                           g.win_dir, g.X, g.st, g.S, clips);
    return launch_mixer_input(g.pyramid, v.off, v.lh, v.lw, g.B, g.R, g.T, g.ffeats, g.coords, g.times, g.N, g.win_start, g.win_dir,
                              g.X, g.st, g.S, clips);
}

// the tiled kernels on a PIPS_S-frame clip; ms3_host != null: the durations of the three launches, and a stream synchronisation
int mixer_input_tiled(GatherCall g, float* ms3_host) {
    PIPS_CHECK_ARG(g.scratch != nullptr, "mixer_input_tiled: null pointer");
    PIPS_CHECK_ARG(g.R == PIPS_S, "mixer_input_tiled: S must be %d", PIPS_S);
    g.route = GATHER_TILED;
    if (ms3_host == nullptr) return mixer_input(g);
    Events ev(4);
    if (!ev.ok()) return PIPS_E_LAUNCH;
    g.ev = ev.ev;
    int rc = mixer_input(g);
    if (rc == PIPS_OK && !ev.wait(3)) rc = PIPS_E_LAUNCH;
    if (rc == PIPS_OK)
        for (int i = 0; i < 3; ++i) ms3_host[i] = ev.elapsed(i, i + 1);
    return rc;
}

// ------------------------------------------------------------------ mixer
struct MixerPlan { size_t x, xn, h, pooled, total; };      // floats; M rows of S tokens per particle
MixerPlan plan_mixer(int M, int S) {
    MixerPlan P;
    Bump b;
    P.x = b.take((size_t)M * PIPS_DMIX); P.xn = b.take((size_t)M * PIPS_DMIX); P.h = b.take((size_t)M * 4 * PIPS_DMIX);
    P.pooled = b.take((size_t)(M / S) * PIPS_DMIX);
    P.total = b.off;
    return P;
}
size_t mixer_workspace_bytes(int M, int S) {
    if (M <= 0 || S < 1 || S > PIPS_S_MAX) return 0;
    return plan_mixer(M, S).total * sizeof(float);
}

// One Linear of the mixer on dense rows: out[M][N] = epi(in[M][K] W^T + bias), EPI_RESIDUAL adding out in place.  w / w_bf16 /
// w_split are the arena offsets of the weight's three forms (floats, ushorts of the bf16 section, ushorts of the split section);
// in_bf16 / out_bf16 say which activations the BF16 mode keeps as bf16 (the other modes are fp32 throughout).
struct Linear { size_t w, w_bf16, w_split, bias; int K, N, epi; bool in_bf16, out_bf16; };

Linear in_proj(const ArenaLayout& A, bool x_bf16) {
    return {A.w_in, A.h_in, A.t_in, A.b_in, PIPS_KIN_PAD, PIPS_DMIX, EPI_BIAS, false, x_bf16};
}
Linear up_proj(const ArenaLayout& A, int d) {
    return {A.mix[d].w1, A.h_w1[d], A.t_w1[d], A.mix[d].b1, PIPS_DMIX, 4 * PIPS_DMIX, EPI_GELU, true, true};
}
Linear down_proj(const ArenaLayout& A, int d, bool x_bf16) {
    return {A.mix[d].w2, A.h_w2[d], A.t_w2[d], A.mix[d].b2, 4 * PIPS_DMIX, PIPS_DMIX, EPI_RESIDUAL | (x_bf16 ? EPI_RES_BF16 : 0),
            true, x_bf16};
}
Linear head_proj(const ArenaLayout& A) {
    return {A.w_head, A.h_head, A.t_head, A.b_head, PIPS_DMIX, A.nout_pad, EPI_BIAS, false, false};
}

int linear(MatMode mode, const float* arena, const ArenaLayout& A, const Linear& L, const float* in, float* out, int M, hipStream_t st) {
    const unsigned short* hw = reinterpret_cast<const unsigned short*>(arena + A.total);
    const bool res = (L.epi & 0xff) == EPI_RESIDUAL;
    const void* W = mode == EXACT ? (const void*)(arena + L.w) : mode == BF16 ? (const void*)(hw + L.w_bf16)
                                                                               : (const void*)(hw + A.total_h + L.w_split);
    const GemmArgs g = gemm_args(in, L.K, W, arena + L.bias, out, L.N, M, L.N, L.K, L.epi, res ? out : nullptr, res ? L.N : 0);
    if (mode == SPLIT) return launch_gemm_x3(g, st);
    return mode == BF16 ? launch_gemm_bf16(g, L.in_bf16, L.out_bf16, st) : launch_gemm(g, st);
}

// X (M, 544) -> delta (M / S, nout_pad(S)).  S: the window length the arena was packed for (tokens per particle).
// ev != nullptr: record ev[2g], ev[2g+1] around GEMM g (g = 0 in-proj, 1+2d up, 2+2d down, 25 head)
int mixer_impl(const void* arena_v, const float* X, int M, int S, MixerMode mm, float* delta, void* workspace, size_t workspace_bytes,
               hipStream_t st, hipEvent_t* ev) {
    PIPS_CHECK_ARG(arena_v && X && delta && workspace, "mixer: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "mixer: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(M > 0 && M % S == 0, "mixer: M=%d must be a positive multiple of S=%d", M, S);
    if (workspace_bytes < mixer_workspace_bytes(M, S)) {
        set_error("mixer: workspace %zu < %zu bytes", workspace_bytes, mixer_workspace_bytes(M, S));
        return PIPS_E_WORKSPACE;
    }
    const ArenaLayout& A = arena_layout(S);
    const float* arena = (const float*)arena_v;
    const MixerPlan W = plan_mixer(M, S);
    float* ws = (float*)workspace;
    float* x = ws + W.x; float* xn = ws + W.xn; float* h = ws + W.h; float* pooled = ws + W.pooled;
    const int P = M / S;
    const bool bf16 = mm.mode == BF16;                 // bf16 operands: the LayerNorm-2 output xn and the hidden activation h are bf16
    const bool xb = bf16 && mm.bf16_stream && S == PIPS_S;
    int g = 0;
    auto timed = [&](const Linear& L, const float* in, float* out, int rows) {
        if (ev) (void)hipEventRecord(ev[2 * g], st);
        RUN(linear(mm.mode, arena, A, L, in, out, rows, st));
        if (ev) (void)hipEventRecord(ev[2 * g + 1], st);
        ++g;
        return (int)PIPS_OK;
    };
    RUN(timed(in_proj(A, xb), X, x, M));
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        RUN(launch_token_mix(arena, A.mix[d], x, xn, P, st, bf16, S, xb));
        RUN(timed(up_proj(A, d), xn, h, M));
        RUN(timed(down_proj(A, d, xb), h, x, M));
    }
    RUN(launch_ln_mean(x, arena + A.lnf_g, arena + A.lnf_b, pooled, P, st, S, xb));
    return timed(head_proj(A), pooled, delta, P);
}

int mixer_timed(const void* arena_v, const float* X, int M, int flags, float* delta, void* workspace, size_t workspace_bytes,
                hipStream_t st, float* ms_host) {
    PIPS_CHECK_ARG(ms_host != nullptr, "mixer_timed: null output");
    constexpr int NG = 2 * PIPS_DEPTH + 2;
    constexpr int NCAL = 8;                      // empty event pairs: the marker-to-marker overhead
    Events ev(2 * NG), cal(2 * NCAL);
    if (!ev.ok() || !cal.ok()) return PIPS_E_LAUNCH;
    int rc = mixer_impl(arena_v, X, M, PIPS_S, mixer_mode(flags), delta, workspace, workspace_bytes, st, ev.ev);
    for (int i = 0; i < 2 * NCAL; ++i) cal.record(i, st);
    if (rc == PIPS_OK && !cal.wait(2 * NCAL - 1)) rc = PIPS_E_LAUNCH;
    if (rc != PIPS_OK) return rc;
    float up = 0.f, down = 0.f, ovh = 0.f;
    for (int i = 0; i < NCAL; ++i) ovh += cal.elapsed(2 * i, 2 * i + 1);
    for (int d = 0; d < PIPS_DEPTH; ++d) {
        up += ev.elapsed(2 * (1 + 2 * d), 2 * (1 + 2 * d) + 1);
        down += ev.elapsed(2 * (2 + 2 * d), 2 * (2 + 2 * d) + 1);
    }
    ms_host[0] = ev.elapsed(0, 1);
    ms_host[1] = up / PIPS_DEPTH;
    ms_host[2] = down / PIPS_DEPTH;
    ms_host[3] = ev.elapsed(2 * (NG - 1), 2 * (NG - 1) + 1);
    ms_host[4] = ovh / NCAL;
    return PIPS_OK;
}

// The two channel-mix GEMM shapes as launch TRAINS: the 12 layers' up-projections (then their down-projections) back to back on the
// layers' own weights between ONE event pair, reps times -> ms2_host = {up, down} milliseconds per launch.  No per-launch event and
// no overhead to subtract: start-to-start durations as the forward pays them (what a rocprofv3 kernel trace of the forward shows).
// The workspace must hold the activations of a mixer pass at this M (pips_mixer_fwd* on the same workspace first).
int mixer_gemm_train(const void* arena_v, int M, int flags, void* workspace, size_t workspace_bytes, hipStream_t st, int reps,
                     float* ms2_host) {
    PIPS_CHECK_ARG(arena_v && workspace && ms2_host && reps > 0, "mixer_gemm_train: bad argument");
    PIPS_CHECK_ARG(M > 0 && M % PIPS_S == 0, "mixer_gemm_train: M=%d must be a positive multiple of %d", M, PIPS_S);
    if (workspace_bytes < mixer_workspace_bytes(M, PIPS_S)) {
        set_error("mixer_gemm_train: workspace %zu < %zu bytes", workspace_bytes, mixer_workspace_bytes(M, PIPS_S));
        return PIPS_E_WORKSPACE;
    }
    // the mode pips_mixer_fwd_s derives from the same flags (incl. PIPS_FLAG_BF16_STREAM: the workspace's x is then a bf16 stream and
    // the down-projection the bf16-residual kernel the forward launches)
    const MixerMode mm = mixer_mode(flags);
    const bool xb = mm.mode == BF16 && mm.bf16_stream;
    const ArenaLayout& A = arena_layout(PIPS_S);
    const float* arena = (const float*)arena_v;
    const MixerPlan W = plan_mixer(M, PIPS_S);
    float* ws = (float*)workspace;
    float* x = ws + W.x; float* xn = ws + W.xn; float* h = ws + W.h;
    Events ev(3);
    if (!ev.ok()) return PIPS_E_LAUNCH;
    int rc = PIPS_OK;
    auto up = [&](int d) { return linear(mm.mode, arena, A, up_proj(A, d), xn, h, M, st); };
    auto down = [&](int d) { return linear(mm.mode, arena, A, down_proj(A, d, xb), h, x, M, st); };    // in place, like the mixer
    for (int d = 0; d < PIPS_DEPTH && rc == PIPS_OK; ++d) rc = up(d);                   // warm: clocks, caches
    ev.record(0, st);
    for (int r = 0; r < reps && rc == PIPS_OK; ++r)
        for (int d = 0; d < PIPS_DEPTH && rc == PIPS_OK; ++d) rc = up(d);
    ev.record(1, st);
    for (int r = 0; r < reps && rc == PIPS_OK; ++r)
        for (int d = 0; d < PIPS_DEPTH && rc == PIPS_OK; ++d) rc = down(d);
    ev.record(2, st);
    if (rc == PIPS_OK && !ev.wait(2)) rc = PIPS_E_LAUNCH;
    if (rc == PIPS_OK) {
        ms2_host[0] = ev.elapsed(0, 1) / (float)(reps * PIPS_DEPTH);
        ms2_host[1] = ev.elapsed(1, 2) / (float)(reps * PIPS_DEPTH);
    }
    return rc;
}

// ------------------------------------------------------------------ tracker driver / whole forward
struct TrackPlan { size_t coords, coords0, ffeats, ffeat0, X, delta, mixer, total; };   // floats
TrackPlan plan_track(int B, int N, int S) {
    TrackPlan P;
    Bump b;
    const int M = B * N * S;
    P.coords = b.take((size_t)M * 2);
    P.coords0 = b.take((size_t)M * 2);
    P.ffeats = b.take((size_t)M * PIPS_C);
    P.ffeat0 = b.take((size_t)B * N * PIPS_C);
    P.X = b.take((size_t)M * PIPS_KIN_PAD);
    P.delta = b.take((size_t)B * N * arena_layout(S).nout_pad);
    P.mixer = b.take(mixer_workspace_bytes(M, S) / sizeof(float));
    P.total = b.off;
    return P;
}
struct FwdPlan { size_t pyramid, enc, track, total; };   // floats
FwdPlan plan_forward(int B, int S, int H, int W, int N, int stride) {
    FwdPlan P;
    Bump b;
    const int F = B * S;
    P.pyramid = b.take(pyramid_view(F, H / stride, W / stride).total());
    P.enc = b.take(plan_encoder(F, H, W, stride).total);
    P.track = b.take(plan_track(B, N, S).total);
    P.total = b.off;
    return P;
}

size_t score_map_workspace_bytes(int B, int S, int H8, int W8) {
    if (B <= 0 || S <= 0 || H8 <= 0 || W8 <= 0) return 0;
    return (size_t)B * S * H8 * W8 * PIPS_C * sizeof(float);
}
int score_map_prepare(const float* pyramid, int B, int S, int H8, int W8, float* U, hipStream_t st) {
    PIPS_CHECK_ARG(pyramid && U && B > 0 && S > 0 && H8 >= 8 && W8 >= 8, "score_map_prepare: bad argument");
    const PyramidView v = pyramid_view(B * S, H8, W8);
    return launch_score_upsum(pyramid, v.off, v.lh, v.lw, B * S, U, st);
}

// The tracker on cached maps.  pyramid: B clips x R frame slots of H8 x W8 level-0 pixels holding T logical frames (a linear
// cache has R = T); S = window length (tokens per particle) the arena was packed for, S == PIPS_S runs the specialised kernels.
// win_start / win_dir / coords_init / feat_init / out_ffeat0 and the score-map block ce_* may be null; so may win_clip, with
// which the pyramid is ONE flat linear cache of V videos (B = 1, R = T = all frames; clip_first / clip_frames: GatherCall) or,
// with ring > 0, of V rings of `ring` slots.
struct TrackCall {
    const void* arena; const float* pyramid;
    int B, T, R, S, H8, W8;
    const float* xys; const float* coords_init; const float* feat_init;
    const int* win_start; const int* win_dir;
    const int* win_clip; const int* clip_first; const int* clip_frames; int V, ring;
    const float* times; int N, stride, iters, flags;
    void* workspace; size_t workspace_bytes;
    float* out_trajs; float* out_vis; float* out_ffeat0;
    const float* ce_tgt; float* ce_terms; void* ce_ws; size_t ce_ws_bytes;
    hipStream_t st;
};

int track_impl(const TrackCall& c) {
    PIPS_CHECK_ARG(c.arena && c.pyramid && c.xys && c.times && c.workspace && c.out_trajs && c.out_vis, "track: null pointer");
    PIPS_CHECK_ARG(c.B > 0 && c.N > 0 && c.T >= 1 && c.R >= 1 && c.iters >= 0 && c.stride >= 1,
                   "track: need B,N,T,R,stride >= 1 and iters >= 0");
    PIPS_CHECK_ARG(c.S >= 1 && c.S <= PIPS_S_MAX, "track: window length S=%d outside 1..%d", c.S, PIPS_S_MAX);
    RUN(check_sampled_map(c.H8, c.W8, "track"));
    PIPS_CHECK_ARG(c.win_dir == nullptr || c.win_start != nullptr, "track: win_dir needs win_start");
    ClipTable ct;
    RUN(clip_table(c.win_clip, c.clip_first, c.clip_frames, c.V, c.win_start, c.B, c.T, c.R, c.ring, "track", ct));
    PIPS_CHECK_ARG(c.win_clip == nullptr || c.ce_tgt == nullptr, "track: no score-map terms on a clip table");
    const int B = c.B, N = c.N, S = c.S;
    const TrackPlan P = plan_track(B, N, S);
    if (c.workspace_bytes < P.total * sizeof(float)) {
        set_error("track: workspace %zu < %zu bytes", c.workspace_bytes, P.total * sizeof(float));
        return PIPS_E_WORKSPACE;
    }
    hipStream_t st = c.st;
    const float* arena = (const float*)c.arena;
    float* ws = (float*)c.workspace;
    const int M = B * N * S;
    float* coords = ws + P.coords; float* coords0 = ws + P.coords0; float* ffeats = ws + P.ffeats;
    float* ffeat0 = c.out_ffeat0 != nullptr ? c.out_ffeat0 : ws + P.ffeat0;
    const size_t traj_sz = (size_t)B * S * N * 2;
    RUN(launch_init_coords(c.xys, c.coords_init, B, N, (float)c.stride, coords, coords0, c.out_trajs, st, S));
    if (c.feat_init != nullptr) {
        if (c.feat_init != ffeat0)
            (void)hipMemcpyAsync(ffeat0, c.feat_init, (size_t)B * N * PIPS_C * sizeof(float), hipMemcpyDeviceToDevice, st);
    } else {
        RUN(launch_point_sample_strided(c.pyramid, B, c.R, c.T, c.H8, c.W8, coords, S * 2, N, c.win_start, ffeat0, st,
                                        c.win_clip != nullptr ? &ct : nullptr));                                  // :463
    }
    RUN(launch_init_ffeats(ffeat0, B * N, ffeats, st, S));                                                    // :466
    if (c.ce_tgt != nullptr) {          // score-map loss terms of every iteration (:501-511, 58-92): evaluation only
        PIPS_CHECK_ARG(c.ce_terms && c.ce_ws && c.win_start == nullptr && c.T == S && c.R == c.T,
                       "track: score-map terms need their output and workspace, S frames per clip and no windows");
        if (c.ce_ws_bytes < score_map_workspace_bytes(B, c.T, c.H8, c.W8)) {
            set_error("track: score-map workspace %zu < %zu bytes", c.ce_ws_bytes, score_map_workspace_bytes(B, c.T, c.H8, c.W8));
            return PIPS_E_WORKSPACE;
        }
        RUN(score_map_prepare(c.pyramid, B, c.T, c.H8, c.W8, (float*)c.ce_ws, st));
    }
    if (c.iters == 0)     // the loop body never runs: vis_e comes from the initial features (:559)
        RUN(launch_vis_head(arena, ffeats, B, N, c.out_vis, st, S));
    // the mixer workspace is idle while the gather runs: it doubles as the binning scratch
    GatherCall g;
    memset(&g, 0, sizeof(g));
    g.pyramid = c.pyramid; g.B = B; g.T = c.T; g.R = c.R; g.S = S; g.H8 = c.H8; g.W8 = c.W8;
    g.ffeats = ffeats; g.coords = coords; g.times = c.times; g.N = N;
    g.win_start = c.win_start; g.win_dir = c.win_dir;
    g.win_clip = c.win_clip; g.clip_first = c.clip_first; g.clip_frames = c.clip_frames; g.V = c.V; g.ring = c.ring;
    g.X = ws + P.X;
    g.bf16_maps = (c.flags & PIPS_FLAG_BF16_MAPS) != 0;
    g.route = GATHER_AUTO;
    g.scratch = ws + P.mixer; g.scratch_bytes = mixer_workspace_bytes(M, S);
    g.st = st;
    for (int it = 0; it < c.iters; ++it) {                                                                   // :499
        if (c.ce_tgt != nullptr)         // fcorr_fn.corr(ffeats) of this iteration (:501), before the update
            RUN(launch_score_terms((const float*)c.ce_ws, B, S, c.H8, c.W8, ffeats, N, c.ce_tgt, c.ce_terms + (size_t)it * M * 2, st));
        RUN(mixer_input(g));
        RUN(mixer_impl(arena, ws + P.X, M, S, mixer_mode(c.flags), ws + P.delta, ws + P.mixer, mixer_workspace_bytes(M, S), st, nullptr));
        RUN(launch_state_update(arena, ws + P.delta, ffeats, coords, coords0, B, N, (float)c.stride,
                                c.out_trajs + (size_t)(it + 1) * traj_sz, it + 1 == c.iters ? c.out_vis : nullptr, st, S));
    }
    PIPS_CHECK_LAUNCH("pips_track");
    return PIPS_OK;
}

// what every pips_track* form shares; the caller names R, S, win_dir and the score-map block
TrackCall track_call(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys, const float* coords_init,
                     const float* feat_init, const int* win_start, const float* times, int N, int stride, int iters, int flags,
                     void* workspace, size_t workspace_bytes, float* out_trajs, float* out_vis, float* out_ffeat0, void* stream) {
    TrackCall c;
    memset(&c, 0, sizeof(c));
    c.arena = arena; c.pyramid = pyramid; c.B = B; c.T = T; c.H8 = H8; c.W8 = W8;
    c.xys = xys; c.coords_init = coords_init; c.feat_init = feat_init; c.win_start = win_start;
    c.times = times; c.N = N; c.stride = stride; c.iters = iters; c.flags = flags;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.out_trajs = out_trajs; c.out_vis = out_vis; c.out_ffeat0 = out_ffeat0;
    c.st = (hipStream_t)stream;
    c.R = T; c.S = PIPS_S;               // a linear cache and the window of the shipped checkpoints, unless the caller says otherwise
    return c;
}

// what every pips_mixer_input_build* form shares: a linear cache of `frames` frames per clip, windows of PIPS_S rows, no
// per-particle window table, fp32 maps, route AUTO
GatherCall gather_call(const float* pyramid, int B, int frames, int H8, int W8, const float* ffeats, const float* coords,
                       const float* times, int N, float* X, void* stream) {
    GatherCall g;
    memset(&g, 0, sizeof(g));
    g.pyramid = pyramid; g.B = B; g.T = g.R = frames; g.S = PIPS_S; g.H8 = H8; g.W8 = W8;
    g.ffeats = ffeats; g.coords = coords; g.times = times; g.N = N; g.X = X;
    g.st = (hipStream_t)stream;
    return g;
}

// ------------------------------------------------------------------ chaining (chain_demo.py:40-83)
// The caller-owned state of a set of chained particles: trajs (L,n,2) / vis (L,n) hold frame f in row (f + base) mod L, cur
// (n) the window starts, dir (n) the time directions (sign; null = forward), feat (n,128) the carried features; active
// (n_act) the particles of this hop, strictly ascending.  vis and dir may be null; so may clip (n), the video of each particle
// in a state that holds the particles of V videos of clip_frames[v] frames each (one trajs / vis buffer, one base, L for the longest).
struct ChainState {
    int n; const int* active; int n_act; int sample_feat;
    float* trajs; float* vis; int L, base;
    int* cur; const int* dir; float* feat;
    const int* clip; const int* clip_frames; int V;
};
int check_chain_state(const ChainState& s, const char* who) {
    PIPS_CHECK_ARG(s.n_act >= 0 && s.n_act <= s.n, "%s: need 0 <= n_act <= n (n_act=%d, n=%d)", who, s.n_act, s.n);
    PIPS_CHECK_ARG(s.L >= PIPS_S, "%s: a window of %d frames needs L >= %d rows (L=%d)", who, PIPS_S, PIPS_S, s.L);
    PIPS_CHECK_ARG(s.active && s.trajs && s.cur && s.feat, "%s: null pointer", who);
    return PIPS_OK;
}
// the video lengths the live test of a state over several videos reads
int check_chain_clips(const ChainState& s, const char* who) {
    PIPS_CHECK_ARG(s.clip == nullptr || s.V >= 1, "%s: a clip table needs V >= 1 videos (V=%d)", who, s.V);
    PIPS_CHECK_ARG(s.clip == nullptr || s.clip_frames != nullptr, "%s: clip needs clip_frames", who);
    return PIPS_OK;
}
// a hop over no particle: *next_count = 0 on the stream and nothing else; a memset that fails is reported as a failed launch is
int clear_chain_count(int* next_count, const char* who, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(next_count, 0, sizeof(int), st);
    if (e != hipSuccess) {
        set_error("%s: clearing next_count: %s", who, hipGetErrorString(e));
        return PIPS_E_LAUNCH;
    }
    return PIPS_OK;
}

// workspace of one hop, in floats: the tracker's for (B = 1, N = n_act, S = 8), the staging arrays of chain_gather and the windows
// the tracker returns (every iterate of the trajectories: the last one is written back)
struct ChainPlan { size_t track, xy, ws, wd, fi, win_trajs, win_vis, win_ffeat0, wc, total; };
ChainPlan plan_chain(int n_act, int iters) {
    ChainPlan P;
    Bump b;
    P.track = b.take(plan_track(1, n_act, PIPS_S).total);
    P.xy = b.take((size_t)n_act * 2);
    P.ws = b.take(n_act);
    P.wd = b.take(n_act);
    P.fi = b.take((size_t)n_act * PIPS_C);
    P.win_trajs = b.take((size_t)(iters + 1) * PIPS_S * n_act * 2);
    P.win_vis = b.take((size_t)PIPS_S * n_act);
    P.win_ffeat0 = b.take((size_t)n_act * PIPS_C);
    P.wc = b.take(n_act);                              // (the staged video indices of a hop over several videos)
    P.total = b.off;
    return P;
}

int chain_gather(const ChainState& s, float* xy, int* ws, int* wd, int* wc, float* fi, hipStream_t st) {
    RUN(check_chain_state(s, "chain_gather"));
    PIPS_CHECK_ARG(xy && ws && wd && (fi || s.sample_feat) && (wc || !s.clip), "chain_gather: null pointer");
    if (s.n_act == 0) return PIPS_OK;
    return launch_chain_gather(s.trajs, s.L, s.base, s.n, s.cur, s.dir, s.feat, s.active, s.n_act, s.sample_feat, xy, ws, wd, fi, st,
                               s.clip, wc);
}

int chain_step(const ChainState& s, const float* win_trajs, const float* win_vis, const float* win_ffeat0, int T, int* next_active,
               int* next_count, int* steps, hipStream_t st) {
    RUN(check_chain_state(s, "chain_step"));
    RUN(check_chain_clips(s, "chain_step"));
    PIPS_CHECK_ARG(T >= 1, "chain_step: need T >= 1 (T=%d)", T);
    PIPS_CHECK_ARG(next_active && next_count, "chain_step: null pointer");
    PIPS_CHECK_ARG(next_active != s.active, "chain_step: next_active may not alias active");
    if (s.n_act == 0) return clear_chain_count(next_count, "chain_step", st);
    PIPS_CHECK_ARG(win_trajs && win_vis && (win_ffeat0 || !s.sample_feat), "chain_step: null pointer");
    return launch_chain_step(win_trajs, win_vis, win_ffeat0, s.n, s.active, s.n_act, s.sample_feat, s.trajs, s.vis, s.L, s.base, T, s.cur,
                             s.dir, s.feat, next_active, next_count, steps, st, s.clip, s.clip_frames, s.V);
}

// One hop: chain_gather, the tracker on (B = 1, N = n_act) windows, chain_step.  Shared by pips_chain_hop* and pips_stream_round*.
// ring > 0: the videos of the clip table are rings of `ring` slots (TrackCall).
int chain_hop(const ChainState& s, const void* arena, const float* pyramid, int T, int R, int H8, int W8, const float* times, int stride,
              int iters, int flags, const int* clip_first, int* next_active, int* next_count, int* steps, void* workspace,
              size_t workspace_bytes, hipStream_t st, int ring = 0) {
    const int n_act = s.n_act;
    // every check ahead of the first launch: a rejected call leaves the caller's state as it was
    RUN(check_chain_state(s, "chain_hop"));
    RUN(check_chain_clips(s, "chain_hop"));
    PIPS_CHECK_ARG(R >= 1 && T >= 1, "chain_hop: need R >= 1 and T >= 1 (R=%d, T=%d)", R, T);
    PIPS_CHECK_ARG(s.clip == nullptr || clip_first != nullptr, "chain_hop: clip needs clip_first and clip_frames");
    PIPS_CHECK_ARG(s.clip == nullptr || R == T, "chain_hop: a clip table needs a linear cache, R = T (R=%d, T=%d)", R, T);
    PIPS_CHECK_ARG(next_active && next_count, "chain_hop: null pointer");
    PIPS_CHECK_ARG(next_active != s.active, "chain_hop: next_active may not alias active");
    PIPS_CHECK_ARG(iters >= 0 && stride >= 1, "chain_hop: need iters >= 0 and stride >= 1");
    RUN(check_sampled_map(H8, W8, "chain_hop"));
    if (n_act == 0) return clear_chain_count(next_count, "chain_hop", st);
    PIPS_CHECK_ARG(arena && pyramid && times && workspace, "chain_hop: null pointer");
    const ChainPlan P = plan_chain(n_act, iters);
    if (workspace_bytes < P.total * sizeof(float)) {
        set_error("chain_hop: workspace %zu < %zu bytes", workspace_bytes, P.total * sizeof(float));
        return PIPS_E_WORKSPACE;
    }
    float* ws = (float*)workspace;
    float* xy = ws + P.xy; float* fi = ws + P.fi;
    int* win_start = reinterpret_cast<int*>(ws + P.ws); int* win_dir = reinterpret_cast<int*>(ws + P.wd);
    int* win_clip = reinterpret_cast<int*>(ws + P.wc);
    float* win_trajs = ws + P.win_trajs; float* win_vis = ws + P.win_vis; float* win_ffeat0 = ws + P.win_ffeat0;
    RUN(chain_gather(s, xy, win_start, win_dir, win_clip, fi, st));
    // the first window samples its features at the start position (feat_init = NULL) and returns them; later ones carry feat
    TrackCall c = track_call(arena, pyramid, 1, T, H8, W8, xy, nullptr, s.sample_feat ? nullptr : fi, win_start, times, n_act, stride,
                             iters, flags, ws + P.track, plan_track(1, n_act, PIPS_S).total * sizeof(float), win_trajs, win_vis,
                             s.sample_feat ? win_ffeat0 : nullptr, st);
    c.R = R;
    c.win_dir = s.dir != nullptr ? win_dir : nullptr;
    if (s.clip != nullptr) { c.win_clip = win_clip; c.clip_first = clip_first; c.clip_frames = s.clip_frames; c.V = s.V; c.ring = ring; }
    RUN(track_impl(c));
    return chain_step(s, win_trajs + (size_t)iters * PIPS_S * n_act * 2, win_vis, win_ffeat0, T, next_active, next_count, steps, st);
}

// ------------------------------------------------------------------ streamed chaining (drivers.StreamTracker)
// workspace of one round over a state of n queries, in floats: a hop's for n_act = n, the staging of the joining queries' point
// sample (its tracker workspace is the hop's, idle until the hop starts) and the hop's compacted list and count, which a stream
// does not read (stream_select_kernel decides who is ready)
// clips: a state over several streams also stages the joining queries' stream indices
struct StreamPlan { size_t chain, jxy, jtq, jfeat, jtrajs, jvis, next_active, next_count, jclip, total; };
StreamPlan plan_stream(int n, int iters, bool clips = false) {
    StreamPlan P;
    Bump b;
    P.chain = b.take(plan_chain(n, iters).total);
    P.jxy = b.take((size_t)n * 2);
    P.jtq = b.take(n);
    P.jfeat = b.take((size_t)n * PIPS_C);
    P.jtrajs = b.take((size_t)PIPS_S * n * 2);
    P.jvis = b.take((size_t)PIPS_S * n);
    P.next_active = b.take(n);
    P.next_count = b.take(1);
    P.jclip = clips ? b.take(n) : 0;
    P.total = b.off;
    return P;
}

// One round of a stream state (pips_stream_round) or of a state over V streams (pips_stream_round_clips: clips != null, T = R = the
// flat slots of the cache, ring = the slots of each stream's ring).  Every check ahead of the first launch.
struct StreamRound {
    const void* arena; const float* pyramid; int T, R, ring, H8, W8; const float* times; int stride, iters, flags, final_;
    int n, n_act, n_new; const int* tq; const float* xy; int* cur; int* status; float* feat; float* trajs; float* vis; int L;
    int* active; int* new_list; int* counts; int* steps; void* workspace; size_t workspace_bytes;
    const StreamClips* clips; const int* clip_first;
};
int check_stream_clips(const StreamClips& k, const char* who) {
    PIPS_CHECK_ARG(k.V >= 1 && k.V <= STREAM_V_MAX, "%s: need 1 <= V <= %d streams (V=%d)", who, STREAM_V_MAX, k.V);
    PIPS_CHECK_ARG(k.clip && k.frames && k.final_, "%s: null pointer", who);
    return PIPS_OK;
}
int stream_round(const StreamRound& r, hipStream_t st) {
    const int n = r.n, n_act = r.n_act, n_new = r.n_new, iters = r.iters;
    const bool clips = r.clips != nullptr;
    PIPS_CHECK_ARG(n >= 1, "stream_round: need n >= 1 (n=%d)", n);
    PIPS_CHECK_ARG(n_act >= 0 && n_act <= n && n_new >= 0 && n_new <= n_act,
                   "stream_round: need 0 <= n_new <= n_act <= n (n_new=%d, n_act=%d, n=%d)", n_new, n_act, n);
    PIPS_CHECK_ARG(r.L >= 2 * PIPS_S, "stream_round: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, r.L);
    const int slots = clips ? r.ring : r.R;
    PIPS_CHECK_ARG(slots >= PIPS_S + 1, "stream_round: a frame ring needs R >= %d slots, a window and a new frame (R=%d)", PIPS_S + 1,
                   slots);
    PIPS_CHECK_ARG(r.T >= 1, "stream_round: need T >= 1 (T=%d)", r.T);
    PIPS_CHECK_ARG(iters >= 0 && r.stride >= 1, "stream_round: need iters >= 0 and stride >= 1");
    RUN(check_sampled_map(r.H8, r.W8, "stream_round"));
    PIPS_CHECK_ARG(r.arena && r.pyramid && r.times && r.tq && r.xy && r.cur && r.status && r.feat && r.trajs && r.vis && r.active &&
                   r.new_list && r.counts && r.workspace, "stream_round: null pointer");
    if (clips) {
        RUN(check_stream_clips(*r.clips, "stream_round"));
        PIPS_CHECK_ARG(r.clip_first != nullptr, "stream_round: null pointer");
        PIPS_CHECK_ARG((long long)r.clips->V * r.ring <= r.T, "stream_round: %d rings of %d slots need a buffer of %lld slots (F=%d)",
                       r.clips->V, r.ring, (long long)r.clips->V * r.ring, r.T);
    }
    // the hop's and the point sample's own plans lie inside the regions sized for n (n_new <= n_act <= n)
    const StreamPlan P = plan_stream(n, iters, clips);
    const ChainPlan CP = plan_chain(n, iters);
    const size_t join_track = n_new > 0 ? plan_track(1, n_new, PIPS_S).total : 0;
    const size_t hop = n_act > 0 ? plan_chain(n_act, iters).total : 0;
    if (r.workspace_bytes < P.total * sizeof(float) || hop > CP.total || join_track > plan_track(1, n, PIPS_S).total) {
        set_error("stream_round: workspace %zu < %zu bytes", r.workspace_bytes, P.total * sizeof(float));
        return PIPS_E_WORKSPACE;
    }
    if (n_act == 0) return PIPS_OK;
    float* ws = (float*)r.workspace;
    const int* clip = clips ? r.clips->clip : nullptr;
    const int* frames = clips ? r.clips->frames : nullptr;
    const int V = clips ? r.clips->V : 0, ring = clips ? r.ring : 0;
    if (n_new > 0) {
        // the joining queries' first-window features: the point sample of a track call without feat_init, at their own frames
        float* jxy = ws + P.jxy; int* jtq = reinterpret_cast<int*>(ws + P.jtq); float* jfeat = ws + P.jfeat;
        int* jclip = clips ? reinterpret_cast<int*>(ws + P.jclip) : nullptr;
        RUN(launch_stream_join_gather(r.new_list, n_new, n, r.xy, r.tq, jxy, jtq, st, clip, jclip));
        TrackCall c = track_call(r.arena, r.pyramid, 1, r.T, r.H8, r.W8, jxy, nullptr, nullptr, jtq, r.times, n_new, r.stride, 0, r.flags,
                                 ws + P.chain + CP.track, join_track * sizeof(float), ws + P.jtrajs, ws + P.jvis, jfeat,
                                 st);
        c.R = r.R;
        if (clips) { c.win_clip = jclip; c.clip_first = r.clip_first; c.clip_frames = frames; c.V = V; c.ring = ring; }
        RUN(track_impl(c));
        RUN(launch_stream_join_scatter(r.new_list, n_new, n, jfeat, r.feat, st));
    }
    const ChainState s = {n, r.active, n_act, 0, r.trajs, r.vis, r.L, 0, r.cur, nullptr, r.feat, clip, frames, V};
    RUN(chain_hop(s, r.arena, r.pyramid, r.T, r.R, r.H8, r.W8, r.times, r.stride, iters, r.flags, r.clip_first,
                  reinterpret_cast<int*>(ws + P.next_active), reinterpret_cast<int*>(ws + P.next_count), r.steps, ws + P.chain,
                  CP.total * sizeof(float), st, ring));
    return launch_stream_select(r.T, r.final_, n, r.tq, r.xy, r.cur, r.status, r.trajs, r.L, r.active, r.new_list, r.counts, st, r.clips);
}

}  // namespace

// ================================================================== the C ABI (include/pips_hip.h)
// Argument checks that belong to one entry point, the descriptor, one call.  Nothing below launches a kernel itself.
extern "C" {

const char* pips_last_error(void) { return g_err; }
int pips_abi_version(void) { return 3; }
int pips_device_cus(void) { return device_cus(); }

// ---- weights
size_t pips_weight_arena_bytes(void) { return pips_weight_arena_bytes_s(PIPS_S); }
int pips_delta_stride(int S) { return (S < 1 || S > PIPS_S_MAX) ? 0 : arena_layout(S).nout_pad; }
size_t pips_weight_arena_bytes_s(int S) {
    if (S < 1 || S > PIPS_S_MAX) return 0;
    return arena_layout(S).total_all * sizeof(float);
}
int pips_repack_weights(const void* const* params, int nparams, void* arena, void* stream) {
    return repack_weights(params, nparams, arena, PIPS_S, PIPS_PACK_FP32 | PIPS_PACK_BF16 | PIPS_PACK_SPLIT, stream);
}
int pips_repack_weights_ex(const void* const* params, int nparams, void* arena, int sections, void* stream) {
    return repack_weights(params, nparams, arena, PIPS_S, sections, stream);
}
int pips_repack_weights_s(const void* const* params, int nparams, void* arena, int S, int sections, void* stream) {
    return repack_weights(params, nparams, arena, S, sections, stream);
}

// ---- building blocks
int pips_gemm_f32(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N,
                  int K, int epi, const float* R, int ldr, void* stream) {
    PIPS_CHECK_ARG(A && W && C, "gemm: null pointer");
    PIPS_CHECK_ARG(epi_ok(epi, R), "gemm: bad epilogue");
    return launch_gemm(gemm_args(A, lda, W, bias, C, ldc, M, N, K, epi, R, ldr), (hipStream_t)stream);
}
int pips_gemm_f32x3(const float* A, int lda, const void* W3, const float* bias, float* C, int ldc, int M, int N,
                    int K, int epi, const float* R, int ldr, void* stream) {
    PIPS_CHECK_ARG(A && W3 && C, "gemm_x3: null pointer");
    PIPS_CHECK_ARG(epi_ok(epi, R), "gemm_x3: bad epilogue");
    return launch_gemm_x3(gemm_args(A, lda, W3, bias, C, ldc, M, N, K, epi, R, ldr), (hipStream_t)stream);
}
int pips_gemm_bf16(const void* A, int a_bf16, int lda, const void* W, const float* bias, void* C, int out_bf16, int ldc,
                   int M, int N, int K, int epi, const float* R, int ldr, void* stream) {
    PIPS_CHECK_ARG(A && W && C, "gemm_bf16: null pointer");
    return launch_gemm_bf16(gemm_args(A, lda, W, bias, C, ldc, M, N, K, epi, R, ldr), a_bf16, out_bf16, (hipStream_t)stream);
}
int pips_gemm_bf16_route(int M, int N, int K, int epi, int a_bf16, int out_bf16) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return gemm_bf16_asm_route(route_args(M, N, K, epi), a_bf16, out_bf16);
}
int pips_gemm_f32_route(int M, int N, int K, int epi) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return gemm_f32_t4_route(route_args(M, N, K, epi), nullptr);
}
int pips_split_bf16x3(const float* src, size_t n, void* dst3, void* stream) {
    PIPS_CHECK_ARG(src && dst3, "split_bf16x3: null pointer");
    return launch_split_bf16x3(src, n, dst3, (hipStream_t)stream);
}

int pips_conv_nhwc_f32(const float* in, int F, int H, int W, int Cin, const float* wgt, const float* bias,
                       int Cout, int ksize, int cstride, int pad, float* out, float* stats, int* tiles_m_host,
                       void* stream) {
    PIPS_CHECK_ARG(in && wgt && out, "conv: null pointer");
    return conv_nhwc(conv_call(in, F, H, W, Cin, wgt, bias, Cout, ksize, cstride, pad, out, stats, tiles_m_host), (hipStream_t)stream);
}
int pips_conv_nhwc_f32_route(const float* in, int F, int H, int W, int Cin, const float* wgt, const float* bias,
                             int Cout, int ksize, int cstride, int pad, float* out, float* stats, int* tiles_m_host,
                             int route, void* stream) {
    PIPS_CHECK_ARG(in && wgt && out, "conv: null pointer");
    PIPS_CHECK_ARG(route >= PIPS_CONV_ROUTE_AUTO && route <= PIPS_CONV_ROUTE_E, "conv: unknown route %d", route);
    ConvCall c = conv_call(in, F, H, W, Cin, wgt, bias, Cout, ksize, cstride, pad, out, stats, tiles_m_host);
    c.route = route;
    return conv_nhwc(c, (hipStream_t)stream);
}
int pips_conv_nhwc_f32_r(const float* in, const float* in_norm, int F, int H, int W, int Cin, const float* wgt, const float* bias,
                         int Cout, int ksize, int cstride, int pad, float* out, float* stats, int stats_parts_cap, int* parts_host,
                         void* stream) {
    PIPS_CHECK_ARG(in && wgt && out, "conv_f32_r: null pointer");
    PIPS_CHECK_ARG(F > 0 && H > 0 && W > 0 && stats_parts_cap >= 0, "conv_f32_r: bad geometry F=%d H=%d W=%d cap=%d", F, H, W, stats_parts_cap);
    PIPS_CHECK_ARG(Cin == 64, "conv_f32_r: Cin=%d, the kernel takes 64 -> 64 layers", Cin);      // ahead of launch_conv's own checks
    ConvCall c = conv_call(in, F, H, W, Cin, wgt, bias, Cout, ksize, cstride, pad, out, stats, parts_host);
    c.route = PIPS_CONV_ROUTE_R;
    c.in_norm = in_norm;
    c.parts_cap = stats_parts_cap;
    return conv_nhwc(c, (hipStream_t)stream);
}
int pips_encoder_l1_fused(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return 0;
    return enc_l1_fused(F, conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)) ? 1 : 0;
}
int pips_inorm_finalize_pivot(const float* partial, int F, int parts, int C, float* mean_rstd, void* stream) {
    PIPS_CHECK_ARG(partial && mean_rstd && F > 0 && parts > 0 && C > 0 && C % 16 == 0, "inorm_finalize_pivot: bad arguments");
    return launch_inorm_finalize_pivot(partial, F, parts, C, mean_rstd, (hipStream_t)stream);
}
int pips_encoder_stem_parts(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return stem_tiles_m(conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3));
}
int pips_encoder_stem(const void* arena, const void* rgbs, int F, int H, int W, int flags, void* out, float* stats, int* parts_host,
                      void* stream) {
    PIPS_CHECK_ARG(arena && rgbs && out && stats, "encoder_stem: null pointer");
    PIPS_CHECK_ARG(F > 0 && H > 0 && W > 0 && (long)3 * H * W < (1L << 31), "encoder_stem: bad geometry F=%d H=%d W=%d", F, H, W);
    PIPS_CHECK_ARG((flags & ~(PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_RGB_U8)) == 0, "encoder_stem: unknown flags %d", flags);
    const ArenaLayout& A = arena_layout();
    const float* a = (const float*)arena;
    const int Ho = conv_out(H, 7, 2, 3), Wo = conv_out(W, 7, 2, 3), u8 = (flags & PIPS_FLAG_RGB_U8) ? 1 : 0;
    if (flags & PIPS_FLAG_BF16_ENCODER)
        return launch_stem_bf16(rgbs, u8, a + A.conv[0].w, a + A.conv[0].b, out, stats, F, H, W, Ho, Wo, parts_host, (hipStream_t)stream);
    return launch_stem(rgbs, u8, a + A.conv[0].w, a + A.conv[0].b, (float*)out, stats, F, H, W, Ho, Wo, parts_host, (hipStream_t)stream);
}
int pips_inorm_apply(const void* x, const float* stats, const void* res, const float* res_stats, int mode, void* y, int F, int HW,
                     int C, int maps_bf16, void* stream) {
    PIPS_CHECK_ARG(x && stats && y, "inorm_apply: null pointer");
    PIPS_CHECK_ARG(F > 0 && HW > 0 && C > 0, "inorm_apply: bad geometry F=%d HW=%d C=%d", F, HW, C);
    PIPS_CHECK_ARG(mode >= 0 && mode <= (maps_bf16 ? 3 : 2), "inorm_apply: mode %d on %s maps", mode, maps_bf16 ? "bf16" : "fp32");
    PIPS_CHECK_ARG(mode == 0 || res != nullptr, "inorm_apply: mode %d needs a shortcut map", mode);
    PIPS_CHECK_ARG(mode < 2 || res_stats != nullptr, "inorm_apply: mode %d needs the shortcut's statistics", mode);
    PIPS_CHECK_ARG(C % (maps_bf16 ? 8 : 4) == 0 && C <= 2048, "inorm_apply: C=%d must be a multiple of %d, at most 2048", C,
                   maps_bf16 ? 8 : 4);
    if (maps_bf16) return launch_inorm_apply_bf16(x, stats, res, res_stats, mode, y, F, HW, C, (hipStream_t)stream);
    // the fp32 launcher reads the mode from the pointers: hand it only those of the mode asked for
    return launch_inorm_apply((const float*)x, stats, mode >= 1 ? (const float*)res : nullptr, mode == 2 ? res_stats : nullptr,
                              (float*)y, F, HW, C, (hipStream_t)stream);
}
int pips_inorm_apply_f32(const float* x, const float* stats, const float* res, const float* res_stats, int mode, float* y, int F,
                         int HW, int C, void* stream) {
    PIPS_CHECK_ARG(x && stats && y, "inorm_apply_f32: null pointer");
    PIPS_CHECK_ARG(F > 0 && HW > 0 && C > 0, "inorm_apply_f32: bad geometry F=%d HW=%d C=%d", F, HW, C);
    PIPS_CHECK_ARG(mode >= 0 && mode <= 3, "inorm_apply_f32: mode %d", mode);
    PIPS_CHECK_ARG(mode == 0 || res != nullptr, "inorm_apply_f32: mode %d needs a shortcut map", mode);
    PIPS_CHECK_ARG(mode < 2 || res_stats != nullptr, "inorm_apply_f32: mode %d needs the shortcut's statistics", mode);
    PIPS_CHECK_ARG(C % 4 == 0 && C <= 2048, "inorm_apply_f32: C=%d must be a multiple of 4, at most 2048", C);
    // the launcher reads the mode from the pointers: hand it only those of the mode asked for
    return launch_inorm_apply(x, stats, mode >= 1 ? res : nullptr, mode >= 2 ? res_stats : nullptr, y, F, HW, C, (hipStream_t)stream,
                              mode == 3);
}
int pips_resize_into(const void* src, int F, int Hs, int Ws, int C, void* dst, int Hd, int Wd, int Cdst, int coff, int maps_bf16,
                     void* stream) {
    PIPS_CHECK_ARG(src && dst, "resize_into: null pointer");
    PIPS_CHECK_ARG(F > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && C > 0, "resize_into: bad geometry");
    const int al = maps_bf16 ? 8 : 4;
    PIPS_CHECK_ARG(C % al == 0 && Cdst % al == 0 && coff % al == 0, "resize_into: C=%d, Cdst=%d, coff=%d must be multiples of %d", C,
                   Cdst, coff, al);
    PIPS_CHECK_ARG(coff >= 0 && (long)coff + C <= Cdst, "resize_into: channels [%d, %d) outside a map of %d", coff, coff + C, Cdst);
    if (maps_bf16) return launch_resize_into_bf16(src, F, Hs, Ws, C, dst, Hd, Wd, Cdst, coff, (hipStream_t)stream);
    return launch_resize_into((const float*)src, F, Hs, Ws, C, (float*)dst, Hd, Wd, Cdst, coff, (hipStream_t)stream);
}
int pips_avgpool2(const float* src, int F, int H, int W, int C, float* dst, void* stream) {
    PIPS_CHECK_ARG(src && dst, "avgpool2: null pointer");
    PIPS_CHECK_ARG(F > 0 && C > 0 && C % 4 == 0, "avgpool2: F=%d, C=%d (a multiple of 4)", F, C);
    PIPS_CHECK_ARG(H >= 2 && W >= 2, "avgpool2: map %dx%d too small", H, W);
    return launch_avgpool2(src, F, H, W, C, dst, (hipStream_t)stream);
}
int pips_conv_nhwc_bf16(const float* in, int F, int H, int W, int Cin, const void* wgt_bf16, const float* bias,
                        int Cout, int ksize, int cstride, int pad, float* out, float* stats, int* tiles_m_host,
                        void* stream) {
    PIPS_CHECK_ARG(in && wgt_bf16 && out, "conv_bf16: null pointer");
    ConvCall c = conv_call(in, F, H, W, Cin, wgt_bf16, bias, Cout, ksize, cstride, pad, out, stats, tiles_m_host);
    c.mode = BF16;
    return conv_nhwc(c, (hipStream_t)stream);
}
int pips_conv_nhwc_f32x3(const float* in, int F, int H, int W, int Cin, const void* wgt3, const float* bias,
                         int Cout, int ksize, int cstride, int pad, float* out, float* stats, int* tiles_m_host,
                         void* stream) {
    PIPS_CHECK_ARG(in && wgt3 && out, "conv_x3: null pointer");
    ConvCall c = conv_call(in, F, H, W, Cin, wgt3, bias, Cout, ksize, cstride, pad, out, stats, tiles_m_host);
    c.mode = SPLIT;
    return conv_nhwc(c, (hipStream_t)stream);
}
int pips_conv_nhwc_bf16_maps(const void* in_bf16, const float* in_norm, int F, int H, int W, int Cin, const void* wgt_bf16,
                             const float* bias, int Cout, int ksize, int cstride, int pad, void* out, int out_is_bf16,
                             float* stats, int stats_parts_cap, int* tiles_m_host, void* stream) {
    PIPS_CHECK_ARG(in_bf16 && wgt_bf16 && out, "conv_bf16_maps: null pointer");
    ConvCall c = conv_call(in_bf16, F, H, W, Cin, wgt_bf16, bias, Cout, ksize, cstride, pad, out, stats, tiles_m_host);
    c.mode = BF16;
    c.in_bf16 = true;
    c.out_bf16 = out_is_bf16 != 0;
    c.in_norm = in_norm;
    c.parts_cap = stats_parts_cap;
    return conv_nhwc(c, (hipStream_t)stream);
}

// ---- encoder and pyramid
size_t pips_encoder_workspace_bytes(int F, int H, int W, int stride) {
    if (F <= 0 || H <= 0 || W <= 0 || stride < 1) return 0;
    return plan_encoder(F, H, W, stride).total * sizeof(float);
}
size_t pips_pyramid_offset(int F, int H, int W, int stride, int level) {
    const PyramidView v = pyramid_view(F, H / stride, W / stride);
    return level <= 0 ? 0 : level < PIPS_LEVELS ? v.off[level] : v.levels;
}
size_t pips_pyramid_mirror_offset(int F, int H, int W, int stride) { return pyramid_view(F, H / stride, W / stride).levels; }
size_t pips_pyramid_floats(int F, int H, int W, int stride) { return pyramid_view(F, H / stride, W / stride).total(); }
int pips_pyramid_mirror(float* pyramid, int F, int H, int W, int stride, void* stream) {
    PIPS_CHECK_ARG(pyramid != nullptr && F > 0, "pyramid_mirror: bad argument");
    const size_t n = pyramid_view(F, H / stride, W / stride).levels;
    return launch_pyramid_mirror(pyramid, n, pyramid + n, (hipStream_t)stream);
}
int pips_pyramid_append(const float* src, int k, float* ring, int R, int T0, int H, int W, int stride, void* stream) {
    PIPS_CHECK_ARG(src != nullptr && ring != nullptr, "pyramid_append: null pointer");
    PIPS_CHECK_ARG(R >= 1 && T0 >= 0 && k >= 1 && k <= R, "pyramid_append: need R >= 1, T0 >= 0 and 1 <= k <= R (k=%d, R=%d, T0=%d)",
                   k, R, T0);
    PIPS_CHECK_ARG(H > 0 && W > 0 && stride >= 1, "pyramid_append: bad geometry");
    const PyramidView from = pyramid_view(k, H / stride, W / stride), to = pyramid_view(R, H / stride, W / stride);
    PIPS_CHECK_ARG(!to.empty(), "pyramid_append: map too small");
    int pf8[PIPS_LEVELS];
    for (int l = 0; l < PIPS_LEVELS; ++l) pf8[l] = to.lh[l] * to.lw[l] * PIPS_C / 8;
    return launch_pyramid_append(src, from.off, k, ring, to.off, ring + to.levels, pf8, R, T0, (hipStream_t)stream);
}
int pips_pyramid_append_at(const float* src, int F_src, int src_first, int k, float* dst, int F, int ring_first, int R, int T0, int H,
                           int W, int stride, void* stream) {
    PIPS_CHECK_ARG(src != nullptr && dst != nullptr, "pyramid_append_at: null pointer");
    PIPS_CHECK_ARG(R >= 1 && T0 >= 0 && k >= 1 && k <= R, "pyramid_append_at: need R >= 1, T0 >= 0 and 1 <= k <= R (k=%d, R=%d, T0=%d)",
                   k, R, T0);
    PIPS_CHECK_ARG(H > 0 && W > 0 && stride >= 1, "pyramid_append_at: bad geometry");
    PIPS_CHECK_ARG(src_first >= 0 && F_src >= 1 && (long long)src_first + k <= F_src,
                   "pyramid_append_at: frames [%d, %d + %d) lie outside a source of %d frames", src_first, src_first, k, F_src);
    PIPS_CHECK_ARG(ring_first >= 0 && F >= 1 && (long long)ring_first + R <= F,
                   "pyramid_append_at: slots [%d, %d + %d) lie outside a buffer of %d slots", ring_first, ring_first, R, F);
    const PyramidView from = pyramid_view(F_src, H / stride, W / stride), to = pyramid_view(F, H / stride, W / stride);
    PIPS_CHECK_ARG(!to.empty(), "pyramid_append_at: map too small");
    int pf8[PIPS_LEVELS];
    for (int l = 0; l < PIPS_LEVELS; ++l) pf8[l] = to.lh[l] * to.lw[l] * PIPS_C / 8;
    return launch_pyramid_append(src, from.off, k, dst, to.off, dst + to.levels, pf8, R, T0, (hipStream_t)stream, src_first, ring_first);
}

int pips_encoder_fwd(const void* arena, const float* rgbs, int F, int H, int W, int stride, float* pyramid,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return encoder_impl(arena, rgbs, F, H, W, stride, 0, pyramid, workspace, workspace_bytes, (hipStream_t)stream);
}
int pips_encoder_fwd_bf16(const void* arena, const float* rgbs, int F, int H, int W, int stride, float* pyramid,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return encoder_impl(arena, rgbs, F, H, W, stride, PIPS_FLAG_BF16_ENCODER, pyramid, workspace, workspace_bytes, (hipStream_t)stream);
}
int pips_encoder_fwd_ex(const void* arena, const void* rgbs, int F, int H, int W, int stride, int flags,
                        float* pyramid, void* workspace, size_t workspace_bytes, void* stream) {
    return encoder_impl(arena, rgbs, F, H, W, stride, flags, pyramid, workspace, workspace_bytes, (hipStream_t)stream);
}

int pips_resize_frames(const void* src, int src_is_u8, int planes, int h, int w, float* dst, int H, int W, void* stream) {
    PIPS_CHECK_ARG(src && dst, "resize_frames: null pointer");
    PIPS_CHECK_ARG(planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_frames: empty image");
    return launch_resize_frames(src, src_is_u8, planes, h, w, dst, H, W, (hipStream_t)stream);
}

// ---- tracker stages
int pips_point_sample(const float* level0, int B, int S, int H8, int W8, const float* xy, int N, float* out,
                      void* stream) {
    PIPS_CHECK_ARG(level0 && xy && out && B > 0 && N > 0 && S > 0 && H8 > 0 && W8 > 0, "point_sample: bad argument");
    return launch_point_sample(level0, B, S, H8, W8, xy, N, out, (hipStream_t)stream);
}

int pips_mixer_input_build(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats,
                           const float* coords, const float* times, int N, float* X, void* stream) {
    return mixer_input(gather_call(pyramid, B, S, H8, W8, ffeats, coords, times, N, X, stream));
}
int pips_mixer_input_build_ex(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats, const float* coords,
                              const float* times, int N, const int* win_start, int flags, float* X, void* stream) {
    GatherCall g = gather_call(pyramid, B, S, H8, W8, ffeats, coords, times, N, X, stream);
    g.win_start = win_start;
    g.bf16_maps = (flags & PIPS_FLAG_BF16_MAPS) != 0;
    g.route = GATHER_DIRECT;
    return mixer_input(g);
}
int pips_mixer_input_build_win(const float* pyramid, int B, int T, int H8, int W8, const float* ffeats, const float* coords,
                               const float* times, int N, const int* win_start, const int* win_dir, int flags, int S, float* X,
                               void* stream) {
    return pips_mixer_input_build_ring(pyramid, B, T, T, H8, W8, ffeats, coords, times, N, win_start, win_dir, flags, S, X, stream);
}
int pips_mixer_input_build_ring(const float* pyramid, int B, int T, int R, int H8, int W8, const float* ffeats,
                                const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                int flags, int S, float* X, void* stream) {
    return pips_mixer_input_build_clips(pyramid, B, T, R, H8, W8, ffeats, coords, times, N, win_start, win_dir, nullptr, nullptr,
                                        nullptr, 0, flags, S, X, stream);
}
int pips_mixer_input_build_clips(const float* pyramid, int B, int T, int R, int H8, int W8, const float* ffeats,
                                 const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                 const int* win_clip, const int* clip_first, const int* clip_frames, int V, int flags, int S,
                                 float* X, void* stream) {
    GatherCall g = gather_call(pyramid, B, T, H8, W8, ffeats, coords, times, N, X, stream);
    g.R = R;
    g.S = S;
    g.win_start = win_start;
    g.win_dir = win_dir;
    g.win_clip = win_clip; g.clip_first = clip_first; g.clip_frames = clip_frames; g.V = V;
    g.bf16_maps = (flags & PIPS_FLAG_BF16_MAPS) != 0;
    g.route = GATHER_DIRECT;
    return mixer_input(g);
}

int pips_mixer_input_build_rings(const float* pyramid, int B, int F, int R, int H8, int W8, const float* ffeats,
                                 const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                 const int* win_clip, const int* clip_first, const int* clip_frames, int V, int flags, int S,
                                 float* X, void* stream) {
    GatherCall g = gather_call(pyramid, B, F, H8, W8, ffeats, coords, times, N, X, stream);
    g.S = S;
    g.win_start = win_start;
    g.win_dir = win_dir;
    g.win_clip = win_clip; g.clip_first = clip_first; g.clip_frames = clip_frames; g.V = V; g.ring = ring_arg(R);
    g.bf16_maps = (flags & PIPS_FLAG_BF16_MAPS) != 0;
    g.route = GATHER_DIRECT;
    return mixer_input(g);
}

size_t pips_gather_scratch_bytes(int B, int N, int H8, int W8) {
    if (B <= 0 || N <= 0 || H8 <= 0 || W8 <= 0) return 0;
    return tiled_gather_scratch_bytes(B, N, H8, W8);
}
int pips_gather_route(int B, int N, int H8, int W8, int flags) {
    if (B <= 0 || N <= 0 || H8 <= 0 || W8 <= 0) return 0;
    if (!tiled_gather_wanted(B, N, H8, W8, (flags & PIPS_FLAG_BF16_MAPS) != 0)) return 0;
    return (flags & PIPS_FLAG_BF16_MAPS) ? 2 : 1;
}
int pips_mixer_input_build_tiled_ex(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats, const float* coords,
                                    const float* times, int N, int flags, float* X, void* scratch, size_t scratch_bytes,
                                    void* stream, float* ms3_host) {
    GatherCall g = gather_call(pyramid, B, S, H8, W8, ffeats, coords, times, N, X, stream);
    g.bf16_maps = (flags & PIPS_FLAG_BF16_MAPS) != 0;
    g.scratch = scratch;
    g.scratch_bytes = scratch_bytes;
    return mixer_input_tiled(g, ms3_host);
}
int pips_mixer_input_build_tiled(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats,
                                 const float* coords, const float* times, int N, float* X, void* scratch,
                                 size_t scratch_bytes, void* stream) {
    return pips_mixer_input_build_tiled_ex(pyramid, B, S, H8, W8, ffeats, coords, times, N, 0, X, scratch, scratch_bytes, stream,
                                           nullptr);
}
int pips_mixer_input_build_tiled_timed(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats,
                                       const float* coords, const float* times, int N, float* X, void* scratch,
                                       size_t scratch_bytes, void* stream, float* ms3_host) {
    PIPS_CHECK_ARG(ms3_host != nullptr, "mixer_input_tiled_timed: null pointer");
    return pips_mixer_input_build_tiled_ex(pyramid, B, S, H8, W8, ffeats, coords, times, N, 0, X, scratch, scratch_bytes, stream,
                                           ms3_host);
}

size_t pips_mixer_workspace_bytes(int M) { return mixer_workspace_bytes(M, PIPS_S); }
size_t pips_mixer_workspace_bytes_s(int M, int S) { return mixer_workspace_bytes(M, S); }

int pips_mixer_fwd_s(const void* arena, const float* X, int M, int S, int flags, float* delta, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return mixer_impl(arena, X, M, S, mixer_mode(flags), delta, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}
int pips_mixer_fwd(const void* arena, const float* X, int M, float* delta, void* workspace, size_t workspace_bytes,
                   void* stream) {
    return pips_mixer_fwd_s(arena, X, M, PIPS_S, 0, delta, workspace, workspace_bytes, stream);
}
int pips_mixer_fwd_bf16(const void* arena, const float* X, int M, float* delta, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return pips_mixer_fwd_s(arena, X, M, PIPS_S, PIPS_FLAG_BF16_MIXER, delta, workspace, workspace_bytes, stream);
}
int pips_mixer_fwd_x3(const void* arena, const float* X, int M, float* delta, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return pips_mixer_fwd_s(arena, X, M, PIPS_S, PIPS_FLAG_SPLIT_BF16, delta, workspace, workspace_bytes, stream);
}
int pips_mixer_fwd_timed_ex(const void* arena, const float* X, int M, int flags, float* delta, void* workspace,
                            size_t workspace_bytes, void* stream, float* ms_host) {
    return mixer_timed(arena, X, M, flags, delta, workspace, workspace_bytes, (hipStream_t)stream, ms_host);
}
int pips_mixer_fwd_timed(const void* arena, const float* X, int M, float* delta, void* workspace,
                         size_t workspace_bytes, void* stream, float* ms_host) {
    return mixer_timed(arena, X, M, 0, delta, workspace, workspace_bytes, (hipStream_t)stream, ms_host);
}
int pips_mixer_gemm_train(const void* arena, int M, int flags, void* workspace, size_t workspace_bytes, void* stream, int reps,
                          float* ms2_host) {
    return mixer_gemm_train(arena, M, flags, workspace, workspace_bytes, (hipStream_t)stream, reps, ms2_host);
}

int pips_state_update_s(const void* arena, const float* delta, float* ffeats, float* coords, const float* coords0,
                        int B, int N, int S, float stride, float* out_traj, float* out_vis, void* stream) {
    PIPS_CHECK_ARG(arena && delta && ffeats && coords && coords0 && out_traj, "state_update: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "state_update: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(B > 0 && N > 0, "state_update: empty");
    return launch_state_update((const float*)arena, delta, ffeats, coords, coords0, B, N, stride, out_traj, out_vis,
                               (hipStream_t)stream, S);
}
int pips_state_update(const void* arena, const float* delta, float* ffeats, float* coords, const float* coords0,
                      int B, int N, float stride, float* out_traj, float* out_vis, void* stream) {
    return pips_state_update_s(arena, delta, ffeats, coords, coords0, B, N, PIPS_S, stride, out_traj, out_vis, stream);
}

// ---- the mixer's stage kernels alone (unit tests): the launches of mixer_impl / track_impl, nothing else
// flags -> {bf16 operands, bf16 stream}; false for anything but the three combinations the mixer itself runs these kernels in
static bool stage_mode(int flags, int S, bool* bf16, bool* xb) {
    *bf16 = (flags & PIPS_FLAG_BF16_MIXER) != 0;
    *xb = (flags & PIPS_FLAG_BF16_STREAM) != 0;
    if (flags & ~(PIPS_FLAG_BF16_MIXER | PIPS_FLAG_BF16_STREAM)) return false;
    return !*xb || (*bf16 && S == PIPS_S);
}
int pips_token_mix(const void* arena, int layer, void* x, void* xn, int particles, int S, int flags, void* stream) {
    PIPS_CHECK_ARG(arena && x && xn, "token_mix: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "token_mix: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(particles > 0, "token_mix: particles=%d", particles);
    PIPS_CHECK_ARG(layer >= 0 && layer < PIPS_DEPTH, "token_mix: layer %d outside 0..%d", layer, PIPS_DEPTH - 1);
    bool bf16, xb;
    PIPS_CHECK_ARG(stage_mode(flags, S, &bf16, &xb), "token_mix: flags %d at S=%d", flags, S);
    return launch_token_mix((const float*)arena, arena_layout(S).mix[layer], (float*)x, (float*)xn, particles, (hipStream_t)stream, bf16,
                            S, xb);
}
int pips_ln_mean(const void* arena, const void* x, float* out, int particles, int S, int flags, void* stream) {
    PIPS_CHECK_ARG(arena && x && out, "ln_mean: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "ln_mean: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(particles > 0, "ln_mean: particles=%d", particles);
    bool bf16, xb;
    PIPS_CHECK_ARG(stage_mode(flags, S, &bf16, &xb), "ln_mean: flags %d at S=%d", flags, S);
    const ArenaLayout& A = arena_layout(S);
    const float* a = (const float*)arena;
    return launch_ln_mean((const float*)x, a + A.lnf_g, a + A.lnf_b, out, particles, (hipStream_t)stream, S, xb);
}
int pips_vis_head(const void* arena, const float* ffeats, int B, int N, int S, float* out_vis, void* stream) {
    PIPS_CHECK_ARG(arena && ffeats && out_vis, "vis_head: null pointer");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "vis_head: S=%d outside 1..%d", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(B > 0 && N > 0, "vis_head: empty");
    return launch_vis_head((const float*)arena, ffeats, B, N, out_vis, (hipStream_t)stream, S);
}

size_t pips_score_map_workspace_bytes(int B, int S, int H8, int W8) { return score_map_workspace_bytes(B, S, H8, W8); }
int pips_score_map_prepare(const float* pyramid, int B, int S, int H8, int W8, float* U, void* stream) {
    return score_map_prepare(pyramid, B, S, H8, W8, U, (hipStream_t)stream);
}
int pips_score_map_terms(const float* U, int B, int S, int H8, int W8, const float* ffeats, int N, const float* tgt,
                         float* out, void* stream) {
    PIPS_CHECK_ARG(U && ffeats && tgt && out && B > 0 && S > 0 && N > 0 && H8 > 0 && W8 > 0, "score_map_terms: bad argument");
    return launch_score_terms(U, B, S, H8, W8, ffeats, N, tgt, out, (hipStream_t)stream);
}

// ---- tracker on cached maps
size_t pips_track_workspace_bytes(int B, int N) { return pips_track_workspace_bytes_s(B, N, PIPS_S); }
size_t pips_track_workspace_bytes_s(int B, int N, int S) {
    if (B <= 0 || N <= 0 || S < 1 || S > PIPS_S_MAX) return 0;
    return plan_track(B, N, S).total * sizeof(float);
}

int pips_track(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys,
               const float* coords_init, const float* feat_init, const int* win_start, const float* times, int N,
               int stride, int iters, int flags, void* workspace, size_t workspace_bytes, float* out_trajs,
               float* out_vis, float* out_ffeat0, void* stream) {
    return track_impl(track_call(arena, pyramid, B, T, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags,
                                 workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream));
}
int pips_track_s(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys,
                 const float* coords_init, const float* feat_init, const int* win_start, const float* times, int N,
                 int stride, int iters, int flags, int S, void* workspace, size_t workspace_bytes, float* out_trajs,
                 float* out_vis, float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws,
                 size_t ce_ws_bytes, void* stream) {
    TrackCall c = track_call(arena, pyramid, B, T, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags,
                             workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream);
    c.S = S;
    c.ce_tgt = ce_tgt; c.ce_terms = ce_terms; c.ce_ws = ce_ws; c.ce_ws_bytes = ce_ws_bytes;
    return track_impl(c);
}
int pips_track_ce(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys,
                  const float* coords_init, const float* feat_init, const int* win_start, const float* times, int N,
                  int stride, int iters, int flags, void* workspace, size_t workspace_bytes, float* out_trajs,
                  float* out_vis, float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws,
                  size_t ce_ws_bytes, void* stream) {
    return pips_track_s(arena, pyramid, B, T, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags, PIPS_S,
                        workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, ce_tgt, ce_terms, ce_ws, ce_ws_bytes, stream);
}
int pips_track_ring(const void* arena, const float* pyramid, int B, int T, int R, int H8, int W8, const float* xys,
                    const float* coords_init, const float* feat_init, const int* win_start, const int* win_dir,
                    const float* times, int N, int stride, int iters, int flags, int S, void* workspace,
                    size_t workspace_bytes, float* out_trajs, float* out_vis, float* out_ffeat0, void* stream) {
    TrackCall c = track_call(arena, pyramid, B, T, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags,
                             workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream);
    c.R = R;
    c.S = S;
    c.win_dir = win_dir;
    return track_impl(c);
}
int pips_track_clips(const void* arena, const float* pyramid, int B, int T, int R, int H8, int W8, const float* xys,
                     const float* coords_init, const float* feat_init, const int* win_start, const int* win_dir,
                     const int* win_clip, const int* clip_first, const int* clip_frames, int V, const float* times, int N,
                     int stride, int iters, int flags, int S, void* workspace, size_t workspace_bytes, float* out_trajs,
                     float* out_vis, float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes,
                     void* stream) {
    TrackCall c = track_call(arena, pyramid, B, T, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags,
                             workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream);
    c.R = R;
    c.S = S;
    c.win_dir = win_dir;
    c.win_clip = win_clip; c.clip_first = clip_first; c.clip_frames = clip_frames; c.V = V;
    c.ce_tgt = ce_tgt; c.ce_terms = ce_terms; c.ce_ws = ce_ws; c.ce_ws_bytes = ce_ws_bytes;
    return track_impl(c);
}
int pips_track_rings(const void* arena, const float* pyramid, int B, int F, int R, int H8, int W8, const float* xys,
                     const float* coords_init, const float* feat_init, const int* win_start, const int* win_dir,
                     const int* win_clip, const int* clip_first, const int* clip_frames, int V, const float* times, int N,
                     int stride, int iters, int flags, int S, void* workspace, size_t workspace_bytes, float* out_trajs,
                     float* out_vis, float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes,
                     void* stream) {
    TrackCall c = track_call(arena, pyramid, B, F, H8, W8, xys, coords_init, feat_init, win_start, times, N, stride, iters, flags,
                             workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream);
    c.S = S;
    c.win_dir = win_dir;
    c.win_clip = win_clip; c.clip_first = clip_first; c.clip_frames = clip_frames; c.V = V; c.ring = ring_arg(R);
    c.ce_tgt = ce_tgt; c.ce_terms = ce_terms; c.ce_ws = ce_ws; c.ce_ws_bytes = ce_ws_bytes;
    return track_impl(c);
}
int pips_track_win(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys,
                   const float* coords_init, const float* feat_init, const int* win_start, const int* win_dir,
                   const float* times, int N, int stride, int iters, int flags, int S, void* workspace,
                   size_t workspace_bytes, float* out_trajs, float* out_vis, float* out_ffeat0, void* stream) {
    return pips_track_ring(arena, pyramid, B, T, T, H8, W8, xys, coords_init, feat_init, win_start, win_dir, times, N, stride, iters,
                           flags, S, workspace, workspace_bytes, out_trajs, out_vis, out_ffeat0, stream);
}

// ---- chaining
float pips_chain_threshold(int k) { return chain_threshold(k); }
size_t pips_chain_workspace_bytes(int n_act, int iters) {
    if (n_act <= 0 || iters < 0) return 0;
    return plan_chain(n_act, iters).total * sizeof(float);
}
int pips_chain_gather(const float* trajs, int L, int base, int n, const int* cur, const int* dir, const float* feat,
                      const int* active, int n_act, int sample_feat, float* xy, int* ws, int* wd, float* fi, void* stream) {
    return pips_chain_gather_clips(trajs, L, base, n, cur, dir, nullptr, feat, active, n_act, sample_feat, xy, ws, wd, nullptr, fi,
                                   stream);
}
int pips_chain_gather_clips(const float* trajs, int L, int base, int n, const int* cur, const int* dir, const int* clip,
                            const float* feat, const int* active, int n_act, int sample_feat, float* xy, int* ws, int* wd, int* wc,
                            float* fi, void* stream) {
    const ChainState s = {n, active, n_act, sample_feat, const_cast<float*>(trajs), nullptr, L, base, const_cast<int*>(cur), dir,
                          const_cast<float*>(feat), clip, nullptr, 0};          // (the gather reads no video length)
    return chain_gather(s, xy, ws, wd, wc, fi, (hipStream_t)stream);
}
int pips_chain_step(const float* win_trajs, const float* win_vis, const float* win_ffeat0, int T, int n, const int* active,
                    int n_act, int sample_feat, float* trajs, float* vis, int L, int base, int* cur, const int* dir, float* feat,
                    int* next_active, int* next_count, int* steps, void* stream) {
    return pips_chain_step_clips(win_trajs, win_vis, win_ffeat0, T, n, active, n_act, sample_feat, trajs, vis, L, base, cur, dir,
                                 nullptr, nullptr, 0, feat, next_active, next_count, steps, stream);
}
int pips_chain_step_clips(const float* win_trajs, const float* win_vis, const float* win_ffeat0, int T, int n, const int* active,
                          int n_act, int sample_feat, float* trajs, float* vis, int L, int base, int* cur, const int* dir,
                          const int* clip, const int* clip_frames, int V, float* feat, int* next_active, int* next_count,
                          int* steps, void* stream) {
    const ChainState s = {n, active, n_act, sample_feat, trajs, vis, L, base, cur, dir, feat, clip, clip_frames, V};
    return chain_step(s, win_trajs, win_vis, win_ffeat0, T, next_active, next_count, steps, (hipStream_t)stream);
}
int pips_chain_hop(const void* arena, const float* pyramid, int T, int R, int H8, int W8, const float* times, int stride, int iters,
                   int flags, int n, const int* active, int n_act, int sample_feat, float* trajs, float* vis, int L, int base,
                   int* cur, const int* dir, float* feat, int* next_active, int* next_count, int* steps, void* workspace,
                   size_t workspace_bytes, void* stream) {
    return pips_chain_hop_clips(arena, pyramid, T, R, H8, W8, times, stride, iters, flags, n, active, n_act, sample_feat, trajs, vis, L,
                                base, cur, dir, nullptr, nullptr, nullptr, 0, feat, next_active, next_count, steps, workspace,
                                workspace_bytes, stream);
}
int pips_chain_hop_clips(const void* arena, const float* pyramid, int T, int R, int H8, int W8, const float* times, int stride,
                         int iters, int flags, int n, const int* active, int n_act, int sample_feat, float* trajs, float* vis, int L,
                         int base, int* cur, const int* dir, const int* clip, const int* clip_first, const int* clip_frames, int V,
                         float* feat, int* next_active, int* next_count, int* steps, void* workspace, size_t workspace_bytes,
                         void* stream) {
    const ChainState s = {n, active, n_act, sample_feat, trajs, vis, L, base, cur, dir, feat, clip, clip_frames, V};
    return chain_hop(s, arena, pyramid, T, R, H8, W8, times, stride, iters, flags, clip_first, next_active, next_count, steps, workspace,
                     workspace_bytes, (hipStream_t)stream);
}

// ---- streamed chaining
size_t pips_stream_workspace_bytes(int n, int iters) {
    if (n <= 0 || iters < 0) return 0;
    return plan_stream(n, iters).total * sizeof(float);
}
int pips_stream_select(int T, int final, int n, const int* tq, const float* xy, int* cur, int* status, float* trajs, int L,
                       int* active, int* new_list, int* counts, void* stream) {
    PIPS_CHECK_ARG(n >= 1 && T >= 1, "stream_select: need n >= 1 and T >= 1 (n=%d, T=%d)", n, T);
    PIPS_CHECK_ARG(L >= 2 * PIPS_S, "stream_select: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, L);
    PIPS_CHECK_ARG(tq && xy && cur && status && trajs && active && new_list && counts, "stream_select: null pointer");
    return launch_stream_select(T, final, n, tq, xy, cur, status, trajs, L, active, new_list, counts, (hipStream_t)stream);
}
int pips_stream_round(const void* arena, const float* pyramid, int T, int R, int H8, int W8, const float* times, int stride, int iters,
                      int flags, int final, int n, int n_act, int n_new, const int* tq, const float* xy, int* cur, int* status,
                      float* feat, float* trajs, float* vis, int L, int* active, int* new_list, int* counts, int* steps,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const StreamRound r = {arena, pyramid, T, R, 0, H8, W8, times, stride, iters, flags, final, n, n_act, n_new, tq, xy, cur, status, feat,
                           trajs, vis, L, active, new_list, counts, steps, workspace, workspace_bytes, nullptr, nullptr};
    return stream_round(r, (hipStream_t)stream);
}
size_t pips_stream_workspace_bytes_clips(int n, int iters, int V) {
    if (n <= 0 || iters < 0 || V < 1 || V > STREAM_V_MAX) return 0;
    return plan_stream(n, iters, true).total * sizeof(float);
}
int pips_stream_select_clips(int n, const int* tq, const float* xy, int* cur, int* status, const int* clip, const int* clip_frames,
                             const int* clip_final, int V, float* trajs, int L, int* active, int* new_list, int* counts,
                             void* stream) {
    const StreamClips k = {clip, clip_frames, clip_final, V};
    PIPS_CHECK_ARG(n >= 1, "stream_select: need n >= 1 (n=%d)", n);
    PIPS_CHECK_ARG(L >= 2 * PIPS_S, "stream_select: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, L);
    PIPS_CHECK_ARG(tq && xy && cur && status && trajs && active && new_list && counts, "stream_select: null pointer");
    RUN(check_stream_clips(k, "stream_select"));
    return launch_stream_select(0, 0, n, tq, xy, cur, status, trajs, L, active, new_list, counts, (hipStream_t)stream, &k);
}
int pips_stream_round_clips(const void* arena, const float* pyramid, int F, int R, int H8, int W8, const float* times, int stride,
                            int iters, int flags, int n, int n_act, int n_new, const int* tq, const float* xy, int* cur, int* status,
                            const int* clip, float* feat, float* trajs, float* vis, int L, const int* clip_first,
                            const int* clip_frames, const int* clip_final, int V, int* active, int* new_list, int* counts, int* steps,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const StreamClips k = {clip, clip_frames, clip_final, V};
    const StreamRound r = {arena, pyramid, F, F, R, H8, W8, times, stride, iters, flags, 0, n, n_act, n_new, tq, xy, cur, status, feat,
                           trajs, vis, L, active, new_list, counts, steps, workspace, workspace_bytes, &k, clip_first};
    return stream_round(r, (hipStream_t)stream);
}
int pips_stream_emit(float* trajs, float* vis, int L, int n, int f0, int f1, float* out_trajs, float* out_vis, void* stream) {
    PIPS_CHECK_ARG(n >= 1, "stream_emit: need n >= 1 (n=%d)", n);
    PIPS_CHECK_ARG(L >= 2 * PIPS_S, "stream_emit: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, L);
    PIPS_CHECK_ARG(f1 >= f0 && (long long)f1 - f0 <= L, "stream_emit: need 0 <= f1 - f0 <= L (f0=%d, f1=%d, L=%d)", f0, f1, L);
    PIPS_CHECK_ARG(f1 - f0 <= PIPS_STREAM_EMIT_FRAMES_MAX, "stream_emit: at most %d frames a call, one on each row of blocks (f0=%d, f1=%d)",
                   PIPS_STREAM_EMIT_FRAMES_MAX, f0, f1);
    PIPS_CHECK_ARG(trajs && vis, "stream_emit: null pointer");
    if (f0 == f1) return PIPS_OK;                 // (no frame: the outputs are empty and may be NULL)
    PIPS_CHECK_ARG(out_trajs && out_vis, "stream_emit: null pointer");
    return launch_stream_emit(trajs, vis, L, n, f0, f1, out_trajs, out_vis, (hipStream_t)stream);
}
int pips_stream_emit_cols(float* trajs, float* vis, int L, int n, int f0, int f1, const int* cols, int m, float* out_trajs,
                          float* out_vis, void* stream) {
    PIPS_CHECK_ARG(n >= 1 && m >= 0, "stream_emit_cols: need n >= 1 and m >= 0 (n=%d, m=%d)", n, m);
    PIPS_CHECK_ARG(L >= 2 * PIPS_S, "stream_emit_cols: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, L);
    PIPS_CHECK_ARG(f1 >= f0 && (long long)f1 - f0 <= L, "stream_emit_cols: need 0 <= f1 - f0 <= L (f0=%d, f1=%d, L=%d)", f0, f1, L);
    PIPS_CHECK_ARG(f1 - f0 <= PIPS_STREAM_EMIT_FRAMES_MAX, "stream_emit_cols: at most %d frames a call, one on each row of blocks (f0=%d, f1=%d)",
                   PIPS_STREAM_EMIT_FRAMES_MAX, f0, f1);
    PIPS_CHECK_ARG(trajs && vis, "stream_emit_cols: null pointer");
    if (f0 == f1 || m == 0) return PIPS_OK;                 // (nothing to move: the outputs are empty and may be NULL)
    PIPS_CHECK_ARG(cols && out_trajs && out_vis, "stream_emit_cols: null pointer");
    return launch_stream_emit_cols(trajs, vis, L, n, f0, f1, cols, m, out_trajs, out_vis, (hipStream_t)stream);
}
int pips_stream_keep(int n, const int* keep, int m, const int* tq, const float* xy, const int* cur, const int* status, const int* clip,
                     const float* feat, const float* trajs, const float* vis, int L, int* tq_out, float* xy_out, int* cur_out,
                     int* status_out, int* clip_out, float* feat_out, float* trajs_out, float* vis_out, int V, int* counts,
                     void* stream) {
    PIPS_CHECK_ARG(n >= 1 && m >= 0 && m <= n, "stream_keep: need n >= 1 and 0 <= m <= n (n=%d, m=%d)", n, m);
    PIPS_CHECK_ARG(L >= 2 * PIPS_S, "stream_keep: a row ring needs L >= %d rows (L=%d)", 2 * PIPS_S, L);
    PIPS_CHECK_ARG(tq && xy && cur && status && feat && trajs && vis && counts, "stream_keep: null pointer");
    if (clip != nullptr) PIPS_CHECK_ARG(V >= 1 && V <= STREAM_V_MAX, "stream_keep: need 1 <= V <= %d streams (V=%d)", STREAM_V_MAX, V);
    if (m > 0) {                      // (m == 0: counts alone is written; keep and the empty outputs are not looked at)
        PIPS_CHECK_ARG(keep && tq_out && xy_out && cur_out && status_out && feat_out && trajs_out && vis_out, "stream_keep: null pointer");
        PIPS_CHECK_ARG((clip != nullptr) == (clip_out != nullptr), "stream_keep: clip and clip_out go together");
    }
    const StreamState in = {tq, xy, cur, status, clip, feat, trajs, vis};
    const StreamStateOut out = {tq_out, xy_out, cur_out, status_out, clip_out, feat_out, trajs_out, vis_out};
    return launch_stream_keep(n, keep, m, in, out, L, clip != nullptr ? V : 0, counts, (hipStream_t)stream);
}

// ---- the cover step
size_t pips_cover_workspace_bytes(int n, int gh, int gw) {
    if (n < 0 || gh < 1 || gw < 1 || (long long)gh * gw > PIPS_COVER_CELLS_MAX) return 0;
    return cover_workspace_ints(n, gh, gw) * sizeof(int);
}
int pips_cover_step(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy, const int* lost,
                    int H, int W, int cell, float vis_logit, int lost_after, int max_queries, int* keep, int* lost_out,
                    float* seeds, int* counts, void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(n >= 0 && m >= 0, "cover_step: need n >= 0 and m >= 0 (n=%d, m=%d)", n, m);
    PIPS_CHECK_ARG(cell >= 8 && H >= 1 && W >= 1, "cover_step: need cell >= 8 and a frame of at least 1x1 (cell=%d, H=%d, W=%d)", cell, H, W);
    PIPS_CHECK_ARG(lost_after >= 1 && max_queries >= 0, "cover_step: need lost_after >= 1 and max_queries >= 0 (%d, %d)", lost_after,
                   max_queries);
    PIPS_CHECK_ARG(m == 0 ? f1 == 0 : f1 >= m, "cover_step: rows of frames [f1 - m, f1) need f1 >= m, and a step without rows is the first (m=%d, f1=%d)", m, f1);
    const int gh = (H - 1) / cell + 1, gw = (W - 1) / cell + 1;
    PIPS_CHECK_ARG((long long)gh * gw <= PIPS_COVER_CELLS_MAX, "cover_step: a grid of %d x %d cells has more than %d", gh, gw,
                   PIPS_COVER_CELLS_MAX);
    PIPS_CHECK_ARG(seeds && counts && workspace, "cover_step: null pointer");
    if (n > 0) {
        PIPS_CHECK_ARG(tq && xy && lost && keep && lost_out, "cover_step: null pointer");
        if (m > 0) PIPS_CHECK_ARG(trajs && vis, "cover_step: null pointer");
    }
    const size_t need = cover_workspace_ints(n, gh, gw) * sizeof(int);
    if (workspace_bytes < need) {
        set_error("cover_step: workspace %zu < %zu bytes", workspace_bytes, need);
        return PIPS_E_WORKSPACE;
    }
    return launch_cover_step(n, m, f1, trajs, vis, tq, xy, lost, H, W, cell, gh, gw, vis_logit, lost_after, max_queries, keep, lost_out,
                             seeds, counts, (int*)workspace, (hipStream_t)stream);
}
size_t pips_cover_thin_workspace_bytes(int n, int m, int gh, int gw) {
    if (n < 0 || m < 0 || gh < 1 || gw < 1 || (long long)gh * gw > PIPS_COVER_CELLS_MAX) return 0;
    return cover_thin_workspace_ints(n, m, gh, gw) * sizeof(int);
}
int pips_cover_step_thin(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy, const int* lost,
                         const int* crowd, int H, int W, int cell, float vis_logit, int lost_after, int max_queries, int per_cell,
                         int crowd_after, int* keep, int* lost_out, int* crowd_out, float* seeds, int* gone, int* reason, int* counts,
                         void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(n >= 0 && m >= 0, "cover_step_thin: need n >= 0 and m >= 0 (n=%d, m=%d)", n, m);
    PIPS_CHECK_ARG(cell >= 8 && H >= 1 && W >= 1, "cover_step_thin: need cell >= 8 and a frame of at least 1x1 (cell=%d, H=%d, W=%d)", cell, H, W);
    PIPS_CHECK_ARG(lost_after >= 1 && max_queries >= 0, "cover_step_thin: need lost_after >= 1 and max_queries >= 0 (%d, %d)", lost_after,
                   max_queries);
    PIPS_CHECK_ARG(per_cell >= 1 && crowd_after >= 1, "cover_step_thin: need per_cell >= 1 and crowd_after >= 1 (%d, %d)", per_cell,
                   crowd_after);
    PIPS_CHECK_ARG(m == 0 ? f1 == 0 : f1 >= m, "cover_step_thin: rows of frames [f1 - m, f1) need f1 >= m, and a step without rows is the first (m=%d, f1=%d)", m, f1);
    const int gh = (H - 1) / cell + 1, gw = (W - 1) / cell + 1;
    PIPS_CHECK_ARG((long long)gh * gw <= PIPS_COVER_CELLS_MAX, "cover_step_thin: a grid of %d x %d cells has more than %d", gh, gw,
                   PIPS_COVER_CELLS_MAX);
    PIPS_CHECK_ARG(seeds && counts && workspace, "cover_step_thin: null pointer");
    if (n > 0) {
        PIPS_CHECK_ARG(tq && xy && lost && crowd && keep && lost_out && crowd_out && gone && reason, "cover_step_thin: null pointer");
        if (m > 0) PIPS_CHECK_ARG(trajs && vis, "cover_step_thin: null pointer");
    }
    const size_t need = cover_thin_workspace_ints(n, m, gh, gw) * sizeof(int);
    if (workspace_bytes < need) {
        set_error("cover_step_thin: workspace %zu < %zu bytes", workspace_bytes, need);
        return PIPS_E_WORKSPACE;
    }
    return launch_cover_step_thin(n, m, f1, trajs, vis, tq, xy, lost, crowd, H, W, cell, gh, gw, vis_logit, lost_after, max_queries,
                                  per_cell, crowd_after, keep, lost_out, crowd_out, seeds, gone, reason, counts, (int*)workspace,
                                  (hipStream_t)stream);
}

// ---- seeding on corners
int pips_corner_table(const void* frames, int src_is_u8, int F, int h, int w, int cell, float* table, void* stream) {
    PIPS_CHECK_ARG(F >= 0, "corner_table: need F >= 0 (F=%d)", F);
    PIPS_CHECK_ARG(cell >= 8 && h >= 1 && w >= 1, "corner_table: need cell >= 8 and a frame of at least 1x1 (cell=%d, h=%d, w=%d)", cell, h, w);
    PIPS_CHECK_ARG((long long)h * w <= INT_MAX, "corner_table: a frame of %d x %d has more than %d pixels", h, w, INT_MAX);
    const int gh = (h - 1) / cell + 1, gw = (w - 1) / cell + 1;
    PIPS_CHECK_ARG((long long)F * gh * gw <= PIPS_CORNER_BLOCKS_MAX, "corner_table: %d frames of %d x %d cells are more than %d blocks", F, gh, gw,
                   PIPS_CORNER_BLOCKS_MAX);
    PIPS_CHECK_ARG(frames && table, "corner_table: null pointer");
    if (F == 0) return PIPS_OK;
    return launch_corner_table(frames, src_is_u8 != 0, F, h, w, cell, gh, gw, table, (hipStream_t)stream);
}
int pips_cover_place(float* seeds, int k, const float* table_of_frame, int h, int w, int cell, int min_corner, void* stream) {
    PIPS_CHECK_ARG(k >= 0, "cover_place: need k >= 0 (k=%d)", k);
    PIPS_CHECK_ARG(cell >= 8 && h >= 1 && w >= 1, "cover_place: need cell >= 8 and a frame of at least 1x1 (cell=%d, h=%d, w=%d)", cell, h, w);
    PIPS_CHECK_ARG(min_corner >= 0, "cover_place: need min_corner >= 0 (min_corner=%d)", min_corner);
    PIPS_CHECK_ARG(seeds && table_of_frame, "cover_place: null pointer");
    if (k == 0) return PIPS_OK;
    return launch_cover_place(seeds, k, table_of_frame, (h - 1) / cell + 1, (w - 1) / cell + 1, cell, min_corner, (hipStream_t)stream);
}

// ---- scene cuts
size_t pips_cut_workspace_bytes(int F, int h, int w) {
    if (F < 0 || F > PIPS_CUT_FRAMES_MAX || h < 1 || w < 1 || (long long)h * w > (1ll << 30)) return 0;
    return (size_t)F * 4 * cut_strips(h) * 128 * sizeof(int);
}
int pips_cut_table(const void* frames, int src_is_u8, int F, int h, int w, const int32_t* prev_hist, int32_t* hist, int32_t* dist,
                   void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(F >= 0 && F <= PIPS_CUT_FRAMES_MAX, "cut_table: need 0 <= F <= %d (F=%d)", PIPS_CUT_FRAMES_MAX, F);
    PIPS_CHECK_ARG(h >= 1 && w >= 1, "cut_table: need a frame of at least 1x1 (h=%d, w=%d)", h, w);
    PIPS_CHECK_ARG((long long)h * w <= (1ll << 30), "cut_table: a frame of %d x %d has more than 2^30 pixels", h, w);
    if (F == 0) return PIPS_OK;
    PIPS_CHECK_ARG(frames && hist && dist && workspace, "cut_table: null pointer");
    const size_t need = pips_cut_workspace_bytes(F, h, w);
    if (workspace_bytes < need) {
        set_error("cut_table: workspace %zu < %zu bytes", workspace_bytes, need);
        return PIPS_E_WORKSPACE;
    }
    return launch_cut_table(frames, src_is_u8 != 0, F, h, w, prev_hist, hist, dist, (int*)workspace, (hipStream_t)stream);
}

// ---- decoder frames in
int pips_frames_import_ex(int format, int matrix, int range, int filter, int F, int h, int w, const void* p0, size_t pitch0,
                          size_t step0, const void* p1, size_t pitch1, size_t step1, const void* p2, size_t pitch2, size_t step2,
                          void* dst, int dst_is_u8, int H, int W, void* stream) {
    PIPS_CHECK_ARG(format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I010, "frames_import: unknown format %d", format);
    PIPS_CHECK_ARG(filter == PIPS_FILTER_BILINEAR || filter == PIPS_FILTER_TRIANGLE, "frames_import: unknown filter %d", filter);
    const bool wide = format == PIPS_FMT_P010 || format == PIPS_FMT_I010;                   // 16-bit samples
    const bool semi = format == PIPS_FMT_NV12 || format == PIPS_FMT_P010;
    const bool yuv = semi || format == PIPS_FMT_I420 || format == PIPS_FMT_I010;
    PIPS_CHECK_ARG(!yuv || ((matrix == PIPS_MATRIX_BT601 || matrix == PIPS_MATRIX_BT709) &&
                            (range == PIPS_RANGE_LIMITED || range == PIPS_RANGE_FULL)),
                   "frames_import: unknown matrix %d or range %d", matrix, range);
    PIPS_CHECK_ARG(F >= 0, "frames_import: need F >= 0 (F=%d)", F);
    PIPS_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1, "frames_import: need frames of at least 1x1 (h=%d, w=%d, H=%d, W=%d)", h, w, H, W);
    PIPS_CHECK_ARG((long long)F * H * W <= PIPS_IMPORT_PIXELS_MAX, "frames_import: %d frames of %d x %d are more than 2^30 output pixels",
                   F, H, W);
    if (filter == PIPS_FILTER_TRIANGLE && (H != h || W != w)) {
        // the triangle filter's accumulators: a weight sum below 2^19, a row sum in int32, 512 num in int64
        PIPS_CHECK_ARG(h <= PIPS_FILTER_DIM_MAX && w <= PIPS_FILTER_DIM_MAX && H <= PIPS_FILTER_DIM_MAX && W <= PIPS_FILTER_DIM_MAX,
                       "frames_import: the triangle filter takes sizes up to %d (h=%d, w=%d, H=%d, W=%d)", PIPS_FILTER_DIM_MAX, h, w, H, W);
        PIPS_CHECK_ARG((long long)h <= 16ll * H && (long long)w <= 16ll * W,
                       "frames_import: the triangle filter scales down by at most 16 (%d x %d to %d x %d)", h, w, H, W);
    }
    // plane k of the format: its rows and the bytes of a row
    const void* p[3] = {p0, p1, p2};
    const size_t pitch[3] = {pitch0, pitch1, pitch2}, step[3] = {step0, step1, step2};
    const size_t ch = ((size_t)h + 1) / 2, cw = ((size_t)w + 1) / 2, sb = wide ? 2 : 1;
    const int planes = semi ? 2 : yuv ? 3 : 1;
    const size_t bpp = (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? 4 : yuv ? sb : 3;
    const size_t rows[3] = {(size_t)h, ch, ch};
    const size_t row_bytes[3] = {(size_t)w * bpp, (semi ? 2 * cw : cw) * sb, cw * sb};
    for (int k = 0; k < planes; ++k) {
        PIPS_CHECK_ARG(pitch[k] >= row_bytes[k], "frames_import: pitch %zu of plane %d is below the %zu bytes of a row", pitch[k], k,
                       row_bytes[k]);
        PIPS_CHECK_ARG(F <= 1 || (step[k] >= pitch[k] && step[k] / pitch[k] >= rows[k]),
                       "frames_import: step %zu of plane %d is below pitch %zu x %zu rows", step[k], k, pitch[k], rows[k]);
        PIPS_CHECK_ARG(!wide || (((uintptr_t)p[k] | pitch[k] | step[k]) & 1) == 0,
                       "frames_import: plane %d of a 16-bit format needs an even pointer, pitch and step (pitch %zu, step %zu)", k,
                       pitch[k], step[k]);
    }
    if (F == 0) return PIPS_OK;
    PIPS_CHECK_ARG(dst != nullptr, "frames_import: null dst");
    for (int k = 0; k < planes; ++k) PIPS_CHECK_ARG(p[k] != nullptr, "frames_import: null plane %d", k);
    return launch_frames_import(format, matrix, range, filter, F, h, w, p, pitch, step, dst, dst_is_u8 != 0, H, W, (hipStream_t)stream);
}

int pips_frames_import(int format, int matrix, int range, int F, int h, int w, const void* p0, size_t pitch0, size_t step0,
                       const void* p1, size_t pitch1, size_t step1, const void* p2, size_t pitch2, size_t step2, void* dst,
                       int dst_is_u8, int H, int W, void* stream) {
    PIPS_CHECK_ARG(format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I420, "frames_import: unknown format %d", format);
    return pips_frames_import_ex(format, matrix, range, PIPS_FILTER_BILINEAR, F, h, w, p0, pitch0, step0, p1, pitch1, step1, p2, pitch2,
                                 step2, dst, dst_is_u8, H, W, stream);
}

// ---- tracks out
size_t pips_draw_workspace_bytes(int F, int n, int trail) {
    if (F < 0 || n < 0 || trail < 0 || trail > PIPS_DRAW_TRAIL_MAX) return 0;
    return (size_t)F * (size_t)n * draw_track_ints(trail) * sizeof(int);
}
// pips_tracks_draw (ex = false, fade = NULL) and pips_tracks_draw_ex: one list of checks, `who` in front of every message
static int tracks_draw_any(const char* who, bool ex, int format, int matrix, int range, int F, int h, int w, void* p0, size_t pitch0,
                           size_t step0, void* p1, size_t pitch1, size_t step1, void* p2, size_t pitch2, size_t step2,
                           const float* trajs, const float* vis, int G, int n, int first, int src_h, int src_w, const uint8_t* colors,
                           int trail, int line8, int dot8, int alpha_vis, int alpha_occ, float vis_logit, const int* fade,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const bool wide = format == PIPS_FMT_P010 || format == PIPS_FMT_I010;                   // 16-bit samples
    if (ex)
        PIPS_CHECK_ARG((format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I010) || format == PIPS_FMT_PLANAR8, "%s: unknown format %d", who,
                       format);
    else
        PIPS_CHECK_ARG((format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I420) || format == PIPS_FMT_PLANAR8,
                       "%s: format %d is not an 8-bit surface (pips_tracks_draw_ex draws on the 10-bit formats)", who, format);
    const bool semi = format == PIPS_FMT_NV12 || format == PIPS_FMT_P010;
    const bool yuv = semi || format == PIPS_FMT_I420 || format == PIPS_FMT_I010;
    PIPS_CHECK_ARG(!yuv || ((matrix == PIPS_MATRIX_BT601 || matrix == PIPS_MATRIX_BT709) &&
                            (range == PIPS_RANGE_LIMITED || range == PIPS_RANGE_FULL)),
                   "%s: unknown matrix %d or range %d", who, matrix, range);
    PIPS_CHECK_ARG(F >= 0 && n >= 0, "%s: need F >= 0 and n >= 0 (F=%d, n=%d)", who, F, n);
    PIPS_CHECK_ARG(h >= 1 && w >= 1 && src_h >= 1 && src_w >= 1, "%s: need sizes of at least 1x1 (h=%d, w=%d, src_h=%d, src_w=%d)", who,
                   h, w, src_h, src_w);
    PIPS_CHECK_ARG(h <= PIPS_DRAW_DIM_MAX && w <= PIPS_DRAW_DIM_MAX, "%s: surfaces up to %d a side (h=%d, w=%d)", who,
                   PIPS_DRAW_DIM_MAX, h, w);
    PIPS_CHECK_ARG(trail >= 0 && trail <= PIPS_DRAW_TRAIL_MAX, "%s: trail=%d outside 0..%d", who, trail, PIPS_DRAW_TRAIL_MAX);
    PIPS_CHECK_ARG(line8 <= PIPS_DRAW_RADIUS8_MAX && dot8 <= PIPS_DRAW_RADIUS8_MAX, "%s: a radius above %d eighths (line8=%d, dot8=%d)",
                   who, PIPS_DRAW_RADIUS8_MAX, line8, dot8);
    PIPS_CHECK_ARG(alpha_vis >= 0 && alpha_vis <= 256 && alpha_occ >= 0 && alpha_occ <= 256,
                   "%s: alphas outside 0..256 (alpha_vis=%d, alpha_occ=%d)", who, alpha_vis, alpha_occ);
    PIPS_CHECK_ARG(first >= 0 && (long long)first + F <= (long long)G, "%s: rows [%d, %d + %d) of %d", who, first, first, F, G);
    if (fade != nullptr)                                                                    // (a host array: read here, passed by value)
        for (int a = 0; a < trail; ++a) PIPS_CHECK_ARG(fade[a] >= 0 && fade[a] <= 256, "%s: fade[%d]=%d outside 0..256", who, a, fade[a]);
    // plane k of the format: its rows and the bytes of a row
    void* p[3] = {p0, p1, p2};
    const size_t pitch[3] = {pitch0, pitch1, pitch2}, step[3] = {step0, step1, step2};
    const size_t ch = ((size_t)h + 1) / 2, cw = ((size_t)w + 1) / 2, sb = wide ? 2 : 1;
    const bool planar = format == PIPS_FMT_PLANAR8;
    const int planes = semi ? 2 : (yuv || planar) ? 3 : 1;
    const size_t bpp = (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? 4 : (yuv || planar) ? sb : 3;
    const size_t rows[3] = {(size_t)h, planar ? (size_t)h : ch, planar ? (size_t)h : ch};
    const size_t row_bytes[3] = {(size_t)w * bpp, planar ? (size_t)w : (semi ? 2 * cw : cw) * sb, planar ? (size_t)w : cw * sb};
    for (int k = 0; k < planes; ++k) {
        PIPS_CHECK_ARG(pitch[k] >= row_bytes[k], "%s: pitch %zu of plane %d is below the %zu bytes of a row", who, pitch[k], k,
                       row_bytes[k]);
        PIPS_CHECK_ARG(F <= 1 || (step[k] >= pitch[k] && step[k] / pitch[k] >= rows[k]),
                       "%s: step %zu of plane %d is below pitch %zu x %zu rows", who, step[k], k, pitch[k], rows[k]);
        PIPS_CHECK_ARG(!wide || (((uintptr_t)p[k] | pitch[k] | step[k]) & 1) == 0,
                       "%s: plane %d of a 16-bit format needs an even pointer, pitch and step (pitch %zu, step %zu)", who, k, pitch[k],
                       step[k]);
    }
    if (F == 0 || n == 0) return PIPS_OK;
    for (int k = 0; k < planes; ++k) PIPS_CHECK_ARG(p[k] != nullptr, "%s: null plane %d", who, k);
    PIPS_CHECK_ARG(trajs && colors && workspace, "%s: null trajs, colors or workspace", who);
    const size_t need = pips_draw_workspace_bytes(F, n, trail);
    PIPS_CHECK_ARG(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    PIPS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: the workspace must lie on a 16-byte address", who);
    const DrawStyle style{trail, line8, dot8, alpha_vis, alpha_occ, vis_logit};
    return launch_tracks_draw(format, matrix, range, F, h, w, p, pitch, step, trajs, vis, n, first, src_h, src_w, colors, style, fade,
                              (int*)workspace, (hipStream_t)stream);
}
int pips_tracks_draw(int format, int matrix, int range, int F, int h, int w, void* p0, size_t pitch0, size_t step0, void* p1,
                     size_t pitch1, size_t step1, void* p2, size_t pitch2, size_t step2, const float* trajs, const float* vis, int G,
                     int n, int first, int src_h, int src_w, const uint8_t* colors, int trail, int line8, int dot8, int alpha_vis,
                     int alpha_occ, float vis_logit, void* workspace, size_t workspace_bytes, void* stream) {
    return tracks_draw_any("tracks_draw", false, format, matrix, range, F, h, w, p0, pitch0, step0, p1, pitch1, step1, p2, pitch2, step2,
                           trajs, vis, G, n, first, src_h, src_w, colors, trail, line8, dot8, alpha_vis, alpha_occ, vis_logit, nullptr,
                           workspace, workspace_bytes, stream);
}
int pips_tracks_draw_ex(int format, int matrix, int range, int F, int h, int w, void* p0, size_t pitch0, size_t step0, void* p1,
                        size_t pitch1, size_t step1, void* p2, size_t pitch2, size_t step2, const float* trajs, const float* vis, int G,
                        int n, int first, int src_h, int src_w, const uint8_t* colors, int trail, int line8, int dot8, int alpha_vis,
                        int alpha_occ, float vis_logit, const int* fade, void* workspace, size_t workspace_bytes, void* stream) {
    return tracks_draw_any("tracks_draw_ex", true, format, matrix, range, F, h, w, p0, pitch0, step0, p1, pitch1, step1, p2, pitch2, step2,
                           trajs, vis, G, n, first, src_h, src_w, colors, trail, line8, dot8, alpha_vis, alpha_occ, vis_logit, fade,
                           workspace, workspace_bytes, stream);
}

// ---- object masks
size_t pips_object_masks_workspace_bytes(int F, int n) {
    if (F < 0 || n < 0 || n > PIPS_MASK_N_MAX) return 0;
    return (size_t)F * (size_t)n * MASK_REC_BYTES;
}
int pips_object_masks(const float* trajs, const uint8_t* labels, int G, int n, int first, int F, int src_h, int src_w, int h, int w,
                      int radius8, int vote, uint8_t* mask, size_t pitch, size_t step, void* workspace, size_t workspace_bytes,
                      void* stream) {
    PIPS_CHECK_ARG(F >= 0 && n >= 0 && G >= 0, "object_masks: need F >= 0, n >= 0 and G >= 0 (F=%d, n=%d, G=%d)", F, n, G);
    PIPS_CHECK_ARG(n <= PIPS_MASK_N_MAX, "object_masks: at most %d columns (n=%d): a key holds 16 bits of column", PIPS_MASK_N_MAX, n);
    PIPS_CHECK_ARG(h >= 1 && w >= 1 && src_h >= 1 && src_w >= 1,
                   "object_masks: need sizes of at least 1x1 (h=%d, w=%d, src_h=%d, src_w=%d)", h, w, src_h, src_w);
    PIPS_CHECK_ARG(h <= PIPS_DRAW_DIM_MAX && w <= PIPS_DRAW_DIM_MAX, "object_masks: masks up to %d a side (h=%d, w=%d)",
                   PIPS_DRAW_DIM_MAX, h, w);
    PIPS_CHECK_ARG(radius8 >= 0 && radius8 <= PIPS_MASK_RADIUS8_MAX, "object_masks: radius8=%d eighths outside 0..%d", radius8,
                   PIPS_MASK_RADIUS8_MAX);
    PIPS_CHECK_ARG(vote >= 1 && vote <= PIPS_MASK_VOTE_MAX, "object_masks: vote=%d outside 1..%d", vote, PIPS_MASK_VOTE_MAX);
    PIPS_CHECK_ARG(first >= 0 && (long long)first + F <= (long long)G, "object_masks: rows [%d, %d + %d) of %d", first, first, F, G);
    PIPS_CHECK_ARG(pitch >= (size_t)w, "object_masks: pitch %zu is below the %d bytes of a row", pitch, w);
    PIPS_CHECK_ARG(F <= 1 || (step >= pitch && step / pitch >= (size_t)h), "object_masks: step %zu is below pitch %zu x %d rows", step,
                   pitch, h);
    if (F == 0) return PIPS_OK;
    PIPS_CHECK_ARG(mask != nullptr, "object_masks: null mask");
    if (n > 0) {
        PIPS_CHECK_ARG(trajs && labels && workspace, "object_masks: null trajs, labels or workspace");
        const size_t need = pips_object_masks_workspace_bytes(F, n);
        PIPS_CHECK_ARG(workspace_bytes >= need, "object_masks: workspace %zu < %zu bytes", workspace_bytes, need);
        PIPS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "object_masks: the workspace must lie on a 16-byte address");
    }
    return launch_object_masks(trajs, labels, n, first, F, src_h, src_w, h, w, radius8, vote, mask, pitch, step, workspace,
                               (hipStream_t)stream);
}
int pips_masks_tint(int format, int matrix, int range, int F, int h, int w, void* p0, size_t pitch0, size_t step0, void* p1,
                    size_t pitch1, size_t step1, void* p2, size_t pitch2, size_t step2, const uint8_t* mask, size_t mask_pitch,
                    size_t mask_step, const uint8_t* colors, const int* alpha, int C, void* stream) {
    PIPS_CHECK_ARG((format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I420) || format == PIPS_FMT_PLANAR8,
                   "masks_tint: format %d is not one of the seven 8-bit surfaces", format);
    const bool semi = format == PIPS_FMT_NV12, yuv = semi || format == PIPS_FMT_I420, planar = format == PIPS_FMT_PLANAR8;
    PIPS_CHECK_ARG(!yuv || ((matrix == PIPS_MATRIX_BT601 || matrix == PIPS_MATRIX_BT709) &&
                            (range == PIPS_RANGE_LIMITED || range == PIPS_RANGE_FULL)),
                   "masks_tint: unknown matrix %d or range %d", matrix, range);
    PIPS_CHECK_ARG(F >= 0, "masks_tint: need F >= 0 (F=%d)", F);
    PIPS_CHECK_ARG(h >= 1 && w >= 1, "masks_tint: need a size of at least 1x1 (h=%d, w=%d)", h, w);
    PIPS_CHECK_ARG(h <= PIPS_DRAW_DIM_MAX && w <= PIPS_DRAW_DIM_MAX, "masks_tint: surfaces up to %d a side (h=%d, w=%d)",
                   PIPS_DRAW_DIM_MAX, h, w);
    PIPS_CHECK_ARG(C >= 1 && C <= PIPS_MASK_LABELS_MAX, "masks_tint: C=%d labels outside 1..%d", C, PIPS_MASK_LABELS_MAX);
    // plane k of the format: its rows and the bytes of a row (pips_tracks_draw's geometry)
    void* p[3] = {p0, p1, p2};
    const size_t pitch[3] = {pitch0, pitch1, pitch2}, step[3] = {step0, step1, step2};
    const size_t ch = ((size_t)h + 1) / 2, cw = ((size_t)w + 1) / 2;
    const int planes = semi ? 2 : (yuv || planar) ? 3 : 1;
    const size_t bpp = (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? 4 : (yuv || planar) ? 1 : 3;
    const size_t rows[3] = {(size_t)h, planar ? (size_t)h : ch, planar ? (size_t)h : ch};
    const size_t row_bytes[3] = {(size_t)w * bpp, planar ? (size_t)w : (semi ? 2 * cw : cw), planar ? (size_t)w : cw};
    for (int k = 0; k < planes; ++k) {
        PIPS_CHECK_ARG(pitch[k] >= row_bytes[k], "masks_tint: pitch %zu of plane %d is below the %zu bytes of a row", pitch[k], k,
                       row_bytes[k]);
        PIPS_CHECK_ARG(F <= 1 || (step[k] >= pitch[k] && step[k] / pitch[k] >= rows[k]),
                       "masks_tint: step %zu of plane %d is below pitch %zu x %zu rows", step[k], k, pitch[k], rows[k]);
    }
    PIPS_CHECK_ARG(mask_pitch >= (size_t)w, "masks_tint: mask pitch %zu is below the %d bytes of a row", mask_pitch, w);
    PIPS_CHECK_ARG(F <= 1 || (mask_step >= mask_pitch && mask_step / mask_pitch >= (size_t)h),
                   "masks_tint: mask step %zu is below pitch %zu x %d rows", mask_step, mask_pitch, h);
    if (F == 0) return PIPS_OK;
    for (int k = 0; k < planes; ++k) PIPS_CHECK_ARG(p[k] != nullptr, "masks_tint: null plane %d", k);
    PIPS_CHECK_ARG(mask && colors && alpha, "masks_tint: null mask, colors or alpha");
    for (size_t k = 0; k < (size_t)F * (size_t)C; ++k)                                      // (a host array: read here, passed by value)
        PIPS_CHECK_ARG(alpha[k] >= 0 && alpha[k] <= 256, "masks_tint: alpha[%zu][%zu]=%d outside 0..256", k / (size_t)C, k % (size_t)C,
                       alpha[k]);
    return launch_masks_tint(format, matrix, range, F, h, w, p, pitch, step, mask, mask_pitch, mask_step, colors, alpha, C,
                             (hipStream_t)stream);
}

// ---- object masks along the image's edges
size_t pips_object_masks_guided_workspace_bytes(int F, int n, int h, int w) {
    if (F < 0 || n < 0 || n > PIPS_MASK_N_MAX || h < 1 || w < 1 || h > PIPS_DRAW_DIM_MAX || w > PIPS_DRAW_DIM_MAX) return 0;
    if (F == 0 || n == 0) return 0;
    return guided_workspace_bytes(F, n, h, w);
}
int pips_object_masks_guided(const float* trajs, const uint8_t* labels, int G, int n, int first, int F, int src_h, int src_w, int h,
                             int w, int edge, int reach, const uint8_t* guide, size_t guide_pitch, size_t guide_step, uint8_t* mask,
                             size_t pitch, size_t step, void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(F >= 0 && n >= 0 && G >= 0, "object_masks_guided: need F >= 0, n >= 0 and G >= 0 (F=%d, n=%d, G=%d)", F, n, G);
    PIPS_CHECK_ARG(n <= PIPS_MASK_N_MAX, "object_masks_guided: at most %d columns (n=%d): a key holds 16 bits of column", PIPS_MASK_N_MAX,
                   n);
    PIPS_CHECK_ARG(h >= 1 && w >= 1 && src_h >= 1 && src_w >= 1,
                   "object_masks_guided: need sizes of at least 1x1 (h=%d, w=%d, src_h=%d, src_w=%d)", h, w, src_h, src_w);
    PIPS_CHECK_ARG(h <= PIPS_DRAW_DIM_MAX && w <= PIPS_DRAW_DIM_MAX, "object_masks_guided: masks up to %d a side (h=%d, w=%d)",
                   PIPS_DRAW_DIM_MAX, h, w);
    PIPS_CHECK_ARG(edge >= 0 && edge <= PIPS_MASK_EDGE_MAX, "object_masks_guided: edge=%d outside 0..%d", edge, PIPS_MASK_EDGE_MAX);
    PIPS_CHECK_ARG(reach >= 0 && reach <= PIPS_MASK_REACH_MAX, "object_masks_guided: reach=%d outside 0..%d", reach, PIPS_MASK_REACH_MAX);
    PIPS_CHECK_ARG(first >= 0 && (long long)first + F <= (long long)G, "object_masks_guided: rows [%d, %d + %d) of %d", first, first, F, G);
    PIPS_CHECK_ARG(pitch >= (size_t)w, "object_masks_guided: pitch %zu is below the %d bytes of a row", pitch, w);
    PIPS_CHECK_ARG(F <= 1 || (step >= pitch && step / pitch >= (size_t)h), "object_masks_guided: step %zu is below pitch %zu x %d rows",
                   step, pitch, h);
    if (F == 0) return PIPS_OK;
    PIPS_CHECK_ARG(mask != nullptr, "object_masks_guided: null mask");
    if (n > 0) {
        PIPS_CHECK_ARG(trajs && labels && workspace, "object_masks_guided: null trajs, labels or workspace");
        PIPS_CHECK_ARG(guide != nullptr, "object_masks_guided: null guide");
        PIPS_CHECK_ARG(guide_pitch >= (size_t)w, "object_masks_guided: guide pitch %zu is below the %d bytes of a row", guide_pitch, w);
        PIPS_CHECK_ARG(F <= 1 || (guide_step >= guide_pitch && guide_step / guide_pitch >= (size_t)h),
                       "object_masks_guided: guide step %zu is below pitch %zu x %d rows", guide_step, guide_pitch, h);
        const size_t need = pips_object_masks_guided_workspace_bytes(F, n, h, w);
        PIPS_CHECK_ARG(workspace_bytes >= need, "object_masks_guided: workspace %zu < %zu bytes", workspace_bytes, need);
        PIPS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "object_masks_guided: the workspace must lie on a 16-byte address");
    }
    return launch_object_masks_guided(trajs, labels, n, first, F, src_h, src_w, h, w, edge, reach, n > 0 ? guide : nullptr, guide_pitch,
                                      guide_step, mask, pitch, step, workspace, (hipStream_t)stream);
}
int pips_guide_plane(int format, int F, int h, int w, const void* p0, size_t pitch0, size_t step0, const void* p1, size_t pitch1,
                     size_t step1, const void* p2, size_t pitch2, size_t step2, uint8_t* guide, size_t guide_pitch, size_t guide_step,
                     void* stream) {
    PIPS_CHECK_ARG((format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_BGRA32) || format == PIPS_FMT_PLANAR8,
                   "guide_plane: format %d is not RGB24, BGR24, RGBA32, BGRA32 or PLANAR8 (the Y plane of NV12 and I420 is a guide as it is)",
                   format);
    PIPS_CHECK_ARG(F >= 0, "guide_plane: need F >= 0 (F=%d)", F);
    PIPS_CHECK_ARG(h >= 1 && w >= 1, "guide_plane: need a size of at least 1x1 (h=%d, w=%d)", h, w);
    PIPS_CHECK_ARG(h <= PIPS_DRAW_DIM_MAX && w <= PIPS_DRAW_DIM_MAX, "guide_plane: surfaces up to %d a side (h=%d, w=%d)",
                   PIPS_DRAW_DIM_MAX, h, w);
    const bool planar = format == PIPS_FMT_PLANAR8;
    const void* p[3] = {p0, p1, p2};
    const size_t pitch[3] = {pitch0, pitch1, pitch2}, step[3] = {step0, step1, step2};
    const int planes = planar ? 3 : 1;
    const size_t row_bytes = (size_t)w * (planar ? 1 : (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? 4 : 3);
    for (int k = 0; k < planes; ++k) {
        PIPS_CHECK_ARG(pitch[k] >= row_bytes, "guide_plane: pitch %zu of plane %d is below the %zu bytes of a row", pitch[k], k, row_bytes);
        PIPS_CHECK_ARG(F <= 1 || (step[k] >= pitch[k] && step[k] / pitch[k] >= (size_t)h),
                       "guide_plane: step %zu of plane %d is below pitch %zu x %d rows", step[k], k, pitch[k], h);
    }
    PIPS_CHECK_ARG(guide_pitch >= (size_t)w, "guide_plane: guide pitch %zu is below the %d bytes of a row", guide_pitch, w);
    PIPS_CHECK_ARG(F <= 1 || (guide_step >= guide_pitch && guide_step / guide_pitch >= (size_t)h),
                   "guide_plane: guide step %zu is below pitch %zu x %d rows", guide_step, guide_pitch, h);
    if (F == 0) return PIPS_OK;
    for (int k = 0; k < planes; ++k) PIPS_CHECK_ARG(p[k] != nullptr, "guide_plane: null plane %d", k);
    PIPS_CHECK_ARG(guide != nullptr, "guide_plane: null guide");
    return launch_guide_plane(format, F, h, w, p, pitch, step, guide, guide_pitch, guide_step, (hipStream_t)stream);
}

// ---- motion
static bool motion_shape_ok(int F, int n, int K) {
    return F >= 0 && F <= PIPS_MOTION_ROWS_MAX && n >= 0 && n <= PIPS_MOTION_N_MAX && K >= 1 && K <= PIPS_MOTION_HYPS_MAX;
}
size_t pips_motion_workspace_bytes(int F, int n, int K) {
    if (!motion_shape_ok(F, n, K) || F <= 1 || n == 0) return 0;
    return motion_workspace_bytes(F, n, K);
}
int pips_motion_fit(const float* trajs, const float* vis, int F, int n, int frame0, float vis_logit, int K, int thr4, int seed,
                    int32_t* head, int64_t* sums, double* model, uint8_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(F >= 0 && F <= PIPS_MOTION_ROWS_MAX, "motion_fit: need 0 <= F <= %d (F=%d)", PIPS_MOTION_ROWS_MAX, F);
    PIPS_CHECK_ARG(n >= 0 && n <= PIPS_MOTION_N_MAX, "motion_fit: need 0 <= n <= %d (n=%d): the sums are exact up to there",
                   PIPS_MOTION_N_MAX, n);
    PIPS_CHECK_ARG(K >= 1 && K <= PIPS_MOTION_HYPS_MAX, "motion_fit: K=%d hypotheses outside 1..%d", K, PIPS_MOTION_HYPS_MAX);
    PIPS_CHECK_ARG(thr4 >= 1 && thr4 <= PIPS_MOTION_THR4_MAX, "motion_fit: thr4=%d quarter pixels outside 1..%d", thr4,
                   PIPS_MOTION_THR4_MAX);
    PIPS_CHECK_ARG(frame0 >= 0 && frame0 <= INT_MAX - F, "motion_fit: frames [%d, %d + %d) do not fit an int", frame0, frame0, F);
    PIPS_CHECK_ARG(vis_logit == vis_logit, "motion_fit: vis_logit is a NaN");
    if (F <= 1) return PIPS_OK;
    PIPS_CHECK_ARG(head && sums && model, "motion_fit: null head, sums or model");
    if (n > 0) {
        PIPS_CHECK_ARG(trajs && flags && workspace, "motion_fit: null trajs, flags or workspace");
        PIPS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "motion_fit: the workspace must lie on a 16-byte address");
        const size_t need = pips_motion_workspace_bytes(F, n, K);
        if (workspace_bytes < need) {
            set_error("motion_fit: workspace %zu < %zu bytes", workspace_bytes, need);
            return PIPS_E_WORKSPACE;
        }
    }
    return launch_motion_fit(trajs, vis, F, n, frame0, vis_logit, K, thr4, (unsigned)seed, (int*)head, (long long*)sums, model,
                             (unsigned char*)flags, workspace, (hipStream_t)stream);
}
size_t pips_motion_layers_workspace_bytes(int F, int n, int K, int L) {
    if (!motion_shape_ok(F, n, K) || L < 1 || L > PIPS_MOTION_LAYERS_MAX || F <= 1 || n == 0) return 0;
    return motion_layers_workspace_bytes(F, n, K);
}
int pips_motion_layers(const float* trajs, const float* vis, const uint8_t* prev_layer, int F, int n, int frame0, float vis_logit, int K,
                       int thr4, int seed, int L, int min_in, int32_t* head, int64_t* sums, double* model, int32_t* box, uint8_t* layer,
                       int32_t* overlap, void* workspace, size_t workspace_bytes, void* stream) {
    PIPS_CHECK_ARG(F >= 0 && F <= PIPS_MOTION_ROWS_MAX, "motion_layers: need 0 <= F <= %d (F=%d)", PIPS_MOTION_ROWS_MAX, F);
    PIPS_CHECK_ARG(n >= 0 && n <= PIPS_MOTION_N_MAX, "motion_layers: need 0 <= n <= %d (n=%d): the sums are exact up to there",
                   PIPS_MOTION_N_MAX, n);
    PIPS_CHECK_ARG(K >= 1 && K <= PIPS_MOTION_HYPS_MAX, "motion_layers: K=%d hypotheses outside 1..%d", K, PIPS_MOTION_HYPS_MAX);
    PIPS_CHECK_ARG(thr4 >= 1 && thr4 <= PIPS_MOTION_THR4_MAX, "motion_layers: thr4=%d quarter pixels outside 1..%d", thr4,
                   PIPS_MOTION_THR4_MAX);
    PIPS_CHECK_ARG(frame0 >= 0 && frame0 <= INT_MAX - F, "motion_layers: frames [%d, %d + %d) do not fit an int", frame0, frame0, F);
    PIPS_CHECK_ARG(vis_logit == vis_logit, "motion_layers: vis_logit is a NaN");
    PIPS_CHECK_ARG(L >= 1 && L <= PIPS_MOTION_LAYERS_MAX, "motion_layers: L=%d layers outside 1..%d", L, PIPS_MOTION_LAYERS_MAX);
    PIPS_CHECK_ARG(min_in >= 2 && min_in <= PIPS_MOTION_N_MAX, "motion_layers: min_in=%d outside 2..%d", min_in, PIPS_MOTION_N_MAX);
    if (F <= 1) return PIPS_OK;
    PIPS_CHECK_ARG(head && sums && model && box && overlap, "motion_layers: null head, sums, model, box or overlap");
    if (n > 0) {
        PIPS_CHECK_ARG(trajs && layer && workspace, "motion_layers: null trajs, layer or workspace");
        PIPS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "motion_layers: the workspace must lie on a 16-byte address");
        // the first launch writes every row of layer before the last one reads prev_layer: they may not share a byte
        const uintptr_t lo = (uintptr_t)layer, hi = lo + ((size_t)F - 1) * (size_t)n, p0 = (uintptr_t)prev_layer;
        PIPS_CHECK_ARG(prev_layer == nullptr || p0 + (size_t)n <= lo || p0 >= hi,
                       "motion_layers: prev_layer lies inside the layer output of this call: copy the row first");
        const size_t need = pips_motion_layers_workspace_bytes(F, n, K, L);
        if (workspace_bytes < need) {
            set_error("motion_layers: workspace %zu < %zu bytes", workspace_bytes, need);
            return PIPS_E_WORKSPACE;
        }
    }
    return launch_motion_layers(trajs, vis, prev_layer, F, n, frame0, vis_logit, K, thr4, (unsigned)seed, L, min_in, (int*)head,
                                (long long*)sums, model, (int*)box, (unsigned char*)layer, (int*)overlap, workspace,
                                (hipStream_t)stream);
}

// ---- frames out, stabilised
namespace {

// plane k of a format of pips_frames_warp: its rows and the bytes of a row (pips_tracks_draw_ex's geometry)
struct WarpGeom {
    bool wide;                                                                          // 16-bit samples
    int planes;
    size_t rows[3], row_bytes[3];
};

// what pips_frames_warp and pips_frames_warp_fill check of their values alike; `fn` is the message prefix
int warp_check_values(const char* fn, int format, int matrix, int range, int border, int fill_rgb) {
    PIPS_CHECK_ARG((format >= PIPS_FMT_RGB24 && format <= PIPS_FMT_I010) || format == PIPS_FMT_PLANAR8, "%s: unknown format %d", fn,
                   format);
    PIPS_CHECK_ARG(border == PIPS_WARP_BORDER_CONSTANT || border == PIPS_WARP_BORDER_REPLICATE, "%s: unknown border %d", fn, border);
    const bool yuv = format == PIPS_FMT_NV12 || format == PIPS_FMT_P010 || format == PIPS_FMT_I420 || format == PIPS_FMT_I010;
    PIPS_CHECK_ARG(!yuv || ((matrix == PIPS_MATRIX_BT601 || matrix == PIPS_MATRIX_BT709) &&
                            (range == PIPS_RANGE_LIMITED || range == PIPS_RANGE_FULL)),
                   "%s: unknown matrix %d or range %d", fn, matrix, range);
    PIPS_CHECK_ARG(fill_rgb >= 0 && fill_rgb <= 0xFFFFFF, "%s: fill_rgb %d outside 0..0xFFFFFF", fn, fill_rgb);
    return PIPS_OK;
}

int warp_check_size(const char* fn, int format, int h, int w, WarpGeom& g) {
    PIPS_CHECK_ARG(h >= 1 && w >= 1, "%s: need a size of at least 1x1 (h=%d, w=%d)", fn, h, w);
    PIPS_CHECK_ARG(h <= PIPS_WARP_DIM_MAX && w <= PIPS_WARP_DIM_MAX, "%s: surfaces up to %d a side (h=%d, w=%d)", fn, PIPS_WARP_DIM_MAX, h,
                   w);
    g.wide = format == PIPS_FMT_P010 || format == PIPS_FMT_I010;
    const bool semi = format == PIPS_FMT_NV12 || format == PIPS_FMT_P010;
    const bool yuv = semi || format == PIPS_FMT_I420 || format == PIPS_FMT_I010;
    const size_t ch = ((size_t)h + 1) / 2, cw = ((size_t)w + 1) / 2, sb = g.wide ? 2 : 1;
    const bool planar = format == PIPS_FMT_PLANAR8;
    g.planes = semi ? 2 : (yuv || planar) ? 3 : 1;
    const size_t bpp = (format == PIPS_FMT_RGBA32 || format == PIPS_FMT_BGRA32) ? 4 : (yuv || planar) ? sb : 3;
    const size_t rows[3] = {(size_t)h, planar ? (size_t)h : ch, planar ? (size_t)h : ch};
    const size_t row_bytes[3] = {(size_t)w * bpp, planar ? (size_t)w : (semi ? 2 * cw : cw) * sb, planar ? (size_t)w : cw * sb};
    for (int k = 0; k < 3; ++k) g.rows[k] = rows[k], g.row_bytes[k] = row_bytes[k];
    return PIPS_OK;
}

// the pitches, steps and 16-bit alignment of the F surfaces `who` ("src" / "dst")
int warp_check_side(const char* fn, const char* who, const WarpGeom& g, int F, const void* const* p, const size_t* pitch,
                    const size_t* step) {
    for (int k = 0; k < g.planes; ++k) {
        PIPS_CHECK_ARG(pitch[k] >= g.row_bytes[k], "%s: pitch %zu of %s plane %d is below the %zu bytes of a row", fn, pitch[k], who, k,
                       g.row_bytes[k]);
        PIPS_CHECK_ARG(F <= 1 || (step[k] >= pitch[k] && step[k] / pitch[k] >= g.rows[k]),
                       "%s: step %zu of %s plane %d is below pitch %zu x %zu rows", fn, step[k], who, k, pitch[k], g.rows[k]);
        PIPS_CHECK_ARG(!g.wide || (((uintptr_t)p[k] | pitch[k] | step[k]) & 1) == 0,
                       "%s: %s plane %d of a 16-bit format needs an even pointer, pitch and step (pitch %zu, step %zu)", fn, who, k,
                       pitch[k], step[k]);
    }
    return PIPS_OK;
}

// the bytes of plane k of F >= 1 surfaces: [p, p + (F - 1) step + (rows - 1) pitch + the bytes of a row)
void warp_range(const WarpGeom& g, int k, int F, const void* p, size_t pitch, size_t step, uintptr_t& lo, uintptr_t& hi) {
    lo = (uintptr_t)p, hi = lo + ((size_t)F - 1) * step + (g.rows[k] - 1) * pitch + g.row_bytes[k];
}

}  // namespace

int pips_frames_warp(int format, int matrix, int range, int border, int fill_rgb, int F, int h, int w, const void* s0, size_t spitch0,
                     size_t sstep0, const void* s1, size_t spitch1, size_t sstep1, const void* s2, size_t spitch2, size_t sstep2, void* d0,
                     size_t dpitch0, size_t dstep0, void* d1, size_t dpitch1, size_t dstep1, void* d2, size_t dpitch2, size_t dstep2,
                     const int32_t* coef, void* stream) {
    const char* fn = "frames_warp";
    if (int e = warp_check_values(fn, format, matrix, range, border, fill_rgb)) return e;
    PIPS_CHECK_ARG(F >= 0, "frames_warp: need F >= 0 (F=%d)", F);
    WarpGeom g;
    if (int e = warp_check_size(fn, format, h, w, g)) return e;
    const void* sp[3] = {s0, s1, s2};
    void* dp[3] = {d0, d1, d2};
    const size_t spitch[3] = {spitch0, spitch1, spitch2}, sstep[3] = {sstep0, sstep1, sstep2};
    const size_t dpitch[3] = {dpitch0, dpitch1, dpitch2}, dstep[3] = {dstep0, dstep1, dstep2};
    if (int e = warp_check_side(fn, "src", g, F, sp, spitch, sstep)) return e;
    if (int e = warp_check_side(fn, "dst", g, F, dp, dpitch, dstep)) return e;
    if (F == 0) return PIPS_OK;
    for (int k = 0; k < g.planes; ++k) PIPS_CHECK_ARG(sp[k] != nullptr && dp[k] != nullptr, "frames_warp: null plane %d", k);
    PIPS_CHECK_ARG(coef != nullptr, "frames_warp: null coef");
    for (int i = 0; i < g.planes; ++i)
        for (int k = 0; k < g.planes; ++k) {
            uintptr_t a0, a1, b0, b1;
            warp_range(g, i, F, sp[i], spitch[i], sstep[i], a0, a1);
            warp_range(g, k, F, dp[k], dpitch[k], dstep[k], b0, b1);
            PIPS_CHECK_ARG(a1 <= b0 || b1 <= a0, "frames_warp: src plane %d and dst plane %d overlap", i, k);
        }
    return launch_frames_warp(format, matrix, range, border, fill_rgb, F, h, w, sp, spitch, sstep, dp, dpitch, dstep, (const int*)coef,
                              (hipStream_t)stream);
}

int pips_frames_warp_fill(int format, int matrix, int range, int border, int fill_rgb, int Fs, int Fd, int K, int h, int w, const void* s0,
                          size_t spitch0, size_t sstep0, const void* s1, size_t spitch1, size_t sstep1, const void* s2, size_t spitch2,
                          size_t sstep2, void* d0, size_t dpitch0, size_t dstep0, void* d1, size_t dpitch1, size_t dstep1, void* d2,
                          size_t dpitch2, size_t dstep2, const int32_t* cand, const int32_t* coef, uint8_t* source, size_t source_pitch,
                          size_t source_step, void* stream) {
    const char* fn = "frames_warp_fill";
    if (int e = warp_check_values(fn, format, matrix, range, border, fill_rgb)) return e;
    PIPS_CHECK_ARG(Fs >= 0 && Fd >= 0, "frames_warp_fill: need Fs >= 0 and Fd >= 0 (Fs=%d, Fd=%d)", Fs, Fd);
    PIPS_CHECK_ARG(K >= 1 && K <= PIPS_WARP_FILL_MAX, "frames_warp_fill: K=%d outside 1..%d", K, PIPS_WARP_FILL_MAX);
    WarpGeom g;
    if (int e = warp_check_size(fn, format, h, w, g)) return e;
    const void* sp[3] = {s0, s1, s2};
    void* dp[3] = {d0, d1, d2};
    const size_t spitch[3] = {spitch0, spitch1, spitch2}, sstep[3] = {sstep0, sstep1, sstep2};
    const size_t dpitch[3] = {dpitch0, dpitch1, dpitch2}, dstep[3] = {dstep0, dstep1, dstep2};
    if (int e = warp_check_side(fn, "src", g, Fs, sp, spitch, sstep)) return e;
    if (int e = warp_check_side(fn, "dst", g, Fd, dp, dpitch, dstep)) return e;
    if (source != nullptr) {
        PIPS_CHECK_ARG(source_pitch >= (size_t)w, "frames_warp_fill: source pitch %zu is below the %d bytes of a row", source_pitch, w);
        PIPS_CHECK_ARG(Fd <= 1 || (source_step >= source_pitch && source_step / source_pitch >= (size_t)h),
                       "frames_warp_fill: source step %zu is below pitch %zu x %d rows", source_step, source_pitch, h);
    }
    if (Fd == 0) return PIPS_OK;
    for (int k = 0; k < g.planes; ++k)
        PIPS_CHECK_ARG((Fs == 0 || sp[k] != nullptr) && dp[k] != nullptr, "frames_warp_fill: null plane %d", k);
    PIPS_CHECK_ARG(cand != nullptr && coef != nullptr, "frames_warp_fill: null cand or coef");
    const uintptr_t m0 = (uintptr_t)source, m1 = m0 + ((size_t)Fd - 1) * source_step + ((size_t)h - 1) * source_pitch + (size_t)w;
    for (int k = 0; k < g.planes; ++k) {
        uintptr_t b0, b1;
        warp_range(g, k, Fd, dp[k], dpitch[k], dstep[k], b0, b1);
        PIPS_CHECK_ARG(source == nullptr || m1 <= b0 || b1 <= m0, "frames_warp_fill: source and dst plane %d overlap", k);
        for (int i = 0; i < g.planes && Fs > 0; ++i) {
            uintptr_t a0, a1;
            warp_range(g, i, Fs, sp[i], spitch[i], sstep[i], a0, a1);
            PIPS_CHECK_ARG(a1 <= b0 || b1 <= a0, "frames_warp_fill: src plane %d and dst plane %d overlap", i, k);
            PIPS_CHECK_ARG(source == nullptr || m1 <= a0 || a1 <= m0, "frames_warp_fill: source and src plane %d overlap", i);
        }
    }
    return launch_frames_warp_fill(format, matrix, range, border, fill_rgb, Fs, Fd, K, h, w, sp, spitch, sstep, dp, dpitch, dstep,
                                   (const int*)cand, (const int*)coef, source, source_pitch, source_step, (hipStream_t)stream);
}

// ---- whole forward
size_t pips_workspace_bytes(int B, int S, int H, int W, int N, int stride) {
    if (B <= 0 || S < 1 || S > PIPS_S_MAX || H <= 0 || W <= 0 || N <= 0 || stride < 1) return 0;
    return plan_forward(B, S, H, W, N, stride).total * sizeof(float);
}

int pips_forward_ce(const void* arena, const float* rgbs, const float* xys, const float* coords_init,
                    const float* feat_init, const float* times, int B, int S, int H, int W, int N, int stride,
                    int iters, int flags, void* workspace, size_t workspace_bytes, float* out_trajs, float* out_vis,
                    float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes,
                    void* stream) {
    PIPS_CHECK_ARG(arena && xys && times && workspace && out_trajs && out_vis, "forward: null pointer");
    PIPS_CHECK_ARG((flags & PIPS_FLAG_REUSE_MAPS) || rgbs != nullptr, "forward: rgbs is null");
    PIPS_CHECK_ARG(S >= 1 && S <= PIPS_S_MAX, "forward: S=%d outside 1..%d (the arena must be packed for the same S, nets/pips.py:295-301)", S, PIPS_S_MAX);
    PIPS_CHECK_ARG(B > 0 && N > 0 && iters >= 0, "forward: need B,N >= 1 and iters >= 0");
    RUN(check_geometry(B * S, H, W, stride));
    RUN(check_sampled_map(H / stride, W / stride, "forward"));      // (ahead of the encoder pass: nothing is launched)
    const FwdPlan P = plan_forward(B, S, H, W, N, stride);
    if (workspace_bytes < P.total * sizeof(float)) {
        set_error("forward: workspace %zu < %zu bytes", workspace_bytes, P.total * sizeof(float));
        return PIPS_E_WORKSPACE;
    }
    float* ws = (float*)workspace;
    float* pyramid = ws + P.pyramid;
    if (!(flags & PIPS_FLAG_REUSE_MAPS))
        RUN(encoder_impl(arena, rgbs, B * S, H, W, stride, flags, pyramid, ws + P.enc, plan_encoder(B * S, H, W, stride).total * sizeof(float),
                         (hipStream_t)stream));
    // both bf16 modes on: the bf16 encoder wrote the mirror with the maps and the gather reads it (with REUSE_MAPS the flags
    // describe the call that produced the maps, so the same forward gives the same result with and without the encoder pass)
    if (!(flags & PIPS_FLAG_SPLIT_BF16) &&
        (flags & (PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_BF16_MIXER)) == (PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_BF16_MIXER) &&
        PIPS_TUNE("PIPS_BF16_MAPS", 1))
        flags |= PIPS_FLAG_BF16_MAPS;
    TrackCall c = track_call(arena, pyramid, B, S, H / stride, W / stride, xys, coords_init, feat_init, nullptr, times, N, stride, iters,
                             flags, ws + P.track, plan_track(B, N, S).total * sizeof(float), out_trajs, out_vis, out_ffeat0, stream);
    c.S = S;
    c.ce_tgt = ce_tgt; c.ce_terms = ce_terms; c.ce_ws = ce_ws; c.ce_ws_bytes = ce_ws_bytes;
    return track_impl(c);
}
int pips_forward(const void* arena, const float* rgbs, const float* xys, const float* coords_init,
                 const float* feat_init, const float* times, int B, int S, int H, int W, int N, int stride,
                 int iters, int flags, void* workspace, size_t workspace_bytes, float* out_trajs, float* out_vis,
                 float* out_ffeat0, void* stream) {
    return pips_forward_ce(arena, rgbs, xys, coords_init, feat_init, times, B, S, H, W, N, stride, iters, flags, workspace,
                           workspace_bytes, out_trajs, out_vis, out_ffeat0, nullptr, nullptr, nullptr, 0, stream);
}

}  // extern "C"
