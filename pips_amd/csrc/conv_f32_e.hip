// The fp32 encoder's convolutions outside conv_f32_t4.hip's reach -- the 128-channel layers at 1/8 and 1/16 resolution, the
// stride-2 entries of layers 2-4, the 1x1 shortcuts and the final 1x1 (nets/pips.py:169-181, 221-223) -- on shape E of
// gemm_f32_t4.hip with the addressing of an implicit GEMM: 64 x 64 tile (64 output pixels of one frame x 64 output channels), every
// wave the whole tile on one quarter of each 32-wide K stage, operands staged by LDS-DMA with per-lane global offsets into four
// buffers, the four partial tiles summed through LDS in the fixed order ((0 + 1) + 2) + 3, every wave finishing one 32 x 32 block:
// + bias, stores, InstanceNorm partials.  Exact fp32 products and fp32 accumulation (v_mfma_f32_32x32x2_f32), K tap-major like
// igemm_f32_kernel<..., CONV>, but in four interleaved chains: the map is NOT bitwise that kernel's (it is the closer one to fp64).
// The statistics come in igemm_f32_kernel's partition for 64-row tiles: one partial per 32-pixel block and channel.
// Bodies: conv_f32_e_asm.inc <- tools/conv_f32_e_gen.py (schedule, register map and edge handling are described there).
#include "common.h"
#include "f4_grid.h"
#ifndef PIPS_CF32E_INC
#define PIPS_CF32E_INC "conv_f32_e_asm.inc"
#endif
#include PIPS_CF32E_INC

namespace pips {

constexpr int CFE_LDS = 4 * 128 * 128;                       // four stage buffers; the four partial tiles at the end use the same 64 KiB

struct ConvEArgs {
    const float* in; const float* wgt; const float* bias; float* out; float* stats;
    int H, W, Wo, M, N, stride, pad, tiles_m, parts;
};

template <int CIN, int KS>
__global__ __launch_bounds__(256) void conv_f32_e_kernel(ConvEArgs p, F4Grid grid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int K = KS * KS * CIN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    int um, tn;                                               // row unit = (frame, row tile)
    f4_tile(grid, &um, &tn);
    const int f = um / p.tiles_m, tm = um - f * p.tiles_m;
    const int m0 = tm * 64, n0 = tn * 64;
    // staging: wave w fills LDS rows 32 w .. 32 w + 31 (waves 0, 1: the tile's pixels, waves 2, 3: its channels); DMA instruction k:
    // rows 8 k .. 8 k + 7 of them, lane = (row q = lane >> 3, chunk slot j = lane & 7) fetching chunk j ^ ((row >> 1) & 7).
    // Rows behind the last pixel / channel are clamped to it: they are never stored and never counted.
    const bool isA = wave < 2;
    const int row0 = 32 * (wave & 1), q = lane >> 3, j = lane & 7;
    unsigned vo[4], vflag = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = row0 + 8 * k + q, chunk = (j ^ ((r >> 1) & 7)) * 16;
        if (isA) {
            const int pix = min(m0 + r, p.M - 1), ho = pix / p.Wo, wo = pix - ho * p.Wo;
            const int hi = ho * p.stride - p.pad, wi = wo * p.stride - p.pad;      // tap (0, 0) of the pixel: may lie outside the image
            vo[k] = (unsigned)((hi * p.W + wi) * (CIN * 4) + chunk);
            if (KS == 3) vflag |= (wi < 0 ? 1u : 0u) << (2 * k) | (wi + 2 >= p.W ? 2u : 0u) << (2 * k);
        } else {
            vo[k] = (unsigned)(min(n0 + r, p.N - 1) * (K * 4) + chunk);
        }
    }
    const float* Xb = isA ? p.in + (size_t)f * p.H * p.W * CIN : p.wgt;
    const unsigned nrecX = isA ? (unsigned)(p.H * p.W) * (CIN * 4) : (unsigned)p.N * (K * 4);
    const unsigned tapH = isA ? (unsigned)p.W * (CIN * 4) : (unsigned)(KS * CIN * 4), tapW = CIN * 4;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned ldsw = lds0 + 32 * wave * 128;
    // fragments: lane = row l31 of a 32-row block, this wave's 8 K values of the stage = chunks 2 wave, 2 wave + 1 (lane half)
    const unsigned rA0 = lds0 + l31 * 128 + (((2 * wave + half) ^ ((l31 >> 1) & 7)) * 16), rW0 = rA0 + 64 * 128;
    const unsigned redW = lds0 + wave * 16384 + lane * 16, redR = lds0 + wave * 4096 + lane * 16;
    // the wave's block: pixels m0 + 32 bi .., channels n0 + 32 bj ..; lane = channel col, register r = pixel (r & 3) + 8 (r >> 2) + 4 half
    const int bi = wave & 1, bj = wave >> 1, rowb = m0 + 32 * bi, col = n0 + 32 * bj + l31;
    const bool col_ok = col < p.N;
    const int left = p.M - rowb, nv = left < 0 ? 0 : (left > 32 ? 32 : left);
    const float* Cb = p.out + ((size_t)f * p.M + rowb) * p.N;
    const float* Sb = p.stats != nullptr ? p.stats + (size_t)f * p.parts * p.N * 4 : nullptr;
    const unsigned nrecC = (unsigned)(left < 0 ? 0 : left) * ((unsigned)p.N * 4u), nrecB = (unsigned)p.N * 4u;
    const unsigned nrecS = p.stats != nullptr ? (unsigned)p.parts * ((unsigned)p.N * 16u) : 0u;
    const unsigned voC = col_ok ? (unsigned)((4 * half * p.N + col) * 4) : 0x80000000u, voB = (unsigned)(col * 4);
    const unsigned voS = (half || !col_ok) ? 0x80000000u : (unsigned)(((2 * tm + bi) * p.N + col) * 16);
    const unsigned vrow = (unsigned)(4 * half), vl31x4 = (unsigned)(l31 * 4), vswap = (unsigned)((lane ^ 32) * 4);
    const unsigned ldcb = (unsigned)p.N * 4u, nvf = __float_as_uint((float)nv);
#define CFE_OPERANDS                                                                                                                 \
    : [rA0] "v"(rA0), [rW0] "v"(rW0), [vo0] "v"(vo[0]), [vo1] "v"(vo[1]), [vo2] "v"(vo[2]), [vo3] "v"(vo[3]), [vflag] "v"(vflag),    \
      [voB] "v"(voB), [voC] "v"(voC), [voS] "v"(voS), [vrow] "v"(vrow), [vl31x4] "v"(vl31x4), [vswap] "v"(vswap),                    \
      [redW] "v"(redW), [redR] "v"(redR), [xlo] "s"(ASM_PTR_LO(Xb)), [xhi] "s"(ASM_PTR_HI(Xb)), [clo] "s"(ASM_PTR_LO(Cb)),           \
      [chi] "s"(ASM_PTR_HI(Cb)), [blo] "s"(ASM_PTR_LO(p.bias)), [bhi] "s"(ASM_PTR_HI(p.bias)), [slo] "s"(ASM_PTR_LO(Sb)),            \
      [shi] "s"(ASM_PTR_HI(Sb)), [nrecX] "s"(asm_sgpr(nrecX)), [nrecC] "s"(asm_sgpr(nrecC)), [nrecB] "s"(asm_sgpr(nrecB)),           \
      [nrecS] "s"(asm_sgpr(nrecS)), [tapH] "s"(asm_sgpr(tapH)), [tapW] "s"(asm_sgpr(tapW)), [ldsw] "s"(asm_sgpr(ldsw)),              \
      [ldcb] "s"(asm_sgpr(ldcb)), [nv] "s"(asm_sgpr((unsigned)nv)), [nvf] "s"(asm_sgpr(nvf))
    if (KS == 3) {
        if (CIN == 64)      asm volatile(PIPS_CF32E_C64_K3_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
        else if (CIN == 96) asm volatile(PIPS_CF32E_C96_K3_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
        else                asm volatile(PIPS_CF32E_C128_K3_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
    } else {
        if (CIN == 64)       asm volatile(PIPS_CF32E_C64_K1_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
        else if (CIN == 96)  asm volatile(PIPS_CF32E_C96_K1_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
        else if (CIN == 128) asm volatile(PIPS_CF32E_C128_K1_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
        else                 asm volatile(PIPS_CF32E_C256_K1_TEXT : CFE_OPERANDS : PIPS_CF32E_CLOBBER);
    }
#undef CFE_OPERANDS
}

// Can the body run this layer at all: 1x1 or 3x3, stride 1 or 2, pad k / 2, one of the generated channel counts, a bias, and every
// buffer offset below 2^31 (the out-of-range offset of the kernels)?
bool conv_f32_e_admits(const GemmArgs& a) {
    if (a.KH != a.KW || (a.KH != 1 && a.KH != 3) || (a.cstride != 1 && a.cstride != 2) || a.pad != a.KH / 2 || a.bias == nullptr) return false;
    if (a.KH == 3 ? (a.Cin != 64 && a.Cin != 96 && a.Cin != 128) : (a.Cin != 64 && a.Cin != 96 && a.Cin != 128 && a.Cin != 256)) return false;
    if (a.N % 32 != 0 || a.ldc != a.N || a.Ho != conv_out(a.H, a.KH, a.cstride, a.pad) || a.Wo != conv_out(a.Win, a.KW, a.cstride, a.pad)) return false;
    const unsigned long long lim = 1ull << 31;
    if ((unsigned long long)(a.H + 2) * (a.Win + 2) * a.Cin * 4ull >= lim || (unsigned long long)a.N * a.K * 4ull >= lim ||
        (unsigned long long)(a.M + 64) * a.N * 4ull >= lim || (unsigned long long)(2 * cdiv(a.M, 64)) * a.N * 16ull >= lim)
        return false;
    const int cap = a.stats_parts_cap > 0 ? a.stats_parts_cap : 2 * cdiv(a.M, 64) + 4;
    return a.stats == nullptr || 2 * cdiv(a.M, 64) <= cap;
}

template <int CIN, int KS>
static int launch_conv_f32_e_cfg(const GemmArgs& a, int frames, int* parts_out, hipStream_t st) {
    static std::atomic<unsigned long long> raised{0};
    const int rc = ensure_dynamic_lds(raised, (const void*)conv_f32_e_kernel<CIN, KS>, CFE_LDS);
    if (rc != PIPS_OK) return rc;
    ConvEArgs p;
    p.in = a.A; p.wgt = a.W; p.bias = a.bias; p.out = a.C; p.stats = a.stats;
    p.H = a.H; p.W = a.Win; p.Wo = a.Wo; p.M = a.M; p.N = a.N; p.stride = a.cstride; p.pad = a.pad;
    p.tiles_m = cdiv(a.M, 64); p.parts = 2 * p.tiles_m;
    const int tiles_n = cdiv(a.N, 64);
    // per XCD: its row tiles' input rows (a row tile reads about 64 s^2 pixels, its halo shared with the neighbours) and its column tiles of W
    const F4Grid grid = f4_grid(frames * p.tiles_m, tiles_n, (long)64 * a.cstride * a.cstride * CIN * 4, (long)64 * a.K * 4);
    hipLaunchKernelGGL((conv_f32_e_kernel<CIN, KS>), dim3(frames * p.tiles_m * tiles_n), dim3(256), CFE_LDS, st, p, grid);
    PIPS_CHECK_LAUNCH("conv_f32_e_kernel");
    if (parts_out) *parts_out = p.parts;
    return PIPS_OK;
}

int launch_conv_f32_e(const GemmArgs& a, int frames, int* parts_out, hipStream_t st) {
    if (a.KH == 3) {
        if (a.Cin == 64) return launch_conv_f32_e_cfg<64, 3>(a, frames, parts_out, st);
        if (a.Cin == 96) return launch_conv_f32_e_cfg<96, 3>(a, frames, parts_out, st);
        return launch_conv_f32_e_cfg<128, 3>(a, frames, parts_out, st);
    }
    if (a.Cin == 64) return launch_conv_f32_e_cfg<64, 1>(a, frames, parts_out, st);
    if (a.Cin == 96) return launch_conv_f32_e_cfg<96, 1>(a, frames, parts_out, st);
    if (a.Cin == 128) return launch_conv_f32_e_cfg<128, 1>(a, frames, parts_out, st);
    return launch_conv_f32_e_cfg<256, 1>(a, frames, parts_out, st);
}

}  // namespace pips
