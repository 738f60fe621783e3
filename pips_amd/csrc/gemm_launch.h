// Host-side launch code shared by the three register-staged matrix-product families (gemm.hip, gemm_x3.hip, gemm_bf16.hip).
// What differs between them -- grid, block, the LDS formula, the swizzle default and the kernel -- stays at their call sites.
#pragma once
#include "common.h"

namespace pips {

// The common tail of every tile launcher: raise the dynamic-LDS limit above 64 KiB (once per kernel instantiation and device:
// the flag is a static of this template, keyed on the kernel), launch, check.
template <auto Kern>
int launch_tiles(const char* name, dim3 grid, dim3 block, size_t lds, const GemmArgs& a, hipStream_t st) {
    if (lds > 64 * 1024) {
        static std::atomic<unsigned long long> raised{0};      // per instantiation, one bit per device
        const int rc = ensure_dynamic_lds(raised, (const void*)Kern, lds);
        if (rc != PIPS_OK) return rc;
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, st, a);
    PIPS_CHECK_LAUNCH(name);
    return PIPS_OK;
}

// XCD-aware tile order (common.h) as a *_SWZ hook of a tuning build asks for it: 0 off, 1 on wherever there are >= 64 tiles;
// -1 = the hook is unset and the family's own default holds.
inline int swizzle_forced(int force, long tiles) { return force < 0 ? -1 : (force != 0 && tiles >= 64); }

// Tile id forced by the *_TILE hooks of a tuning build: `all` for every plain GEMM, `up` / `down` only for N > K / N < K (the
// mixer's up- and down-projections, for in-situ A/B runs of tools/mixer_bench.py); -1 = none.
inline int forced_tile(int all, int up, int down, const GemmArgs& a) {
    if (all >= 0) return all;
    if (a.N > a.K && up >= 0) return up;
    if (a.N < a.K && down >= 0) return down;
    return -1;
}

// Operand checks of a plain GEMM; `who` prefixes the error text, lda_align is in elements of A.
inline int check_gemm_operands(const GemmArgs& a, const char* who, int lda_align) {
    PIPS_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "%s: empty problem", who);
    PIPS_CHECK_ARG(a.K % 32 == 0, "%s: K=%d must be a multiple of 32", who, a.K);
    PIPS_CHECK_ARG(a.lda % lda_align == 0, "%s: lda must be a multiple of %d elements", who, lda_align);
    PIPS_CHECK_ARG((unsigned long long)a.M * (unsigned long long)a.lda < (1ull << 32) &&
                       (unsigned long long)a.N * (unsigned long long)a.K < (1ull << 32),
                   "%s: operand exceeds 2^32 elements", who);
    return PIPS_OK;
}

}  // namespace pips
