// The XCD-aware tile grid of the four-wave fp32 assembly kernels (gemm_f32_t4.hip, conv_f32_e.hip).
#pragma once
#include "common.h"

namespace pips {

// Block -> (row unit, column tile).  Blocks go to the XCDs round robin (block & 7), every XCD has its own L2, and the operands
// come out of the Infinity Cache: in the linear order (column tile fastest) the eight column tiles of the M = 2048 down-projection
// land on eight XCDs and EVERY XCD pulls all of A through its L2 -- 132 MB per launch for 20 MB of operands.  Instead the XCDs
// split the tile grid gm x gn (host: the split with the smallest per-XCD footprint) and each works through its own sub-grid.
struct F4Grid { int units_m, tiles_n, gm, gn; };
__device__ __forceinline__ void f4_tile(const F4Grid& g, int* um, int* tn) {
    const int b = blockIdx.x;
    if (g.gm == 0) { *um = b / g.tiles_n; *tn = b - *um * g.tiles_n; return; }
    const int xcd = b & 7, local = b >> 3, xm = xcd / g.gn, xn = xcd - xm * g.gn;
    const int pm = g.units_m / g.gm, pn = g.tiles_n / g.gn, lm = local / pn, ln = local - lm * pn;
    *um = xm * pm + lm; *tn = xn * pn + ln;
    (void)pm;
}
static inline F4Grid f4_grid(int units_m, int tiles_n, long bytes_unit_m, long bytes_tile_n) {
    F4Grid g = {units_m, tiles_n, 0, 1};
    if (!PIPS_TUNE("PIPS_F32_T4_XCD", 1) || ((long)units_m * tiles_n) % 8 != 0) return g;
    long best = -1;
    for (int gm = 8; gm >= 1; gm >>= 1) {
        const int gn = 8 / gm;
        if (units_m % gm != 0 || tiles_n % gn != 0) continue;
        const long foot = (units_m / gm) * bytes_unit_m + (tiles_n / gn) * bytes_tile_n;
        if (best < 0 || foot < best) { best = foot; g.gm = gm; g.gn = gn; }
    }
    return g;
}

}  // namespace pips
