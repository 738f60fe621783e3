// Frames out, stabilised (pips_frames_warp; drivers.warp_frames, drivers.Stabilizer): F frames resampled from the src surfaces into
// the dst surfaces of the same format and size through a per-frame affine map from output pixel indices to source positions --
// packed RGB / BGR / RGBA / BGRA, NV12, I420, P010, I010 or planar RGB, with any base address, row pitch and frame step.
// The rule (include/pips_hip.h; yuv.h for the fill colour's RGB -> YCbCr constants) is integer arithmetic from the Q24 / Q16
// coefficients on: positions in int64 (a 32 x 32 -> 64 multiply-add per term), the two-by-two blend in int32, no floating point
// anywhere, so the bytes are drivers.warp_frames_torch's.  Plain HIP, one launch: a 256-thread block owns a WARP_TILE_W x
// WARP_TILE_H tile of output luma of one frame and that tile's chroma samples; a thread produces two or four adjacent samples of a row
// (a whole number of dwords) and stores them as dwords where the address allows.  The block computes the box of source samples its tile can tap from the same
// integers at the tile's four corners (an affine map takes its extremes there; the +1 tap added).  When the box of every plane fits
// WARP_LDS_BYTES the box's rows are staged in LDS -- aligned dwords where a row's address allows, bytes at its ragged ends -- and the
// taps are read from there; otherwise they are read straight from global memory.  The criterion reads the coefficients, the format
// and the tile alone; both paths give the same bits.  A tile whose box lies inside the plane leaves the border rule out (the
// same integers: no tap of it can be outside).  No atomics, no workspace; nothing outside the w x h image of a dst plane is
// written, nothing outside that of a src plane is read.
// Border fill (pips_frames_warp_fill; drivers.warp_frames_fill): the same block and passes with a list of K candidate (source frame,
// row) pairs per output frame.  A tile whose candidate-0 box lies inside every plane is the pass above, unchanged, reading frame
// cand[j][0]; any other tile walks the list sample by sample (warp_walk: a done-mask in registers, taps from global memory, the
// border rule of candidate 0 for what nobody covers).
#include "common.h"
#include "yuv.h"

namespace pips {

namespace {

constexpr int WARP_THREADS = 256;
enum { WARP_PACKED3 = 0, WARP_PACKED4 = 1, WARP_NV12 = 2, WARP_I420 = 3, WARP_PLANAR8 = 4, WARP_P010 = 5, WARP_I010 = 6 };

// frame f, row y of a plane starts at src + f sstep + y spitch (dst likewise)
struct WarpPlane {
    const unsigned char* src;
    unsigned char* dst;
    size_t spitch, sstep, dpitch, dstep;
};

// fill: the border colour in the surface's components -- the bytes of a packed pixel in memory order, R G B of the three planes,
// or Y Cb Cr
struct WarpArgs {
    WarpPlane pl[3];
    int h, w, border;
    int fill[3];
};

// the candidate lists of pips_frames_warp_fill: cand (Fd,K) indices into the Fs source frames, coef (Fd,K,6), and the optional
// (Fd,h,w) map of the list position that supplied each sample of plane 0 (nullptr: none).  pips_frames_warp leaves it empty.
struct WarpFill {
    const int* cand;
    const int* coef;
    int K, Fs;
    unsigned char* source;
    size_t mpitch, mstep;
};

// how a tile gets its taps: from global memory, from its box staged in LDS, or candidate by candidate (warp_walk)
enum { WARP_DIRECT = 0, WARP_STAGED = 1, WARP_WALK = 2 };
constexpr int FRAMES_A_LAUNCH = 65535;                         // the grid's y: one launch for any call below that

// The source position, in 1/256 sample of its plane's grid, of output sample (x, y): m = (m0, m1, m2) gives U, (m3, m4, m5) gives V.
// A chroma sample (cx, cy) stands at luma (2 cx + 0.5, 2 cy + 0.5).  warp_lin is the sum ahead of the rounding -- it grows by
// warp_step(m0) from a sample to its right neighbour, exactly, in int64 -- and warp_round the rounding; >> is the arithmetic shift.
template <bool CHROMA>
__device__ __forceinline__ long long warp_lin(int a, int b, int c, int x, int y) {
    if constexpr (CHROMA)
        return (long long)a * (4 * x + 1) + (long long)b * (4 * y + 1) + 512ll * c - (1ll << 24);
    else
        return (long long)a * x + (long long)b * y + 256ll * c;
}
template <bool CHROMA>
__device__ __forceinline__ long long warp_step(int a) { return CHROMA ? 4ll * a : (long long)a; }
template <bool CHROMA>
__device__ __forceinline__ long long warp_round(long long X) { return CHROMA ? (X + (1ll << 17)) >> 18 : (X + 32768) >> 16; }
template <bool CHROMA>
__device__ __forceinline__ long long warp_pos(int a, int b, int c, int x, int y) {
    return warp_round<CHROMA>(warp_lin<CHROMA>(a, b, c, x, y));
}

// the tap indices a tile can reach, inclusive, not yet held to the plane
struct WarpBox {
    long long x0, x1, y0, y1;
};

template <bool CHROMA>
__device__ __forceinline__ WarpBox warp_box(const int (&m)[6], int tx0, int ty0) {
    constexpr int TW = CHROMA ? WARP_TILE_W / 2 : WARP_TILE_W, TH = CHROMA ? WARP_TILE_H / 2 : WARP_TILE_H;
    WarpBox b{LLONG_MAX, LLONG_MIN, LLONG_MAX, LLONG_MIN};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = tx0 + ((k & 1) ? TW - 1 : 0), y = ty0 + ((k & 2) ? TH - 1 : 0);
        const long long u = warp_pos<CHROMA>(m[0], m[1], m[2], x, y) >> 8, v = warp_pos<CHROMA>(m[3], m[4], m[5], x, y) >> 8;
        b.x0 = min(b.x0, u), b.x1 = max(b.x1, u + 1), b.y0 = min(b.y0, v), b.y1 = max(b.y1, v + 1);
    }
    return b;
}

// bytes of a staged row of n sample bytes: up to three bytes of lead to the dword grid of its global address, rounded up to dwords
__device__ __forceinline__ long long warp_row_stride(long long n) { return (n + 6) & ~3ll; }

// the staging criterion: the whole box, rows of `pxb` bytes a sample, within WARP_LDS_BYTES
__device__ __forceinline__ bool warp_fits(const WarpBox& b, int pxb) {
    const long long bw = b.x1 - b.x0 + 1, bh = b.y1 - b.y0 + 1;
    if (bw > WARP_LDS_BYTES || bh > WARP_LDS_BYTES) return false;
    return bh * warp_row_stride(bw * pxb) <= WARP_LDS_BYTES;
}

__device__ __forceinline__ int warp_clamp(long long v, int lo, int hi) { return (int)min(max(v, (long long)lo), (long long)hi); }

// value v of component c of the thread's sample p into the thread's bytes as they lie in memory (wd starts as zeros); the fourth
// byte of a four-byte pixel is written 255
template <int C, int BPS, int VSHIFT, int WORDS>
__device__ __forceinline__ void warp_put(unsigned (&wd)[WORDS], int p, int c, int v) {
    const int at = (p * C + c) * BPS;
    wd[at >> 2] |= (unsigned)(v << VSHIFT) << (8 * (at & 3));
    if (C == 4 && c == 2) wd[p] |= 255u << 24;
}

// The thread's sample p at the position (U, V): the four taps through read(xi, yi, c) -- indices inside the plane -- blended.
// INSIDE: no tap can be outside, so the clamps and the fill are left out, the integers are the same.  Otherwise a tap outside
// takes the fill (constant) or its index is clamped into the plane.
template <int C, int BPS, int VSHIFT, bool INSIDE, int WORDS, class Read>
__device__ __forceinline__ void warp_blend(const Read& read, long long U, long long V, int pw, int ph, bool constant, const int* fill, int p,
                                           unsigned (&wd)[WORDS]) {
    constexpr int CV = C == 4 ? 3 : C;
    const int fx = (int)(U & 255), fy = (int)(V & 255);
    int cx0, cx1, cy0, cy1;
    bool ix0 = true, ix1 = true, iy0 = true, iy1 = true;
    if constexpr (INSIDE) {
        cx0 = (int)(U >> 8), cy0 = (int)(V >> 8), cx1 = cx0 + 1, cy1 = cy0 + 1;
    } else {
        // the first tap's index, compared as int64: anything further out than one sample is as far out as -2 or pw
        const int x0 = warp_clamp(U >> 8, -2, pw), y0 = warp_clamp(V >> 8, -2, ph);
        const int x1 = x0 + 1, y1 = y0 + 1;
        ix0 = x0 >= 0 && x0 < pw, ix1 = x1 >= 0 && x1 < pw, iy0 = y0 >= 0 && y0 < ph, iy1 = y1 >= 0 && y1 < ph;
        cx0 = min(max(x0, 0), pw - 1), cx1 = min(max(x1, 0), pw - 1);
        cy0 = min(max(y0, 0), ph - 1), cy1 = min(max(y1, 0), ph - 1);
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
        int p00 = read(cx0, cy0, c), p01 = read(cx1, cy0, c), p10 = read(cx0, cy1, c), p11 = read(cx1, cy1, c);
        if (!INSIDE && constant) {
            const int fv = fill[c];
            p00 = (ix0 && iy0) ? p00 : fv, p01 = (ix1 && iy0) ? p01 : fv;
            p10 = (ix0 && iy1) ? p10 : fv, p11 = (ix1 && iy1) ? p11 : fv;
        }
        const int v = ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16;
        warp_put<C, BPS, VSHIFT>(wd, p, c, v);
    }
}

// the thread's first nbytes bytes to d: dwords where d allows, bytes otherwise and at a ragged end
template <int WORDS>
__device__ __forceinline__ void warp_store(unsigned char* d, const unsigned (&wd)[WORDS], int nbytes) {
    const bool aligned = ((uintptr_t)d & 3u) == 0;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
        if (aligned && 4 * k + 4 <= nbytes) {
            *(unsigned*)(d + 4 * k) = wd[k];
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * k + b < nbytes) d[4 * k + b] = (unsigned char)(wd[k] >> (8 * b));
        }
    }
}

// One plane of one tile.  C samples of BPS bytes lie interleaved in a pixel of the plane (C = 4: three are resampled, the fourth
// is written 255); a 16-bit sample holds its ten bits at VSHIFT.  (tx0, ty0) is the tile's first sample in this plane's grid, pw x
// ph the plane's samples.  Every thread of the block comes here (the staged form has barriers); the first TW TH / Q produce Q
// adjacent samples of a row each, Q such that they are a whole number of dwords.  FIRST: the block's first pass (nobody reads
// the LDS yet).  INSIDE: the tile's whole box lies inside the plane, so no tap needs the border rule (warp_blend).  Source frame
// fs is read, frame f of dst written.
template <int C, int BPS, int VSHIFT, bool CHROMA, int Q, bool FIRST, bool STAGED, bool INSIDE>
__device__ __forceinline__ void warp_pass(const WarpPlane& P, int fs, int f, int pw, int ph, const int* fill, int border,
                                          const int (&m)[6], int tx0, int ty0, const WarpBox& box, unsigned* lds_w) {
    constexpr int TW = CHROMA ? WARP_TILE_W / 2 : WARP_TILE_W, TH = CHROMA ? WARP_TILE_H / 2 : WARP_TILE_H;
    constexpr int QR = TW / Q;                                  // threads on a row of the tile
    static_assert((Q * C * BPS) % 4 == 0 && TW % Q == 0 && QR * TH <= WARP_THREADS, "a thread stores whole dwords");
    constexpr int PXB = C * BPS;
    const int tid = (int)threadIdx.x;
    const unsigned char* src_f = P.src + (size_t)fs * P.sstep;
    unsigned char* lds = (unsigned char*)lds_w;
    int sx0 = 0, sy0 = 0, stride = 0;
    unsigned lead0 = 0;
    if constexpr (STAGED) {
        // the box held to the plane: clamping is monotone, so a clamped tap index lies in the clamped box
        sx0 = warp_clamp(box.x0, 0, pw - 1), sy0 = warp_clamp(box.y0, 0, ph - 1);
        const int sx1 = warp_clamp(box.x1, 0, pw - 1), sy1 = warp_clamp(box.y1, 0, ph - 1);
        const int n = (sx1 - sx0 + 1) * PXB, rows = sy1 - sy0 + 1;
        stride = (int)warp_row_stride(n);
        const int slots = stride >> 2;
        const unsigned char* base = src_f + (size_t)sy0 * P.spitch + (size_t)sx0 * PXB;
        lead0 = (unsigned)(uintptr_t)base & 3u;
        if constexpr (!FIRST) __syncthreads();                  // the pass before has read its taps
        for (int idx = tid; idx < rows * slots; idx += WARP_THREADS) {
            const int r = idx / slots, j = idx - r * slots;
            const unsigned char* row = base + (size_t)r * P.spitch;
            const int lead = (int)((uintptr_t)row & 3u);        // byte i of the row lies at lead + i of its staged row
            const int lo = 4 * j;
            if (lo >= lead && lo + 4 <= lead + n) {
                lds_w[(r * stride + lo) >> 2] = *(const unsigned*)(row - lead + lo);
            } else {
#pragma unroll
                for (int b = lo; b < lo + 4; ++b)
                    if (b >= lead && b < lead + n) lds[r * stride + b] = row[b - lead];
            }
        }
        __syncthreads();
    }
    const unsigned pitch_lo = (unsigned)P.spitch & 3u;
    // sample c of the pixel (xi, yi) of the plane, both inside it
    auto read = [&](int xi, int yi, int c) -> int {
        int v;
        if constexpr (STAGED) {
            const int r = yi - sy0;
            const int off = r * stride + (int)((lead0 + (unsigned)r * pitch_lo) & 3u) + (xi - sx0) * PXB + c * BPS;
            v = BPS == 2 ? (int)*(const unsigned short*)(lds + off) : (int)lds[off];
        } else {
            const unsigned char* q = src_f + (size_t)yi * P.spitch + (size_t)xi * PXB + c * BPS;
            v = BPS == 2 ? (int)*(const unsigned short*)q : (int)*q;
        }
        return BPS == 2 ? (v >> VSHIFT) & 1023 : v;
    };
    if (tid >= QR * TH) return;                                 // (no barrier behind this point)
    const int x = tx0 + Q * (tid % QR), y = ty0 + tid / QR;
    if (x >= pw || y >= ph) return;
    const bool constant = border == PIPS_WARP_BORDER_CONSTANT;
    constexpr int WORDS = Q * PXB / 4;
    unsigned wd[WORDS];                                         // the thread's bytes as they lie in memory
#pragma unroll
    for (int k = 0; k < WORDS; ++k) wd[k] = 0u;
    long long XU = warp_lin<CHROMA>(m[0], m[1], m[2], x, y), XV = warp_lin<CHROMA>(m[3], m[4], m[5], x, y);
#pragma unroll
    for (int p = 0; p < Q; ++p, XU += warp_step<CHROMA>(m[0]), XV += warp_step<CHROMA>(m[3])) {
        const int px = x + p;
        if (px < pw)
            warp_blend<C, BPS, VSHIFT, INSIDE>(read, warp_round<CHROMA>(XU), warp_round<CHROMA>(XV), pw, ph, constant, fill, p, wd);
    }
    warp_store(P.dst + (size_t)f * P.dstep + (size_t)y * P.dpitch + (size_t)x * PXB, wd, min(Q, pw - x) * PXB);
}

// "every tap that has weight lies inside the plane", along one axis of n samples, for the position P in 1/256 sample (int64)
__device__ __forceinline__ bool warp_covers(long long P, int n) {
    const long long i = P >> 8;
    return i >= 0 && (i + 1 <= n - 1 || ((P & 255) == 0 && i <= n - 1));
}

// four positions of the source map at (x, y) of frame j, one a byte of `who`: a dword where the address allows
__device__ __forceinline__ void warp_map_put(const WarpFill& wf, int j, int x, int y, int w, unsigned who) {
    unsigned char* d = wf.source + (size_t)j * wf.mstep + (size_t)y * wf.mpitch + (size_t)x;
    const int n = min(4, w - x);
    if (n == 4 && ((uintptr_t)d & 3u) == 0) {
        *(unsigned*)d = who;
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b < n) d[b] = (unsigned char)(who >> (8 * b));
    }
}

// One plane of one tile of pips_frames_warp_fill off the fast path, warp_pass's template and thread layout: the thread walks the K
// candidates of output frame j in list order with a done-mask over its Q samples.  An invalid candidate and one whose box misses
// the plane are skipped (the same for the whole block; neither can cover a sample), and the thread leaves the list once nothing
// of it is left to fill.  A covered sample is the plain blend -- warp_blend with clamped indices, which only moves a tap of
// weight 0 -- read from global memory.  What no candidate covered is candidate 0 under the border rule, or the fill when
// candidate 0 is invalid.  No LDS, no barrier.  map: the plane's samples are the source map's (plane 0; Q = 4).
template <int C, int BPS, int VSHIFT, bool CHROMA, int Q>
__device__ __forceinline__ void warp_walk(const WarpPlane& P, int j, int pw, int ph, const int* fill, int border, int tx0, int ty0,
                                          const WarpFill& wf, bool map) {
    constexpr int TW = CHROMA ? WARP_TILE_W / 2 : WARP_TILE_W, TH = CHROMA ? WARP_TILE_H / 2 : WARP_TILE_H;
    constexpr int QR = TW / Q, PXB = C * BPS, CV = C == 4 ? 3 : C, WORDS = Q * PXB / 4;
    constexpr unsigned FULL = (1u << Q) - 1u;
    const int tid = (int)threadIdx.x;
    if (tid >= QR * TH) return;
    const int x = tx0 + Q * (tid % QR), y = ty0 + tid / QR;
    if (x >= pw || y >= ph) return;
    const unsigned char* src_f = P.src;
    auto read = [&](int xi, int yi, int c) -> int {
        const unsigned char* q = src_f + (size_t)yi * P.spitch + (size_t)xi * PXB + c * BPS;
        const int v = BPS == 2 ? (int)*(const unsigned short*)q : (int)*q;
        return BPS == 2 ? (v >> VSHIFT) & 1023 : v;
    };
    unsigned wd[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; ++k) wd[k] = 0u;
    unsigned done = 0u, who = 0xFFFFFFFFu;                      // bit p: sample p has its value; byte p: who gave it
#pragma unroll
    for (int p = 0; p < Q; ++p)
        if (x + p >= pw) done |= 1u << p;
    const int* cand = wf.cand + (size_t)j * wf.K;
    const int* coef = wf.coef + 6 * (size_t)j * wf.K;
    int m[6];
    for (int k = 0; k < wf.K && done != FULL; ++k) {
        const int cf = cand[k];
        if (cf < 0 || cf >= wf.Fs) continue;
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = coef[6 * k + i];
        const WarpBox b = warp_box<CHROMA>(m, tx0, ty0);
        if (b.x1 < 0 || b.y1 < 0 || b.x0 > pw - 1 || b.y0 > ph - 1) continue;
        src_f = P.src + (size_t)cf * P.sstep;
        long long XU = warp_lin<CHROMA>(m[0], m[1], m[2], x, y), XV = warp_lin<CHROMA>(m[3], m[4], m[5], x, y);
#pragma unroll
        for (int p = 0; p < Q; ++p, XU += warp_step<CHROMA>(m[0]), XV += warp_step<CHROMA>(m[3])) {
            const long long U = warp_round<CHROMA>(XU), V = warp_round<CHROMA>(XV);
            if (!((done >> p) & 1u) && warp_covers(U, pw) && warp_covers(V, ph)) {
                warp_blend<C, BPS, VSHIFT, false>(read, U, V, pw, ph, false, fill, p, wd);
                done |= 1u << p;
                who = (who & ~(255u << (8 * (p & 3)))) | ((unsigned)k << (8 * (p & 3)));
            }
        }
    }
    if (done != FULL) {
        const int cf = cand[0];
        const bool valid = cf >= 0 && cf < wf.Fs;
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = coef[i];
        src_f = P.src + (size_t)(valid ? cf : 0) * P.sstep;
        const bool constant = border == PIPS_WARP_BORDER_CONSTANT;
        long long XU = warp_lin<CHROMA>(m[0], m[1], m[2], x, y), XV = warp_lin<CHROMA>(m[3], m[4], m[5], x, y);
#pragma unroll
        for (int p = 0; p < Q; ++p, XU += warp_step<CHROMA>(m[0]), XV += warp_step<CHROMA>(m[3])) {
            if ((done >> p) & 1u) continue;
            if (valid) {
                warp_blend<C, BPS, VSHIFT, false>(read, warp_round<CHROMA>(XU), warp_round<CHROMA>(XV), pw, ph, constant, fill, p, wd);
            } else {
#pragma unroll
                for (int c = 0; c < CV; ++c) warp_put<C, BPS, VSHIFT>(wd, p, c, fill[c]);
            }
        }
    }
    warp_store(P.dst + (size_t)j * P.dstep + (size_t)y * P.dpitch + (size_t)x * PXB, wd, min(Q, pw - x) * PXB);
    if (map && wf.source != nullptr) warp_map_put(wf, j, x, y, pw, who);
}

// One plane of one tile by MODE.  Staged or direct: the pass with or without the border rule, by where the tile's box lies (the
// same for every thread of the block).
template <int C, int BPS, int VSHIFT, bool CHROMA, int Q, bool FIRST, int MODE>
__device__ __forceinline__ void warp_plane(const WarpPlane& P, int fs, int f, int pw, int ph, const int* fill, int border,
                                           const int (&m)[6], int tx0, int ty0, const WarpBox& box, unsigned* lds_w, const WarpFill& wf,
                                           bool map) {
    if constexpr (MODE == WARP_WALK) {
        warp_walk<C, BPS, VSHIFT, CHROMA, Q>(P, f, pw, ph, fill, border, tx0, ty0, wf, map);
    } else {
        constexpr bool STAGED = MODE == WARP_STAGED;
        if (box.x0 >= 0 && box.y0 >= 0 && box.x1 < pw && box.y1 < ph)
            warp_pass<C, BPS, VSHIFT, CHROMA, Q, FIRST, STAGED, true>(P, fs, f, pw, ph, fill, border, m, tx0, ty0, box, lds_w);
        else
            warp_pass<C, BPS, VSHIFT, CHROMA, Q, FIRST, STAGED, false>(P, fs, f, pw, ph, fill, border, m, tx0, ty0, box, lds_w);
    }
}

// The planes of one tile: source frame fs (staged or direct) or the list wf (walk) into frame f of dst
template <int LAYOUT, int MODE>
__device__ __forceinline__ void warp_tile(const WarpArgs& a, int fs, int f, const int (&m)[6], int X0, int Y0, const WarpBox& lb,
                                          const WarpBox& cb, unsigned* lds, const WarpFill& wf) {
    const int h = a.h, w = a.w, ch = (h + 1) >> 1, cw = (w + 1) >> 1, CX0 = X0 >> 1, CY0 = Y0 >> 1;
    if constexpr (LAYOUT == WARP_PACKED3) {
        warp_plane<3, 1, 0, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
    } else if constexpr (LAYOUT == WARP_PACKED4) {
        warp_plane<4, 1, 0, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
    } else if constexpr (LAYOUT == WARP_PLANAR8) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            warp_plane<1, 1, 0, false, 4, false, MODE>(a.pl[k], fs, f, w, h, a.fill + k, a.border, m, X0, Y0, lb, lds, wf, k == 0);
    } else if constexpr (LAYOUT == WARP_NV12) {
        warp_plane<1, 1, 0, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
        warp_plane<2, 1, 0, true, 2, false, MODE>(a.pl[1], fs, f, cw, ch, a.fill + 1, a.border, m, CX0, CY0, cb, lds, wf, false);
    } else if constexpr (LAYOUT == WARP_I420) {
        warp_plane<1, 1, 0, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
#pragma unroll
        for (int k = 1; k < 3; ++k)
            warp_plane<1, 1, 0, true, 4, false, MODE>(a.pl[k], fs, f, cw, ch, a.fill + k, a.border, m, CX0, CY0, cb, lds, wf, false);
    } else if constexpr (LAYOUT == WARP_P010) {
        warp_plane<1, 2, 6, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
        warp_plane<2, 2, 6, true, 2, false, MODE>(a.pl[1], fs, f, cw, ch, a.fill + 1, a.border, m, CX0, CY0, cb, lds, wf, false);
    } else {
        warp_plane<1, 2, 0, false, 4, true, MODE>(a.pl[0], fs, f, w, h, a.fill, a.border, m, X0, Y0, lb, lds, wf, true);
#pragma unroll
        for (int k = 1; k < 3; ++k)
            warp_plane<1, 2, 0, true, 2, false, MODE>(a.pl[k], fs, f, cw, ch, a.fill + k, a.border, m, CX0, CY0, cb, lds, wf, false);
    }
}

// what both kernels ask of a layout
template <int LAYOUT>
struct WarpLayout {
    static constexpr bool YUV = LAYOUT == WARP_NV12 || LAYOUT == WARP_I420 || LAYOUT == WARP_P010 || LAYOUT == WARP_I010;
    static constexpr int SB = (LAYOUT == WARP_P010 || LAYOUT == WARP_I010) ? 2 : 1;
    static constexpr int LPX = LAYOUT == WARP_PACKED3 ? 3 : LAYOUT == WARP_PACKED4 ? 4 : SB;        // bytes of a pixel of plane 0
    static constexpr int CPX = (LAYOUT == WARP_NV12 || LAYOUT == WARP_P010) ? 2 * SB : SB;          // ... of a chroma plane
};

// the tile's boxes under m -> whether every plane's box fits the staging budget
template <int LAYOUT>
__device__ __forceinline__ bool warp_boxes(const int (&m)[6], int X0, int Y0, WarpBox& lb, WarpBox& cb) {
    using L = WarpLayout<LAYOUT>;
    lb = warp_box<false>(m, X0, Y0);
    cb = lb;
    bool staged = warp_fits(lb, L::LPX);
    if constexpr (L::YUV) {
        cb = warp_box<true>(m, X0 >> 1, Y0 >> 1);
        staged = staged && warp_fits(cb, L::CPX);
    }
    return staged;
}

// One block per tile and frame.  The coefficients, the boxes and the choice of path are the same for every thread of the block.
template <int LAYOUT>
__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(WarpArgs a, const int* __restrict__ coef, int tiles_x, int f_base) {
    __shared__ unsigned lds[WARP_LDS_BYTES / 4];
    const int f = f_base + (int)blockIdx.y;
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * WARP_TILE_W, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * WARP_TILE_H;
    int m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = coef[6 * (size_t)f + k];
    WarpBox lb, cb;
    const bool staged = warp_boxes<LAYOUT>(m, X0, Y0, lb, cb);
    const WarpFill none{};
    if (staged)
        warp_tile<LAYOUT, WARP_STAGED>(a, f, f, m, X0, Y0, lb, cb, lds, none);
    else
        warp_tile<LAYOUT, WARP_DIRECT>(a, f, f, m, X0, Y0, lb, cb, lds, none);
}

// pips_frames_warp_fill: one block per tile and OUTPUT frame j.  The fast path -- candidate 0 valid and its box inside every
// plane, so that candidate 0 covers every sample of the tile -- is warp_kernel's tile reading frame cand[j][0], and zeros in the
// source map; every other tile walks the list.  The choice is the same for every thread of the block.
template <int LAYOUT>
__global__ __launch_bounds__(WARP_THREADS) void warp_fill_kernel(WarpArgs a, WarpFill wf, int tiles_x, int f_base) {
    __shared__ unsigned lds[WARP_LDS_BYTES / 4];
    const int j = f_base + (int)blockIdx.y;
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * WARP_TILE_W, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * WARP_TILE_H;
    const int c0 = wf.cand[(size_t)j * wf.K];
    int m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = wf.coef[6 * (size_t)j * wf.K + k];
    WarpBox lb, cb;
    const bool staged = warp_boxes<LAYOUT>(m, X0, Y0, lb, cb);
    const int cw = (a.w + 1) >> 1, ch = (a.h + 1) >> 1;
    bool inside = c0 >= 0 && c0 < wf.Fs && lb.x0 >= 0 && lb.y0 >= 0 && lb.x1 < a.w && lb.y1 < a.h;
    if constexpr (WarpLayout<LAYOUT>::YUV) inside = inside && cb.x0 >= 0 && cb.y0 >= 0 && cb.x1 < cw && cb.y1 < ch;
    if (!inside) {
        warp_tile<LAYOUT, WARP_WALK>(a, 0, j, m, X0, Y0, lb, cb, lds, wf);
        return;
    }
    if (staged)
        warp_tile<LAYOUT, WARP_STAGED>(a, c0, j, m, X0, Y0, lb, cb, lds, wf);
    else
        warp_tile<LAYOUT, WARP_DIRECT>(a, c0, j, m, X0, Y0, lb, cb, lds, wf);
    if (wf.source != nullptr) {
        const int x = X0 + 4 * ((int)threadIdx.x % (WARP_TILE_W / 4)), y = Y0 + (int)threadIdx.x / (WARP_TILE_W / 4);
        if (x < a.w && y < a.h) warp_map_put(wf, j, x, y, a.w, 0u);
    }
}

WarpArgs warp_args(int format, int matrix, int range, int border, int fill_rgb, int h, int w, const void* const* sp, const size_t* spitch,
                   const size_t* sstep, void* const* dp, const size_t* dpitch, const size_t* dstep) {
    WarpArgs a;
    for (int k = 0; k < 3; ++k)
        a.pl[k] = WarpPlane{(const unsigned char*)sp[k], (unsigned char*)dp[k], spitch[k], sstep[k], dpitch[k], dstep[k]};
    a.h = h, a.w = w, a.border = border;
    const int R = (fill_rgb >> 16) & 255, G = (fill_rgb >> 8) & 255, B = fill_rgb & 255;
    const bool bgr = format == PIPS_FMT_BGR24 || format == PIPS_FMT_BGRA32;
    a.fill[0] = bgr ? B : R, a.fill[1] = G, a.fill[2] = bgr ? R : B;
    if (format == PIPS_FMT_NV12 || format == PIPS_FMT_I420) rgb_to_yuv(RGB_RULES[matrix][range], R, G, B, a.fill[0], a.fill[1], a.fill[2]);
    if (format == PIPS_FMT_P010 || format == PIPS_FMT_I010)
        rgb_to_yuv10(RGB10_RULES[matrix][range], R, G, B, a.fill[0], a.fill[1], a.fill[2]);
    return a;
}

// launch(layout, grid, tiles_x, f0) once per FRAMES_A_LAUNCH frames of F, f0 the first frame of the launch and layout the
// std::integral_constant of the kernel layout of `format`
template <class Launch>
void warp_launches(int format, int F, int h, int w, const Launch& launch) {
    const int tiles_x = (w + WARP_TILE_W - 1) / WARP_TILE_W, tiles_y = (h + WARP_TILE_H - 1) / WARP_TILE_H;     // <= 128 x 512
    for (int f0 = 0; f0 < F; f0 += FRAMES_A_LAUNCH) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)std::min(F - f0, FRAMES_A_LAUNCH));
#define PIPS_WARP_CASE(L) launch(std::integral_constant<int, L>{}, grid, tiles_x, f0)
        switch (format) {
            case PIPS_FMT_RGB24:
            case PIPS_FMT_BGR24: PIPS_WARP_CASE(WARP_PACKED3); break;
            case PIPS_FMT_RGBA32:
            case PIPS_FMT_BGRA32: PIPS_WARP_CASE(WARP_PACKED4); break;
            case PIPS_FMT_NV12: PIPS_WARP_CASE(WARP_NV12); break;
            case PIPS_FMT_I420: PIPS_WARP_CASE(WARP_I420); break;
            case PIPS_FMT_P010: PIPS_WARP_CASE(WARP_P010); break;
            case PIPS_FMT_I010: PIPS_WARP_CASE(WARP_I010); break;
            default: PIPS_WARP_CASE(WARP_PLANAR8); break;
        }
#undef PIPS_WARP_CASE
    }
}

}  // namespace

int launch_frames_warp(int format, int matrix, int range, int border, int fill_rgb, int F, int h, int w, const void* const* sp,
                       const size_t* spitch, const size_t* sstep, void* const* dp, const size_t* dpitch, const size_t* dstep,
                       const int* coef, hipStream_t st) {
    const WarpArgs a = warp_args(format, matrix, range, border, fill_rgb, h, w, sp, spitch, sstep, dp, dpitch, dstep);
    warp_launches(format, F, h, w, [&](auto layout, dim3 grid, int tiles_x, int f0) {
        hipLaunchKernelGGL(warp_kernel<decltype(layout)::value>, grid, dim3(WARP_THREADS), 0, st, a, coef, tiles_x, f0);
    });
    PIPS_CHECK_LAUNCH("frames_warp");
    return PIPS_OK;
}

int launch_frames_warp_fill(int format, int matrix, int range, int border, int fill_rgb, int Fs, int Fd, int K, int h, int w,
                            const void* const* sp, const size_t* spitch, const size_t* sstep, void* const* dp, const size_t* dpitch,
                            const size_t* dstep, const int* cand, const int* coef, unsigned char* source, size_t source_pitch,
                            size_t source_step, hipStream_t st) {
    const WarpArgs a = warp_args(format, matrix, range, border, fill_rgb, h, w, sp, spitch, sstep, dp, dpitch, dstep);
    const WarpFill wf{cand, coef, K, Fs, source, source_pitch, source_step};
    warp_launches(format, Fd, h, w, [&](auto layout, dim3 grid, int tiles_x, int f0) {
        hipLaunchKernelGGL(warp_fill_kernel<decltype(layout)::value>, grid, dim3(WARP_THREADS), 0, st, a, wf, tiles_x, f0);
    });
    PIPS_CHECK_LAUNCH("frames_warp_fill");
    return PIPS_OK;
}

}  // namespace pips
