"""Builders, reference and gate of the gather probes (tests/test_gather_probes.py on the CPU, tests/test_gather_probes_gpu.py on the
GPU): pure torch / numpy, importable without a device; every builder takes a ``device``; nothing here calls the library.

The operation: CorrBlock.corr + CorrBlock.sample fused into columns 128:324 of the mixer input -- per mixer row m = (b, n, s) and
pyramid level l the 49 bilinear taps (k = ix * 7 + iy) of the correlation map c_p = sum_c f_c m_{p,c} / sqrt(128) around the row's
position / 2^l.  Four kernels compute it (track.hip: mixer_input_kernel, mixer_input_bf16maps_kernel; gather_tiled.hip:
gather_tiled_kernel, gather_mfma_kernel), all from ONE geometry per (row, level): level_sample_geometry / corr_window.

Layouts.  ``levels``: four tensors (F, H_l, W_l, 128), channel last, F = B * S frames, filled INDEPENDENTLY (not pooled: a level
mix-up shows) with frame s scaled by 2^s (a frame mix-up shows).  ``ffeats`` (M, 128) and ``coords`` (M, 2) particle-major,
m = (b * N + n) * S + s, which reads frame b * S + s.

Reference.  ``geometry`` is the twin of the kernels' geometry in numpy float32, operation by operation and without fused
multiply-add: coordinate * 2^-l, 2c / (size - 1), - 1, + 1, * ((size - 1) / 2), floor, subtract.  The POSITION is fp32 on purpose:
an fp64 position differs from the kernels' by the rounding of that chain, and paying for it was most of the 5e-5 of the older
tests.  ``reference`` evaluates, in fp64, ref = nw (1-wy)(1-wx) + ne (1-wy) wx + sw wy (1-wx) + se wy wx with the twin's weights
widened to fp64 and pixels outside the map counting 0.  bf16 routes: maps ``level.bfloat16()``, features ``ffeats.bfloat16()``.

Bound, per element:   (n + 8) u blend(A) + K_POS (ulp32(max(|ix|, 1)) Dx + ulp32(max(|iy|, 1)) Dy),   u = 2^-24.
  * A_p = sum_c |f_c| |m_{p,c}| / sqrt(128), blended with the reference's four weights; n = the number of non-zero products of
    the four pixels' dots (128 on dense data, 1 on impulses): the forward bound n u sum|f m| of an n-term fp32 sum in any order
    (products of bf16 operands are exact in fp32; fp32 products cost one more rounding each, inside the + 8).
  * + 8: the division by sqrt(128) (or 1/sqrt(128) folded into the weights: one rounding of the constant, one of the product), the
    three products forming a weight, the three additions of the blend, and the rounding of 1 - w.
  * Dx = the largest |c_p - c_q| over horizontally adjacent pixels in columns x0-1 .. x0+2 of the two rows of the tap's cell, Dy
    likewise over vertically adjacent pixels in rows y0-1 .. y0+2 of its two columns: a weight that moves by d changes the tap by
    at most d * D, also when the position rounds across a pixel boundary.  The kernels' weights can differ from the twin's by
    ulp(ix) / 2: hipcc may contract ``ix - floorf(ix)`` with the product that made ix into one fma (see corr_window).
  * K_POS = 4, about twice what the reference project's own fp32 path needs at positions of 4 pixels and more.  Its sampler
    (oracle.pips_oracle.corr_sample) normalises each of the 49 taps separately, so its positions carry the rounding of the chain,
    which is not a multiple of ulp32(ix) but 2^-24 (size - 1) / 2 pixels whatever ix is (the "- 1" rounds g to 2^-25): 5 ulp32(1) on
    a 40-wide map.  ``chain_slack`` is that term.  The kernels have ONE geometry per (row, level), the twin's, so the gate of the
    kernels does not include it; the CPU comparisons with the sampler do, with a second-order companion (a tap that floors to the
    other side of a pixel boundary in x and in y picks up the diagonal neighbour at a weight of dx dy).
  * A tap whose bound is 0 has every pixel of that neighbourhood outside the map or zero: the output must be +0.0, bit for bit.

MEASURED (tests/test_gather_probes.py and tests/test_gather_probes_gpu.py print them):
  * position allowance of oracle.corr_sample in float32 against this reference, impulse maps of 33 x 40, integer and quarter-pixel
    positions over the whole map: 2.60 / 2.02 / 1.09 / 0.55 ulp32 of the position per level; from 4 pixels on 1.55 / 2.26 / 1.09 /
    0.37; beside one chain term, none.  (The 2.60 is above the 2.5 expected when the bound was proposed; the cause is the
    chain term above, and K_POS was not raised.)
  * the kernel-formula emulation (``emulate``): error / bound 0.019 .. 0.081 on every family, shape, mode and summation variant.
  * the kernels on an MI355X, largest error / bound per level: direct routes 0.007 .. 0.082, tiled routes 0.010 .. 0.116, run-time-S
    routes 0.006 .. 0.064; every bound-0 tap +0.0.
"""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
K_POS = 4.0
RADIUS = 3
SQRT_C = math.sqrt(128.0)
K128_F32 = np.float32(0.08838834764831845)          # gather_tiled.hip: the 1/sqrt(128) that rides on the weights
S1 = (1, 200, 33, 40)
S2 = (2, 40, 16, 31)
WIN = (1, 24, 17, 24)                                # the run-time-S routes: T = S frames of 17 x 24 maps
LADDER = (1, 6, 7, 32, 33, 96, 97, 193)
TS = 16                                              # level-0 tile edge of the tiled routes
LATTICE_OFFSET = ((1, 1), (2, 0), (0, 0), (1, 0))    # (x, y) of the impulse lattice per level: the coarse levels hold as many as fit

MUTANTS = ("tap_order", "swap_weights", "anchor_l2", "no_scale_l3", "replicate_border", "leak_east", "leak_frame", "leak_particle",
           "offset_1e-6", "feat_truncate", "feat_ties_away", "feat_fp32")


def level_sizes(H8, W8):
    return [(H8 >> l, W8 >> l) for l in range(4)]


# ============================================================================================ geometry twin
def geometry(coords, sizes):
    """level_sample_geometry / corr_window in numpy float32.  coords (M, 2) -> dict of (M, 4) arrays: ix, iy, fx, fy (floors),
    wx, wy (float32)."""
    c = np.ascontiguousarray(torch.as_tensor(coords).detach().cpu().numpy(), dtype=np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    out = {k: [] for k in ("ix", "iy", "fx", "fy", "wx", "wy")}
    for l, (H, W) in enumerate(sizes):
        inv = one / np.float32(1 << l)
        for a, size, ki, kf, kw in ((0, W, "ix", "fx", "wx"), (1, H, "iy", "fy", "wy")):
            cl = c[:, a] * inv                                   # coords / 2**l
            g = (two * cl) / np.float32(size - 1)                # 2 c / (size - 1)
            g = g - one                                          # - 1
            t = g + one                                          # + 1
            i = t * (np.float32(size - 1) / two)                 # * ((size - 1) / 2)
            f = np.floor(i)
            assert i.dtype == np.float32 and f.dtype == np.float32
            out[ki].append(i), out[kf].append(f), out[kw].append(i - f)
    return {k: np.stack(v, axis=1) for k, v in out.items()}


def ulp32(x):
    """spacing of float32 at max(|x|, 1)"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(1.0))).astype(np.float64)


def chain_slack(sizes):
    """(4, 2) the position error, in pixels, that a SEPARATE evaluation of the fp32 chain can add to a tap of level l (x, y):
    2 c / (size - 1) - 1 rounds g (|g| <= 2 here) to 2^-24, (g + 1) again, and the product by (size - 1) / 2 scales both; the last
    product's own rounding is within ulp32(ix).  Used on the CPU only, where the reference project's sampler (which normalises
    every tap on its own, in fp32 or fp64) is compared with the twin."""
    return np.array([[2.0 * 2.0 ** -24 * (W - 1) / 2.0, 2.0 * 2.0 ** -24 * (H - 1) / 2.0] for H, W in sizes])


# ============================================================================================ windows
def _to_frames(t, B, S):
    """particle-major (B*N*S, ...) -> frame-major (B*S, N, ...)"""
    M = t.shape[0]
    N = M // (B * S)
    return t.reshape(B, N, S, *t.shape[1:]).transpose(1, 2).reshape(B * S, N, *t.shape[1:])


def _to_rows(t, B, S):
    """frame-major (B*S, N, ...) -> particle-major (B*N*S, ...)"""
    N = t.shape[1]
    return t.reshape(B, S, N, *t.shape[2:]).transpose(1, 2).reshape(B * N * S, *t.shape[2:])


def _window(cmap, fx, fy, off, size, replicate=False):
    """cmap (F, N, H, W); fx, fy (F, N) int64 floors -> (F, N, size, size) pixels [fy + off .. , fx + off ..], 0 outside the map
    (replicate: the border pixel instead -- a mutant)"""
    F_, N, H, W = cmap.shape
    r = torch.arange(size, device=cmap.device)
    yy, xx = (fy + off)[..., None] + r, (fx + off)[..., None] + r
    ok = ((yy >= 0) & (yy < H))[..., :, None] & ((xx >= 0) & (xx < W))[..., None, :]
    idx = yy.clamp(0, H - 1)[..., :, None] * W + xx.clamp(0, W - 1)[..., None, :]
    win = torch.gather(cmap.reshape(F_, N, H * W), 2, idx.reshape(F_, N, size * size)).reshape(F_, N, size, size)
    return win if replicate else torch.where(ok, win, torch.zeros_like(win))          # (not win * ok: -x * 0 = -0.0)


def _taps(x):
    """(..., 7 rows tj, 7 columns ti) -> (..., 49) in the transposed order k = ti * 7 + tj"""
    return x.transpose(-1, -2).reshape(*x.shape[:-2], 49)


def _blend(win, o, w):
    """four-weight blend of a window whose pixel (fx - 3, fy - 3) sits at [o, o]; w = (w00, w01, w10, w11) each (F, N, 1, 1)"""
    return (win[..., o:o + 7, o:o + 7] * w[0] + win[..., o:o + 7, o + 1:o + 8] * w[1] + win[..., o + 1:o + 8, o:o + 7] * w[2]
            + win[..., o + 1:o + 8, o + 1:o + 8] * w[3])


def _operands(levels, ffeats, bf16, dtype):
    if bf16:
        levels, ffeats = [lv.bfloat16() for lv in levels], ffeats.bfloat16()
    return [lv.to(dtype) for lv in levels], ffeats.to(dtype)


def reference(levels, ffeats, coords, B, S, bf16=False):
    """-> dict: ref, bound (M, 196) float64 on the operands' device; geo (the twin's arrays); per element also ``pos`` (the position
    term at K_POS = 1: ulp32 Dx + ulp32 Dy), ``sum`` (the summation term (n + 8) u blend(A)) and ``slack``, ``second`` (chain_slack's
    Dx, Dy term and its second-order companion: CPU comparisons with the reference project's sampler only)."""
    dev = ffeats.device
    lv64, f64 = _operands(levels, ffeats, bf16, torch.float64)
    sizes = [tuple(lv.shape[1:3]) for lv in levels]
    geo = geometry(coords, sizes)
    slack_px = chain_slack(sizes)
    ff = _to_frames(f64, B, S)                                                    # (F, N, 128)
    F_, N = ff.shape[:2]
    cols = {k: [] for k in ("ref", "sum", "pos", "slack", "second")}
    for l, m in enumerate(lv64):
        H, W = sizes[l]
        m = m.reshape(F_, H * W, 128)
        c = torch.einsum("fnc,fpc->fnp", ff, m).div_(SQRT_C).reshape(F_, N, H, W)
        A = torch.einsum("fnc,fpc->fnp", ff.abs(), m.abs()).div_(SQRT_C).reshape(F_, N, H, W)
        nnz = torch.einsum("fnc,fpc->fnp", (ff != 0).double(), (m != 0).double()).reshape(F_, N, H, W)
        t = lambda k: _to_frames(torch.from_numpy(geo[k][:, l].astype(np.float64)).to(dev), B, S)
        fx, fy = t("fx").long(), t("fy").long()
        wx, wy = t("wx")[..., None, None], t("wy")[..., None, None]
        w = ((1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx)
        win = _window(c, fx, fy, -RADIUS - 1, 10)
        ref = _blend(win, 1, w)
        bA = _blend(_window(A, fx, fy, -RADIUS - 1, 10), 1, w)
        nw = _window(nnz, fx, fy, -RADIUS, 8)
        n = torch.stack([nw[..., :7, :7], nw[..., :7, 1:], nw[..., 1:, :7], nw[..., 1:, 1:]]).amax(0)
        dh = (win[..., :, 1:] - win[..., :, :-1]).abs()                           # (10, 9): pair (column c, c + 1)
        dv = (win[..., 1:, :] - win[..., :-1, :]).abs()                           # (9, 10)
        Dx = torch.stack([dh[..., r:r + 7, q:q + 7] for r in (1, 2) for q in (0, 1, 2)]).amax(0)
        Dy = torch.stack([dv[..., r:r + 7, q:q + 7] for r in (0, 1, 2) for q in (1, 2)]).amax(0)
        ux = _to_frames(torch.from_numpy(ulp32(geo["ix"][:, l])).to(dev), B, S)[..., None, None]
        uy = _to_frames(torch.from_numpy(ulp32(geo["iy"][:, l])).to(dev), B, S)[..., None, None]
        cols["ref"].append(_taps(ref))
        cols["sum"].append(_taps((n + 8) * U24 * bA))
        cols["pos"].append(_taps(ux * Dx + uy * Dy))
        sx, sy = float(slack_px[l, 0]), float(slack_px[l, 1])
        cols["slack"].append(_taps(sx * Dx + sy * Dy))
        # second order: a tap evaluated on its own can floor to the other side of a pixel boundary in x AND y and pick up the
        # diagonal neighbour, which the plus-shaped neighbourhood of Dx, Dy does not hold, at a weight of (dx)(dy)
        cols["second"].append(((sx + K_POS * ux) * (sy + K_POS * uy) * win.abs().amax(dim=(-1, -2), keepdim=True)).expand(F_, N, 7, 7)
                              .reshape(F_, N, 49))
    out = {k: _to_rows(torch.cat(v, dim=-1), B, S) for k, v in cols.items()}
    out["bound"] = out["sum"] + K_POS * out["pos"]
    out["geo"] = geo
    return out


def ratios(got, r, k_pos=K_POS, slack=0.0, sum_term=1.0):
    """(4,) per level the largest error / bound, counting a miss of an exact zero as inf; (4,) number of wrong exact zeros.
    Every element is judged.  The gate of the kernels is the default.  ``slack`` > 0 (CPU comparisons with the reference project's
    sampler, whose every tap runs the fp32 chain on its own): that many chain terms and the second-order term are added, and a
    bound-0 tap has to be within the second-order term instead of being +0.0."""
    got = got.to(r["ref"].device)
    bound = sum_term * r["sum"] + k_pos * r["pos"] + slack * r["slack"] + (r["second"] if slack > 0 else 0.0)
    err = (got.double() - r["ref"]).abs()
    zero = r["bound"] == 0
    assert bool(torch.isfinite(got).all())
    bad0 = zero & (((got != 0) | torch.signbit(got)) if slack == 0 else (err > bound))      # +0.0, bit for bit
    q = torch.where(zero, torch.where(bad0, torch.full_like(err, float("inf")), torch.zeros_like(err)), err / bound.clamp_min(1e-300))
    return q.reshape(-1, 4, 49).amax(dim=(0, 2)).cpu(), bad0.reshape(-1, 4, 49).sum(dim=(0, 2)).cpu()


def census(r):
    """per level: fraction of taps with a non-zero reference, fraction that are bound-0 exact zeros"""
    nz = (r["ref"] != 0).reshape(-1, 4, 49).double().mean(dim=(0, 2)).cpu()
    z = (r["bound"] == 0).reshape(-1, 4, 49).double().mean(dim=(0, 2)).cpu()
    return nz, z


# ============================================================================================ kernel-formula emulation
def bf16_round(x, mode):
    """fp32 -> bf16 value (as fp32) by the wrong rules of the mutants: "truncate", "ties_away" (round half away from zero)"""
    bits = x.contiguous().view(torch.int32)
    if mode == "ties_away":
        bits = bits + 0x8000                                                       # sign-magnitude: half and above go up in magnitude
    return (bits & -65536).view(torch.float32)


def sort_order(geo, sizes, B, S):
    """(F, N) particle numbers of every frame in the order of bin_particles_kernel: by level-0 tile, then 4x4 cell in Morton order"""
    H0, W0 = sizes[0]
    ax = np.clip(geo["fx"][:, 0].astype(np.int64), 0, W0 - 1)
    ay = np.clip(geo["fy"][:, 0].astype(np.int64), 0, H0 - 1)
    cx, cy = (ax >> 2) & 3, (ay >> 2) & 3
    tiles_x = (W0 + TS - 1) // TS
    key = ((ay // TS) * tiles_x + ax // TS) * 16 + ((cx & 1) | ((cy & 1) << 1) | ((cx & 2) << 1) | ((cy & 2) << 2))
    key = _to_frames(torch.from_numpy(key), B, S)
    return torch.sort(key, dim=1, stable=True).indices, key


def emulate(levels, ffeats, coords, B, S, bf16=False, fold=False, mutant=None):
    """What the kernels compute, in torch float32 from the twin's geometry: per-pixel dots in fp32, the division by sqrtf(128) (fold:
    the weights scaled by its reciprocal, as the tiled kernels do), the four-term blend in the kernels' order; bf16: operands rounded
    to bf16 first.  ``mutant``: one of MUTANTS.  -> (M, 196) float32."""
    assert mutant is None or mutant in MUTANTS
    f32 = torch.float32
    dev = ffeats.device
    if bf16:
        lv = [x.bfloat16().to(f32) for x in levels]
        ff = {"feat_truncate": lambda: bf16_round(ffeats, "truncate"), "feat_ties_away": lambda: bf16_round(ffeats, "ties_away"),
              "feat_fp32": lambda: ffeats.to(f32)}.get(mutant, lambda: ffeats.bfloat16().to(f32))()
    else:
        lv, ff = [x.to(f32) for x in levels], ffeats.to(f32)
    sizes = [tuple(x.shape[1:3]) for x in levels]
    geo = geometry(coords, sizes)
    ff = _to_frames(ff, B, S)
    F_, N = ff.shape[:2]
    cols = []
    for l, m in enumerate(lv):
        H, W = sizes[l]
        m = m.reshape(F_, H * W, 128)
        c = torch.bmm(ff, m.transpose(1, 2))
        if mutant == "leak_frame":
            c = c + 2.0 ** -20 * torch.bmm(ff, torch.roll(m, -1, 0).transpose(1, 2))
        c = c.reshape(F_, N, H, W)
        if mutant == "leak_east":
            c = c + 2.0 ** -20 * torch.cat([c[..., 4:], torch.zeros_like(c[..., :4])], dim=-1)
        t = lambda k: _to_frames(torch.from_numpy(geo[k][:, l]).to(dev), B, S)
        fx, fy, wx, wy = t("fx").long(), t("fy").long(), t("wx")[..., None, None], t("wy")[..., None, None]
        if mutant == "swap_weights":
            wx, wy = wy, wx
        if mutant == "anchor_l2" and l == 2:
            fx = fx + 1
        scaled = not (mutant == "no_scale_l3" and l == 3)
        win = _window(c, fx, fy, -RADIUS, 8, replicate=mutant == "replicate_border")
        e, so = 1.0 - wx, 1.0 - wy
        w = (so * e, so * wx, wy * e, wy * wx)
        if fold:
            w = tuple(x * float(K128_F32) for x in w) if scaled else w
        elif scaled:
            win = win / float(np.sqrt(np.float32(128.0)))
        nw, ne, sw, se = win[..., :7, :7], win[..., :7, 1:], win[..., 1:, :7], win[..., 1:, 1:]
        o = nw * w[0]
        o = o + ne * w[1]
        o = o + sw * w[2]
        o = o + se * w[3]
        assert o.dtype == f32
        if mutant == "offset_1e-6":
            r = torch.arange(7, device=dev)
            yy, xx = (fy - RADIUS)[..., None] + r, (fx - RADIUS)[..., None] + r
            inmap = ((yy >= 0) & (yy < H))[..., :, None] & ((xx >= 0) & (xx < W))[..., None, :]
            o = o + 1e-6 * inmap
        cols.append(o.reshape(F_, N, 49) if mutant == "tap_order" else _taps(o))
    out = torch.cat(cols, dim=-1)
    if mutant == "leak_particle":
        order, _ = sort_order(geo, sizes, B, S)
        order = order.to(dev)
        prev = torch.gather(out, 1, torch.roll(order, 1, 1)[..., None].expand(-1, -1, 196))      # sorted slot i -> the row before it
        leak = torch.zeros_like(out).scatter_(1, order[..., None].expand(-1, -1, 196), prev)
        out = out + 2.0 ** -20 * leak
    return _to_rows(out, B, S)


# ============================================================================================ positions
def named_positions(H8, W8):
    """the positions every family shares, in map pixels: (x, y) pairs"""
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(-1e9)))
    pts = [(5.0, 7.0), (12.0, 3.0), (float(W8 - 4), float(H8 - 3))]                            # integers
    pts += [(6.25, 9.5), (13.5, 2.25), (W8 - 7.75, H8 - 5.5)]                                   # integer + 0.25 / 0.5
    pts += [(below(9.0), 4.3), (7.6, below(11.0)), (below(3.0), below(8.0))]                    # just below an integer
    for e in (16, 32):                                                                         # both sides of the tile edges
        if e <= W8:
            pts += [(below(e), 6.4), (float(e), 6.4)]
        if e <= H8:
            pts += [(10.3, below(e)), (10.3, float(e))]
        if e <= W8 and e <= H8:
            pts += [(below(e), below(e)), (float(e), float(e)), (below(e), float(e))]
    pts += [(0.0, 0.0), (W8 - 1.0, 0.0), (0.0, H8 - 1.0), (W8 - 1.0, H8 - 1.0)]                 # the map corners
    pts += [(-2.0, 1.5), (W8 + 2.5, 4.0)]                                                       # windows partly outside
    pts += [(-11.0, 5.0)]                                                                      # wholly outside
    pts += [(8.7, 10.2), (8.7, 10.2)]                                                           # identical coordinates
    pts += [(20.9 if W8 > 24 else 4.9, 12.6), (21.1 if W8 > 24 else 5.1, 13.4)]                 # one 4x4 cell, two level-0 anchors
    return pts


def positions(B, S, N, H8, W8, seed, device="cpu"):
    """(B*N*S, 2) particle-major: per frame the named positions first (N below their number: a third of a frame's particles take
    them, and the list runs on through the frames), then seeded uniform positions over the map and a margin of 1.5 pixels"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.tensor(named_positions(H8, W8), dtype=torch.float32)
    L = pts.shape[0]
    co = torch.rand(B * S, N, 2, generator=g) * torch.tensor([W8 + 2.0, H8 + 2.0]) - 1.5
    for f in range(B * S):
        if N >= L:
            co[f, :L] = pts
        else:
            K = N // 3
            assert B * S * K >= L
            co[f, :K] = pts[(f * K + torch.arange(K)) % L]
    return _to_rows(co, B, S).contiguous().to(device)


def ladder_positions(S, N, seed, device="cpu"):
    """family C on S1 (B = 1): frame s puts LADDER[s] particles into level-0 tile (1, 1) and the others into tile (0, 0), cycling
    through the sixteen 4x4 cells; the fraction keeps the anchor 0.1 pixels clear of the cell's edges"""
    assert S == len(LADDER)
    g = torch.Generator().manual_seed(seed)
    co = torch.empty(S, N, 2)
    for s, k in enumerate(LADDER):
        for first, cnt, tile in ((0, k, 1), (k, N - k, 0)):
            i = torch.arange(cnt)
            cell = torch.stack([(i % 16) % 4, (i % 16) // 4], dim=1).float()
            co[s, first:first + cnt] = tile * TS + cell * 4 + 0.1 + 3.8 * torch.rand(cnt, 2, generator=g)
    return _to_rows(co, 1, S).contiguous().to(device)


# ============================================================================================ family A: impulse response
def impulse_levels(B, S, H8, W8, device="cpu"):
    """Each level zero except on a pitch-3 lattice whose offset differs per level; lattice pixel p = (i, j) holds
    (-1)^(i+j) 2^k(p) 2^s in the single channel c(p), k in -6..6, c(p) walking through all 128 channels."""
    out = []
    for l, (H, W) in enumerate(level_sizes(H8, W8)):
        ox, oy = LATTICE_OFFSET[l]
        m = torch.zeros(B * S, H, W, 128)
        ys, xs = torch.arange(oy, H, 3), torch.arange(ox, W, 3)
        j, i = torch.meshgrid(torch.arange(ys.numel()), torch.arange(xs.numel()), indexing="ij")
        for f in range(B * S):
            lin = j * xs.numel() + i
            ch = (lin * 5 + 3 * l + 7 * f) % 128
            k = (i * 5 + j * 3 + l + f) % 13 - 6
            val = torch.where((i + j) % 2 == 0, 1.0, -1.0) * 2.0 ** (k + f % S).float()
            m[f, ys[j], xs[i], ch] = val
        out.append(m.to(device))
    return out


def impulse_features(M, seed, device="cpu"):
    """every channel +-2^e(c), e in -3..3, the signs seeded per row"""
    g = torch.Generator().manual_seed(seed)
    e = (torch.arange(128) * 3 % 7 - 3).float()
    sign = torch.where(torch.rand(M, 128, generator=g) < 0.5, -1.0, 1.0)
    return (sign * 2.0 ** e).to(device)


def tie_features(M, seed, device="cpu"):
    """family A': fp32 patterns around bf16 ties -- the exact half (low 16 bits 0x8000) under an even and under an odd kept
    mantissa, one fp32 ulp either side of it (0x7fff, 0x8001), both signs, exponents -20..20"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.arange(M * 128).reshape(M, 128) + torch.randint(0, 1 << 20, (M, 1), generator=g)
    low = torch.tensor([0x8000, 0x7FFF, 0x8001])[idx % 3]
    keep = (idx // 3) % 128                                                        # 7 kept mantissa bits, even and odd alternate
    expo = 127 - 20 + (idx // 7) % 41
    sign = (idx // 11 + torch.randint(0, 2, (M, 128), generator=g)) % 2
    bits = (sign << 31) | (expo << 23) | (keep << 16) | low
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).to(device)


# ============================================================================================ family B: mixed scales
def channel_exponents(seed):
    """(a, b): a in -8..8 per map channel, b = clip(-a - 3 + d, -8, 8) with d in -1..1 per feature channel.  The operands' channels
    differ by up to 2^16 while every channel's PRODUCT is 2^-4 .. 2^-2: all 128 channels weigh in the sum (with independent a and b two
    or three channels would carry it and hide the others), and in the darkest blocks of frame 0 the correlations are ~1e-3, where an
    absolute error of 1e-6 is many times the bound."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (128,), generator=g)
    b = (-a - 3 + torch.randint(-1, 2, (128,), generator=g)).clamp(-8, 8)
    return a.float(), b.float()


def mixed_levels(B, S, H8, W8, seed, device="cpu"):
    """per level independently: Gaussian * 2^a[c] (a in -8..8 per channel) * 2^p[y // 4, x // 4] (p in -6..6 per 4x4 block, drawn per
    level) * 2^s.  Stored magnitudes: a float32 normal deviate of torch is a multiple of 2^-24 or so and at most ~6, so every stored
    value is 0 or within 2^-38 .. 2^24 (maps, S <= 12), 2^-32 .. 2^11 (features), and family B2's rescaling (2^+-10 per channel, 2^7)
    keeps values and products far inside the normal range: no subnormal, no overflow."""
    g = torch.Generator().manual_seed(seed + 2)
    a, _ = channel_exponents(seed)
    out = []
    for H, W in level_sizes(H8, W8):
        p = torch.randint(-6, 7, ((H + 3) // 4, (W + 3) // 4), generator=g).float()
        p = p.repeat_interleave(4, 0).repeat_interleave(4, 1)[:H, :W]
        s = (torch.arange(B * S) % S).float()
        m = torch.randn(B * S, H, W, 128, generator=g) * 2.0 ** a * 2.0 ** p[None, :, :, None] * 2.0 ** s[:, None, None, None]
        out.append(m.to(device))
    return out


def mixed_features(M, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed + 3)
    _, b = channel_exponents(seed)
    return (torch.randn(M, 128, generator=g) * 2.0 ** b).to(device)


def channel_shift(seed):
    """t in -10..10 per channel (family B2)"""
    return torch.randint(-10, 11, (128,), generator=torch.Generator().manual_seed(seed)).float()


# ============================================================================================ cases
FAMILIES = ("A", "A'", "B", "C")


def case(family, shape, S=8, device="cpu"):
    """the inputs of one probe: dict(levels, ffeats, coords, B, S, N, H8, W8).  A: impulse maps and power-of-two features; A': impulse
    maps and features on bf16 ties; B: mixed scales; C: family B's data on the occupancy ladder (S1 only)."""
    B, N, H8, W8 = shape
    M = B * N * S
    seed = 1000 * H8 + 10 * W8 + S
    if family == "C":
        assert shape == S1 and S == 8
        coords = ladder_positions(S, N, seed, device)
    else:
        coords = positions(B, S, N, H8, W8, seed, device)
    if family in ("A", "A'"):
        levels = impulse_levels(B, S, H8, W8, device)
        ffeats = impulse_features(M, seed + 1, device) if family == "A" else tie_features(M, seed + 1, device)
    else:
        levels, ffeats = mixed_levels(B, S, H8, W8, seed, device), mixed_features(M, seed, device)
    return dict(levels=levels, ffeats=ffeats, coords=coords, B=B, S=S, N=N, H8=H8, W8=W8)


def args(c):
    return c["levels"], c["ffeats"], c["coords"], c["B"], c["S"]


def position_ulps(got, r, slack=0.0):
    """(4,) per level the K_POS that ``got`` would need: the largest (error - summation term - ``slack`` chain terms) / position term
    over the taps whose position term is not 0"""
    err = (got.to(r["ref"].device).double() - r["ref"]).abs() - r["sum"] - slack * r["slack"]
    q = torch.where(r["pos"] > 0, err / r["pos"].clamp_min(1e-300), torch.zeros_like(err))
    return q.reshape(-1, 4, 49).amax(dim=(0, 2)).cpu()
