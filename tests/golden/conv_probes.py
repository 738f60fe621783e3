"""Builders and gates of the convolution probes (tests/test_conv_probes.py on the CPU, tests/test_conv_probes_gpu.py on the
GPU): pure torch / numpy, importable without a device.  Every builder takes a ``device`` so that the GPU tests can form the
large operands and fp64 references where the kernels run; nothing here calls the library.

Three families.
A. Impulse response: a map that is zero except for power-of-two impulses on a lattice (pitch 3, pitch 4 at stride 2) makes
   every output exactly one weight times a power of two, or zero.  Expected output by indexing; gate: equality.
B. Mixed scales: 2^a[ci] per input channel, 2^b[co] per output channel; every element against the componentwise forward
   bound (K + 3) u (conv(|x|, |w|) + |b|); statistics per (frame, channel).
C. |mean| >> std: the pivoted partials {sum(x-p), sum((x-p)^2), p, n} part by part (pivot inside the part's range, n the
   part's pixel count) and the variance they combine to.

Routes.  The library has no route query for convolutions; ``predict`` mirrors the host-side choices of launch_conv,
launch_conv_x3 and launch_conv_bf16 for a device of ``cus`` compute units and names the kernel, the number of statistics
partials per frame and the partition of the output pixels into parts.  The tests compare the number the call reports.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import value_range as V

U24 = V.U24

Row = namedtuple("Row", "id entry route F H W Cin Cout k s p norm out_bf16")
Route = namedtuple("Route", "name parts layout size")        # layout "linear": runs of ``size`` pixels; "tile": 4 rows x ``size`` columns


def _r(id_, entry, route, F_, H, W, Cin, Cout, k=3, s=1, p=None, norm=False, out_bf16=False):
    return Row(id_, entry, route, F_, H, W, Cin, Cout, k, s, k // 2 if p is None else p, norm, out_bf16)


# entry: f32 = conv_nhwc, x3 = conv_nhwc_x3, bf16 = conv_nhwc_bf16 (fp32 maps), maps = conv_nhwc_bf16_maps
ROWS = (
    _r("igemm_64", "f32", "igemm_f32", 2, 23, 31, 64, 64),
    _r("igemm_416", "f32", "igemm_f32", 1, 15, 19, 416, 256),
    _r("igemm_s2", "f32", "igemm_f32", 2, 23, 31, 64, 96, s=2),
    _r("igemm_1x1", "f32", "igemm_f32", 2, 23, 31, 96, 128, k=1, s=2),
    _r("t4_cfg0", "f32", "f32_t4_cfg0", 16, 93, 125, 64, 64),
    _r("t4_cfg0_tiny", "f32", "f32_t4_cfg0", 640, 5, 7, 64, 64),
    _r("t4_cfg1", "f32", "f32_t4_cfg1", 8, 93, 125, 96, 96),
    _r("t4_cfg2", "f32", "f32_t4_cfg2", 8, 45, 63, 416, 256),
    _r("t4_linear", "f32", "f32_t4_cfg0", 19, 93, 125, 64, 64),
    _r("x3_small", "x3", "x3_bm64", 2, 23, 31, 64, 64),
    _r("x3_128row", "x3", "x3_bm128", 8, 93, 125, 64, 64),
    _r("x3_256row", "x3", "x3_bm256", 8, 93, 125, 96, 96),
    _r("bf16_igemm", "bf16", "gemm_bf16_bm64", 2, 46, 62, 64, 64),
    _r("c64_lds", "bf16", "c64_lds", 16, 93, 125, 64, 64),
    _r("c64_pp", "maps", "c64_pp", 16, 93, 125, 64, 64, out_bf16=True),
    _r("c64_pp_norm", "maps", "c64_pp", 16, 93, 125, 64, 64, norm=True, out_bf16=True),
    _r("maps_igemm", "maps", "gemm_bf16_bm64", 2, 46, 62, 64, 64, out_bf16=True),
    _r("maps_s2", "maps", "gemm_bf16_bm64", 8, 93, 125, 64, 96, s=2, out_bf16=True),
    _r("maps_1x1_f32out", "maps", "gemm_bf16_bm64", 8, 46, 62, 256, 128, k=1),
    _r("c96_t4c", "maps", "c96_t4c", 24, 93, 125, 96, 96, out_bf16=True),
)
ROW = {r.id: r for r in ROWS}


def out_hw(r):
    return (r.H + 2 * r.p - r.k) // r.s + 1, (r.W + 2 * r.p - r.k) // r.s + 1


def cdiv(a, b):
    return (a + b - 1) // b


def predict(r, cus):
    """The kernel a call of row ``r`` with statistics takes on a device of ``cus`` compute units (gemm.hip: launch_conv,
    conv_f32_t4.hip: conv_f32_t4_config, gemm_x3.hip: launch_conv_x3, gemm_bf16.hip: launch_conv_bf16,
    conv_bf16_c64.hip: conv3x3_c64_takes, conv_bf16_t4c.hip: conv_c96_t4_takes), with its partition of the statistics."""
    Ho, Wo = out_hw(r)
    M = Ho * Wo
    same = r.k == 3 and r.s == 1 and r.p == 1 and r.W >= 3
    if r.entry == "f32":
        cfg = {(64, 64): (0, 256, 1), (96, 96): (1, 128, 1), (416, 256): (2, 128, 4)}.get((r.Cin, r.Cout))
        if same and cfg is not None and cdiv(M, cfg[1]) * cfg[2] * r.F * 100 >= cus * 250:
            return Route(f"f32_t4_cfg{cfg[0]}", cdiv(M, cfg[1] // 4), "linear", cfg[1] // 4)
        n = 128 if r.Cout % 128 == 0 else (96 if r.Cout % 96 == 0 else 64)
        bm = 128 if (cdiv(M, 128) * (r.Cout // n) * r.F >= 384 and n != 64) else 64
        wgm = 4 if (n == 96 and bm == 128) else 2
        return Route("igemm_f32", cdiv(M, bm) * wgm, "linear", bm // wgm)
    if r.entry == "x3":
        bn = 64 if r.Cout <= 64 else 128
        bm = 128 if cdiv(M, 128) * cdiv(r.Cout, bn) * r.F >= 256 else 64
        if bn == 128 and cdiv(M, 256) * cdiv(r.Cout, 128) * r.F >= 160:
            bm = 256
        return Route(f"x3_bm{bm}", cdiv(M, bm) * (4 if bm == 256 else 2), "linear", 64 if bm >= 128 else 32)
    in_bf16 = r.entry == "maps"
    if (in_bf16 and r.out_bf16 and not r.norm and same and (r.Cin, r.Cout) == (96, 96) and cdiv(M, 256) * r.F >= 4 * cus
            and cdiv(M, 256) <= max(2 * cdiv(M, 64) + 4, cdiv(Wo, 32) * cdiv(Ho, 4) * 4)):
        return Route("c96_t4c", cdiv(M, 256), "linear", 256)
    if in_bf16 == r.out_bf16 and same and (r.Cin, r.Cout) == (64, 64) and r.W >= 48:
        tpf = cdiv(r.W, 64) * cdiv(r.H, 4)
        if tpf * r.F >= 512 and tpf * 4 <= 2 * cdiv(M, 64) + 4:
            if in_bf16:
                return Route("c64_pp", cdiv(r.W, 32) * cdiv(r.H, 4) * 4, "tile", 32)
            return Route("c64_lds", tpf * 4, "tile", 64)
    bn = 64 if r.Cout <= 64 else 128
    bm = 128 if cdiv(M, 128) * cdiv(r.Cout, bn) * r.F >= 512 else 64
    return Route(f"gemm_bf16_bm{bm}", cdiv(M, bm) * 2, "linear", bm // 2)


def part_of_pixel(route, Ho, Wo, device="cpu"):
    """(Ho * Wo,) part number of every output pixel (row-major) under the route's partition"""
    if route.layout == "linear":
        return torch.arange(Ho * Wo, device=device) // route.size
    y = torch.arange(Ho, device=device)[:, None]
    x = torch.arange(Wo, device=device)[None, :]
    return (((y // 4) * cdiv(Wo, route.size) + x // route.size) * 4 + y % 4).reshape(-1)


def part_sizes(route, Ho, Wo):
    """(parts,) pixels of every part (trailing parts of a ragged last tile hold none)"""
    return torch.bincount(part_of_pixel(route, Ho, Wo), minlength=route.parts)


def stats_of_stored(r, route):
    """whether the route's statistics describe the map it stores (fp32 outputs; the 96 -> 96 kernel's separate statistics
    kernel reads the stored bf16 map) or the fp32 accumulators behind a bf16 store"""
    return (not r.out_bf16) or route.name == "c96_t4c"


# ----------------------------------------------------------------------------------------------- A. impulse response
def pitch(r):
    return 4 if r.s == 2 else 3


def impulse_calls(r):
    """calls of r.F frames that run every lattice phase, and as many passes as it takes to visit every input channel"""
    passes = max(1, cdiv(r.Cin, r.H * r.W))
    return cdiv(pitch(r) ** 2 * passes, r.F)


def lattice(r, call, device="cpu"):
    """Frame f of call ``call`` has the global index g = call * F + f, the phase g % P^2 and the pass g // P^2.  Returns
    (site, ci, e, neg): (F, H, W) tensors -- whether the pixel holds an impulse, its input channel (every pixel is a site in
    exactly one phase of a pass: 7 (pass * H W + y W + x) + 3 pass mod Cin visits all channels, 7 being coprime to every Cin),
    the exponent of its amplitude in [-3, 3] (a second integer hash) and a mark on a third of the sites (case (a) of the
    normalise-on-load test makes those negative)."""
    P = pitch(r)
    g = call * r.F + torch.arange(r.F, device=device)
    ph, pas = g % (P * P), g // (P * P)
    py, px = (ph // P)[:, None, None], (ph % P)[:, None, None]
    yy = torch.arange(r.H, device=device)[None, :, None]
    xx = torch.arange(r.W, device=device)[None, None, :]
    gg, pas = g[:, None, None], pas[:, None, None]
    site = (yy % P == py) & (xx % P == px)
    ci = (7 * (pas * r.H * r.W + yy * r.W + xx) + 3 * pas) % r.Cin
    hh = ((yy * 31 + xx * 17 + gg * 7) ^ (yy * xx + gg * 5)) & 0xFFFF
    e = hh % 7 - 3
    neg = (hh // 7) % 3 == 0
    return site, ci.expand_as(site), e.expand_as(site), neg.expand_as(site)


def impulse_weights(r, device="cpu", seed=11):
    """unit normal / sqrt(K), (Cout, k, k, Cin); rounded to bf16 for the routes with bf16 operands, full fp32 otherwise"""
    g = torch.Generator().manual_seed(seed + r.Cin + r.Cout + r.k)
    w = torch.randn(r.Cout, r.k, r.k, r.Cin, generator=g) / math.sqrt(r.k * r.k * r.Cin)
    if r.entry in ("bf16", "maps"):
        w = w.bfloat16().float()
    return w.to(device)


def impulse_map(r, call, device="cpu"):
    """(F, H, W, Cin) fp32: 2^e in channel ci at the lattice sites, zero elsewhere"""
    site, ci, e, _ = lattice(r, call, device)
    x = torch.zeros(r.F * r.H * r.W, r.Cin, device=device)
    flat = site.reshape(-1).nonzero().squeeze(1)
    x[flat, ci.reshape(-1)[flat]] = torch.exp2(e.reshape(-1)[flat].float())
    return x.view(r.F, r.H, r.W, r.Cin)


def _tap_index(r, n_out, n_in, kk, device):
    i = torch.arange(n_out, device=device) * r.s - r.p + kk
    return i.clamp(0, n_in - 1), (i >= 0) & (i < n_in)


def impulse_expected(r, call, w, device="cpu", drop_neg=False):
    """(F, Ho, Wo, Cout) fp32 by indexing: 2^e * w[co, ky, kx, ci] for the one impulse in the output's window, else 0.
    drop_neg: the marked third of the sites contributes nothing (what a ReLU leaves of a negative impulse)."""
    site, ci, e, neg = lattice(r, call, device)
    if drop_neg:
        site = site & ~neg
    Ho, Wo = out_hw(r)
    amp = torch.where(site, torch.exp2(e.float()), torch.zeros((), device=device))
    exp = torch.zeros(r.F, Ho, Wo, r.Cout, device=device)
    hits = torch.zeros(r.F, Ho, Wo, dtype=torch.int32, device=device)
    for ky in range(r.k):
        iy, vy = _tap_index(r, Ho, r.H, ky, device)
        for kx in range(r.k):
            ix, vx = _tap_index(r, Wo, r.W, kx, device)
            a = amp[:, iy][:, :, ix] * (vy[:, None] & vx[None, :])
            nz = a != 0
            hits += nz
            c = ci[:, iy][:, :, ix][nz]
            exp[nz] = a[nz][:, None] * w[:, ky, kx, :].t()[c]
    assert int(hits.max()) <= 1, "two impulses in one window"
    return exp


def impulse_coverage(r):
    """Asserts, on the CPU, that over the phases every (output pixel, tap) pair whose tap lies inside the image is hit, that no
    window holds two impulses, and that over all calls every input channel carries an impulse.  Returns the number of pairs."""
    P = pitch(r)
    Ho, Wo = out_hw(r)
    yy, xx = torch.arange(r.H)[:, None], torch.arange(r.W)[None, :]
    cover = torch.zeros(Ho, Wo, r.k * r.k, dtype=torch.bool)
    inside = torch.zeros_like(cover)
    for ph in range(P * P):
        site = (yy % P == ph // P) & (xx % P == ph % P)
        per_window = torch.zeros(Ho, Wo, dtype=torch.int32)
        for ky in range(r.k):
            iy, vy = _tap_index(r, Ho, r.H, ky, "cpu")
            for kx in range(r.k):
                ix, vx = _tap_index(r, Wo, r.W, kx, "cpu")
                v = vy[:, None] & vx[None, :]
                hit = site[iy][:, ix] & v
                cover[:, :, ky * r.k + kx] |= hit
                inside[:, :, ky * r.k + kx] = v
                per_window += hit
        assert int(per_window.max()) <= 1, f"{r.id}: phase {ph} puts two impulses into one window"
    assert torch.equal(cover, inside), f"{r.id}: {int((inside & ~cover).sum())} (pixel, tap) pairs are never hit"
    used = torch.zeros(r.Cin, dtype=torch.bool)
    phases = set()
    for call in range(impulse_calls(r)):
        site, ci, _, _ = lattice(r, call)
        used[ci[site]] = True
        phases |= set(((call * r.F + torch.arange(r.F)) % (P * P)).tolist())
    assert len(phases) == P * P, f"{r.id}: phases {sorted(phases)} of {P * P}"
    assert bool(used.all()), f"{r.id}: {int((~used).sum())} input channels never carry an impulse"
    return int(inside.sum())


def norm_params(r, device="cpu", seed=5):
    """(F, Cin, 2) = {mean, rstd}: mean a multiple of 1/4 in [-2, 2], rstd in {1/2, 1, 2}"""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randint(-8, 9, (r.F, r.Cin), generator=g).float() / 4
    rstd = torch.exp2(torch.randint(-1, 2, (r.F, r.Cin), generator=g).float())
    return torch.stack([mean, rstd], dim=-1).to(device)


def impulse_map_prenorm(r, call, nrm, device="cpu"):
    """Case (a): the bf16 map whose relu((x - mean) * rstd) is impulse_map with the marked third of the sites deleted: the
    background equals mean, a site holds mean + 2^e / rstd or (marked) mean - 2^e / rstd in its channel.  Every value has at
    most 8 significant bits (|mean| <= 2 in quarters, 2^e / rstd in [2^-4, 2^4]): exact in bf16, and staged exactly."""
    site, ci, e, neg = lattice(r, call, device)
    mean, rstd = nrm[..., 0], nrm[..., 1]
    x = mean[:, None, None, :].expand(r.F, r.H, r.W, r.Cin).clone().view(-1, r.Cin)
    flat = site.reshape(-1).nonzero().squeeze(1)
    f = flat // (r.H * r.W)
    c = ci.reshape(-1)[flat]
    sign = torch.where(neg.reshape(-1)[flat], -1.0, 1.0)
    x[flat, c] = mean[f, c] + sign * torch.exp2(e.reshape(-1)[flat].float()) / rstd[f, c]
    x = x.view(r.F, r.H, r.W, r.Cin)
    assert torch.equal(x.bfloat16().float(), x)
    return x.bfloat16()


def ones_map_prenorm(r, nrm):
    """Case (b): background mean + 1 / rstd, staged to exactly 1 inside the image (taps outside the image must stay 0)"""
    x = (nrm[..., 0] + 1.0 / nrm[..., 1])[:, None, None, :].expand(r.F, r.H, r.W, r.Cin).contiguous()
    assert torch.equal(x.bfloat16().float(), x)
    return x.bfloat16()


def exact_stats_bound(exp, n):
    """Family A's statistics gate per (frame, channel): 4 n u sum|expected| for s1 and 4 n u sum expected^2 for s2"""
    e = exp.double()
    return 4 * n * U24 * e.abs().sum(dim=(1, 2)), 4 * n * U24 * (e * e).sum(dim=(1, 2))


# ----------------------------------------------------------------------------------------------- B. mixed scales
def scale_exponents(r, a_max=6, b_max=10):
    """a[ci] in [-a_max, a_max] and b[co] in [-b_max, b_max]: fixed permutation patterns (5 ci + 3 mod 2 a_max + 1,
    8 co + 5 mod 2 b_max + 1: both multipliers coprime to the moduli), not sorted"""
    a = (5 * torch.arange(r.Cin) + 3) % (2 * a_max + 1) - a_max
    b = (8 * torch.arange(r.Cout) + 5) % (2 * b_max + 1) - b_max
    return a, b


def mixed_case(r, device="cpu", frames=None, a_max=6):
    """dict x (F, H, W, Cin) carrying 2^a[ci]; w, b unscaled; sw = 2^b[co].  x and w rounded to bf16 first where the route
    sees bf16 (the scales are powers of two: rounding and scaling commute)."""
    Fr = r.F if frames is None else frames
    g = torch.Generator().manual_seed(1000 + r.H * 7 + r.Cin + r.Cout + r.k)
    x = torch.randn(Fr, r.H, r.W, r.Cin, generator=g)
    w = torch.randn(r.Cout, r.k, r.k, r.Cin, generator=g) / math.sqrt(r.k * r.k * r.Cin)
    b = torch.randn(r.Cout, generator=g)
    if r.entry in ("bf16", "maps"):
        x, w = x.bfloat16().float(), w.bfloat16().float()
    a, bb = scale_exponents(r, a_max)
    return dict(x=(x * torch.exp2(a.float())).to(device), w=w.to(device), b=b.to(device), sw=torch.exp2(bb.float()).to(device))


def ref_and_mag(r, x, w, b):
    """fp64 reference and magnitude sum conv(|x|, |w|) + |b|"""
    bd = None if b is None else b.double()
    return V.conv_ref64(x, w, bd, r.k, r.s, r.p), V.conv_ref64(x.abs(), w.abs(), None if b is None else bd.abs(), r.k, r.s, r.p)


def element_bound(r, ref, mag, out_bf16=None):
    """|out - ref| <= (K + 3) u mag, plus half a bf16 ulp of the reference where the map is stored as bf16"""
    K = r.k * r.k * r.Cin
    b = (K + 3) * U24 * mag
    if r.out_bf16 if out_bf16 is None else out_bf16:
        b = b + V.BF16_HALF_ULP * ref.abs()
    return b


def bf16_ulp(ref):
    """the bf16 ulp at |ref| (8 significant bits)"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120))) - 7)


def stats_bounds_accum(r, ref, mag, n):
    """Statistics from fp32 accumulators, per (frame, channel): |s1 - sum ref| <= gamma sum mag, gamma = (K + 3 + n) u;
    for s2 the same to first order: an element error e = (K + 3) u mag moves x^2 by 2 |x| e + e^2, and the pivoted sum of n
    squares with its fp64 recombination (q + 2 p s + n p^2) adds 4 (n + 2) u sum (|x| + e)^2."""
    K = r.k * r.k * r.Cin
    e = (K + 3) * U24 * mag
    b1 = (K + 3 + n) * U24 * mag.sum(dim=(1, 2))
    b2 = (2 * ref.abs() * e + e * e).sum(dim=(1, 2)) + 4 * (n + 2) * U24 * ((ref.abs() + e) ** 2).sum(dim=(1, 2))
    return b1, b2


def stats_bounds_stored(out, n):
    """Statistics of a stored map (the 96 -> 96 route): gamma = n u against the fp64 sums of the map itself"""
    o = out.double()
    return n * U24 * o.abs().sum(dim=(1, 2)), n * U24 * (o * o).sum(dim=(1, 2))


def rotate_bias(b):
    """wrong implementation: the bias of the neighbouring channel"""
    return torch.roll(b, 1)


def swap_taps(w, co):
    """wrong implementation: two kernel taps of output channel co exchanged"""
    w = w.clone()
    k = w.shape[1]
    t = w[co, 0, 0].clone()
    w[co, 0, 0] = w[co, k - 1, k - 1]
    w[co, k - 1, k - 1] = t
    return w


# ----------------------------------------------------------------------------------------------- C. |mean| >> std
def lowvar_case(r, device="cpu"):
    """Unit-normal map; weights unit normal / sqrt(K) times the output's std; one bias for every channel.  fp32 stores:
    bias 64, std 1/16 (mean / std = 2^10).  bf16 stores (ulp 1/32 .. 1/64 at 4): bias 4, std 1/4 (mean / std = 2^4), so that
    the stored map still carries variance.  Operands rounded to bf16 where the route sees bf16."""
    bias, std = (4.0, 0.25) if r.out_bf16 else (64.0, 1.0 / 16)
    g = torch.Generator().manual_seed(2000 + r.H + r.Cin + r.Cout + r.k)
    x = torch.randn(r.F, r.H, r.W, r.Cin, generator=g)
    w = torch.randn(r.Cout, r.k, r.k, r.Cin, generator=g) / math.sqrt(r.k * r.k * r.Cin) * std
    if r.entry in ("bf16", "maps"):
        x, w = x.bfloat16().float(), w.bfloat16().float()
    return dict(x=x.to(device), w=w.to(device), b=torch.full((r.Cout,), bias, device=device), ratio=bias / std)


def mean_var_from_sums(s1, s2, npix):
    mean = s1 / npix
    return mean, s2 / npix - mean * mean


def part_min_max(m, part, parts):
    """m (F, M, C), part (M,) -> (min, max) of every part, (F, parts, C); parts without a pixel keep +-inf"""
    Fr, _, Cc = m.shape
    idx = part[None, :, None].expand_as(m)
    lo = torch.full((Fr, parts, Cc), float("inf"), dtype=m.dtype, device=m.device).scatter_reduce(1, idx, m, "amin")
    hi = torch.full((Fr, parts, Cc), float("-inf"), dtype=m.dtype, device=m.device).scatter_reduce(1, idx, m, "amax")
    return lo, hi


def check_partials(stats, route, Ho, Wo, summed, widen=None):
    """The layout claims of one call's partials (F, parts, C, 4) against the map ``summed`` (F, Ho, Wo, C) the route is
    specified to sum (``widen``: per-element slack of that map, (F, Ho, Wo, C)): n of every part is its pixel count, the n of
    a frame add up to Ho Wo, the pivot of every part that holds a pixel lies between the part's minimum and maximum.
    Returns a list of complaints (empty: all well)."""
    bad = []
    st = stats.double()
    want_n = part_sizes(route, Ho, Wo).to(st.device).double()
    if st.shape[1] != route.parts:
        return [f"{st.shape[1]} parts, the route {route.name} writes {route.parts}"]
    n = st[..., 3]
    if not bool((n == want_n[None, :, None]).all()):
        bad.append(f"n differs from the parts' pixel counts at {int((n != want_n[None, :, None]).sum())} entries")
    if not bool((n.sum(dim=1) == Ho * Wo).all()):
        bad.append("the n of a frame do not add up to Ho * Wo")
    m = summed.double().reshape(summed.shape[0], Ho * Wo, -1)
    part = part_of_pixel(route, Ho, Wo, m.device)
    if widen is None:
        lo, hi = part_min_max(m, part, route.parts)
    else:
        wd = widen.double().reshape(m.shape)
        lo, _ = part_min_max(m - wd, part, route.parts)
        _, hi = part_min_max(m + wd, part, route.parts)
    piv = st[..., 2]
    held = (want_n > 0)[None, :, None].expand_as(piv)
    out = held & ((piv < lo) | (piv > hi))
    if bool(out.any()):
        f, p, c = [int(t[0]) for t in out.nonzero(as_tuple=True)]
        bad.append(f"{int(out.sum())} pivots outside their part's range, e.g. frame {f} part {p} channel {c}: "
                   f"pivot {float(piv[f, p, c]):.6g}, range [{float(lo[f, p, c]):.6g}, {float(hi[f, p, c]):.6g}]")
    return bad


def partial_sums(stats):
    """pips_amd.ops.partial_sums, restated for the CPU proofs (the GPU tests call the library's)"""
    st = stats.double()
    s, q, p, n = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
    p = torch.where(n > 0, p, torch.zeros_like(p))
    return (n * p + s).sum(dim=1), (q + 2 * p * s + n * p * p).sum(dim=1)


def emulate_partials(x, size, pivoted=True, wrong=None):
    """x (M,) fp32 -> partials (1, parts, 1, 4) as a kernel writes them: sequential fp32 sums over runs of ``size`` pixels.
    pivoted: about the run's first value; otherwise plain sum / sum of squares (pivot 0).
    wrong = 'pivot': sums about the first value, but the NEXT value stored as the pivot; 'sum_x': the right pivot stored
    beside sums of x instead of x - p."""
    xn = x.numpy().astype(np.float32)
    rows = []
    for i in range(0, len(xn), size):
        run = xn[i:i + size]
        p = run[0] if pivoted else np.float32(0)
        d = run if wrong == "sum_x" else (run - p).astype(np.float32)
        s = np.cumsum(d, dtype=np.float32)[-1]
        q = np.cumsum((d * d).astype(np.float32), dtype=np.float32)[-1]
        if wrong == "pivot":
            p = run[min(1, len(run) - 1)]
        rows.append([s, q, p, np.float32(len(run))])
    return torch.tensor(np.array(rows, dtype=np.float32)).view(1, -1, 1, 4)


def variance_gate_stored(n):
    """relative bound of the variance combined from pivoted partials of n pixels against the fp64 variance of the same map"""
    return 4 * n * U24


def variance_gate_accum(delta, sigma, n):
    """the same where the partials sum accumulators the test cannot read: an element error delta moves the variance by at
    most 2 delta / sigma + (delta / sigma)^2 relative"""
    t = delta / sigma
    return 2 * t + t * t + 4 * n * U24


# ----------------------------------------------------------------------------------------------- encoder-level frames
def low_variance_frames(kind, Fr, H, W, seed=3):
    """the three frame kinds of tests/test_kernels_gpu.py::test_encoder_low_variance_frames at another size"""
    g = torch.Generator().manual_seed(seed)
    if kind == "low_contrast":
        return (200 + torch.randint(-2, 3, (Fr, 3, H, W), generator=g)).float()
    if kind == "letterbox":
        bar = (H * 5) // 16
        return torch.cat([torch.zeros(Fr, 3, bar, W), torch.randint(0, 256, (Fr, 3, H - 2 * bar, W), generator=g).float(),
                          torch.zeros(Fr, 3, bar, W)], 2)
    rgbs = torch.full((Fr, 3, H, W), 128.0)
    rgbs[0, 0, H // 2, W // 2] = 255.0
    return rgbs


def conv2d_nhwc(x, w, b, r, dtype):
    """F.conv2d of NHWC operands in ``dtype`` -> (F, Ho, Wo, Cout)"""
    out = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(0, 3, 1, 2), None if b is None else b.to(dtype),
                   stride=r.s, padding=r.p)
    return out.permute(0, 2, 3, 1)
