"""CPU: frames out, stabilised -- drivers.warp_frames_torch (the integer resampling rule of pips_frames_warp, include/pips_hip.h),
warp_coefficients, motion_smooth and Stabilizer(engine="torch").  The rule is restated here as a plain-Python loop over frames,
planes, samples and channels on Python ints (which cannot overflow), and each sample is also held to its closed form: floor(B + 0.5)
with B the float64 bilinear interpolation of the taps at (U / 256, V / 256), exact because every term stays below 2^27.  (The
kernel and ``engine="library"``: tests/test_warp_gpu.py, which takes its surfaces and coefficient sets from here.)"""
import ctypes
import math
import os
import re
from fractions import Fraction

import pytest
import torch

from pips_amd import drivers, ops
from test_motion import _f64_bits, _life_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("rgb24", "bgr24", "rgba32", "bgra32", "nv12", "i420", "p010", "i010", "planar8")
YUV, WIDE, SEMI = ("nv12", "i420", "p010", "i010"), ("p010", "i010"), ("nv12", "p010")
BORDERS = ("constant", "replicate")
ONE, I32_MIN, I32_MAX = 1 << 24, -2 ** 31, 2 ** 31 - 1
IDENTITY = [ONE, 0, 0, 0, ONE, 0]
POISON = 0xA5


# ---------------------------------------------------------------------------------------------- surfaces
def plane_shapes(fmt, F, h, w):
    """the shapes of the planes of F surfaces of h x w, in samples"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "planar8":
        return [(F, 3, h, w)]
    if fmt in SEMI:
        return [(F, h, w), (F, ch, cw, 2)]
    if fmt in YUV:
        return [(F, h, w), (F, ch, cw), (F, ch, cw)]
    return [(F, h, w, 4 if fmt in ("rgba32", "bgra32") else 3)]


def make_surfaces(fmt, F, h, w, seed=None, off=0, pad=0, gap=0):
    """F surfaces of ``fmt`` as views of larger allocations -> (allocations, views).  Each plane lies in a flat allocation of its
    own behind a guard band of 256 bytes and ``off`` more elements (8-bit: bytes, so the base address is ``off`` mod 4; 16-bit: words),
    its rows ``pad`` elements longer than their samples, its frames ``gap`` elements apart beyond their rows, and a guard band of
    256 bytes behind.  ``seed=None``: every byte of the allocation is POISON (a destination); otherwise every element is random -- 16-bit
    words with junk in the six bits that hold no value -- padding and guards included (a source)."""
    wide = fmt in WIDE
    dtype, guard = (torch.int16, 128) if wide else (torch.uint8, 256)
    g = None if seed is None else torch.Generator().manual_seed(seed)
    flats, views = [], []
    for shape in plane_shapes(fmt, F, h, w):
        if fmt == "planar8":
            pitch = w + pad
            plane = pitch * h + gap // 2
            strides, step = (3 * plane + gap, plane, pitch, 1), 3 * plane + gap
        else:
            row = 1
            for d in shape[2:]:
                row *= d
            pitch = row + pad
            step = pitch * shape[1] + gap
            strides = (step, pitch) + ((shape[3], 1) if len(shape) == 4 else (1,))
        n = guard + off + step * F + guard
        if g is None:
            flat = torch.full((n,), POISON if not wide else (POISON << 8 | POISON) - 65536, dtype=dtype)
        elif wide:
            flat = (torch.randint(0, 65536, (n,), generator=g) - 32768).to(torch.int16)
        else:
            flat = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
        flats.append(flat)
        views.append(flat.as_strided(shape, strides, guard + off))
    return flats, views


def views_like(flats, views, device):
    """the allocations on ``device`` and the same views of them"""
    moved = [f.to(device) for f in flats]
    return moved, [m.as_strided(v.shape, v.stride(), v.storage_offset()) for m, v in zip(moved, views)]


def untouched_outside(flats, views):
    """every element of the destination allocations outside the views still POISON (checked by poisoning the views themselves)"""
    for f, v in zip(flats, views):
        f = f.clone()
        f.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(POISON if f.dtype == torch.uint8 else (POISON << 8 | POISON) - 65536)
        if not bool((f == f[0]).all()):
            return False
    return True


def _values(fmt, p):
    """the values 0..255 / 0..1023 held by a plane"""
    p = p.to(torch.int64)
    return (p & 0xFFFF) >> 6 if fmt == "p010" else (p & 1023 if fmt == "i010" else p)


# ---------------------------------------------------------------------------------------------- coefficient sets
def affine_about(h, w, a, b, d, e, sx=0.0, sy=0.0):
    """the forward map p -> L (p - c) + c + s about the centre c of an h x w surface, L = (a b; d e): six floats"""
    cx, cy = (w - 1) / 2, (h - 1) / 2
    return [a, b, cx - a * cx - b * cy + sx, d, e, cy - d * cx - e * cy + sy]


def _rot(h, w, deg, sx=0.0, sy=0.0):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return drivers.warp_coefficients(torch.tensor([affine_about(h, w, c, -s, s, c, sx, sy)], dtype=torch.float64), (h, w))[0].tolist()


def coefficient_sets(h, w):
    """name -> the six integers, for an h x w surface.  By the staging criterion (ops.warp_staged: the source box of every plane
    of the tile within 12288 bytes) on the tile at (0, 0):
      staged in LDS on every format: identity, shift, rot2, quarter, scale_quarter, shear (and rot45 on all but rgba32 / bgra32);
      read from global memory on every format: scale4, extreme_a, extreme_b (and rot45 on rgba32 / bgra32: 58 rows of 236 bytes)."""
    return {
        "identity": list(IDENTITY),
        "shift": [ONE, 0, int(2.25 * 65536) + 77, 0, ONE, -int(1.5 * 65536) + 3],
        "rot2": _rot(h, w, 2.0, 1.5, -0.75),
        "rot45": _rot(h, w, 45.0),
        "quarter": [0, ONE, 0, -ONE, 0, (h - 1) << 16],
        "scale_quarter": [ONE >> 2, 0, 1 << 14, 0, ONE >> 2, 3 << 13],
        "scale4": [ONE << 2, 0, -(3 << 16), 0, ONE << 2, -(1 << 16) + 999],
        "shear": [ONE, ONE >> 2, -(1 << 16), -(ONE >> 3), ONE + (ONE >> 4), 1 << 15],
        "extreme_a": [I32_MAX, I32_MIN, I32_MIN, I32_MIN, I32_MAX, I32_MAX],
        "extreme_b": [I32_MIN, I32_MAX, I32_MAX, I32_MAX, I32_MIN, I32_MIN],
    }


STAGED_SETS = ("identity", "shift", "rot2", "quarter", "scale_quarter", "shear")
DIRECT_SETS = ("scale4", "extreme_a", "extreme_b")


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_sets_lie_on_both_sides_of_the_staging_criterion(fmt):
    for h, w in ((1, 1), (16, 64), (33, 130)):
        sets = coefficient_sets(h, w)
        assert all(ops.warp_staged(sets[k], fmt) for k in STAGED_SETS)
        assert not any(ops.warp_staged(sets[k], fmt) for k in DIRECT_SETS)
    assert ops.warp_staged(coefficient_sets(33, 130)["rot45"], fmt) == (fmt not in ("rgba32", "bgra32"))
    # the figure itself: identity on 8-bit luma is 17 rows of 72 bytes; four source pixels a pixel are 62 rows of 260 bytes
    assert ops.WARP_LDS_BYTES == 12288 and 62 * 260 > 12288 > 17 * 72
    common = open(os.path.join(ROOT, "pips_amd", "csrc", "common.h")).read()
    assert int(re.search(r"constexpr int WARP_LDS_BYTES = (\d+);", common).group(1)) == ops.WARP_LDS_BYTES
    m = re.search(r"constexpr int WARP_TILE_W = (\d+), WARP_TILE_H = (\d+);", common)
    assert (int(m.group(1)), int(m.group(2))) == (ops.WARP_TILE_W, ops.WARP_TILE_H)


# ---------------------------------------------------------------------------------------------- the rule, sample by sample
def _pos(m, x, y, chroma):
    if chroma:
        return ((m[0] * (4 * x + 1) + m[1] * (4 * y + 1) + 512 * m[2] - 2 ** 24 + 2 ** 17) >> 18,
                (m[3] * (4 * x + 1) + m[4] * (4 * y + 1) + 512 * m[5] - 2 ** 24 + 2 ** 17) >> 18)
    return (m[0] * x + m[1] * y + 256 * m[2] + 32768) >> 16, (m[3] * x + m[4] * y + 256 * m[5] + 32768) >> 16


def _sample(get, pw, ph, m, x, y, chroma, border, fill):
    U, V = _pos(m, x, y, chroma)
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255

    def tap(xi, yi):
        if border == "replicate":
            return get(min(max(xi, 0), pw - 1), min(max(yi, 0), ph - 1))
        return get(xi, yi) if 0 <= xi < pw and 0 <= yi < ph else fill
    p00, p01, p10, p11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    v = ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16
    assert 0 <= v < 2 ** 11
    ax, ay = fx / 256.0, fy / 256.0                                       # the closed form, exact in float64
    B = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
    assert v == math.floor(B + 0.5)
    return v


def _fill(fmt, fill, matrix, range_):
    rgb = torch.tensor(list(fill), dtype=torch.int64)
    if fmt in YUV:
        return drivers.rgb_to_yuv_torch(rgb, matrix, range_, 10 if fmt in WIDE else 8).tolist()
    return list(fill)[::-1] if fmt in ("bgr24", "bgra32") else list(fill)


def _rule(planes, fmt, coef, border, fill=(0, 0, 0), matrix="bt709", range_="limited"):
    """the rule -> the stored words of every plane as nested lists (16-bit words as 0..65535)"""
    comp = _fill(fmt, fill, matrix, range_)
    vals = [_values(fmt, p).tolist() for p in planes]
    F = len(vals[0])
    shift = 6 if fmt == "p010" else 0
    out = []
    if fmt == "planar8":
        h, w = len(vals[0][0][0]), len(vals[0][0][0][0])
        out.append([[[[_sample(lambda xi, yi: vals[0][f][c][yi][xi], w, h, coef[f], x, y, False, border, comp[c]) for x in range(w)]
                      for y in range(h)] for c in range(3)] for f in range(F)])
        return out
    h, w = len(vals[0][0]), len(vals[0][0][0])
    if fmt not in YUV:
        C = len(vals[0][0][0][0])
        out.append([[[[_sample(lambda xi, yi: vals[0][f][yi][xi][c], w, h, coef[f], x, y, False, border, comp[c]) if c < 3 else 255
                       for c in range(C)] for x in range(w)] for y in range(h)] for f in range(F)])
        return out
    out.append([[[_sample(lambda xi, yi: vals[0][f][yi][xi], w, h, coef[f], x, y, False, border, comp[0]) << shift for x in range(w)]
                 for y in range(h)] for f in range(F)])
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt in SEMI:
        out.append([[[[_sample(lambda xi, yi: vals[1][f][yi][xi][k], cw, ch, coef[f], x, y, True, border, comp[1 + k]) << shift
                       for k in range(2)] for x in range(cw)] for y in range(ch)] for f in range(F)])
    else:
        for k in (1, 2):
            out.append([[[_sample(lambda xi, yi: vals[k][f][yi][xi], cw, ch, coef[f], x, y, True, border, comp[k]) << shift
                          for x in range(cw)] for y in range(ch)] for f in range(F)])
    return out


def _words(p):
    return (p.to(torch.int64) & 0xFFFF).tolist() if p.dtype in (torch.int16, torch.uint16) else p.tolist()


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_twin_is_the_rule_sample_by_sample(fmt, border):
    """7 x 9 and 10 x 13 surfaces (pitched views with junk around them), F = the ten coefficient sets, a row each: every stored word
    equals the plain loop's, and every sample its closed form"""
    for (h, w), seed in (((7, 9), 1), ((10, 13), 2)):
        sets = coefficient_sets(h, w)
        coef = [sets[k] for k in sets]
        _, planes = make_surfaces(fmt, len(coef), h, w, seed=seed, off=1, pad=2 if fmt in WIDE else 3, gap=6)
        before = [p.clone() for p in planes]
        kw = dict(fill=(200, 40, 90), matrix="bt601" if seed == 1 else "bt709", range="full" if seed == 2 else "limited")
        got = _list(drivers.warp_frames_torch(planes, fmt, torch.tensor(coef), border, **kw))
        want = _rule(planes, fmt, coef, border, kw["fill"], kw["matrix"], kw["range"])
        assert len(got) == len(want)
        for a, b, p in zip(got, want, planes):
            assert a.dtype == p.dtype and a.shape == p.shape and _words(a) == b
        assert all(torch.equal(a, b) for a, b in zip(planes, before))


# ---------------------------------------------------------------------------------------------- named cases
def _clean(fmt, planes):
    """16-bit planes with the six unused bits of every word zero (what a warp writes)"""
    if fmt not in WIDE:
        return planes
    keep = 0xFFC0 - 65536 if fmt == "p010" else 1023
    return [p & keep for p in planes]


@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_copies_every_sample_under_both_borders(fmt):
    for h, w in ((7, 9), (10, 13)):
        _, planes = make_surfaces(fmt, 2, h, w, seed=3)
        for border in BORDERS:
            got = _list(drivers.warp_frames_torch(planes, fmt, torch.tensor([IDENTITY] * 2), border, fill=(255, 255, 255)))
            for a, b in zip(got, _clean(fmt, planes)):
                if fmt in ("rgba32", "bgra32"):
                    assert torch.equal(a[..., :3], b[..., :3]) and bool((a[..., 3] == 255).all())
                else:
                    assert torch.equal(a, b)
            if fmt == "p010":
                assert all(not bool((a.to(torch.int64) & 63).any()) for a in got)          # the low six bits of every written word


def _shifted(v, dx, dy, border, fill):
    """v (..., h, w) values: out[y][x] = v[y + dy][x + dx], the fill or the clamped sample outside"""
    h, w = v.shape[-2:]
    ys, xs = torch.arange(h) + dy, torch.arange(w) + dx
    out = v[..., ys.clamp(0, h - 1), :][..., xs.clamp(0, w - 1)]
    if border == "constant":
        inside = ((ys >= 0) & (ys < h)).view(h, 1) & ((xs >= 0) & (xs < w)).view(1, w)
        out = torch.where(inside, out, torch.full_like(out, fill))
    return out


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_integer_shifts_are_shifted_copies(fmt, border):
    """source = output + (3, -2): every full-resolution plane is the shifted copy, the fill (CONSTANT) or the repeated edge
    (REPLICATE) outside; 4:2:0 chroma, which moves by half as many samples, is checked with (4, -2) -> (2, -1)"""
    fill = (200, 40, 90)
    comp = _fill(fmt, fill, "bt709", "limited")
    for h, w in ((7, 9), (10, 13)):
        _, planes = make_surfaces(fmt, 1, h, w, seed=4)
        for dx, dy in ((3, -2), (4, -2)):
            coef = torch.tensor([[ONE, 0, dx << 16, 0, ONE, dy * 65536]])
            got = [_values(fmt, p) for p in _list(drivers.warp_frames_torch(planes, fmt, coef, border, fill=fill))]
            src = [_values(fmt, p) for p in planes]
            if fmt == "planar8":
                for c in range(3):
                    assert torch.equal(got[0][:, c], _shifted(src[0][:, c], dx, dy, border, comp[c]))
            elif fmt not in YUV:
                for c in range(3):
                    assert torch.equal(got[0][..., c], _shifted(src[0][..., c], dx, dy, border, comp[c]))
            else:
                assert torch.equal(got[0], _shifted(src[0], dx, dy, border, comp[0]))
                if dx % 2 == 0:
                    if fmt in SEMI:
                        for k in range(2):
                            assert torch.equal(got[1][..., k], _shifted(src[1][..., k], dx // 2, dy // 2, border, comp[1 + k]))
                    else:
                        for k in (1, 2):
                            assert torch.equal(got[k], _shifted(src[k], dx // 2, dy // 2, border, comp[k]))


@pytest.mark.parametrize("fmt", ("planar8", "nv12", "i010", "bgr24"))
def test_half_pixel_shift_is_the_mean_rounded_half_up(fmt):
    _, planes = make_surfaces(fmt, 1, 7, 9, seed=5)
    got = _values(fmt, _list(drivers.warp_frames_torch(planes, fmt, torch.tensor([[ONE, 0, 1 << 15, 0, ONE, 0]]), "replicate"))[0])
    v = _values(fmt, planes[0])
    v, got = (v, got) if fmt in ("planar8", "nv12", "i010") else (v.permute(0, 3, 1, 2), got.permute(0, 3, 1, 2))
    right = torch.cat([v[..., 1:], v[..., -1:]], dim=-1)
    assert torch.equal(got, (v + right + 1) >> 1)


def test_quarter_turn_of_a_square_image_is_the_exact_rotation():
    n = 11
    _, planes = make_surfaces("planar8", 1, n, n, seed=6)
    coef = drivers.warp_coefficients(torch.tensor([affine_about(n, n, 0.0, -1.0, 1.0, 0.0)], dtype=torch.float64), (n, n))
    assert coef.tolist() == [[0, ONE, 0, -ONE, 0, (n - 1) << 16]]
    for border in BORDERS:
        got = drivers.warp_frames_torch(planes, "planar8", coef, border, fill=(9, 9, 9))
        # output (x, y) shows the source at (y, n - 1 - x)
        assert torch.equal(got, planes[0].transpose(2, 3).flip(3))


@pytest.mark.parametrize("fmt", YUV)
def test_a_grey_fill_is_grey_in_ycbcr(fmt):
    far = torch.tensor([[ONE, 0, 1000 << 16, 0, ONE, 0]])
    mid = 512 if fmt in WIDE else 128
    for matrix in ("bt601", "bt709"):
        for range_ in ("limited", "full"):
            _, planes = make_surfaces(fmt, 1, 7, 9, seed=7)
            got = [_values(fmt, p) for p in drivers.warp_frames_torch(planes, fmt, far, "constant", fill=(77, 77, 77), matrix=matrix, range=range_)]
            Y = drivers.rgb_to_yuv_torch(torch.tensor([77, 77, 77]), matrix, range_, 10 if fmt in WIDE else 8)[0]
            assert bool((got[0] == Y).all()) and all(bool((c == mid).all()) for c in got[1:])


@pytest.mark.parametrize("fmt", FORMATS)
def test_coefficients_at_the_int32_extremes_land_outside(fmt):
    h, w = 7, 9
    sets = coefficient_sets(h, w)
    coef = torch.tensor([sets["extreme_a"], sets["extreme_b"]])
    _, planes = make_surfaces(fmt, 2, h, w, seed=8)
    fill = (200, 40, 90)
    filled = _list(drivers.warp_frames_torch(planes, fmt, coef, "constant", fill=fill))
    far = _list(drivers.warp_frames_torch(planes, fmt, torch.tensor([[ONE, 0, 30000 << 16, 0, ONE, 0]] * 2), "constant", fill=fill))
    assert all(torch.equal(a, b) for a, b in zip(filled, far))                             # nothing but the fill
    assert len(set(filled[0][0].reshape(-1, filled[0].shape[-1] if fmt not in YUV and fmt != "planar8" else 1).sum(1).tolist())) <= 3
    got = _list(drivers.warp_frames_torch(planes, fmt, coef, "replicate"))
    for a, p in zip(got, _clean(fmt, planes)):
        if fmt == "planar8":
            a, p = a.permute(0, 2, 3, 1), p.permute(0, 2, 3, 1)                            # a pixel's samples last
        if fmt in ("rgba32", "bgra32"):
            a, p = a[..., :3], p[..., :3]
        a, p = (a, p) if a.dim() == 4 else (a.unsqueeze(-1), p.unsqueeze(-1))
        corners = torch.stack([p[:, 0, 0], p[:, 0, -1], p[:, -1, 0], p[:, -1, -1]], dim=1)              # (F,4,C)
        hit = (a.unsqueeze(3) == corners.view(a.shape[0], 1, 1, 4, -1)).all(dim=-1).any(dim=-1)
        assert bool(hit.all())                                                             # every pixel is one of the four corners


def test_negative_positions_round_half_up_through_the_arithmetic_shift():
    m = [ONE, 0, -(1 << 15), 0, ONE, 0]
    assert _pos(m, 0, 0, False) == (-128, 0) and (-128 >> 8, -128 & 255) == (-1, 128)
    assert _pos([ONE, 0, -(1 << 15) - 1, 0, ONE, 0], 0, 0, False)[0] == -129 + 1           # (-2^23 - 256 + 2^15) >> 16: half up
    _, planes = make_surfaces("planar8", 1, 7, 9, seed=9)
    got = drivers.warp_frames_torch(planes, "planar8", torch.tensor([m]), "constant", fill=(201, 201, 201)).to(torch.int64)
    v = planes[0].to(torch.int64)
    assert torch.equal(got[..., 0], (201 + v[..., 0] + 1) >> 1) and torch.equal(got[..., 1:], (v[..., :-1] + v[..., 1:] + 1) >> 1)
    up = drivers.warp_frames_torch(planes, "planar8", torch.tensor([[ONE, 0, 0, 0, ONE, -(1 << 15)]]), "replicate").to(torch.int64)
    assert torch.equal(up[..., 0, :], v[..., 0, :]) and torch.equal(up[..., 1:, :], (v[..., :-1, :] + v[..., 1:, :] + 1) >> 1)


def test_twin_rejects_what_the_library_rejects():
    _, planes = make_surfaces("nv12", 2, 7, 9, seed=10)
    ident = torch.tensor([IDENTITY] * 2)
    for bad in (dict(border="wrap"), dict(fill=(0, 0, 256)), dict(fill=(0, 0)), dict(fill=(0.5, 0, 0)), dict(matrix="bt2020"),
                dict(range="tv")):
        with pytest.raises(ValueError):
            drivers.warp_frames_torch(planes, "nv12", ident, **bad)
    for coef in (ident[:1], ident.double(), torch.zeros(2, 5, dtype=torch.int32), torch.full((2, 6), 2 ** 31, dtype=torch.int64)):
        with pytest.raises(ValueError):
            drivers.warp_frames_torch(planes, "nv12", coef)
    with pytest.raises(ValueError):
        drivers.warp_frames_torch(planes, "yuy2", ident)
    with pytest.raises(ValueError):
        drivers.warp_frames_torch(planes[:1], "nv12", ident)


# ---------------------------------------------------------------------------------------------- warp_coefficients
def _exact_rows(t, size, surface, zoom):
    """the same composition in fractions.Fraction: rows 0 and 1 of the 3 x 3 product"""
    (H, W), (h, w) = size, surface
    a, b, c, d, e, f = (Fraction(v) for v in t)
    sx, sy, z = Fraction(w, W), Fraction(h, H), 1 / Fraction(zoom)
    cx, cy = Fraction(w - 1, 2), Fraction(h - 1, 2)

    def mul(A, B):
        return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    last = [Fraction(0), Fraction(0), Fraction(1)]
    Z = [[z, 0, cx - cx * z], [0, z, cy - cy * z], last]
    S1 = [[1 / sx, 0, Fraction(1, 2) / sx - Fraction(1, 2)], [0, 1 / sy, Fraction(1, 2) / sy - Fraction(1, 2)], last]
    det = a * e - b * d
    inv = [[e / det, -b / det, (b * f - e * c) / det], [-d / det, a / det, (d * c - a * f) / det], last]
    S4 = [[sx, 0, sx / 2 - Fraction(1, 2)], [0, sy, sy / 2 - Fraction(1, 2)], last]
    M = mul(S4, mul(inv, mul(S1, Z)))
    return [M[0][0] * 2 ** 24, M[0][1] * 2 ** 24, M[0][2] * 2 ** 16, M[1][0] * 2 ** 24, M[1][1] * 2 ** 24, M[1][2] * 2 ** 16]


def test_coefficients_are_the_exact_composition_within_one_unit():
    g = torch.Generator().manual_seed(11)
    for size, surface, zoom in (((64, 96), (64, 96), 1.0), ((64, 96), (128, 192), 1.1), ((64, 96), (100, 192), 1.1), ((368, 496), (1080, 1920), 0.9)):
        t = torch.randn(6, 6, generator=g, dtype=torch.float64) * torch.tensor([0.1, 0.1, 9.0, 0.1, 0.1, 9.0], dtype=torch.float64)
        t[:, 0] += 1.0
        t[:, 4] += 1.0
        got = drivers.warp_coefficients(t, size, surface, zoom)
        assert got.dtype == torch.int32 and tuple(got.shape) == (6, 6) and got.device.type == "cpu"
        for row, q in zip(t.tolist(), got.tolist()):
            assert all(abs(Fraction(a) - b) <= 1 for a, b in zip(q, _exact_rows(row, size, surface, zoom)))
    # the identity on its own size is the identity; on a larger surface too
    assert drivers.warp_coefficients(torch.tensor([[1.0, 0.0, 0.0, 0.0]]), (64, 96)).tolist() == [IDENTITY]
    assert drivers.warp_coefficients(torch.tensor([[1.0, 0.0, 0.0, 0.0]]), (64, 96), (128, 192)).tolist() == [IDENTITY]
    assert drivers.warp_coefficients(torch.zeros(0, 4), (64, 96)).shape == (0, 6)


def test_similarity_and_affine_rows_agree():
    g = torch.Generator().manual_seed(12)
    s = torch.randn(5, 4, generator=g, dtype=torch.float64) * torch.tensor([0.1, 0.1, 9.0, 9.0], dtype=torch.float64)
    s[:, 0] += 1.0
    aff = torch.stack([s[:, 0], -s[:, 1], s[:, 2], s[:, 1], s[:, 0], s[:, 3]], dim=1)
    for surface, zoom in ((None, 1.0), ((100, 192), 1.25)):
        assert torch.equal(drivers.warp_coefficients(s, (64, 96), surface, zoom), drivers.warp_coefficients(aff, (64, 96), surface, zoom))


def test_coefficients_reject_what_cannot_be_a_row():
    ok = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    for bad in ([1.0, 2.0, 0.0, 2.0, 4.0, 0.0], [0.0] * 6, [float("nan")] + ok[1:], ok[:2] + [float("inf")] + ok[3:],
                [1.0 / 200.0, 0.0, 0.0, 0.0, 1.0, 0.0],                     # the inverse has a linear term of 200
                [1.0, 0.0, 40000.0, 0.0, 1.0, 0.0]):                        # ... an offset of -40000 px
        with pytest.raises(ValueError):
            drivers.warp_coefficients(torch.tensor([bad], dtype=torch.float64), (64, 96))
    for zoom in (0.0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            drivers.warp_coefficients(torch.tensor([ok], dtype=torch.float64), (64, 96), zoom=zoom)
    with pytest.raises(ValueError):
        drivers.warp_coefficients(torch.zeros(2, 5), (64, 96))
    with pytest.raises(ValueError):
        drivers.warp_coefficients(torch.tensor([ok]), (0, 96))
    # just inside the limits: a linear term of 127.99, an offset of 32767 px
    drivers.warp_coefficients(torch.tensor([[1.0 / 127.99, 0.0, 0.0, 0.0, 1.0, -32767.0]], dtype=torch.float64), (64, 96))


# ---------------------------------------------------------------------------------------------- motion_smooth
def _random_path(P, seed):
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.1
    sc = 1.0 + (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.06
    models = torch.stack([sc * torch.cos(ang), sc * torch.sin(ang), torch.randn(P, generator=g, dtype=torch.float64) * 4.0,
                          torch.randn(P, generator=g, dtype=torch.float64) * 4.0], dim=1)
    return drivers.motion_path(models)


def test_smooth_without_a_radius_and_with_radius_zero():
    path = _random_path(12, 13)
    assert _f64_bits(drivers.motion_smooth(path, None)) == _f64_bits(path)
    still = drivers.motion_smooth(path, 0)
    assert tuple(still.shape) == (13, 4) and still.dtype == torch.float64
    assert torch.allclose(still, torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand(13, 4), rtol=0.0, atol=1e-12)
    assert drivers.motion_smooth(torch.zeros(0, 4), 3).shape == (0, 4)
    for bad in (-1, 2.5, True, float("nan")):
        with pytest.raises(ValueError):
            drivers.motion_smooth(path, bad)
    with pytest.raises(ValueError):
        drivers.motion_smooth(torch.zeros(3, 3), 2)
    with pytest.raises(ValueError):
        drivers.motion_smooth(torch.zeros(3, 4), 2)                                         # A = 0 has no logarithm
    assert drivers.motion_smooth(path, 3.0).shape == (13, 4)                               # a whole number


def test_a_steady_pan_needs_no_correction_away_from_the_ends():
    F, r = 30, 4
    path = drivers.motion_path(torch.tensor([[1.0, 0.0, 2.5, -1.25]] * (F - 1), dtype=torch.float64))
    W = drivers.motion_smooth(path, r)
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    assert torch.allclose(W[r:F - r], ident.expand(F - 2 * r, 4), rtol=0.0, atol=1e-9)
    assert float((W[0] - ident).abs().max()) > 1.0                                         # the clamped windows at the ends do correct


def test_theta_is_unwrapped_across_pi():
    """a camera that turns 0.3 rad a frame passes +-pi: the smoothed angle follows it, so the correction stays a small rotation"""
    F, r = 40, 3
    a = complex(math.cos(0.3), math.sin(0.3))
    path = drivers.motion_path(torch.tensor([[a.real, a.imag, 0.0, 0.0]] * (F - 1), dtype=torch.float64))
    ang = torch.atan2(path[:, 1], path[:, 0])
    assert bool(((ang[1:] - ang[:-1]).abs() > 3.0).any())                                  # the principal value does jump
    W = drivers.motion_smooth(path, r)
    assert torch.allclose(W[r:F - r], torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand(F - 2 * r, 4), rtol=0.0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- Stabilizer
@pytest.mark.parametrize("radius", [None, 0, 2, 50])
def test_stabilizer_push_by_push_is_the_one_shot_smoothing(radius):
    """T = 19, 40 identities that come and go, pushes of 3 rows with the identities alive in them: the corrections handed back,
    concatenated, are motion_smooth(motion_path(motion_fit_torch(the whole video)), radius) in every bit; a frame comes back once
    frame + radius has been seen"""
    T, K = 19, 40
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5)
    models = drivers.motion_fit_torch(trajs[None], vis[None], ids=torch.arange(K), **kw)[0]
    want = drivers.motion_smooth(drivers.motion_path(models), radius)
    assert tuple(want.shape) == (T, 4)
    st = drivers.Stabilizer(radius=radius, engine="torch", **kw)
    assert st.step(0, trajs[None][:, :0, :0])[1].shape == (0, 4)                            # a push without rows
    got, done = [], 0
    for f0 in range(0, T, 3):
        f1 = min(f0 + 3, T)
        ids = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
        g0, rows = st.step(f0, trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids], ids=ids)
        assert g0 == done and rows.dtype == torch.float64 and rows.shape[1] == 4
        done += rows.shape[0]
        assert done == (f1 if radius is None else max(f1 - radius, 0))
        got.append(rows)
    g0, rows = st.finish()
    assert g0 == done and done + rows.shape[0] == T
    got.append(rows)
    assert _f64_bits(torch.cat(got)) == _f64_bits(want)
    assert st.finish()[1].shape == (0, 4)
    with pytest.raises(ValueError):
        drivers.Stabilizer(radius=-1, engine="torch")
    with pytest.raises(ValueError):
        drivers.Stabilizer(engine="cpu")
    with pytest.raises(ValueError):
        drivers.Stabilizer(engine="torch", trail=3)


# ---------------------------------------------------------------------------------------------- end to end
def test_a_shaken_ramp_is_held_still_within_two_levels():
    """Frame 0 is a 96 x 128 planar8 ramp whose gradient is at most one level a pixel (|gx| + |gy| <= 1); frames 1..5 are made from
    it by the twin under known similarities (scale 0.95..1.05, |rotation| <= 3 degrees, |shift| <= 6 px) and 200 tracks move by the
    same similarities exactly.  Stabilizer(radius=None) and a second resampling bring every frame back onto frame 0: inside the
    region that every frame covers the difference is at most 2 levels -- 0.5 from rounding frame 0, 0.5 from each of the two
    resamplings, at most 0.26 from the quarter-pixel quantisation of the tracks and the 1/256 px position grid at gradient 1: under
    1.8, so a difference of 1 is expected and 2 is the cap."""
    H, W = 96, 128
    y, x = torch.arange(H, dtype=torch.float64).view(H, 1), torch.arange(W, dtype=torch.float64).view(1, W)
    ramp = 30.0 + 0.4 * x + 0.3 * y + 4.0 * torch.sin(x / 40.0) + 3.0 * torch.cos(y / 30.0)
    assert float((ramp[:, 1:] - ramp[:, :-1]).abs().max() + (ramp[1:] - ramp[:-1]).abs().max()) <= 1.0 and 0 < float(ramp.min()) and float(ramp.max()) < 255
    frame0 = torch.floor(ramp + 0.5).to(torch.uint8).expand(3, H, W).contiguous()[None]             # (1,3,H,W)
    sims = [(1.0, 0.0, 0.0, 0.0), (1.03, 2.0, 4.0, -3.0), (0.96, -3.0, -6.0, 2.5), (1.05, 1.0, 5.5, 6.0), (0.95, -1.5, -2.0, -5.0),
            (1.0, 3.0, 3.0, 1.0)]                                                          # (scale, degrees, shift x, shift y): frame 0 -> f
    assert all(0.95 <= s <= 1.05 and abs(d) <= 3.0 and abs(tx) <= 6.0 and abs(ty) <= 6.0 for s, d, tx, ty in sims)
    fwd = []
    for s, d, tx, ty in sims:
        c, sn = s * math.cos(math.radians(d)), s * math.sin(math.radians(d))
        cx, cy = (W - 1) / 2, (H - 1) / 2
        fwd.append([c, sn, cx - (c * cx - sn * cy) + tx, cy - (sn * cx + c * cy) + ty])                 # about the centre
    fwd = torch.tensor(fwd, dtype=torch.float64)
    coef = drivers.warp_coefficients(fwd, (H, W))
    six = frame0.expand(6, 3, H, W).contiguous()
    white = torch.full_like(six, 255)
    frames = drivers.warp_frames_torch(six, "planar8", coef, "constant")
    seen = drivers.warp_frames_torch(white, "planar8", coef, "constant")
    assert torch.equal(frames[0], frame0[0])
    g = torch.Generator().manual_seed(14)
    p = torch.rand(200, 2, generator=g, dtype=torch.float64) * torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    rows = torch.stack([torch.stack([a[0] * p[:, 0] - a[1] * p[:, 1] + a[2], a[1] * p[:, 0] + a[0] * p[:, 1] + a[3]], dim=1) for a in fwd])
    st = drivers.Stabilizer(radius=None, engine="torch")
    g0, corr = st.step(0, rows.float()[None])
    assert g0 == 0 and tuple(corr.shape) == (6, 4) and st.finish()[1].shape == (0, 4)
    back = drivers.warp_coefficients(corr, (H, W))
    still = drivers.warp_frames_torch(frames, "planar8", back, "constant")
    covered = (drivers.warp_frames_torch(seen, "planar8", back, "constant") == 255).all(dim=1).all(dim=0)      # (H,W)
    assert float(covered.float().mean()) > 0.6
    diff = (still.to(torch.int64) - frame0.to(torch.int64)).abs()[:, :, covered]
    print(f"stabilised ramp: {float(covered.float().mean()):.1%} covered by all six frames, max |diff| = {int(diff.max())}, "
          f"mean |diff| = {float(diff.float().mean()):.3f}")
    assert int(diff.max()) <= 2


# ---------------------------------------------------------------------------------------------- the ABI
def test_frames_warp_is_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_frames_warp" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)      # the history comment
    for words in ("U = (X + 32768) >> 16", "XL = m0 (4 cx + 1) + m1 (4 cy + 1) + 512 m2", "Uc = (XL - 2^24 + 2^17) >> 18",
                  "v = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16", "12288 bytes",
                  "bilinear only", "alpha is not resampled", "chroma siting is not"):
        assert words in hdr, words                                         # the rule stands in the header
    assert int(re.search(r"#define PIPS_WARP_DIM_MAX\s+(\d+)", hdr).group(1)) == ops.WARP_DIM_MAX
    for name, value in ops.WARP_BORDERS.items():
        assert int(re.search(rf"#define PIPS_WARP_BORDER_{name.upper()}\s+(\d+)", hdr).group(1)) == value
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_frames_warp\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 28
    res, args = _lib.SIGNATURES["pips_frames_warp"]
    assert res is ctypes.c_int and len(args) == 28 and args[:8] == [ctypes.c_int] * 8 and args[9] is ctypes.c_size_t
    assert "warp.hip" in _build.SOURCES and any(h.endswith("yuv.h") for h in _build.headers())
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_frames_warp") and callable(ops.warp_frames)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the host-side rejections need no device: nothing is launched

    def call(fmt=4, matrix=1, range_=0, border=0, fill=0, F=0, h=8, w=8, pitch=8):
        surf = [None, pitch, 0, None, pitch, 0, None, 0, 0]
        return lib.pips_frames_warp(fmt, matrix, range_, border, fill, F, h, w, *surf, *surf, None, None)

    assert call() == 0                                                     # F = 0 launches nothing
    for bad in (dict(fmt=9), dict(fmt=-1), dict(border=2), dict(matrix=2), dict(range_=-1), dict(fill=-1), dict(fill=1 << 24), dict(F=-1),
                dict(h=0), dict(w=8193), dict(pitch=7), dict(F=1)):
        assert call(**bad) == -1, bad
        assert lib.pips_last_error().decode().startswith("frames_warp:"), bad
    assert call(fmt=0, matrix=7, range_=7, pitch=24) == 0                  # matrix and range are looked at for YCbCr alone
