"""CPU: the border of stabilised frames filled from neighbouring frames -- drivers.warp_frames_fill_torch (the rule of
pips_frames_warp_fill, include/pips_hip.h) held to plain Python loops over the rule's points, to drivers.warp_frames_torch at K = 1,
and to named boundary cases; fill_candidates, Stabilizer.candidates and crop_zoom; a planted mosaic end to end; the ABI.  The
candidate tables of tests/test_warp_fill_gpu.py are made here and shown not to be vacuous: every covering candidate supplies
samples, some frames leave samples uncovered and some none, and the tiles lie on both sides of the kernel's fast path.  Surfaces
and coefficient sets come from tests/test_warp.py."""
import ctypes
import math
import os
import re

import pytest
import torch

from pips_amd import drivers, ops
from test_motion import _f64_bits, _life_video
from test_seams import FRAME_SIZE, PERIOD, WARP_BORDER, WARP_FILL, periodic, periodic_index
from test_warp import (BORDERS, FORMATS, IDENTITY, ONE, SEMI, WIDE, YUV, _fill, _list, _pos, _sample, _values, coefficient_sets,
                       make_surfaces)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 255
FILL = (200, 40, 90)


# ---------------------------------------------------------------------------------------------- the rule, sample by sample
def channels(fmt, planes):
    """the surfaces as single-component planes: [(values (F,ph,pw) int64, chroma, index of the fill component, is plane 0)]"""
    v = [_values(fmt, p) for p in planes]
    if fmt == "planar8":
        return [(v[0][:, c], False, c, c == 0) for c in range(3)]
    if fmt in SEMI:
        return [(v[0], False, 0, True), (v[1][..., 0], True, 1, False), (v[1][..., 1], True, 2, False)]
    if fmt in YUV:
        return [(v[0], False, 0, True), (v[1], True, 1, False), (v[2], True, 2, False)]
    return [(v[0][..., c], False, c, c == 0) for c in range(3)]


def covers(m, x, y, pw, ph, chroma):
    """rule point 3 on Python ints"""
    U, V = _pos(m, x, y, chroma)
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
    return x0 >= 0 and (x0 + 1 <= pw - 1 or (fx == 0 and x0 <= pw - 1)) and y0 >= 0 and (y0 + 1 <= ph - 1 or (fy == 0 and y0 <= ph - 1))


def rule_sample(src, Fs, pw, ph, cands, rows, x, y, chroma, border, fill):
    """rule points 1-4 for one sample of one single-component plane: src[f][yi][xi] -> (value, list position or 255)"""
    for k, (c, m) in enumerate(zip(cands, rows)):
        if 0 <= c < Fs and covers(m, x, y, pw, ph, chroma):
            U, V = _pos(m, x, y, chroma)
            x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
            taps = ((x0, y0, (256 - fx) * (256 - fy)), (x0 + 1, y0, fx * (256 - fy)), (x0, y0 + 1, (256 - fx) * fy), (x0 + 1, y0 + 1, fx * fy))
            assert all(0 <= xi < pw and 0 <= yi < ph for xi, yi, wgt in taps if wgt)         # every tap that has weight lies inside
            return (sum(wgt * src[c][yi][xi] for xi, yi, wgt in taps if wgt) + 32768) >> 16, k
    if 0 <= cands[0] < Fs:
        return _sample(lambda xi, yi: src[cands[0]][yi][xi], pw, ph, rows[0], x, y, chroma, border, fill), NONE
    return fill, NONE


def rule(planes, fmt, cand, coef, border, fill=FILL, matrix="bt709", range_="limited"):
    """-> (values of every channel of channels() as (Fd,ph,pw) nested lists, the map (Fd,h,w) as nested lists)"""
    comp = _fill(fmt, fill, matrix, range_)
    out, smap = [], None
    for vals, chroma, ci, first in channels(fmt, planes):
        Fs, ph, pw = vals.shape
        src = vals.tolist()
        got = [[[rule_sample(src, Fs, pw, ph, cand[j], coef[j], x, y, chroma, border, comp[ci]) for x in range(pw)] for y in range(ph)]
               for j in range(len(cand))]
        out.append([[[s[0] for s in row] for row in fr] for fr in got])
        if first:
            smap = [[[s[1] for s in row] for row in fr] for fr in got]
    return out, smap


def small_tables(h, w):
    """K = 3, Fs = 3, Fd = 2: a shift, a candidate >= Fs and a turn; an invalid candidate 0, half a sample off and an extreme row"""
    sets = coefficient_sets(h, w)
    shift = [ONE, 0, int(1.25 * 65536), 0, ONE, -int(0.5 * 65536)]
    half = [ONE, 0, -(1 << 15), 0, ONE, 1 << 15]
    return [[1, 5, 0], [-1, 2, 0]], [[shift, IDENTITY, sets["rot2"]], [sets["shear"], half, sets["extreme_a"]]]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_twin_is_the_rule_sample_by_sample(fmt, border):
    for (h, w), seed in (((5, 7), 1), ((17, 33), 2)):
        cand, coef = small_tables(h, w)
        _, planes = make_surfaces(fmt, 3, h, w, seed=seed, off=1, pad=2 if fmt in WIDE else 3, gap=6)
        before = [p.clone() for p in planes]
        kw = dict(fill=FILL, matrix="bt601" if seed == 1 else "bt709", range="full" if seed == 2 else "limited")
        got, smap = drivers.warp_frames_fill_torch(planes, fmt, torch.tensor(cand), torch.tensor(coef), border, source=True, **kw)
        got = _list(got)
        want, wmap = rule(planes, fmt, cand, coef, border, kw["fill"], kw["matrix"], kw["range"])
        assert [c[0].tolist() for c in channels(fmt, got)] == want and smap.tolist() == wmap and smap.dtype == torch.uint8
        assert all(a.dtype == p.dtype and a.shape[1:] == p.shape[1:] and a.shape[0] == 2 for a, p in zip(got, planes))
        if fmt in ("rgba32", "bgra32"):
            assert bool((got[0][..., 3] == 255).all())
        if fmt == "p010":
            assert all(not bool((a.to(torch.int64) & 63).any()) for a in got)
        assert all(torch.equal(a, b) for a, b in zip(planes, before))
        assert {0, 2, NONE} <= set(smap[0].unique().tolist()) or (h, w) == (5, 7)
        assert set(smap[1].unique().tolist()) == {1, NONE}
        without = _list(drivers.warp_frames_fill_torch(planes, fmt, torch.tensor(cand), torch.tensor(coef), border, **kw))
        assert all(torch.equal(a, b) for a, b in zip(without, got))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_candidate_per_frame_is_warp_frames(fmt, border):
    """K = 1 with cand = arange(F): pips_frames_warp's twin byte for byte, on all ten coefficient sets"""
    for (h, w), seed in (((7, 9), 3), ((10, 13), 4)):
        sets = coefficient_sets(h, w)
        coef = torch.tensor([sets[k] for k in sets])
        F = coef.shape[0]
        _, planes = make_surfaces(fmt, F, h, w, seed=seed, off=1, pad=2, gap=6)
        want = _list(drivers.warp_frames_torch(planes, fmt, coef, border, fill=FILL))
        got, smap = drivers.warp_frames_fill_torch(planes, fmt, torch.arange(F).view(F, 1), coef.view(F, 1, 6), border, fill=FILL, source=True)
        assert all(torch.equal(a, b) for a, b in zip(_list(got), want))
        assert set(smap.unique().tolist()) <= {0, NONE} and bool((smap[0] == 0).all())


# ---------------------------------------------------------------------------------------------- boundary and validity
def _plain(fmt, planes):
    """what a warp writes for a copied sample: unused bits of 16-bit words zero, alpha 255"""
    if fmt in WIDE:
        keep = 0xFFC0 - 65536 if fmt == "p010" else 1023
        return [p & keep for p in planes]
    if fmt in ("rgba32", "bgra32"):
        out = planes[0].clone()
        out[..., 3] = 255
        return [out]
    return [p.clone() for p in planes]


@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_as_candidate_zero_copies_every_sample(fmt):
    for h, w in ((7, 9), (10, 13)):
        _, planes = make_surfaces(fmt, 2, h, w, seed=5)
        cand, coef = torch.tensor([[1, 0], [0, 1]]), torch.tensor([[IDENTITY, coefficient_sets(h, w)["rot2"]]] * 2)
        for border in BORDERS:
            got, smap = drivers.warp_frames_fill_torch(planes, fmt, cand, coef, border, fill=(255, 255, 255), source=True)
            assert bool((smap == 0).all())
            for a, b in zip(_list(got), _plain(fmt, planes)):
                assert torch.equal(a, b.flip(0))


def test_an_integer_shift_covers_exactly_the_shifted_rectangle():
    """source = output + (3, -2) and output + (-3, 2) on 10 x 13: exactly the samples whose source lies in the image are covered --
    the edge row and column, where fx = fy = 0 and the second tap has no weight, included.  One unit of 1/256 px further out
    that edge is not covered (its second tap has weight and lies outside); one unit further in, the opposite edge is not"""
    h, w = 10, 13
    _, planes = make_surfaces("planar8", 1, h, w, seed=6)

    def axis(n, shift, extra):
        pos = torch.arange(n) + shift                                           # the first tap at extra = 0
        if extra == 0:
            return (pos >= 0) & (pos <= n - 1)
        return (pos >= 0) & (pos + 1 <= n - 1) if extra > 0 else (pos - 1 >= 0) & (pos <= n - 1)
    for dx, dy in ((3, -2), (-3, 2)):
        for ex, ey in ((0, 0), (256, 0), (0, 256), (-256, 0), (0, -256), (256, -256)):              # 256 units of m2 are 1/256 px
            row = [ONE, 0, dx * 65536 + ex, 0, ONE, dy * 65536 + ey]
            smap = drivers.warp_frames_fill_torch(planes, "planar8", torch.tensor([[0]]), torch.tensor([[row]]), "constant", source=True)[1][0]
            want = axis(h, dy, ey).view(h, 1) & axis(w, dx, ex).view(1, w)
            assert torch.equal(smap == 0, want) and torch.equal(smap == NONE, ~want), (dx, dy, ex, ey)
            assert torch.equal(drivers._warp_covers(h, w, row, False), want)
            assert 0 < int(want.sum()) <= (h - 2) * (w - 3) and (int(want.sum()) == (h - 2) * (w - 3)) == (ex == ey == 0 or (dx * ex <= 0 and dy * ey <= 0))
    got = drivers.warp_frames_fill_torch(planes, "planar8", torch.tensor([[0]]), torch.tensor([[[ONE, 0, 3 << 16, 0, ONE, -(2 << 16)]]]), "constant",
                                         fill=(9, 9, 9))
    assert torch.equal(got[0, :, 2:, :w - 3], planes[0][0, :, :h - 2, 3:]) and bool((got[0, :, :2] == 9).all()) and bool((got[0, :, :, w - 3:] == 9).all())


@pytest.mark.parametrize("fmt", ("nv12", "rgb24", "i010", "planar8"))
def test_extreme_rows_cover_nothing_and_invalid_candidates_are_skipped(fmt):
    h, w = 7, 9
    sets = coefficient_sets(h, w)
    _, planes = make_surfaces(fmt, 2, h, w, seed=7)
    for border in BORDERS:
        # the extremes cover nothing, -1 and an index >= Fs are skipped: the identity behind them supplies every sample
        cand = torch.tensor([[0, -1, 2, 1, 1]])
        coef = torch.tensor([[sets["extreme_a"], IDENTITY, IDENTITY, sets["extreme_b"], IDENTITY]])
        got, smap = drivers.warp_frames_fill_torch(planes, fmt, cand, coef, border, fill=FILL, source=True)
        assert bool((smap == 4).all()) and all(torch.equal(a[0], b[1]) for a, b in zip(_list(got), _plain(fmt, planes)))
        assert not drivers._warp_covers(h, w, sets["extreme_a"], False).any() and not drivers._warp_covers(4, 5, sets["extreme_b"], True).any()
        # nothing covers: candidate 0 under the border rule, pips_frames_warp's bytes
        got, smap = drivers.warp_frames_fill_torch(planes, fmt, cand[:, :4], coef[:, :4], border, fill=FILL, source=True)
        want = _list(drivers.warp_frames_torch([p[:1] for p in planes], fmt, coef[:, 0], border, fill=FILL))
        assert bool((smap == NONE).all()) and all(torch.equal(a, b) for a, b in zip(_list(got), want))
        # an invalid candidate 0 and nothing covering: the fill, whatever the border
        for c0 in (-1, 2, -2 ** 31, 2 ** 31 - 1):
            got, smap = drivers.warp_frames_fill_torch(planes, fmt, torch.tensor([[c0, 1]]), torch.tensor([[IDENTITY, sets["extreme_a"]]]), border,
                                                       fill=FILL, source=True)
            far = _list(drivers.warp_frames_torch([p[:1] for p in planes], fmt, torch.tensor([[ONE, 0, 30000 << 16, 0, ONE, 0]]), "constant", fill=FILL))
            assert bool((smap == NONE).all()) and all(torch.equal(a, b) for a, b in zip(_list(got), far))
    # no source frame at all: every candidate is invalid
    got = _list(drivers.warp_frames_fill_torch([p[:0] for p in planes], fmt, torch.tensor([[0, 1]]), torch.tensor([[IDENTITY, IDENTITY]]), fill=FILL))
    assert all(torch.equal(a, b) for a, b in zip(got, far))


def test_the_twin_rejects_what_the_library_rejects():
    _, planes = make_surfaces("nv12", 2, 7, 9, seed=8)
    cand, coef = torch.tensor([[0, 1]] * 3), torch.tensor([[IDENTITY, IDENTITY]] * 3)
    assert drivers.warp_frames_fill_torch(planes, "nv12", cand, coef)[0].shape == (3, 7, 9)
    for bad in (dict(border="wrap"), dict(fill=(0, 0, 256)), dict(matrix="bt2020"), dict(range="tv")):
        with pytest.raises(ValueError):
            drivers.warp_frames_fill_torch(planes, "nv12", cand, coef, **bad)
    for c, m in ((cand[:2], coef), (cand.double(), coef), (cand, coef.double()), (cand, coef[:, :1]), (cand[:, :0], coef[:, :0]),
                 (torch.zeros(3, 17, dtype=torch.int64), torch.zeros(3, 17, 6, dtype=torch.int64)), (cand.view(-1), coef),
                 (cand, torch.full((3, 2, 6), 2 ** 31, dtype=torch.int64)), (torch.full((3, 2), 2 ** 31, dtype=torch.int64), coef)):
        with pytest.raises(ValueError):
            drivers.warp_frames_fill_torch(planes, "nv12", c, m)
    assert ops.WARP_FILL_MAX == 16 and ops.WARP_FILL_NONE == NONE
    assert _list(drivers.warp_frames_fill_torch(planes, "nv12", cand[:0], coef[:0]))[0].shape == (0, 7, 9)


# ---------------------------------------------------------------------------------------------- the tables of the GPU test
GPU_SHAPES = ((1, 1), (15, 63), (17, 65), (33, 130))
GPU_FS, GPU_FD = 5, 3
BIG = (80, 300)


def _frac_shifts():
    """two fractional shifts that leave the image through opposite sides: the first uncovers the right and the top, the second the
    left and the bottom"""
    return ([ONE, 0, int(5.3 * 65536), 0, ONE, -int(2.6 * 65536)], [ONE, 0, -int(4.7 * 65536), 0, ONE, int(3.2 * 65536)])


def gpu_tables(h, w):
    """cand (3,4) and coef (3,4,6) for Fs = 5: frame 0 -- two fractional shifts out of opposite sides, an extreme row in the middle of
    the list, the first source frame again under a turn; frame 1 -- a shift, an empty slot, four source pixels a pixel (taps from
    global memory as a later candidate) and a trailing quarter scale that covers whatever is left; frame 2 -- four source pixels a
    pixel as candidate 0, the two shifts from one source frame each, an index >= Fs.  K = 1, 2, 4 take the first K slots."""
    sets = coefficient_sets(h, w)
    left, right = _frac_shifts()
    cand = [[0, 3, 1, 0], [2, -1, 4, 1], [4, 4, 2, 7]]
    coef = [[left, right, sets["extreme_a"], sets["rot2"]], [right, IDENTITY, sets["scale4"], sets["scale_quarter"]],
            [sets["scale4"], right, left, IDENTITY]]
    return cand, coef


GPU_SUPPLIERS = [[0, 1, 3], [0, 2, 3], [0, 1, 2]]                     # the slots of gpu_tables that supply samples, per frame


def big_tables():
    """80 x 300, K = 3: frame 0 -- a turn whose interior tiles take the fast path beside edge tiles that walk to the shifts; frame 1
    -- four source pixels a pixel as candidate 0 (its first tile on the fast path with taps from global memory), a turn, a quarter
    scale; frame 2 -- a shift, four source pixels a pixel as a LATER candidate, a turn"""
    h, w = BIG
    sets = coefficient_sets(h, w)
    left, right = _frac_shifts()
    four = [ONE << 2, 0, 1 << 16, 0, ONE << 2, 2 << 16]
    return [[1, 0, 3], [2, 4, 0], [3, 1, 2]], [[sets["rot2"], left, right], [four, sets["rot2"], sets["scale_quarter"]], [left, sets["scale4"], sets["rot2"]]]


def tile_fast(row, fmt, h, w, x0, y0):
    """the kernel's fast-path test, restated on Python ints like ops.warp_staged: the tap box of the tile's four corners under
    ``row``, the +1 tap added, lies inside every plane of ``fmt`` (candidate 0 is taken to be valid)"""
    def inside(chroma, tx, ty, tw, th, pw, ph):
        pts = [_pos(row, x, y, chroma) for x, y in ((tx, ty), (tx + tw - 1, ty), (tx, ty + th - 1), (tx + tw - 1, ty + th - 1))]
        us, vs = [p[0] >> 8 for p in pts], [p[1] >> 8 for p in pts]
        return min(us) >= 0 and min(vs) >= 0 and max(us) + 1 < pw and max(vs) + 1 < ph
    ok = inside(False, x0, y0, ops.WARP_TILE_W, ops.WARP_TILE_H, w, h)
    if fmt in YUV:
        ok = ok and inside(True, x0 // 2, y0 // 2, ops.WARP_TILE_W // 2, ops.WARP_TILE_H // 2, (w + 1) // 2, (h + 1) // 2)
    return ok


def _chroma_counts(h, w, Fs, cand, rows):
    """how many 4:2:0 chroma samples each slot of one frame supplies, and how many nobody covers"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    who = torch.full((ch, cw), NONE, dtype=torch.int64)
    for k in reversed(range(len(cand))):
        if 0 <= cand[k] < Fs:
            who = torch.where(drivers._warp_covers(ch, cw, rows[k], True), k, who)
    return who


def test_the_gpu_tables_are_not_vacuous():
    """from the twin's map and a chroma coverage count: on every shape >= 15 x 63 each supplier slot gives at least one luma and one
    chroma sample and no other slot gives any, frames 0 and 2 leave samples uncovered, frame 1 leaves none; at K = 2 the second
    slot still supplies on frames 0 and 2; the tiles of the 80 x 300 tables lie on both sides of the fast path, with both tap paths
    on it"""
    for h, w in GPU_SHAPES[1:] + (BIG,):
        cand, coef = gpu_tables(h, w) if (h, w) != BIG else big_tables()
        suppliers = GPU_SUPPLIERS if (h, w) != BIG else [[0, 1, 2]] * 3
        Fs = GPU_FS
        _, planes = make_surfaces("nv12", Fs, h, w, seed=9)
        smap = drivers.warp_frames_fill_torch(planes, "nv12", torch.tensor(cand), torch.tensor(coef), "constant", source=True)[1]
        for j in range(GPU_FD):
            luma = {k: int((smap[j] == k).sum()) for k in range(len(cand[j]))}
            cmap = _chroma_counts(h, w, Fs, cand[j], coef[j])
            chroma = {k: int((cmap == k).sum()) for k in range(len(cand[j]))}
            print(f"{h}x{w} frame {j}: luma {luma} none {int((smap[j] == NONE).sum())}; chroma {chroma} none {int((cmap == NONE).sum())}")
            for k in range(len(cand[j])):
                assert (luma[k] > 0) == (k in suppliers[j]) and (chroma[k] > 0) == (k in suppliers[j]), (h, w, j, k)
        if (h, w) != BIG:
            none = [int((smap[j] == NONE).sum()) for j in range(3)]
            assert none[0] > 0 and none[2] > 0 and none[1] == 0
            two = drivers.warp_frames_fill_torch(planes, "nv12", torch.tensor(cand)[:, :2], torch.tensor(coef)[:, :2], "constant", source=True)[1]
            assert bool((two[0] == 1).any()) and bool((two[2] == 1).any()) and not bool((two[1] == 1).any())
    h, w = BIG
    cand, coef = big_tables()
    for fmt in FORMATS:
        fast = [[tile_fast(coef[j][0], fmt, h, w, x0, y0) for y0 in range(0, h, 16) for x0 in range(0, w, 64)] for j in range(3)]
        assert any(fast[0]) and not all(fast[0]) and fast[1][0] and not all(fast[1]) and not any(fast[2][:5])
        assert ops.warp_staged(coef[0][0], fmt, 64, 32) and tile_fast(coef[0][0], fmt, h, w, 64, 32)          # staged, on the fast path
        assert not ops.warp_staged(coef[1][0], fmt) and not ops.warp_staged(coef[2][1], fmt)             # taps from global memory


# ---------------------------------------------------------------------------------------------- the 65535-frame seam
SEAM_FS = 4


def fill_seam_inputs(fmt):
    """one period: cand (PERIOD,2) into SEAM_FS random 3 x 5 source surfaces and coef (PERIOD,2,6) -- an invalid candidate 0, an
    empty slot and the same frame twice among them"""
    h, w = FRAME_SIZE
    sets = coefficient_sets(h, w)
    half = [ONE, 0, 1 << 15, 0, ONE, -(1 << 15)]
    first = [sets[k] for k in ("shift", "identity", "rot2", "quarter", "scale_quarter", "shear", "scale4")]
    second = [IDENTITY, half, sets["shear"], IDENTITY, half, sets["scale_quarter"], IDENTITY]
    cand = torch.tensor([[0, 1], [1, -1], [2, 3], [-1, 0], [3, 2], [0, 0], [1, 2]], dtype=torch.int64)
    coef = torch.tensor([[a, b] for a, b in zip(first, second)], dtype=torch.int64)
    assert cand.shape[0] == PERIOD
    return cand, coef, make_surfaces(fmt, SEAM_FS, h, w, seed=90 + len(fmt), off=1, pad=3, gap=6)


def fill_seam_reference(fmt):
    cand, coef, (_, planes) = fill_seam_inputs(fmt)
    out, smap = drivers.warp_frames_fill_torch(planes, fmt, cand, coef, WARP_BORDER[fmt], fill=WARP_FILL, source=True)
    return _list(out), smap


def test_the_periodic_expectation_of_the_seam_is_the_twin_over_every_frame():
    """Fd = 17 frames whose lists repeat with PERIOD, every one through the twin, against the PERIOD reference frames picked by
    periodic_index: what the GPU test relies on at 65537 frames.  The reference frames are pairwise different"""
    Fd = 2 * PERIOD + 3
    for fmt in WARP_BORDER:
        cand, coef, (_, planes) = fill_seam_inputs(fmt)
        whole, wmap = drivers.warp_frames_fill_torch(planes, fmt, periodic(cand, Fd), periodic(coef, Fd), WARP_BORDER[fmt], fill=WARP_FILL, source=True)
        want, smap = fill_seam_reference(fmt)
        at = periodic_index(Fd)
        assert all(torch.equal(a, b[at]) for a, b in zip(_list(whole), want)) and torch.equal(wmap, smap[at])
        assert all(any(not torch.equal(p[a], p[b]) for p in want) for a in range(PERIOD) for b in range(a)), fmt
        assert {0, 1, NONE} <= set(smap.unique().tolist())


# ---------------------------------------------------------------------------------------------- fill_candidates
def _compose(a, b):
    """a o b for similarity rows (a_re, a_im, tx, ty)"""
    A, T, B, U = complex(a[0], a[1]), complex(a[2], a[3]), complex(b[0], b[1]), complex(b[2], b[3])
    R, S = A * B, A * U + T
    return [R.real, R.imag, S.real, S.imag]


def _inverse(a):
    A, T = complex(a[0], a[1]), complex(a[2], a[3])
    return [(1 / A).real, (1 / A).imag, (-T / A).real, (-T / A).imag]


def _a_path(P, seed):
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.1
    sc = 1.0 + (torch.rand(P, generator=g, dtype=torch.float64) - 0.5) * 0.06
    models = torch.stack([sc * torch.cos(ang), sc * torch.sin(ang), torch.randn(P, generator=g, dtype=torch.float64) * 4.0,
                          torch.randn(P, generator=g, dtype=torch.float64) * 4.0], dim=1)
    return drivers.motion_path(models)


def test_fill_candidates_slot_order_ends_and_transforms():
    F = 9
    path = _a_path(F - 1, 31)
    corr = drivers.motion_smooth(path, 2)
    frames, tr = drivers.fill_candidates(path, corr, (3, 1))
    assert tuple(frames.shape) == (F, 5) and frames.dtype == torch.int64 and tuple(tr.shape) == (F, 5, 4) and tr.dtype == torch.float64
    offsets = [0, -1, 1, -2, -3]
    for f in range(F):
        want = [f + o if 0 <= f + o < F else -1 for o in offsets]
        assert frames[f].tolist() == want                                   # -1 at both ends, never a farther frame in its place
        for k, g in enumerate(want):
            if g < 0:
                assert tr[f, k].tolist() == [1.0, 0.0, 0.0, 0.0]
            else:
                exact = _compose(corr[f].tolist(), _compose(_inverse(path[f].tolist()), path[g].tolist()))
                assert torch.allclose(tr[f, k], torch.tensor(exact, dtype=torch.float64), rtol=0.0, atol=1e-10)
    assert frames[0].tolist() == [0, -1, 1, -1, -1] and frames[F - 1].tolist() == [F - 1, F - 2, -1, F - 3, F - 4]
    assert drivers.fill_candidates(path, corr, (2, 2))[0][4].tolist() == [4, 3, 5, 2, 6]
    assert drivers.fill_candidates(path, corr, (0, 2))[0][4].tolist() == [4, 5, 6]
    # radius=None: the stabilised frame is frame 0, so the transform of slot g is P_g
    still, ts = drivers.fill_candidates(path, drivers.motion_smooth(path, None), (3, 1))
    for f in range(F):
        for k, g in enumerate(still[f].tolist()):
            if g >= 0:
                assert torch.allclose(ts[f, k], path[g], rtol=0.0, atol=1e-10)
    # no neighbours: the corrections themselves, in every bit
    only, t0 = drivers.fill_candidates(path, corr, (0, 0))
    assert only.tolist() == [[f] for f in range(F)] and _f64_bits(t0[:, 0]) == _f64_bits(corr) and _f64_bits(tr[:, 0]) == _f64_bits(corr)
    # a window of the corrections: the rows of the whole
    part_f, part_t = drivers.fill_candidates(path, corr[3:6], (3, 1), first=3)
    assert torch.equal(part_f, frames[3:6]) and _f64_bits(part_t) == _f64_bits(tr[3:6])
    for bad in ((3,), (-1, 1), (8, 8), (1.5, 0), "31"):
        with pytest.raises(ValueError):
            drivers.fill_candidates(path, corr, bad)
    with pytest.raises(ValueError):
        drivers.fill_candidates(path, corr, (1, 1), first=1)


@pytest.mark.parametrize("neighbors", [(3, 1), (2, 2)])
def test_stabilizer_candidates_push_by_push_are_the_one_shot(neighbors):
    T, K = 19, 40
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5)
    models = drivers.motion_fit_torch(trajs[None], vis[None], ids=torch.arange(K), **kw)[0]
    path = drivers.motion_path(models)
    want_f, want_t = drivers.fill_candidates(path, drivers.motion_smooth(path, 2), neighbors)
    st = drivers.Stabilizer(radius=2, engine="torch", neighbors=neighbors, **kw)
    done = 0
    for f0 in list(range(0, T, 3)) + [None]:
        if f0 is None:
            g0, rows = st.finish()
        else:
            f1 = min(f0 + 3, T)
            ids = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
            g0, rows = st.step(f0, trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids], ids=ids)
        k = rows.shape[0]
        frames, tr = st.candidates(g0, k)
        assert g0 == done and tuple(frames.shape) == (k, 1 + sum(neighbors)) and frames.dtype == torch.int64
        assert torch.equal(frames, want_f[g0:g0 + k]) and _f64_bits(tr) == _f64_bits(want_t[g0:g0 + k]), (f0, g0, k)
        assert _f64_bits(tr[:, 0]) == _f64_bits(rows)
        done += k
    assert done == T and bool((want_f[T - 1] == -1).any())
    with pytest.raises(ValueError):
        st.candidates(T - 1, 2)
    with pytest.raises(ValueError):
        drivers.Stabilizer(radius=2, engine="torch", neighbors=(1, 3))               # ahead > radius
    with pytest.raises(ValueError):
        drivers.Stabilizer(radius=None, engine="torch", neighbors=(1, 1))
    drivers.Stabilizer(radius=None, engine="torch", neighbors=(4, 0))
    with pytest.raises(ValueError):
        drivers.Stabilizer(radius=2, engine="torch").candidates(0, 0)


# ---------------------------------------------------------------------------------------------- crop_zoom
def _uncovered(coef, h, w):
    """luma samples of an h x w surface that the rows leave uncovered, all frames"""
    return sum(int((~drivers._warp_covers(h, w, row, False)).sum()) for row in coef.tolist())


def test_crop_zoom_is_the_smallest_zoom_without_a_border():
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    assert drivers.crop_zoom(ident, (64, 96), margin=0) == 1.0 and drivers.crop_zoom(ident, (64, 96), (128, 192), margin=0) == 1.0
    assert 1.0 < drivers.crop_zoom(ident, (64, 96)) < 1.001
    sims = torch.tensor([[1, 0, 0, 0], [1.02, 0.03, 3.5, -2.25], [0.97, -0.05, -4, 1.5], [1, 0.02, 0, 6]], dtype=torch.float64)
    seen = []
    for surface in ((64, 96), (100, 192), (1080, 1920)):
        z = drivers.crop_zoom(sims, (64, 96), surface)
        at = _uncovered(drivers.warp_coefficients(sims, (64, 96), surface, z), *surface)
        below = _uncovered(drivers.warp_coefficients(sims, (64, 96), surface, 0.995 * z), *surface)
        print(f"crop_zoom {surface}: z = {z:.4f}, uncovered {at} at z, {below} at 0.995 z")
        assert at == 0 and below > 0
        seen.append(round(z, 4))
    assert seen == [1.3222, 1.3199, 1.3161]                                    # (the closed form, worked out beforehand)
    six = torch.tensor([[1.0, 0.1, 2.0, -0.05, 0.95, -3.0]], dtype=torch.float64)
    z = drivers.crop_zoom(six, (64, 96))
    assert _uncovered(drivers.warp_coefficients(six, (64, 96), None, z), 64, 96) == 0
    for bad in ([[1.0, 0.0, 60.0, 0.0]], [[1.0, 0.0, 0.0, -40.0]], [[0.0, 0.0, 0.0, 0.0]]):                     # the centre outside; singular
        with pytest.raises(ValueError):
            drivers.crop_zoom(torch.tensor(bad, dtype=torch.float64), (64, 96))
    for margin in (-1.0, float("nan"), True):
        with pytest.raises(ValueError):
            drivers.crop_zoom(ident, (64, 96), margin=margin)


# ---------------------------------------------------------------------------------------------- the planted mosaic
WORLD, CROP, AT = (160, 192), (96, 128), (32, 32)
SIMS = [(1.0, 0.0, 0.0, 0.0), (1.03, 2.0, 4.0, -3.0), (0.96, -3.0, -6.0, 2.5), (1.05, 1.0, 5.5, 6.0), (0.95, -1.5, -2.0, -5.0), (1.0, 3.0, 3.0, 1.0)]
_MOSAIC = {}


def mosaic():
    """-> (frames (6,3,96,128) uint8 planar8, path (6,4)): the world, a 160 x 192 ramp by test_warp's formula, seen by six cameras --
    the twin under test_warp's six similarities about the world centre, cropped to 96 x 128 at (32, 32) -- and P_f = G_0 o G_f^-1
    with G_f world -> frame f.  Made once; nobody writes to it"""
    if not _MOSAIC:
        H, W = WORLD
        y, x = torch.arange(H, dtype=torch.float64).view(H, 1), torch.arange(W, dtype=torch.float64).view(1, W)
        ramp = 30.0 + 0.4 * x + 0.3 * y + 4.0 * torch.sin(x / 40.0) + 3.0 * torch.cos(y / 30.0)
        assert float((ramp[:, 1:] - ramp[:, :-1]).abs().max() + (ramp[1:] - ramp[:-1]).abs().max()) <= 1.0 and 0 < float(ramp.min()) and float(ramp.max()) < 255
        world = torch.floor(ramp + 0.5).to(torch.uint8).expand(6, 3, H, W).contiguous()
        G = []
        for s, d, tx, ty in SIMS:
            c, sn = s * math.cos(math.radians(d)), s * math.sin(math.radians(d))
            cx, cy = (W - 1) / 2, (H - 1) / 2
            G.append([c, sn, cx - (c * cx - sn * cy) + tx, cy - (sn * cx + c * cy) + ty])                   # about the world centre
        coef = drivers.warp_coefficients(torch.tensor(G, dtype=torch.float64), WORLD)
        crop = (slice(None), slice(None), slice(AT[1], AT[1] + CROP[0]), slice(AT[0], AT[0] + CROP[1]))
        seen = drivers.warp_frames_torch(torch.full_like(world, 255), "planar8", coef, "constant")[crop]
        assert bool((seen == 255).all())                                       # the crop holds no fill
        frames = drivers.warp_frames_torch(world, "planar8", coef, "constant")[crop].contiguous()
        G = [[g[0], g[1], g[2] - AT[0], g[3] - AT[1]] for g in G]              # world -> the cropped frame
        path = torch.tensor([_compose(G[0], _inverse(g)) for g in G], dtype=torch.float64)
        _MOSAIC["made"] = (frames, path)
    return _MOSAIC["made"]


def test_the_planted_mosaic_is_filled_from_its_neighbours_within_two_levels():
    """neighbors = (3, 1) at zoom 1 on the cameras held still (radius=None): no sample of any frame is uncovered, every frame >= 1
    takes samples from slot 1 and frames 2-5 from at least two neighbours, and every sample is within 2 levels of frame 0 -- the
    argument of test_warp.test_a_shaken_ramp_is_held_still_within_two_levels (rounding of the world, two resamplings, 1/256 px
    positions at gradient 1: under 1.8).  With neighbors = (2, 1) frame 5 leaves exactly the samples uncovered that only frame 2
    could give: the fallback is exercised"""
    frames, path = mosaic()
    corr = drivers.motion_smooth(path, None)
    cand, tr = drivers.fill_candidates(path, corr, (3, 1))
    coef = drivers.warp_coefficients(tr.reshape(-1, 4), CROP).reshape(6, 5, 6)
    out, smap = drivers.warp_frames_fill_torch(frames, "planar8", cand, coef, "constant", source=True)
    counts = [[int((smap[f] == k).sum()) for k in range(5)] for f in range(6)]
    diff = (out.to(torch.int64) - frames[0].to(torch.int64)).abs()
    print(f"mosaic: supplied per slot {counts}, uncovered {int((smap == NONE).sum())}, max |diff| = {int(diff.max())}")
    assert int((smap == NONE).sum()) == 0
    assert all(counts[f][1] > 0 for f in range(1, 6)) and all(sum(c > 0 for c in counts[f][1:]) >= 2 for f in range(2, 6))
    assert all(0 < counts[f][0] <= 96 * 128 for f in range(6)) and counts[0][0] == 96 * 128
    assert int(diff.max()) <= 2
    cand2, tr2 = drivers.fill_candidates(path, corr, (2, 1))
    coef2 = drivers.warp_coefficients(tr2.reshape(-1, 4), CROP).reshape(6, 4, 6)
    out2, smap2 = drivers.warp_frames_fill_torch(frames, "planar8", cand2, coef2, "constant", fill=(255, 0, 255), source=True)
    only_2 = smap[5] == 4                                                      # slot 4 of (3, 1) is offset -3: frame 2
    assert cand[5].tolist() == [5, 4, -1, 3, 2] and cand2[5].tolist() == [5, 4, -1, 3]
    print(f"mosaic: frame 5 without frame 2 leaves {int(only_2.sum())} samples uncovered")
    assert int(only_2.sum()) > 0 and torch.equal(smap2[5] == NONE, only_2) and int((smap2[:5] == NONE).sum()) == 0
    plain = drivers.warp_frames_torch(frames[5:], "planar8", coef2[5, :1], "constant", fill=(255, 0, 255))
    assert torch.equal(out2[5][:, only_2], plain[0][:, only_2])                # candidate 0 under the border rule


# ---------------------------------------------------------------------------------------------- the driver's own checks
def test_the_driver_maps_absolute_frames_onto_the_held_surfaces():
    frames, path = mosaic()
    cand, tr = drivers.fill_candidates(path, path, (2, 1))
    got, coef = drivers._fill_setup(frames[1:5], "planar8", cand[3:4], tr[3:4], 1, None, 1.0)
    assert cand[3].tolist() == [3, 2, 4, 1] and got.tolist() == [[2, 1, 3, 0]]
    assert torch.equal(coef, drivers.warp_coefficients(tr[3], CROP).view(1, 4, 6))
    assert drivers._fill_setup(frames[1:5], "planar8", cand[0:1], tr[0:1], 0, None, 1.0)[0].tolist() == [[0, -1, 1, -1]]
    for first, rows in ((2, cand[3:4]), (0, cand[5:6])):                       # frame 1 not held; frames 4 and 5 not held
        with pytest.raises(ValueError):
            drivers._fill_setup(frames[1:5], "planar8", rows, tr[3:4], first, None, 1.0)
    with pytest.raises(ValueError):
        drivers._fill_setup(frames, "planar8", cand, tr[:, :2], 0, None, 1.0)


# ---------------------------------------------------------------------------------------------- the ABI
def test_frames_warp_fill_is_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_frames_warp_fill" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)
    for words in ("x0 >= 0 and (x0 + 1 <= pw - 1, or fx == 0 and x0 <= pw - 1)", "first candidate in list order",
                  "K = 1 with cand[j][0] = j is pips_frames_warp, byte for byte", "every tap that has weight lies inside the plane",
                  "ghosts in the border", "feathering", "choose their candidate independently", "nothing comes from frames outside the list"):
        assert words in hdr, words
    assert int(re.search(r"#define PIPS_WARP_FILL_MAX\s+(\d+)", hdr).group(1)) == ops.WARP_FILL_MAX == 16
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_frames_warp_fill\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 34
    res, args = _lib.SIGNATURES["pips_frames_warp_fill"]
    assert res is ctypes.c_int and len(args) == 34 and args[:10] == [ctypes.c_int] * 10 and args[11] is ctypes.c_size_t
    assert "warp.hip" in _build.SOURCES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_frames_warp_fill") and callable(ops.warp_frames_fill) and callable(drivers.warp_frames_fill)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the host-side rejections need no device: nothing is launched

    def call(fmt=4, matrix=1, range_=0, border=0, fill=0, Fs=0, Fd=0, K=1, h=8, w=8, pitch=8, mpitch=8, source=None):
        surf = [None, pitch, 0, None, pitch, 0, None, 0, 0]
        return lib.pips_frames_warp_fill(fmt, matrix, range_, border, fill, Fs, Fd, K, h, w, *surf, *surf, None, None, source, mpitch, 0, None)

    assert call() == 0 and call(Fs=1) == 0 and call(K=16) == 0                  # Fd = 0 launches nothing
    for bad in (dict(fmt=9), dict(fmt=-1), dict(border=2), dict(matrix=2), dict(range_=-1), dict(fill=-1), dict(fill=1 << 24), dict(Fs=-1),
                dict(Fd=-1), dict(Fs=2), dict(K=0), dict(K=17), dict(h=0), dict(w=8193), dict(pitch=7), dict(Fd=1), dict(Fs=1, Fd=1),
                dict(source=ctypes.c_void_p(4096), mpitch=7)):
        assert call(**bad) == -1, bad
        assert lib.pips_last_error().decode().startswith("frames_warp_fill:"), bad
    assert call(fmt=0, matrix=7, range_=7, pitch=24) == 0                  # matrix and range are looked at for YCbCr alone
