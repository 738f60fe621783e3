"""CPU: pips_tracks_draw_ex (include/pips_hip.h) -- tracks drawn onto the 16-bit P010 / I010 surfaces, and trails that fade with
age.  drivers.draw_tracks_torch, the torch twin, against the rule restated here as plain loops on Python integers: the 10-bit
formats with junk in the six unused bits of every word, and fade tables on planar8, nv12 and p010; the joint of a bright and a
faint segment; the 10-bit RGB -> YCbCr table against the float64 formula and against yuv.h and the header; every PIPS_E_ARG case of
the new entry through the loaded library (nothing is launched); the Python layers' ValueErrors; TrackPainter on p010 with a linear
fade against one whole-video call.  The surfaces and cases of tests/test_draw_ex_gpu.py are made here, and the twin's output on them
is checked not to be vacuous.  Positions, primitives and the inside test are pips_tracks_draw's: tests/test_draw.py has them, and
its helpers are used here."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from pips_amd import drivers, ops
from test_draw import (FAT, GOOD, KRKB, MATRICES, NAN, RANGES, STYLE, THIN, buffers, inside, not_vacuous, outside_untouched,
                       restate_points, tracks, views)

WIDE = ("p010", "i010")
ROWS = [(m, r) for m in MATRICES for r in RANGES]
SENTINEL16 = 0xA5A5 - 65536                                          # the int16 that holds the word 0xA5A5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- 16-bit siblings of test_draw's helpers
def buffers16(fmt, F, h, w, seed, pad=(5, 2)):
    """test_draw.buffers for p010 / i010: int16 allocations, ``pad[0]`` more elements a row and ``pad[1]`` more rows a frame than the
    image; inside the image random WORDS -- all 16 bits, so the six bits the format does not use hold junk -- and the word 0xA5A5
    everywhere else"""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    shapes = [(h, w), (ch, cw, 2)] if fmt == "p010" else [(h, w), (ch, cw), (ch, cw)]
    out = []
    for s in shapes:
        full = torch.full((F, s[0] + pad[1], s[1] + pad[0]) + s[2:], SENTINEL16, dtype=torch.int16)
        full[:, :s[0], :s[1]] = torch.randint(-32768, 32768, (F,) + s, generator=g, dtype=torch.int16)
        out.append(full)
    return out


def any_buffers(fmt, F, h, w, seed, pad=(5, 2)):
    return buffers16(fmt, F, h, w, seed, pad) if fmt in WIDE else buffers(fmt, F, h, w, seed, pad)


def untouched_outside(bufs, before, fmt, h, w):
    """test_draw.outside_untouched, for the 16-bit formats too: every element outside the w x h image of each plane is what it was,
    and is the sentinel"""
    if fmt not in WIDE:
        return outside_untouched(bufs, before, fmt, h, w)
    masks = [torch.ones_like(b, dtype=torch.bool) for b in bufs]
    for v in views(masks, fmt, h, w):
        v[...] = False
    return all(torch.equal(b[m], b0[m]) and bool((b[m] == SENTINEL16).all()) for b, b0, m in zip(bufs, before, masks))


def value10(word, fmt):
    return (word & 0xFFFF) >> 6 if fmt == "p010" else word & 1023


def word16(v, fmt):
    """the int16 that holds the rewritten word of the 10-bit value v"""
    u = v << 6 if fmt == "p010" else v
    return u - 65536 if u >= 32768 else u


def linear(trail):
    """fade="linear" in the rule's integers: round_half_up(256 (trail - a) / trail), in exact integer arithmetic"""
    return [(2 * 256 * (trail - a) + trail) // (2 * trail) for a in range(trail)]


# ------------------------------------------------------------------------------------------------------- the rule, restated
def restate_weights(trajs, r, h, w, src, trail, line8, dot8, fade):
    """Wp[i][y][x] in 0..1024 by plain loops: per subsample the largest factor among the primitives of track i that hold it -- 256
    for the head's disc, fade[a] for the capsule of age a (256 without a table) -- summed over the pixel's four"""
    trajs = trajs.numpy()
    n = trajs.shape[1]
    qx, qy = restate_points(trajs, r, trail, src[1], w, 0), restate_points(trajs, r, trail, src[0], h, 1)
    Wp = [[[0] * w for _ in range(h)] for _ in range(n)]
    for i in range(n):
        pts = [None if qx[g][i] is None or qy[g][i] is None else (qx[g][i], qy[g][i]) for g in range(len(qx))]
        if pts[-1] is None:
            continue
        prims = [(pts[-1], pts[-1], dot8, 256)] if dot8 >= 0 else []
        for g in range(1, len(pts)):
            a, b = pts[g - 1], pts[g]
            age = len(pts) - 1 - g                                  # the segment that ends on the head has age 0
            if line8 >= 0 and a is not None and b is not None and abs(b[0] - a[0]) <= 2047 and abs(b[1] - a[1]) <= 2047:
                prims.append((a, b, line8, 256 if fade is None else fade[age]))
        for y in range(h):
            for x in range(w):
                for dx, dy in ((-2, -2), (2, -2), (-2, 2), (2, 2)):
                    c = (8 * x + dx, 8 * y + dy)
                    Wp[i][y][x] += max([f for P0, P1, R, f in prims if inside(c, P0, P1, R)], default=0)
    return Wp


def restate_color_ex(rgb, fmt, matrix, range_):
    R, G, B = (int(v) for v in rgb)
    if fmt in WIDE:
        y0, sh, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB10_RULES[(matrix, range_)]
        half, mid, top = 1 << (sh - 1), 512, 1023
    elif fmt == "nv12":
        y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB_RULES[(matrix, range_)]
        sh, half, mid, top = 16, 32768, 128, 255
    else:
        return R, G, B
    clamp = lambda v: min(max(v, 0), top)
    return (y0 + ((yr * R + yg * G + yb * B + half) >> sh), clamp(mid + ((ur * R + ug * G + ub * B + half) >> sh)),
            clamp(mid + ((vr * R + vg * G + vb * B + half) >> sh)))


def restate_draw_ex(planes, fmt, Wp, A, colors, matrix, range_, faded):
    """the blend by plain loops on clones of ``planes`` (planar8, nv12, p010 or i010): Wp[f][i][y][x], A[f][i].  Without a table the
    weight is k A = (Wp / 256) A, with one it is (Wp A + 128) >> 8; a 16-bit word is rewritten when a track gave it a weight"""
    P = [p.clone().tolist() for p in planes]
    F, h, w = len(Wp), len(Wp[0][0]), len(Wp[0][0][0])
    wide, semi = fmt in WIDE, fmt in ("nv12", "p010")
    weight = (lambda s, a: (s * a + 128) >> 8) if faded else (lambda s, a: (s // 256) * a)
    get = (lambda v: value10(v, fmt)) if wide else (lambda v: v)
    put = (lambda v: word16(v, fmt)) if wide else (lambda v: v)
    for f in range(F):
        for i in range(len(Wp[f])):
            col = restate_color_ex(colors[i], fmt, matrix, range_)
            k = Wp[f][i]
            for y in range(h):
                for x in range(w):
                    wg = weight(k[y][x], A[f][i])
                    if wg == 0:
                        continue
                    assert 0 < wg <= 1024
                    if fmt == "planar8":
                        for q in range(3):
                            P[0][f][q][y][x] = (P[0][f][q][y][x] * (1024 - wg) + col[q] * wg + 512) >> 10
                    else:
                        P[0][f][y][x] = put((get(P[0][f][y][x]) * (1024 - wg) + col[0] * wg + 512) >> 10)
            if fmt == "planar8":
                continue
            for cy in range((h + 1) // 2):
                for cx in range((w + 1) // 2):
                    K = weight(sum(k[y][x] for y in (2 * cy, 2 * cy + 1) for x in (2 * cx, 2 * cx + 1) if y < h and x < w), A[f][i])
                    if K == 0:
                        continue
                    assert 0 < K <= 4096
                    mix = lambda p, c: put((get(p) * (4096 - K) + c * K + 2048) >> 12)
                    if semi:
                        P[1][f][cy][cx] = [mix(P[1][f][cy][cx][0], col[1]), mix(P[1][f][cy][cx][1], col[2])]
                    else:
                        P[1][f][cy][cx], P[2][f][cy][cx] = mix(P[1][f][cy][cx], col[1]), mix(P[2][f][cy][cx], col[2])
    return [torch.tensor(p, dtype=q.dtype).view(q.shape) for p, q in zip(P, planes)]


STYLE_Q = dict(width=1.5, dot=1.75, alpha=0.9, alpha_occ=0.4, vis_thr=0.6)
LINE8, DOT8, A_VIS, A_OCC = 6, 14, 230, 102                          # STYLE_Q in the rule's integers


def _scene(h, w, n, src, F=2, trail=3):
    """seeded tracks, logits and colours for F frames; first = trail"""
    first = trail
    G = first + F
    g = torch.Generator().manual_seed(h * w + n)
    H, W = src or (h, w)
    trajs = torch.rand(1, 1, n, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0]) + torch.randn(1, G, n, 2, generator=g).cumsum(1) * 1.2
    trajs[0, 1, 0] = NAN                                            # a gap in the first track's past
    vis = torch.randn(1, G, n, generator=g)
    vis[0, first, 1] = NAN                                          # a NaN logit: occluded
    vis[0, first, 0], vis[0, first + 1, 2] = 3.0, -3.0
    colors = torch.randint(0, 256, (n, 3), generator=g, dtype=torch.uint8)
    logit = float(torch.logit(torch.tensor(0.6, dtype=torch.float32)))
    A = [[A_VIS if float(vis[0, first + f, i]) > logit else A_OCC for i in range(n)] for f in range(F)]
    return trajs, vis, colors, A, first, (H, W)


def _twin(planes, fmt, trajs, vis, colors, **kw):
    out = drivers.draw_tracks_torch(planes, fmt, trajs, vis, colors, **kw)
    return [out] if torch.is_tensor(out) else list(out)


def test_style_q_in_integers():
    assert (LINE8, DOT8) == (math.floor(4 * 1.5 + 0.5), math.floor(8 * 1.75 + 0.5))
    assert (A_VIS, A_OCC) == (math.floor(256 * 0.9 + 0.5), math.floor(256 * 0.4 + 0.5))


@pytest.mark.parametrize("src", [None, (24, 32)], ids=["own", "from24x32"])
@pytest.mark.parametrize("h,w", [(9, 13), (17, 33)])
def test_twin_on_p010_and_i010_is_the_rule_by_plain_loops(h, w, src):
    """both formats under the four matrix / range rows, five tracks with trails of three: the twin's words are the loops'; a touched
    word has its six other bits zero, every other word -- junk included -- is bit-identical, in place too"""
    F, trail, n = 2, 3, 5
    trajs, vis, colors, A, first, (H, W) = _scene(h, w, n, src, F, trail)
    Wp = [restate_weights(trajs[0], first + f, h, w, (H, W), trail, LINE8, DOT8, None) for f in range(F)]
    for f in range(F):                                              # the twin's coverage is the loops'
        got = drivers.draw_coverage_torch(trajs[0], first + f, h, w, (H, W), trail, LINE8, DOT8)
        assert (got * 256).tolist() == Wp[f]
    assert any(0 < v < 1024 for f in Wp for t in f for row in t for v in row)
    for fmt in WIDE:
        low = 63 if fmt == "p010" else 0xFC00                       # the bits the format does not use
        for matrix, range_ in ROWS:
            bufs = buffers16(fmt, F, h, w, 7 * h + w)
            before = [b.clone() for b in bufs]
            planes = views(bufs, fmt, h, w)
            want = restate_draw_ex(planes, fmt, Wp, A, colors.tolist(), matrix, range_, False)
            kw = dict(size=src, first=first, trail=trail, matrix=matrix, range=range_, **STYLE_Q)
            got = _twin(planes, fmt, trajs, vis, colors, **kw)
            assert all(a.dtype == torch.int16 and torch.equal(a, b) for a, b in zip(got, want)), (fmt, matrix, range_)
            assert all(torch.equal(a, b) for a, b in zip(bufs, before))              # inplace=False drew on clones
            for a, b in zip(got, planes):
                changed = a != b
                assert bool(changed.any()) and not bool(changed.all())
                assert bool(((a.to(torch.int64) & low)[changed] == 0).all())         # rewritten words: the other six bits are zero
                assert bool(((b.to(torch.int64) & low)[~changed] != 0).any())        # junk that survived, bit for bit (a == b there)
            out = _twin(planes, fmt, trajs, vis, colors, inplace=True, **kw)
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, planes))
            assert all(torch.equal(a, b) for a, b in zip(planes, want)) and untouched_outside(bufs, before, fmt, h, w)
            # uint16 planes are the same bits and come back as uint16
            u16 = [p.clone().view(torch.uint16) for p in views(before, fmt, h, w)]
            got16 = _twin(u16, fmt, trajs, vis, colors, **kw)
            assert all(a.dtype == torch.uint16 and torch.equal(a.view(torch.int16), b) for a, b in zip(got16, want))


FADES = {"linear": None, "non-monotone": [64, 256, 0], "all-256": [256, 256, 256], "all-0": [0, 0, 0]}


@pytest.mark.parametrize("kind", list(FADES))
@pytest.mark.parametrize("fmt", ["planar8", "nv12", "p010"])
def test_fade_tables_are_the_rule_by_plain_loops(fmt, kind):
    h, w, F, trail, n = 9, 13, 2, 3, 5
    table = FADES[kind] or linear(trail)
    assert kind != "linear" or table == [256, 171, 85]
    arg = "linear" if kind == "linear" else [v / 256.0 for v in table]
    trajs, vis, colors, A, first, size = _scene(h, w, n, None, F, trail)
    Wp = [restate_weights(trajs[0], first + f, h, w, size, trail, LINE8, DOT8, table) for f in range(F)]
    for f in range(F):
        assert drivers.draw_coverage_torch(trajs[0], first + f, h, w, size, trail, LINE8, DOT8, table).tolist() == Wp[f]
    bufs = any_buffers(fmt, F, h, w, 31)
    before = [b.clone() for b in bufs]
    planes = views(bufs, fmt, h, w)
    kw = dict(first=first, matrix="bt601", range="limited", **STYLE_Q)
    want = restate_draw_ex(planes, fmt, Wp, A, colors.tolist(), "bt601", "limited", True)
    got = _twin(planes, fmt, trajs, vis, colors, trail=trail, fade=arg, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and any(not torch.equal(a, b) for a, b in zip(got, planes))
    plain = _twin(planes, fmt, trajs, vis, colors, trail=trail, **kw)
    heads = _twin(planes, fmt, trajs, vis, colors, trail=0, **kw)
    assert any(not torch.equal(a, b) for a, b in zip(plain, heads))
    if kind == "all-256":                                           # the collapse clause: pips_tracks_draw's bytes
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
    elif kind == "all-0":                                           # heads only
        assert all(torch.equal(a, b) for a, b in zip(got, heads))
    else:
        assert any(not torch.equal(a, b) for a, b in zip(got, plain)) and any(not torch.equal(a, b) for a, b in zip(got, heads))
        assert any(0 < v < 1024 and v % 256 for f in Wp for t in f for row in t for v in row)      # a faded factor on a pixel
    _twin(planes, fmt, trajs, vis, colors, trail=trail, fade=arg, inplace=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(planes, want)) and untouched_outside(bufs, before, fmt, h, w)


def test_a_joint_takes_the_larger_factor_not_the_sum():
    """(4,10) -> (12,10) -> (12,18), lines 4 px wide, no dot: pixel (12,10) lies with all four subsamples in both capsules.  With
    factors 64 (age 0, the segment that ends on the head) and 256 (age 1) it is drawn at 256, the larger; swapped, the bytes change"""
    bufs = buffers("planar8", 1, 24, 24, 3)
    planes = views(bufs, "planar8", 24, 24)
    t = torch.tensor([(4.0, 10.0), (12.0, 10.0), (12.0, 18.0)]).view(1, 3, 1, 2)
    red = torch.tensor([[255, 0, 0]], dtype=torch.uint8)
    kw = dict(first=2, trail=2, width=4.0, dot=-1.0, alpha=0.5)
    a = _twin(planes, "planar8", t, None, red, fade=[0.25, 1.0], **kw)[0]
    b = _twin(planes, "planar8", t, None, red, fade=[1.0, 0.25], **kw)[0]
    assert not torch.equal(a, b)
    mix = lambda p, c, wg: (p * (1024 - wg) + c * wg + 512) >> 10
    A = 128
    for out, (young, old) in ((a, (64, 256)), (b, (256, 64))):
        for (x, y), factor in (((12, 10), max(young, old)), ((12, 14), young), ((8, 10), old)):
            wg = (4 * factor * A + 128) >> 8
            want = [mix(int(planes[0][0, q, y, x]), c, wg) for q, c in enumerate((255, 0, 0))]
            assert out[0, :, y, x].tolist() == want, ((x, y), factor)
    # (the sum would be 4 x 320 at the joint: a weight of 640 where the rule gives 512)
    assert (4 * 256 * A + 128) >> 8 == 512


# ------------------------------------------------------------------------------------------------------- the colour table
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("range_", RANGES)
def test_colour_table_10bit(matrix, range_):
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    y0, sh, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB10_RULES[(matrix, range_)]
    ys, cs = (876.0 / 255.0, 896.0 / 255.0) if range_ == "limited" else (1023.0 / 255.0, 1023.0 / 255.0)
    assert (y0, sh) == ((64, 14) if range_ == "limited" else (0, 16))
    assert ur + ug + ub == 0 and vr + vg + vb == 0                   # each chroma row sums to 0
    if range_ == "limited":                                          # the 8-bit constants with two more result bits
        assert (yr, yg, yb, ur, ug, ub, vr, vg, vb) == drivers.RGB_RULES[(matrix, range_)][1:]
    else:
        s = 65536.0 * 1023.0 / 255.0
        exact = (kr, kg, kb, -kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5, 0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))
        assert all(abs(c - s * e) <= 1.0 for c, e in zip((yr, yg, yb, ur, ug, ub, vr, vg, vb), exact))
        assert yr + yg + yb == math.floor(s + 0.5) == 262915
    grey = torch.arange(256).view(-1, 1).expand(-1, 3)
    out = drivers.rgb_to_yuv_torch(grey, matrix, range_, bits=10)
    assert bool((out[:, 1:] == 512).all())                          # greys give (Y, 512, 512) over all 256 levels
    assert out[0].tolist() == [y0, 512, 512] and out[255].tolist() == [940 if range_ == "limited" else 1023, 512, 512]
    assert bool((out[1:, 0] > out[:-1, 0]).all())                   # (a level of grey is 3.4 or 4 levels of luma)
    v = torch.linspace(0, 255, 17).round().to(torch.int64)
    rgb = torch.cartesian_prod(v, v, v)
    got = drivers.rgb_to_yuv_torch(rgb, matrix, range_, bits=10)
    R, G, B = rgb.double().unbind(1)
    Y = kr * R + kg * G + kb * B
    exact = torch.stack([y0 + ys * Y, 512 + cs * (B - Y) / (2 * (1 - kb)), 512 + cs * (R - Y) / (2 * (1 - kr))], dim=1)
    assert bool(((got - torch.floor(exact + 0.5).clamp(0, 1023)).abs() <= 1).all())
    half = 1 << (sh - 1)
    if range_ == "limited":
        assert 64 <= int(got[:, 0].min()) and int(got[:, 0].max()) == 940
        assert 64 <= int(got[:, 1:].min()) and int(got[:, 1:].max()) == 960
    else:                                                           # pure blue / red reach 1024 ahead of the clamp
        assert 512 + ((ub * 255 + half) >> sh) == 1024 and 512 + ((vr * 255 + half) >> sh) == 1024
        pure = drivers.rgb_to_yuv_torch(torch.tensor([[0, 0, 255], [255, 0, 0]]), matrix, range_, bits=10)
        assert int(pure[0, 1]) == 1023 and int(pure[1, 2]) == 1023
        assert int(got.max()) == 1023 and int(got.min()) == 0
    # the accumulators' extremes: the triples that switch on every positive, or every negative, constant of a row
    for row in ((yr, yg, yb), (ur, ug, ub), (vr, vg, vb)):
        hi = sum(c * 255 for c in row if c > 0) + half
        lo = sum(c * 255 for c in row if c < 0) + half
        assert -2 ** 27 < lo <= hi < 2 ** 27
    # python integers give what the int64 tensors give
    for R_, G_, B_ in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (13, 200, 77)):
        assert list(restate_color_ex((R_, G_, B_), "p010", matrix, range_)) == \
            drivers.rgb_to_yuv_torch(torch.tensor([R_, G_, B_]), matrix, range_, bits=10).tolist()
    with pytest.raises(ValueError):
        drivers.rgb_to_yuv_torch(grey, matrix, range_, bits=12)


def test_colour_table_10bit_is_stated_once_per_layer():
    want = [drivers.RGB10_RULES[(m, r)] for m in MATRICES for r in RANGES]
    src = open(os.path.join(ROOT, "pips_amd", "csrc", "yuv.h")).read()
    assert src.count("RGB10_RULES[2][2]") == 1 and src.index("RGB10_RULES[2][2]") > src.index("RGB_RULES[2][2]")
    body = src[src.index("RGB10_RULES[2][2]"):]
    rows = re.findall(r"\{(-?\d+(?:, -?\d+){10})\}", body[:body.index("};")])
    assert [tuple(int(v) for v in row.split(",")) for row in rows] == want
    header = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    rows = re.findall(r"10-bit PIPS_MATRIX_(BT\d+) (limited|full)\s+((?:-?\d+ +){10}-?\d+)\n", header)
    assert [(m.lower(), r) for m, r, _ in rows] == ROWS
    assert [tuple(int(v) for v in row.split()) for _, _, row in rows] == want


# ------------------------------------------------------------------------------------------------- the library's checks
E_ARG = -1
KEYS = list(GOOD)
KEYS.insert(KEYS.index("workspace"), "fade")                        # the signature is pips_tracks_draw's with fade ahead of workspace
GOOD_EX = dict(GOOD, fade=None)
GOOD_P010 = dict(GOOD_EX, format=6, pitch0=24, step0=240, pitch1=24, step1=120)
GOOD_I010 = dict(GOOD_EX, format=7, pitch0=24, step0=240, p1=0x2000, pitch1=12, step1=60, p2=0x6000, pitch2=12, step2=60)


def _rc(lib, base, **change):
    a = dict(base, **change)
    return lib.pips_tracks_draw_ex(*[a[k] for k in KEYS])


def test_tracks_draw_ex_rejects_bad_arguments_ahead_of_any_launch():
    """every PIPS_E_ARG case of pips_tracks_draw_ex through the loaded library: the pointers are never followed (nothing is
    launched), so this runs without a device; the fade table alone is read, and is a real host array"""
    from pips_amd import _lib
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    need = lib.pips_draw_workspace_bytes(2, 3, 4)
    table = lambda *v: (C.c_int * len(v))(*v)
    ok = table(256, 128, 64, 0)
    for base in (GOOD_EX, GOOD_P010, GOOD_I010):
        assert _rc(lib, base, F=0) == 0 and _rc(lib, base, n=0) == 0 and _rc(lib, base, F=0, first=5) == 0
        assert _rc(lib, base, F=0, fade=ok) == 0 and _rc(lib, base, n=0, fade=table(0, 0, 0, 0)) == 0
        assert _rc(lib, base, F=0, trail=0, fade=None) == 0 and _rc(lib, base, F=0, trail=0, fade=table(999)) == 0     # no entry is read
    assert _rc(lib, GOOD_P010, n=0, p0=None, p1=None, trajs=None, colors=None, workspace=None, workspace_bytes=0) == 0
    # everything pips_tracks_draw rejects (tests/test_draw.py), on an 8-bit surface
    bad = [dict(format=9), dict(format=-1), dict(matrix=2), dict(range=-1), dict(range=2), dict(F=-1),
           dict(n=-1), dict(h=0), dict(w=0), dict(src_h=0), dict(src_w=0), dict(h=8193, step0=8193 * 12, step1=4097 * 12),
           dict(w=8193, pitch0=8193, pitch1=8194, step0=81930, step1=8194 * 5), dict(trail=-1), dict(trail=33), dict(line8=129),
           dict(dot8=129), dict(alpha_vis=257), dict(alpha_vis=-1), dict(alpha_occ=257), dict(alpha_occ=-1), dict(first=-1),
           dict(first=4), dict(G=2), dict(pitch0=11), dict(pitch1=11), dict(step0=119), dict(step1=59), dict(p0=None), dict(p1=None),
           dict(trajs=None), dict(colors=None), dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=0x5004),
           dict(format=5), dict(format=5, p2=0x6000, pitch2=5, step2=30), dict(format=5, p2=0x6000, pitch2=6, step2=29),
           dict(format=8), dict(format=8, p2=0x6000, pitch2=12, step2=119), dict(format=2, pitch0=47), dict(format=0, pitch0=35),
           dict(fade=table(256, 128, 64, 257)), dict(fade=table(-1, 0, 0, 0)), dict(fade=table(256, 1000, 0, 0))]
    cases = [(GOOD_EX, c) for c in bad]
    # the 16-bit formats: the same list where it applies, minimums counted in bytes of the 16-bit rows, and evenness
    wide = [dict(matrix=2), dict(matrix=-1), dict(range=2), dict(F=-1), dict(n=-1), dict(h=0), dict(trail=33), dict(alpha_vis=257),
            dict(first=4), dict(pitch0=22), dict(pitch0=12), dict(step0=238), dict(p0=None), dict(p1=None), dict(trajs=None),
            dict(workspace_bytes=need - 1), dict(workspace=0x5004), dict(p0=0x1001), dict(pitch0=25, step0=250), dict(step0=241),
            dict(p1=0x2001), dict(fade=table(0, 0, 0, 300))]
    cases += [(GOOD_P010, c) for c in wide + [dict(pitch1=22), dict(pitch1=12), dict(step1=118), dict(pitch1=25, step1=250),
                                              dict(step1=121)]]
    cases += [(GOOD_I010, c) for c in wide + [dict(pitch1=10), dict(pitch2=10), dict(step1=58), dict(step2=58), dict(p2=None),
                                              dict(p2=0x6001), dict(pitch1=13, step1=130), dict(pitch2=13, step2=130), dict(step2=61)]]
    for base, change in cases:
        assert _rc(lib, base, **change) == E_ARG, (base["format"], change)
        assert lib.pips_last_error().decode().startswith("tracks_draw_ex:"), (base["format"], change)
    # formats 6 and 7 are legal here with good, even arguments; odd ones are legal for the 8-bit formats
    assert _rc(lib, GOOD_P010, F=0) == 0 and _rc(lib, GOOD_I010, F=0) == 0 and _rc(lib, GOOD_P010, F=0, fade=ok) == 0
    assert _rc(lib, GOOD_EX, F=0, p0=0x1001, pitch0=13, step0=131) == 0
    assert _rc(lib, GOOD_EX, format=0, matrix=7, range=7, pitch0=36, step0=360, F=0) == 0
    assert _rc(lib, GOOD_P010, F=0, line8=-5, dot8=-1, h=8192, w=8192, pitch0=16384, pitch1=16384, step0=16384 * 8192, step1=16384 * 4096) == 0
    # pips_tracks_draw is not touched: the two formats stay illegal there
    a6 = dict(GOOD, format=6, pitch0=24, step0=240, pitch1=24, step1=120)
    assert lib.pips_tracks_draw(*[a6[k] for k in GOOD]) == E_ARG and lib.pips_last_error().decode().startswith("tracks_draw:")


def test_python_layers_reject_bad_arguments_ex():
    h, w = 12, 16
    t = torch.tensor([(3.0, 3.0), (9.0, 7.0), (13.0, 9.0)]).view(1, 3, 1, 2)
    p8 = views(buffers("nv12", 1, h, w, 3), "nv12", h, w)
    p16 = views(buffers16("p010", 1, h, w, 3), "p010", h, w)
    draw = lambda planes, fmt, **kw: drivers.draw_tracks_torch(planes, fmt, t, first=2, trail=2, **kw)
    draw(p8, "nv12", fade=[1.0, 0.5]), draw(p16, "p010", fade="linear"), draw(p16, "p010", fade=torch.tensor([1.0, 0.0]))
    for fade in ([1.0], [1.0, 0.5, 0.25], [1.0, 1.5], [-0.1, 1.0], [1.0, float("nan")], "cubic", [True, 1.0], ["1", "0"]):
        with pytest.raises(ValueError):
            draw(p8, "nv12", fade=fade)
        with pytest.raises(ValueError):
            drivers.TrackPainter((h, w), trail=2, fade=fade)
    drivers.TrackPainter((h, w), trail=2, fade="linear"), drivers.TrackPainter((h, w), trail=0, fade=[])
    with pytest.raises(ValueError):
        draw(p8, "p010")                                            # uint8 planes given as p010
    with pytest.raises(ValueError):
        draw(p16, "nv12")
    with pytest.raises(ValueError):
        draw(p16, "i010")                                           # two planes where the format has three
    with pytest.raises(ValueError):
        draw([p16[0], p16[1][:, :, :-1]], "p010")
    with pytest.raises(ValueError):
        draw(p16, "p016")
    # ops: the table in the rule's integers
    assert ops.draw_fade(None, 3) is None and ops.draw_fade([256, 0, 7], 3) == [256, 0, 7] and ops.draw_fade([], 0) == []
    for fade, trail in (([256], 2), ([257, 0], 2), ([-1, 0], 2), ([0.5, 0], 2), ([True, 0], 2)):
        with pytest.raises(ValueError):
            ops.draw_fade(fade, trail)
    # a view whose strides cannot be pitch and step cannot be drawn on in place: every second column, a transposed plane, frames
    # that overlap (an int16 tensor cannot state an odd pitch in bytes: the library's own check is met through raw pointers above)
    full = buffers16("p010", 2, h, w, 4, pad=(6, 2))
    good = views(full, "p010", h, w)
    args = ops.draw_surfaces(good, "p010")
    assert args[1:3] == [2 * (w + 6), 2 * (w + 6) * (h + 2)] and args[4:6] == [2 * 2 * (w // 2 + 6), 2 * 2 * (w // 2 + 6) * (h // 2 + 2)]
    assert args[6:] == [None, 0, 0] and all(a % 2 == 0 for a in args[1:3] + args[4:6])
    for bad in (full[0][:, :h, ::2][:, :, :w // 2], full[0].transpose(1, 2)[:, :h, :w], full[0][:1].expand(2, -1, -1)[:, :h, :w]):
        with pytest.raises(ValueError):
            ops.draw_surfaces([bad, good[1]], "p010")
    assert set(ops.DRAW_FORMATS_EX) == set(ops.DRAW_FORMATS) | set(WIDE) and (ops.DRAW_FORMATS_EX["p010"], ops.DRAW_FORMATS_EX["i010"]) == (6, 7)


# ----------------------------------------------------------------------------------------------------------- TrackPainter
def test_painter_on_p010_with_a_linear_fade_is_one_whole_video_call():
    """tests/test_draw.py's scheme: three pushes of 3, 4 and 3 frames; identity 1 leaves after the first, identity 4 joins in the
    second: the painter's words are those of one draw_tracks_torch over the video with trajs by identity"""
    fmt, h, w, T, K, trail = "p010", 20, 28, 10, 5, 4
    g = torch.Generator().manual_seed(9)
    trajs = torch.rand(1, 1, K, 2, generator=g) * torch.tensor([w - 8.0, h - 8.0]) + 4 + torch.randn(1, T, K, 2, generator=g).cumsum(1) * 1.5
    vis = torch.randn(1, T, K, generator=g)
    trajs[0, 3:, 1] = NAN                                           # retired on frame 2
    trajs[0, :4, 4] = NAN                                           # born on frame 4
    style = dict(width=1.5, dot=2.0, alpha=0.8, alpha_occ=0.3, vis_thr=0.4, matrix="bt601", range="full")
    bufs = buffers16(fmt, T, h, w, 12)
    planes = views(bufs, fmt, h, w)
    want = _twin(planes, fmt, trajs, vis, colors=drivers.track_colors(torch.arange(K)), trail=trail, fade="linear", **style)
    plain = _twin(planes, fmt, trajs, vis, colors=drivers.track_colors(torch.arange(K)), trail=trail, **style)
    assert any(not torch.equal(a, b) for a, b in zip(want, plain)) and any(not torch.equal(a, b) for a, b in zip(want, planes))
    painter = drivers.TrackPainter((h, w), trail=trail, engine="torch", fade="linear", **style)
    got = []
    for (a, b), ids in zip(((0, 3), (3, 7), (7, 10)), ([0, 1, 2, 3], [0, 2, 3, 4], [0, 2, 3, 4])):
        out = painter.paint([p[a:b] for p in planes], fmt, a, trajs[:, a:b][:, :, ids], vis[:, a:b][:, :, ids], ids=torch.tensor(ids),
                            inplace=False)
        got.append(out)
    for k in range(len(planes)):
        assert torch.equal(torch.cat([p[k] for p in got]), want[k])


# ------------------------------------------------------------------------------------------ the cases of the GPU grid
# (fmt, matrix, range, h, w, F, n, trail, src, style, fade, pad): test_draw's case with the fade (None, "linear" or floats) and the
# padding of the allocation -- elements a row, rows a frame -- behind it
NON_MONOTONE = lambda trail: [(0.25, 1.0, 0.0, 0.5)[a % 4] for a in range(trail)]
ZEROS = lambda trail: [0.0] * trail
PADS = {(16, 16): (0, 0), (17, 33): (1, 2), (37, 51): (32, 1)}       # pitches of +0, +2 and +64 bytes; the last two step over rows


def format_cases_ex():
    """P010 and I010 under the four matrix / range rows at one tile, at a one-pixel row and column of tiles and at a size odd both
    ways; F = 3, five tracks, trail 4, without a fade and with the linear one"""
    return [(fmt, m, r, h, w, 3, 5, 4, None, STYLE, fade, PADS[(h, w)])
            for fmt in WIDE for m, r in ROWS for h, w in PADS for fade in (None, "linear")]


def grid_cases_ex():
    """37x51: P010 without a fade, BGRA and NV12 with one -- linear, non-monotone and all-zero in turn -- over n in {0, 1, 5, 300} x
    trail in {0, 1, 4, 32} x positions in surface pixels and in those of a 24x32 model frame"""
    out = []
    for fmt in ("p010", "bgra32", "nv12"):
        for a, n in enumerate((0, 1, 5, 300)):
            for b, trail in enumerate((0, 1, 4, 32)):
                for c, src in enumerate((None, (24, 32))):
                    kind = (a + b + c + (fmt == "nv12")) % 3
                    fade = None if fmt == "p010" else ("linear", NON_MONOTONE(trail), ZEROS(trail))[kind]
                    heads = fmt != "p010" and kind == 2              # an all-zero table draws heads alone: fat ones, to be seen
                    style = THIN if n == 300 else FAT if n == 1 or heads else STYLE
                    out.append((fmt, "bt601", "full", 37, 51, 3, n, trail, src, style, fade, (5, 2)))
    return out


def case_id_ex(c):
    fmt, matrix, range_, h, w, F, n, trail, src, _, fade, _ = c
    kind = "plain" if fade is None else fade if isinstance(fade, str) else "zeros" if not any(fade) else "nonmono"
    return f"{fmt}-{matrix}-{range_}-{h}x{w}-n{n}-t{trail}-{kind}" + ("" if src is None else f"-from{src[0]}x{src[1]}")


def case_inputs_ex(c, with_vis=True):
    """test_draw.case_inputs with the fade among the keywords and 16-bit allocations where the format asks for them"""
    fmt, matrix, range_, h, w, F, n, trail, src, style, fade, pad = c
    G = max(trail, 6) + F + 2
    seed = 1000 * h + 10 * w + n + trail
    trajs, vis = tracks(G, n, h, w, seed, src)
    kw = dict(size=src, first=G - F - 1, trail=trail, matrix=matrix, range=range_, fade=fade, **style)
    return any_buffers(fmt, F, h, w, seed + 1, pad), trajs, (vis if with_vis else None), kw


def not_vacuous_ex(c, before, after, trajs, kw):
    """test_draw.not_vacuous on the twin's output, and of a case with a fade and at least five tracks: a pixel whose faded
    coverage is partial (0 < Wp < 1024)"""
    fmt, _, _, h, w, F, n, trail, src, style, fade, _ = c
    ok, what = not_vacuous(c[:10], before, after, trajs, kw)
    if fade is not None and n >= 5:
        table = drivers._draw_fade(fade, trail)
        line8, dot8 = int(math.floor(4 * style["width"] + 0.5)), int(math.floor(8 * style["dot"] + 0.5))
        Wp = [drivers.draw_coverage_torch(trajs[0], kw["first"] + f, h, w, src or (h, w), trail, line8, dot8, table) for f in range(F)]
        what["faded_partial"] = any(bool(((k > 0) & (k < 1024)).any()) for k in Wp)
        ok = ok and what["faded_partial"]
    return ok, what


def _light(c):                                                      # (300 tracks with 33 points each: once on the CPU)
    return not (c[6] == 300 and c[7] == 32 and c[0] != "nv12")


@pytest.mark.parametrize("case", [c for c in format_cases_ex() + grid_cases_ex() if _light(c)], ids=case_id_ex)
def test_the_gpu_cases_are_not_vacuous_ex(case):
    """the seeds of tests/test_draw_ex_gpu.py's grids: the twin's output shows partial coverage, overlap, partial chroma coverage and
    a changed share of 2 % .. 60 % of the luma samples (pixels for BGRA), faded cases partial faded coverage too"""
    fmt, h, w = case[0], case[3], case[4]
    bufs, trajs, vis, kw = case_inputs_ex(case)
    planes = views(bufs, fmt, h, w)
    after = _twin(planes, fmt, trajs, vis, None, **kw)
    ok, what = not_vacuous_ex(case, planes, after, trajs, kw)
    assert ok, what
