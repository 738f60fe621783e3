"""CPU: the antialiasing triangle filter and the 10-bit formats of pips_frames_import_ex (include/pips_hip.h) in their torch twin,
drivers.import_frames_torch(..., antialias=True) and fmt "p010" / "i010".  The filter is restated pixel by pixel on Python
Fractions and held to torch's own antialiased bilinear within the rounding of its 8.8 fixed point; its accumulator bounds are
summed up at the worst admitted shape; the 10-bit constants are recomputed from Kr / Kb and the fixed-point matrix is held to the
fp64 formula within one level.  (The kernels: tests/test_import_aa_gpu.py.)"""
import ctypes
import math
import os
import re
from fractions import Fraction

import pytest
import torch

from pips_amd import drivers, ops
from test_import import KRKB, MATRICES, RANGES, ROOT, source

FORMATS16 = ["p010", "i010"]
COMBOS = [(m, r) for m in MATRICES for r in RANGES]


def source16(fmt, F, h, w, seed, pitch_pad=0, step_pad=0):
    """random planes of ``fmt`` ("p010" / "i010") as uint16: all 16 bits of every word random, so the six bits a format does not
    read are too; views of wider and taller allocations as ``source``'s"""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    shapes = [(h, w), (ch, cw, 2)] if fmt == "p010" else [(h, w), (ch, cw), (ch, cw)]
    planes = []
    for s in shapes:
        full = torch.randint(0, 65536, (F, s[0] + step_pad, s[1] + pitch_pad) + s[2:], generator=g).to(torch.uint16)
        planes.append(full[:, :s[0], :s[1]])
    return planes


def _ints(p):
    """a uint16 (or int16) plane as int64 0..65535"""
    return p.view(torch.int16).to(torch.int64) & 0xFFFF


def restate16(planes, fmt, matrix, range_):
    """the 10-bit rule of the header, pixel by pixel on Python integers -> (F,3,h,w) uint8"""
    F, h, w = planes[0].shape[:3]
    P = [_ints(p).tolist() for p in planes]
    ten = (lambda v: v >> 6) if fmt == "p010" else (lambda v: v & 1023)
    out = torch.zeros(F, 3, h, w, dtype=torch.uint8)
    y0, ky, rv, gu, gv, bu = drivers.YUV10_RULES[(matrix, range_)]
    clamp = lambda v: min(max(v, 0), 255)
    for f in range(F):
        for y in range(h):
            for x in range(w):
                Y = ten(P[0][f][y][x])
                if fmt == "p010":
                    Cb, Cr = (ten(v) for v in P[1][f][y >> 1][x >> 1])
                else:
                    Cb, Cr = ten(P[1][f][y >> 1][x >> 1]), ten(P[2][f][y >> 1][x >> 1])
                c, d, e = Y - y0, Cb - 512, Cr - 512
                rgb = [clamp((ky * c + rv * e + (1 << 17)) >> 18), clamp((ky * c + gu * d + gv * e + (1 << 17)) >> 18),
                       clamp((ky * c + bu * d + (1 << 17)) >> 18)]
                for k in range(3):
                    out[f, k, y, x] = rgb[k]
    return out


def _raw(i, j, n, N):
    return max(0, 2 * max(n, N) - abs((2 * j + 1) * N - (2 * i + 1) * n))


def triangle_restated(u8, H, W):
    """the filter of the header on (F,3,h,w) uint8, pixel by pixel over ALL source pixels on exact rationals -> q (F,3,H,W) int64"""
    F, _, h, w = u8.shape
    P = u8.tolist()
    ry = [[_raw(i, j, h, H) for j in range(h)] for i in range(H)]
    rx = [[_raw(i, j, w, W) for j in range(w)] for i in range(W)]
    q = torch.zeros(F, 3, H, W, dtype=torch.int64)
    for f in range(F):
        for c in range(3):
            for Y in range(H):
                for X in range(W):
                    num = sum(ry[Y][y] * rx[X][x] * P[f][c][y][x] for y in range(h) if ry[Y][y] for x in range(w) if rx[X][x])
                    v = Fraction(num, sum(ry[Y]) * sum(rx[X]))                   # the filtered value, exactly
                    q[f, c, Y, X] = math.floor(v * 256 + Fraction(1, 2))         # 8.8 fixed point, round half up
    return q


SHAPES = [((3, 5), (2, 2)), ((7, 4), (7, 2)), ((37, 53), (8, 12)), ((30, 40), (45, 16))]


def _planes(fmt, F, h, w, seed):
    return source16(fmt, F, h, w, seed, 3, 1) if fmt in FORMATS16 else source(fmt, F, h, w, seed, 3, 1)


@pytest.mark.parametrize("fmt", ["bgr24", "nv12", "i010"])
@pytest.mark.parametrize("src,dst", SHAPES + [((16, 20), (16, 20))])
def test_twin_is_the_filter_pixel_by_pixel(fmt, src, dst):
    F = 1 if src == (37, 53) else 2
    planes = _planes(fmt, F, src[0], src[1], 11 + src[0])
    plain = drivers.import_frames_torch(planes, fmt, None, "bt601", "limited")
    q = triangle_restated(plain, *dst)
    got = drivers.import_frames_torch(planes, fmt, dst, "bt601", "limited", torch.float32, antialias=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (F, 3) + dst
    assert torch.equal(got, q.float() / 256.0) and torch.equal((got * 256.0).to(torch.int64), q)       # q / 256 is exact in fp32
    as_u8 = drivers.import_frames_torch(planes, fmt, dst, "bt601", "limited", antialias=True)
    assert as_u8.dtype == torch.uint8 and torch.equal(as_u8, ((q + 128) >> 8).to(torch.uint8))
    if src == dst:                                                                                     # the plain conversion, exactly
        assert torch.equal(as_u8, plain) and torch.equal(got, plain.float())
        assert torch.equal(drivers.import_frames_torch(planes, fmt, None, "bt601", "limited", antialias=True), plain)


@pytest.mark.parametrize("fmt", ["rgb24", "p010"])
@pytest.mark.parametrize("src,dst", SHAPES + [((270, 480), (92, 124))])
def test_twin_is_torchs_antialiased_bilinear_within_the_rounding_of_q(fmt, src, dst):
    planes = _planes(fmt, 2, src[0], src[1], 5 + src[1])
    plain = drivers.import_frames_torch(planes, fmt, None, "bt709", "full")
    got = drivers.import_frames_torch(planes, fmt, dst, "bt709", "full", torch.float32, antialias=True)
    ref = torch.nn.functional.interpolate(plain.double(), dst, mode="bilinear", antialias=True, align_corners=False)
    assert float((got.double() - ref).abs().max()) <= 1.0 / 512 + 1e-9
    # the outputs' relations: the uint8 output is floor(float + 0.5); values in [0, 255] on the 1/256 grid
    as_u8 = drivers.import_frames_torch(planes, fmt, dst, "bt709", "full", antialias=True)
    assert torch.equal(as_u8, (got + 0.5).floor().to(torch.uint8))
    assert float(got.min()) >= 0.0 and float(got.max()) <= 255.0 and torch.equal(got * 256.0, (got * 256.0).round())


def test_equal_size_on_one_axis_is_identity_on_that_axis():
    (p,) = source("rgb24", 1, 9, 14, 4)
    got = drivers.import_frames_torch(p, "rgb24", (9, 5), dtype=torch.float32, antialias=True)
    by_row = [drivers.import_frames_torch(p[:, y:y + 1], "rgb24", (1, 5), dtype=torch.float32, antialias=True) for y in range(9)]
    assert torch.equal(got, torch.cat(by_row, dim=2))
    # scaling up is the two-tap bilinear with the clamped edge: the weights of output i are those of align_corners=False
    idx, wgt = drivers.triangle_taps(5, 8)
    assert idx.shape[1] == 2 and idx[0].tolist() == [0, 1] and wgt[0, 1] == 0 and wgt[7, 1] == 0 and bool((wgt.sum(1)[1:7] == 16).all())
    ref = torch.nn.functional.interpolate(torch.arange(5.0).double().view(1, 1, 1, 5), (1, 8), mode="bilinear")
    assert torch.allclose((idx * wgt).sum(1).double() / wgt.sum(1), ref.view(-1), atol=1e-12)


def test_accumulators_stay_in_their_types_at_the_worst_admitted_shape():
    """(8192, 8192) -> (512, 512): the largest sizes at the largest ratio, summed from the weight tables without an image.  A weight
    sum along an axis stays below 2^19, a row sum of 255s below 2^27 (int32), 512 num below 2^55 (int64) and den below 2^38"""
    assert ops.FILTER_DIM_MAX == 8192
    for n, N in ((8192, 512), (8191, 512), (8192, 8191), (4097, 8192), (16, 1), (8192, 8192), (1, 8192)):
        idx, wgt = drivers.triangle_taps(n, N)
        assert idx.shape[1] <= 2 * -(-max(n, N) // N) + 1 and int(idx.min()) >= 0 and int(idx.max()) <= n - 1
        assert bool((wgt[:, 0] > 0).all()) and bool((wgt >= 0).all())
        total = wgt.sum(dim=1)
        assert int(total.min()) >= 1 and int(total.max()) < 2 ** 19
        assert 255 * int(total.max()) < 2 ** 27 < 2 ** 31
        assert 512 * 255 * int(total.max()) ** 2 < 2 ** 55 and 2 * int(total.max()) ** 2 < 2 ** 39
        assert (2 * n - 1) * N + 2 * max(n, N) < 2 ** 31 and (2 * N - 1) * n + 2 * max(n, N) < 2 ** 31      # the weight itself, in int32
    idx, wgt = drivers.triangle_taps(8192, 512)
    assert int(wgt.sum(dim=1).max()) == 2 ** 18                                   # 2 m = 16384 high, 32 samples wide
    # a frame of 255s keeps its value: q = 65280 everywhere, whatever the weights
    y = torch.full((1, 1, 31, 47, 3), 255, dtype=torch.uint8)[0]
    assert bool((drivers.import_frames_torch(y, "rgb24", (2, 3), dtype=torch.float32, antialias=True) == 255.0).all())


def test_antialias_removes_the_moire_of_a_checkerboard():
    h, w, H, W = 270, 480, 92, 124
    board = (((torch.arange(h).view(h, 1) + torch.arange(w).view(1, w)) % 2) * 255).to(torch.uint8)
    p = board.view(1, h, w, 1).expand(1, h, w, 3)
    aa = drivers.import_frames_torch(p, "rgb24", (H, W), dtype=torch.float32, antialias=True)
    plain = drivers.import_frames_torch(p, "rgb24", (H, W), dtype=torch.float32)
    assert float(aa.min()) >= 126.0 and float(aa.max()) <= 130.0
    assert float(plain.std()) > 20.0
    assert torch.equal(plain, drivers.import_frames_torch(p, "rgb24", (H, W), dtype=torch.float32, antialias=False))   # the default


# ------------------------------------------------------------------------------------------------------------------- 10-bit
def test_ten_bit_constants_are_the_rounded_standard_coefficients():
    for matrix, (kr, kb) in KRKB.items():
        kg = 1.0 - kr - kb
        for range_ in RANGES:
            ys, cs = (255.0 / 876.0, 255.0 / 896.0) if range_ == "limited" else (255.0 / 1023.0, 255.0 / 1023.0)
            real = [ys, 2 * (1 - kr) * cs, -2 * kb * (1 - kb) / kg * cs, -2 * kr * (1 - kr) / kg * cs, 2 * (1 - kb) * cs]
            want = (64 if range_ == "limited" else 0,) + tuple(math.floor(2 ** 18 * k + 0.5) for k in real)
            assert drivers.YUV10_RULES[(matrix, range_)] == want, (matrix, range_)
            if range_ == "limited":                                              # the 8-bit constants
                assert want[1:] == drivers.YUV_RULES[(matrix, range_)][1:]
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    yuv = open(os.path.join(ROOT, "pips_amd", "csrc", "yuv.h")).read()
    for (matrix, range_), rule in drivers.YUV10_RULES.items():
        row = r"\s+".join(str(v) for v in rule[1:])
        assert re.search(r"10-bit PIPS_MATRIX_%s %s\s+%s" % (matrix.upper(), range_, row), hdr), (matrix, range_)
        assert "{%s}" % ", ".join(str(v) for v in rule) in yuv


def test_every_ten_bit_accumulator_stays_in_int32():
    for (y0, ky, rv, gu, gv, bu) in drivers.YUV10_RULES.values():
        lo = hi = 0
        for terms in ((rv, 0), (gu, gv), (bu, 0)):
            for c in (-y0, 1023 - y0):
                acc = [ky * c + terms[0] * d + terms[1] * e + (1 << 17) for d in (-512, 511) for e in (-512, 511)]
                lo, hi = min(lo, *acc), max(hi, *acc)
        assert -2 ** 31 <= -7.7e7 <= lo and hi <= 1.5e8 <= 2 ** 31 - 1


def _exact10(Y, Cb, Cr, matrix, range_):
    """clamp(floor(exact + 0.5)) of the real-valued 10-bit formula in fp64: (n,) int64 each -> (n,3)"""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = (255.0 / 876.0, 255.0 / 896.0, 64) if range_ == "limited" else (255.0 / 1023.0, 255.0 / 1023.0, 0)
    c, d, e = (Y - y0).double() * ys, (Cb - 512).double() * cs, (Cr - 512).double() * cs
    rgb = torch.stack([c + 2 * (1 - kr) * e, c - 2 * kb * (1 - kb) / kg * d - 2 * kr * (1 - kr) / kg * e, c + 2 * (1 - kb) * d], dim=1)
    return (rgb + 0.5).floor().clamp(0, 255).to(torch.int64)


def _twin_triples16(Y, Cb, Cr, matrix, range_, fmt="i010"):
    """the twin on n triples as one frame of 1 x 2n pixels whose pixel pairs share a chroma sample -> (n,3) int64"""
    n = Y.numel()
    word = (lambda v: (v << 6).to(torch.uint16)) if fmt == "p010" else (lambda v: v.to(torch.uint16))
    y = word(Y).repeat_interleave(2).view(1, 1, 2 * n)
    if fmt == "p010":
        planes = (y, torch.stack([word(Cb), word(Cr)], dim=-1).view(1, 1, n, 2))
    else:
        planes = (y, word(Cb).view(1, 1, n), word(Cr).view(1, 1, n))
    out = drivers.import_frames_torch(planes, fmt, None, matrix, range_)
    assert torch.equal(out[..., 0::2], out[..., 1::2])
    return out[0, :, 0, 0::2].t().to(torch.int64)


@pytest.mark.parametrize("matrix,range_", COMBOS)
def test_ten_bit_twin_is_within_one_level_of_the_fp64_formula(matrix, range_):
    Y = torch.arange(1024)
    grey = torch.full((1024,), 512)
    got = _twin_triples16(Y, grey, grey, matrix, range_)
    assert int((got - _exact10(Y, grey, grey, matrix, range_)).abs().max()) <= 1
    assert bool((got[:, 0] == got[:, 1]).all()) and bool((got[:, 1] == got[:, 2]).all())           # grey stays grey
    if range_ == "limited":
        assert got[64].tolist() == [0, 0, 0] and got[940].tolist() == [255, 255, 255]
        assert got[:64].max() == 0 and got[940:].min() == 255
    else:
        assert got[0].tolist() == [0, 0, 0] and got[1023].tolist() == [255, 255, 255]
    # a lattice of triples (every 33rd level, and the last) and the extremes of every sample
    ax = torch.tensor(sorted(set(range(0, 1024, 33)) | {1, 63, 64, 511, 512, 513, 940, 960, 1022, 1023}))
    Y, Cb, Cr = (t.reshape(-1) for t in torch.meshgrid(ax, ax, ax, indexing="ij"))
    for fmt in FORMATS16:
        diff = (_twin_triples16(Y, Cb, Cr, matrix, range_, fmt) - _exact10(Y, Cb, Cr, matrix, range_)).abs()
        assert int(diff.max()) <= 1


@pytest.mark.parametrize("fmt", FORMATS16)
def test_ten_bit_twin_is_the_rule_pixel_by_pixel(fmt):
    for h, w in ((1, 1), (3, 5), (7, 4)):
        for F, pads in ((0, (0, 0)), (2, (5, 2))):
            planes = source16(fmt, F, h, w, 100 * h + w + F, *pads)
            for matrix, range_ in COMBOS:
                want = restate16(planes, fmt, matrix, range_)
                got = drivers.import_frames_torch(planes, fmt, None, matrix, range_)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (F, 3, h, w) and torch.equal(got, want), (fmt, h, w, F)
                assert torch.equal(drivers.import_frames_torch(planes, fmt, None, matrix, range_, torch.float32), want.float())
                # int16 planes holding the same bits are the same frames
                assert torch.equal(drivers.import_frames_torch([p.view(torch.int16) for p in planes], fmt, None, matrix, range_), want)


@pytest.mark.parametrize("matrix", MATRICES)
def test_ten_bit_samples_of_four_times_the_bytes_import_as_the_eight_bit_surface(matrix):
    """limited range: the constants are the 8-bit ones and 2^17 / 2^18 the same half, so (4 v) converts as v does.  Full range
    differs by design: 4 x 255 = 1020 is not the 10-bit white 1023, and the constants are scaled by 255/1023, not by 1/4"""
    for fmt8, fmt16 in (("nv12", "p010"), ("i420", "i010")):
        planes = source(fmt8, 2, 37, 53, 8)
        word = (lambda p: (p.to(torch.int32) << 8).to(torch.uint16)) if fmt16 == "p010" else (lambda p: (p.to(torch.int32) << 2).to(torch.uint16))
        wide = [word(p) for p in planes]
        assert torch.equal(drivers.import_frames_torch(wide, fmt16, None, matrix, "limited"),
                           drivers.import_frames_torch(planes, fmt8, None, matrix, "limited"))
        for kw in (dict(size=(16, 20), dtype=torch.float32), dict(size=(8, 12), dtype=torch.float32, antialias=True)):
            assert torch.equal(drivers.import_frames_torch(wide, fmt16, matrix=matrix, **kw),
                               drivers.import_frames_torch(planes, fmt8, matrix=matrix, **kw))
        assert not torch.equal(drivers.import_frames_torch(wide, fmt16, None, matrix, "full"),
                               drivers.import_frames_torch(planes, fmt8, None, matrix, "full"))


def test_the_six_bits_a_format_does_not_read_are_ignored():
    g = torch.Generator().manual_seed(12)
    for fmt, mask in (("p010", 0xFFC0), ("i010", 0x03FF)):
        planes = source16(fmt, 2, 9, 14, 3)
        want = drivers.import_frames_torch(planes, fmt)
        for fill in (0, 0xFFFF, None):
            junk = [torch.randint(0, 65536, p.shape, generator=g) if fill is None else torch.full(p.shape, fill) for p in planes]
            other = [((_ints(p) & mask) | (j & ~mask & 0xFFFF)).to(torch.uint16) for p, j in zip(planes, junk)]
            assert torch.equal(drivers.import_frames_torch(other, fmt), want)
        cleared = [(_ints(p) & mask).to(torch.uint16) for p in planes]
        assert any(not torch.equal(_ints(a), _ints(b)) for a, b in zip(cleared, planes))            # (the bits were there)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_raise_value_error():
    y, uv = torch.zeros(2, 6, 8, dtype=torch.uint8), torch.zeros(2, 3, 4, 2, dtype=torch.uint8)
    y16, uv16, u16 = y.to(torch.uint16), uv.to(torch.uint16), uv[..., 0].to(torch.uint16)
    for fn in (drivers.import_frames_torch, ops.import_frames):
        for args in (((y, uv), "p010"), ((y16, uv), "p010"), ((y, uv[..., 0], uv[..., 0]), "i010"), ((y16.view(torch.int16), uv16), "nv12"),
                     ((y16, uv16), "nv12"), ((y16, u16, u16), "i420"), ((y16, uv16.float()), "p010"), ((y16.to(torch.int32), uv16), "p010"),
                     ((y16, u16, u16), "p010"), ((y16, uv16), "i010"), ((y16, uv16[:, :2]), "p010"), ((y16, u16, uv16), "i010"),
                     ((y16,), "p010"), ((y16[0], uv16[0]), "p010")):
            with pytest.raises(ValueError):
                fn(*args)
        for kw in (dict(matrix="bt2020"), dict(range="tv"), dict(size=(0, 4), antialias=True)):
            with pytest.raises(ValueError):
                fn((y16, uv16), "p010", **kw)
    big = torch.zeros(1, 1, 8200, 3, dtype=torch.uint8)
    for fn in (drivers.import_frames_torch, ops.import_frames):
        for planes, size in ((big, (1, 4100)), (big[:, :, :8192], (1, 511)), (big[:, :, :33].transpose(1, 2), (2, 1)),
                             (big[:, :, :4], (1, 8193)), (big[:, :, :4], (8193, 4))):
            with pytest.raises(ValueError):
                fn(planes, "rgb24", size, antialias=True)
    # the limits are the filter's: the default takes the same sizes, and an equal size runs no filter
    assert tuple(drivers.import_frames_torch(big[:, :, :33].transpose(1, 2), "rgb24", (2, 1)).shape) == (1, 3, 2, 1)
    assert tuple(drivers.import_frames_torch(big, "rgb24", None, antialias=True).shape) == (1, 3, 1, 8200)
    assert tuple(drivers.import_frames_torch(big[:, :, :32].transpose(1, 2), "rgb24", (2, 1), antialias=True).shape) == (1, 3, 2, 1)
    assert tuple(drivers.import_frames_torch((y16[:0], uv16[:0]), "p010", (5, 7), antialias=True).shape) == (0, 3, 5, 7)


def test_frames_import_ex_is_declared_bound_and_exported():
    from pips_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_frames_import_ex" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)   # the history comment
    for name, value in (("FMT_P010", 6), ("FMT_I010", 7), ("FILTER_BILINEAR", 0), ("FILTER_TRIANGLE", 1), ("FILTER_DIM_MAX", 8192)):
        assert re.search(r"#define\s+PIPS_%s\s+%d\b" % (name, value), hdr), name
    assert ops.IMPORT_FORMATS["p010"] == 6 and ops.IMPORT_FORMATS["i010"] == 7
    assert (ops.FILTER_BILINEAR, ops.FILTER_TRIANGLE) == (0, 1)
    limits = re.search(r"Known limits:.*?\*/", hdr, flags=re.S).group(0)
    assert "two extra bits" in limits and "BT.2020" in limits
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_frames_import_ex\s*\(([^)]*)\)\s*;", bare)
    assert proto is not None and len(proto.group(1).split(",")) == 21
    res, args = _lib.SIGNATURES["pips_frames_import_ex"]
    assert res is ctypes.c_int and len(args) == 21 and args[:7] == [ctypes.c_int] * 7
    assert args[7:16] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t] * 3
    assert args[16:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pips_frames_import_ex")
    lib = _lib.load()
    assert lib.pips_abi_version() == 3

    # the host-side rejections need no device: nothing is launched (the pointers are never read)
    def call(fmt=6, matrix=1, range_=0, filt=0, F=2, h=6, w=9, p=(8, 8, 0), pitch=(18, 20, 0), step=(108, 60, 0), dst=8, H=6, W=9):
        return lib.pips_frames_import_ex(fmt, matrix, range_, filt, F, h, w, p[0] or None, pitch[0], step[0], p[1] or None, pitch[1],
                                         step[1], p[2] or None, pitch[2], step[2], dst or None, 1, H, W, None)

    i010 = dict(fmt=7, p=(8, 8, 8), pitch=(18, 10, 10), step=(108, 30, 30))
    nv12 = dict(fmt=4, pitch=(9, 10, 0), step=(54, 30, 0))
    assert call(F=0) == 0 and call(F=0, p=(0, 0, 0), dst=0) == 0 and call(**dict(i010, F=0)) == 0 and call(**dict(nv12, F=0)) == 0
    assert call(F=0, filt=1, H=3, W=4) == 0 and call(**dict(nv12, F=0, filt=1, h=8192, w=16, pitch=(16, 16, 0), step=(1 << 20, 1 << 20, 0),
                                                            H=512, W=1)) == 0
    for over in (dict(fmt=-1), dict(fmt=8), dict(filt=2), dict(filt=-1), dict(matrix=2), dict(range_=-1), dict(F=-1), dict(h=0), dict(W=-2),
                 dict(dst=0), dict(p=(0, 8, 0)), dict(p=(8, 0, 0)), dict(H=1 << 15, W=1 << 15),
                 dict(pitch=(16, 20, 0)), dict(pitch=(18, 18, 0)), dict(step=(106, 60, 0)), dict(step=(108, 58, 0)),
                 dict(p=(9, 8, 0)), dict(p=(8, 9, 0)), dict(pitch=(19, 20, 0), step=(120, 60, 0)), dict(pitch=(18, 21, 0), step=(108, 64, 0)),
                 dict(step=(109, 60, 0)), dict(step=(108, 61, 0)), dict(F=1, p=(8, 7, 0)), dict(F=1, step=(1, 0, 0)),
                 dict(i010, p=(8, 8, 0)), dict(i010, p=(8, 8, 9)), dict(i010, pitch=(18, 10, 8)), dict(i010, pitch=(18, 10, 11), step=(108, 30, 34)),
                 dict(i010, step=(108, 30, 31)),
                 dict(filt=1, H=1 << 14, W=9), dict(filt=1, F=1, H=6, W=8193), dict(filt=1, F=1, h=97, pitch=(18, 20, 0), H=6),
                 dict(nv12, filt=1, F=1, w=8193, pitch=(8193, 8194, 0), W=4096), dict(nv12, filt=1, F=1, w=161, pitch=(161, 162, 0), W=10),
                 dict(nv12, filt=2), dict(nv12, fmt=5)):
        assert call(**over) == -1, over
        assert lib.pips_last_error()
    # an 8-bit format takes odd pointers, pitches and steps through the new entry as through the old one
    assert call(**dict(nv12, F=0, p=(9, 7, 0), pitch=(9, 11, 0), step=(55, 33, 0))) == 0

    def old(fmt):
        return lib.pips_frames_import(fmt, 1, 0, 0, 6, 9, None, 18, 108, None, 20, 60, None, 10, 30, None, 1, 6, 9, None)

    assert old(6) == -1 and lib.pips_last_error() and old(7) == -1 and old(4) == 0
