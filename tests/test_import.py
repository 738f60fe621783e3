"""CPU: decoder frames in -- drivers.import_frames_torch, the torch twin of pips_frames_import (include/pips_hip.h).  The rule is
restated here as a plain-Python loop over the pixels (conversion) and as numpy float32 arithmetic (resize_frames_kernel's resize);
the constants are recomputed from Kr / Kb; the fixed-point matrix is held to the fp64 formula within one level.  (The kernels:
tests/test_import_gpu.py.)"""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from pips_amd import drivers, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgba32": (4, (0, 1, 2)), "bgra32": (4, (2, 1, 0))}
FORMATS = list(PACKED) + ["nv12", "i420"]
MATRICES, RANGES = ["bt601", "bt709"], ["limited", "full"]
KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SIZES = [(1, 1), (2, 2), (3, 5), (7, 4), (37, 53)]


def source(fmt, F, h, w, seed, pitch_pad=0, step_pad=0):
    """random planes of ``fmt``: views [:, :rows, :row elements] of allocations with ``pitch_pad`` more elements a row and
    ``step_pad`` more rows a frame (0, 0: contiguous tensors), the slack filled with other random bytes"""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt in PACKED:
        shapes = [(h, w, PACKED[fmt][0])]
    elif fmt == "nv12":
        shapes = [(h, w), (ch, cw, 2)]
    else:
        shapes = [(h, w), (ch, cw), (ch, cw)]
    planes = []
    for s in shapes:
        full = torch.randint(0, 256, (F, s[0] + step_pad, s[1] + pitch_pad) + s[2:], generator=g, dtype=torch.uint8)
        planes.append(full[:, :s[0], :s[1]])
    return planes


def restate(planes, fmt, matrix, range_):
    """the rule of the header, pixel by pixel on Python integers -> (F,3,h,w) uint8"""
    F, h, w = planes[0].shape[:3]
    P = [p.tolist() for p in planes]
    out = torch.zeros(F, 3, h, w, dtype=torch.uint8)
    y0, ky, rv, gu, gv, bu = drivers.YUV_RULES[(matrix, range_)]
    clamp = lambda v: min(max(v, 0), 255)
    for f in range(F):
        for y in range(h):
            for x in range(w):
                if fmt in PACKED:
                    px = P[0][f][y][x]
                    rgb = [px[k] for k in PACKED[fmt][1]]
                else:
                    Y = P[0][f][y][x]
                    if fmt == "nv12":
                        Cb, Cr = P[1][f][y >> 1][x >> 1]
                    else:
                        Cb, Cr = P[1][f][y >> 1][x >> 1], P[2][f][y >> 1][x >> 1]
                    c, d, e = Y - y0, Cb - 128, Cr - 128
                    rgb = [clamp((ky * c + rv * e + 32768) >> 16), clamp((ky * c + gu * d + gv * e + 32768) >> 16),
                           clamp((ky * c + bu * d + 32768) >> 16)]
                for k in range(3):
                    out[f, k, y, x] = rgb[k]
    return out


def resize_np(u8, H, W):
    """resize_frames_kernel (pips_amd/csrc/encoder.hip) on (F,3,h,w) uint8 as numpy float32 arithmetic: the source index one fused
    multiply-add (checked against exact rationals), every product and sum of the blend rounded once"""
    f32 = np.float32
    p = u8.numpy().astype(f32)
    h, w = p.shape[-2:]

    def taps(n, N):
        s = f32(n) / f32(N)
        exact = [Fraction(float(s)) * Fraction(2 * i + 1, 2) - Fraction(1, 2) for i in range(N)]     # the fused multiply-add, exactly
        wide = np.float64(s) * (np.arange(N) + 0.5) - 0.5
        assert [Fraction(float(v)) for v in wide] == exact          # float64 holds it unrounded: its rounding to float32 is the fused one
        f = np.maximum(wide.astype(f32), f32(0))
        i0 = np.minimum(f.astype(np.int64), n - 1)
        i1 = i0 + (i0 < n - 1)
        l1 = f - i0.astype(f32)
        return i0, i1, f32(1) - l1, l1

    y0, y1, ly0, ly1 = taps(h, H)
    x0, x1, lx0, lx1 = taps(w, W)
    r0, r1 = p[:, :, y0], p[:, :, y1]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    v = ly0[:, None] * top + ly1[:, None] * bot
    assert v.dtype == f32
    return torch.from_numpy(v)


@pytest.mark.parametrize("fmt", FORMATS)
def test_twin_is_the_rule_pixel_by_pixel(fmt):
    combos = [("bt709", "limited")] if fmt in PACKED else [(m, r) for m in MATRICES for r in RANGES]
    for h, w in SIZES:
        for F, pads in ((0, (0, 0)), (1, (0, 0)), (3, (5, 2))):
            planes = source(fmt, F, h, w, 100 * h + w + F, *pads)
            assert F < 3 or h * w == 1 or not planes[0].is_contiguous()
            for matrix, range_ in combos:
                want = restate(planes, fmt, matrix, range_)
                got = drivers.import_frames_torch(planes, fmt, None, matrix, range_)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (F, 3, h, w) and torch.equal(got, want), (fmt, h, w, F)
                as_float = drivers.import_frames_torch(planes, fmt, None, matrix, range_, torch.float32)
                assert as_float.dtype == torch.float32 and torch.equal(as_float, want.float())
                # the views and their contiguous copies are the same frames
                assert torch.equal(drivers.import_frames_torch([p.contiguous() for p in planes], fmt, None, matrix, range_), want)


def test_constants_are_the_rounded_standard_coefficients():
    for matrix, (kr, kb) in KRKB.items():
        kg = 1.0 - kr - kb
        for range_ in RANGES:
            ys, cs = (255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (1.0, 1.0)
            real = [ys, 2 * (1 - kr) * cs, -2 * kb * (1 - kb) / kg * cs, -2 * kr * (1 - kr) / kg * cs, 2 * (1 - kb) * cs]
            want = (16 if range_ == "limited" else 0,) + tuple(math.floor(65536 * k + 0.5) for k in real)
            assert drivers.YUV_RULES[(matrix, range_)] == want, (matrix, range_)
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    yuv = open(os.path.join(ROOT, "pips_amd", "csrc", "yuv.h")).read()
    for (matrix, range_), rule in drivers.YUV_RULES.items():
        row = r"\s+".join(str(v) for v in rule[1:])
        assert re.search(r"PIPS_MATRIX_%s %s\s+%s" % (matrix.upper(), range_, row), hdr), (matrix, range_)    # the table in the header
        assert "{%s}" % ", ".join(str(v) for v in rule) in yuv                                               # and the kernels' copy


def _exact(Y, Cb, Cr, matrix, range_):
    """clamp(floor(exact + 0.5)) of the real-valued formula in fp64: (n,) int64 each -> (n,3)"""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = (255.0 / 219.0, 255.0 / 224.0, 16) if range_ == "limited" else (1.0, 1.0, 0)
    c, d, e = (Y - y0).double() * ys, (Cb - 128).double() * cs, (Cr - 128).double() * cs
    rgb = torch.stack([c + 2 * (1 - kr) * e, c - 2 * kb * (1 - kb) / kg * d - 2 * kr * (1 - kr) / kg * e, c + 2 * (1 - kb) * d], dim=1)
    return (rgb + 0.5).floor().clamp(0, 255).to(torch.int64)


def _twin_triples(Y, Cb, Cr, matrix, range_):
    """the twin on n triples as one I420 frame of 1 x 2n pixels whose pixel pairs share a chroma sample -> (n,3) int64"""
    n = Y.numel()
    y = Y.to(torch.uint8).repeat_interleave(2).view(1, 1, 2 * n)
    u, v = Cb.to(torch.uint8).view(1, 1, n), Cr.to(torch.uint8).view(1, 1, n)
    out = drivers.import_frames_torch((y, u, v), "i420", None, matrix, range_)
    assert torch.equal(out[..., 0::2], out[..., 1::2])
    return out[0, :, 0, 0::2].t().to(torch.int64)


@pytest.mark.parametrize("range_", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_twin_is_within_one_level_of_the_fp64_formula(matrix, range_):
    Y = torch.arange(256)
    grey = torch.full((256,), 128)
    got = _twin_triples(Y, grey, grey, matrix, range_)
    assert int((got - _exact(Y, grey, grey, matrix, range_)).abs().max()) <= 1
    assert bool((got[:, 0] == got[:, 1]).all()) and bool((got[:, 1] == got[:, 2]).all())           # grey stays grey
    if range_ == "full":
        assert got[:, 0].tolist() == list(range(256))                                               # the identity
    else:
        assert got[16].tolist() == [0, 0, 0] and got[235].tolist() == [255, 255, 255]
        assert got[:16].max() == 0 and got[235:].min() == 255
    g = torch.Generator().manual_seed(len(matrix + range_))
    Y, Cb, Cr = (torch.randint(0, 256, (100000,), generator=g) for _ in range(3))
    diff = (_twin_triples(Y, Cb, Cr, matrix, range_) - _exact(Y, Cb, Cr, matrix, range_)).abs()
    assert int(diff.max()) <= 1


def test_every_accumulator_stays_in_int32():
    for (y0, ky, rv, gu, gv, bu) in drivers.YUV_RULES.values():
        lo = hi = 0
        for terms in ((rv, 0), (gu, gv), (bu, 0)):
            for c in (-y0, 255 - y0):
                acc = [ky * c + terms[0] * d + terms[1] * e + 32768 for d in (-128, 127) for e in (-128, 127)]
                lo, hi = min(lo, *acc), max(hi, *acc)
        assert -2 ** 31 <= -1.9e7 <= lo and hi <= 3.6e7 <= 2 ** 31 - 1


def test_packed_formats_return_the_planar_frame_and_ignore_alpha():
    g = torch.Generator().manual_seed(3)
    planar = torch.randint(0, 256, (2, 3, 9, 14), generator=g, dtype=torch.uint8)
    hwc = planar.permute(0, 2, 3, 1)
    alpha = torch.randint(0, 256, (2, 9, 14, 1), generator=g, dtype=torch.uint8)
    assert torch.equal(drivers.import_frames_torch(hwc, "rgb24"), planar)                           # a permuted view, not contiguous
    assert torch.equal(drivers.import_frames_torch(hwc.contiguous(), "rgb24"), planar)
    assert torch.equal(drivers.import_frames_torch(hwc.flip(-1).contiguous(), "bgr24"), planar)
    for a in (alpha, 255 - alpha):
        assert torch.equal(drivers.import_frames_torch(torch.cat([hwc, a], dim=-1), "rgba32"), planar)
        assert torch.equal(drivers.import_frames_torch(torch.cat([hwc.flip(-1), a], dim=-1), "bgra32"), planar)
    # matrix and range are not read
    assert torch.equal(drivers.import_frames_torch(hwc, "rgb24", None, "bt601", "full"), planar)


@pytest.mark.parametrize("fmt", ["nv12", "bgr24", "i420", "rgba32"])
@pytest.mark.parametrize("src,dst", [((3, 5), (8, 8)), ((37, 53), (16, 20)), ((16, 20), (16, 20))])
def test_resize_is_resize_frames_kernels_arithmetic(fmt, src, dst):
    planes = source(fmt, 2, src[0], src[1], 7 + src[0], 3, 1)
    plain = drivers.import_frames_torch(planes, fmt, None, "bt601", "limited")
    got = drivers.import_frames_torch(planes, fmt, dst, "bt601", "limited", torch.float32)
    want = resize_np(plain, *dst)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3) + dst
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if src == dst:
        assert torch.equal(got, plain.float())                                                      # the plain conversion, exactly
    as_u8 = drivers.import_frames_torch(planes, fmt, dst, "bt601", "limited", torch.uint8)
    assert as_u8.dtype == torch.uint8 and torch.equal(as_u8, (got + 0.5).floor().to(torch.uint8))
    assert float(got.min()) >= 0.0 and float(got.max()) <= 255.0


def test_bad_arguments_raise_value_error():
    y, uv, u = torch.zeros(2, 6, 8, dtype=torch.uint8), torch.zeros(2, 3, 4, 2, dtype=torch.uint8), torch.zeros(2, 3, 4, dtype=torch.uint8)
    rgb = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    for fn in (drivers.import_frames_torch, ops.import_frames):
        for args in (((y, uv), "nv21"), ((y,), "nv12"), ((y, uv, u), "nv12"), ((y, u), "i420"), ((y, uv.float()), "nv12"),
                     ((y.float(), uv), "nv12"), ((y, uv[:, :2]), "nv12"), ((y, uv[..., 0]), "nv12"), ((y, u, uv), "i420"),
                     ((y, u, u[:, :, :3]), "i420"), ((y[0], uv[0]), "nv12"), (rgb, "rgba32"), (rgb[0], "rgb24"), (rgb.float(), "bgr24"),
                     (rgb[..., :2], "rgb24"), ((y, "uv"), "nv12"), (y[:, :0], "rgb24"), ((y[:, :, :0], uv[:, :, :0]), "nv12")):
            with pytest.raises(ValueError):
                fn(*args)
        for kw in (dict(matrix="bt2020"), dict(range="tv"), dict(dtype=torch.float16), dict(size=(0, 4)), dict(size=(4, -1))):
            with pytest.raises(ValueError):
                fn((y, uv), "nv12", **kw)
    assert tuple(drivers.import_frames_torch((y[:0], uv[:0]), "nv12", (5, 7)).shape) == (0, 3, 5, 7)


def test_frames_import_is_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_frames_import" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)   # the history comment
    for name, value in dict(ops.IMPORT_FORMATS, **{"matrix_" + k: v for k, v in ops.IMPORT_MATRICES.items()},
                            **{"range_" + k: v for k, v in ops.IMPORT_RANGES.items()}).items():
        assert re.search(r"#define\s+PIPS_%s\s+%d\b" % (name.upper() if "_" in name else "FMT_" + name.upper(), value), hdr), name
    assert re.search(r"#define\s+PIPS_IMPORT_PIXELS_MAX\s+\(1 << 30\)", hdr)
    assert "nearest" in hdr and "antialias" in hdr and "may not overlap" in hdr                    # the limits stand in the header
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_frames_import\s*\(([^)]*)\)\s*;", bare)
    assert proto is not None and len(proto.group(1).split(",")) == 20
    res, args = _lib.SIGNATURES["pips_frames_import"]
    assert res is ctypes.c_int and len(args) == 20 and args[:6] == [ctypes.c_int] * 6
    assert args[6:15] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t] * 3
    assert args[15:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert "frames_import.hip" in _build.SOURCES and any(h.endswith("yuv.h") for h in _build.headers())
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pips_frames_import")
    assert callable(ops.import_frames) and callable(drivers.import_frames) and callable(drivers.import_frames_torch)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3

    # the host-side rejections need no device: nothing is launched (the pointers are never read)
    def call(fmt=4, matrix=1, range_=0, F=2, h=6, w=9, p=(8, 8, 0), pitch=(9, 10, 0), step=(54, 30, 0), dst=8, H=6, W=9):
        return lib.pips_frames_import(fmt, matrix, range_, F, h, w, p[0] or None, pitch[0], step[0], p[1] or None, pitch[1], step[1],
                                      p[2] or None, pitch[2], step[2], dst or None, 1, H, W, None)

    assert call(F=0) == 0 and call(F=0, p=(0, 0, 0), dst=0) == 0
    for over in (dict(fmt=-1), dict(fmt=6), dict(matrix=2), dict(matrix=-1), dict(range_=2), dict(range_=-1), dict(F=-1), dict(h=0),
                 dict(w=0), dict(H=0), dict(W=-2), dict(dst=0), dict(p=(0, 8, 0)), dict(p=(8, 0, 0)), dict(pitch=(8, 10, 0)),
                 dict(pitch=(9, 9, 0)), dict(step=(53, 30, 0)), dict(step=(54, 29, 0)), dict(H=1 << 15, W=1 << 15),
                 dict(fmt=5), dict(fmt=5, p=(8, 8, 8), pitch=(9, 5, 4), step=(54, 15, 15)),
                 dict(fmt=5, p=(8, 8, 8), pitch=(9, 5, 5), step=(54, 15, 14)), dict(fmt=0, pitch=(26, 0, 0), step=(200, 0, 0)),
                 dict(fmt=2, pitch=(35, 0, 0), step=(300, 0, 0))):
        assert call(**over) == -1, over
        assert lib.pips_last_error()
    # matrix and range are not looked at for a packed format, nor are planes 1 and 2
    assert call(fmt=0, matrix=7, range_=-3, F=0, p=(8, 0, 0), pitch=(27, 0, 0), step=(162, 0, 0)) == 0
    # a step is checked with F > 1 only
    assert call(F=0, step=(0, 0, 0)) == 0
