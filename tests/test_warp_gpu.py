"""GPU: pips_frames_warp in the library.  ops.warp_frames / drivers.warp_frames are held, byte for byte, to the torch twin run on the
CPU (drivers.warp_frames_torch, itself held to plain loops and to the closed form in tests/test_warp.py) on the surfaces and
coefficient sets made there.  The surfaces are views of larger allocations: the destination is poisoned with 0xA5 and has a
256-byte guard band before and behind every plane, rows longer than their samples and gaps between frames, all of which must
survive; the source -- junk in its padding and in the unused bits of its 16-bit words -- is compared unchanged afterwards.  Sizes
stand around the 64 x 16 tile and the four-sample store, bases at every offset of a dword, and the coefficient sets lie on both
sides of the staging criterion (test_warp.coefficient_sets names which is which; test_warp asserts it)."""
import ctypes as C

import pytest
import torch

from test_motion import _f64_bits, _life_video
from test_warp import (BORDERS, FORMATS, IDENTITY, ONE, WIDE, YUV, coefficient_sets, make_surfaces, untouched_outside, views_like)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
SHAPES = ((1, 1), (15, 63), (16, 64), (17, 65), (33, 130))
RULES = (("bt709", "limited"), ("bt601", "full"), ("bt601", "limited"), ("bt709", "full"))


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


def _check(fmt, F, h, w, coef, border, off, pad, gap, seed, fill=(200, 40, 90), matrix="bt709", range_="limited", dst_off=None):
    """one library call on pitched views against the twin on the CPU: the bytes, the poison around them, the source unchanged"""
    from pips_amd import drivers, ops
    s_flats, s_views = make_surfaces(fmt, F, h, w, seed=seed, off=off, pad=pad, gap=gap)
    d_flats, d_views = make_surfaces(fmt, F, h, w, seed=None, off=off if dst_off is None else dst_off, pad=pad + (2 if fmt in WIDE else 1),
                                     gap=gap + 4)
    coef = torch.tensor(coef, dtype=torch.int64)
    want = _list(drivers.warp_frames_torch(s_views, fmt, coef, border, fill=fill, matrix=matrix, range=range_))
    s_dev, s_planes = views_like(s_flats, s_views, DEV)
    d_dev, d_planes = views_like(d_flats, d_views, DEV)
    step = 2 if fmt in WIDE else 1
    assert s_planes[0].data_ptr() % 4 == (off * step) % 4
    got = ops.warp_frames(s_planes, fmt, coef.to(torch.int32), border, fill, matrix, range_, out=d_planes)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, d_planes))               # written where they lie, no copy
    for k, (a, b) in enumerate(zip(d_planes, want)):
        a = a.cpu()
        assert torch.equal(a, b), (fmt, h, w, border, k, int((a != b).sum()), torch.nonzero(a != b)[:4].tolist())
    assert untouched_outside([f.cpu() for f in d_dev], d_views)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_set_on_shapes_around_the_tile(fmt, shape):
    """the ten coefficient sets, a frame each (a different row per frame), under both borders; the base address, the pitch padding,
    the matrix and the range change with the shape"""
    h, w = shape
    i = SHAPES.index(shape)
    sets = coefficient_sets(h, w)
    coef = [sets[k] for k in sets]
    matrix, range_ = RULES[i % 4]
    wide = fmt in WIDE
    for b, border in enumerate(BORDERS):
        off = (i + 2 * b) % 4 if not wide else (i + b) % 2                                 # bytes / words off the dword grid
        pad = (2 * (i % 3)) if wide else (1, 3, 0, 2, 5)[i]                                # pitches that are no multiple of 4
        _check(fmt, len(coef), h, w, coef, border, off, pad, 6 + 2 * i, seed=100 + 10 * i + b, matrix=matrix, range_=range_)


@pytest.mark.parametrize("F", (1, 3))
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_counts_and_every_base_offset(fmt, F):
    """F = 1 and 3 at 17 x 65 with the source and the destination at different offsets of a dword, both paths"""
    sets = coefficient_sets(17, 65)
    rows = [sets[k] for k in ("rot2", "scale4", "shear")][:F]
    for off in range(2 if fmt in WIDE else 4):
        _check(fmt, F, 17, 65, rows, BORDERS[off % 2], off, 3 - off if fmt not in WIDE else 2, 10, seed=200 + off,
               dst_off=(off + 1) % (2 if fmt in WIDE else 4))


@pytest.mark.parametrize("fmt", FORMATS)
def test_tiles_whose_box_lies_inside_the_image(fmt):
    """80 x 300: tiles whose box lies inside every plane, where the kernel leaves the border rule out -- the first tile under the
    identity (staged) and under four source pixels a pixel (62 rows of 254 samples from (1, 2) on: taps from global memory), the
    interior tiles under a turn of 2 degrees (staged) -- beside tiles that reach over an edge and keep it.  The same bytes either way"""
    from pips_amd import ops
    h, w = 80, 300
    sets = coefficient_sets(h, w)
    four = [ONE << 2, 0, 1 << 16, 0, ONE << 2, 2 << 16]
    assert not ops.warp_staged(four, fmt) and ops.warp_staged(sets["rot2"], fmt) and ops.warp_staged(IDENTITY, fmt)
    for b, border in enumerate(BORDERS):
        _check(fmt, 3, h, w, [IDENTITY, four, sets["rot2"]], border, b, 0 if fmt in WIDE else 1, 4, seed=250 + b)


@pytest.mark.parametrize("fmt", YUV)
def test_fill_under_every_matrix_and_range(fmt):
    for matrix, range_ in RULES:
        _check(fmt, 2, 15, 63, [coefficient_sets(15, 63)[k] for k in ("rot45", "extreme_a")], "constant", 0, 0, 0, seed=300,
               fill=(250, 128, 3), matrix=matrix, range_=range_)


def test_contiguous_surfaces_and_an_allocated_output():
    """plain contiguous tensors, ``out=None``: new surfaces of the source's shapes; coefficients from the host and from the device"""
    from pips_amd import drivers, ops
    for fmt in ("nv12", "rgba32", "p010", "planar8"):
        _, views = make_surfaces(fmt, 2, 33, 130, seed=400)
        planes = [v.contiguous() for v in views]
        coef = torch.tensor([coefficient_sets(33, 130)[k] for k in ("rot2", "scale4")], dtype=torch.int32)
        want = _list(drivers.warp_frames_torch(planes, fmt, coef, "replicate"))
        for c in (coef, coef.to(DEV)):
            got = ops.warp_frames([p.to(DEV) for p in planes], fmt, c, "replicate")
            assert all(torch.equal(a.cpu(), b) and a.is_contiguous() for a, b in zip(got, want))


# ------------------------------------------------------------------ the driver
@pytest.mark.parametrize("surface", [(64, 96), (128, 192), (100, 192)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_driver_maps_model_transforms_onto_larger_surfaces(surface):
    """transforms in the pixels of a 64 x 96 model, surfaces of the model's size, twice it and an anisotropic 100 x 192, zoom 1.1:
    drivers.warp_frames is warp_coefficients + the kernel, the twin's bytes on NV12 and BGRA"""
    from pips_amd import drivers
    h, w = surface
    g = torch.Generator().manual_seed(15)
    sims = torch.tensor([[1.0, 0.0, 0.0, 0.0], [1.02, 0.03, 3.5, -2.25], [0.97, -0.05, -4.0, 1.5]], dtype=torch.float64)
    affine = torch.tensor([[1.0, 0.1, 2.0, -0.05, 0.95, -3.0]] * 3, dtype=torch.float64)
    for fmt, t in (("nv12", sims), ("bgra32", affine)):
        _, views = make_surfaces(fmt, 3, h, w, seed=int(torch.randint(0, 1000, (1,), generator=g)), pad=4, gap=8)
        coef = drivers.warp_coefficients(t, (64, 96), (h, w), 1.1)
        want = _list(drivers.warp_frames_torch(views, fmt, coef, "replicate"))
        got = _list(drivers.warp_frames([v.to(DEV) for v in views], fmt, t, size=(64, 96), zoom=1.1, border="replicate"))
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
        assert any(not torch.equal(b, v) for b, v in zip(want, views))


def test_stabilizer_across_engines_and_the_warped_surfaces():
    """the pushes of tests/test_warp.py's stabiliser test on the device: Stabilizer(engine="library") hands back what engine="torch"
    does, push by push, in every bit, and the NV12 surfaces warped by its corrections are the CPU twin's"""
    from pips_amd import drivers
    T, K, H, W = 19, 40, 64, 96
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5)
    _, views = make_surfaces("nv12", T, H, W, seed=500, pad=4, gap=8)
    planes = [v.to(DEV) for v in views]
    lib, ref = drivers.Stabilizer(radius=2, engine="library", **kw), drivers.Stabilizer(radius=2, engine="torch", **kw)
    pushes = []
    for f0 in range(0, T, 3):
        f1 = min(f0 + 3, T)
        ids = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
        t, v = trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids]
        pushes.append((lib.step(f0, t.to(DEV), v.to(DEV), ids=ids), ref.step(f0, t, v, ids=ids)))
    pushes.append((lib.finish(), ref.finish()))
    done = 0
    for (g0, rows), (r0, want_rows) in pushes:
        assert g0 == r0 == done and _f64_bits(rows) == _f64_bits(want_rows)
        k = rows.shape[0]
        if k:
            # the model's frame is 480 x 640 in _life_video's coordinates; the surfaces are 64 x 96
            got = _list(drivers.warp_frames([p[g0:g0 + k] for p in planes], "nv12", rows, size=(480, 640), zoom=1.05))
            want = _list(drivers.warp_frames_torch([p[g0:g0 + k] for p in views], "nv12", drivers.warp_coefficients(want_rows, (480, 640), (H, W), 1.05)))
            assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
        done += k
    assert done == T


# ------------------------------------------------------------------ the entry point itself
def _raw(fmt, src, dst, coef, F=None, h=None, w=None, border=0, fill=0, matrix=1, range_=0, s_surf=None, d_surf=None):
    from pips_amd import _lib, ops
    lib = _lib.load()
    src, Fs, hs, ws = ops.draw_planes(src, fmt)
    dst = ops.draw_planes(dst, fmt)[0]
    head = (ops.DRAW_FORMATS_EX.get(fmt, fmt) if isinstance(fmt, str) else fmt, matrix, range_, border, fill, Fs if F is None else F,
            hs if h is None else h, ws if w is None else w)
    return lib.pips_frames_warp(*head, *(s_surf or ops.draw_surfaces(src, fmt)), *(d_surf or ops.draw_surfaces(dst, fmt)),
                                None if coef is None else _lib.ptr(coef), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("fmt", ("nv12", "p010"))
def test_bad_arguments_with_device_pointers_write_nothing(fmt):
    from pips_amd import _lib, ops
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    F, h, w = 3, 17, 33
    s_flats, s_views = make_surfaces(fmt, F, h, w, seed=600, pad=2, gap=4)
    d_flats, d_views = make_surfaces(fmt, F, h, w, seed=None, pad=2, gap=4)
    s_dev, src = views_like(s_flats, s_views, DEV)
    d_dev, dst = views_like(d_flats, d_views, DEV)
    coef = torch.tensor([IDENTITY] * F, dtype=torch.int32, device=DEV)
    good_s, good_d = ops.draw_surfaces(src, fmt), ops.draw_surfaces(dst, fmt)

    def with_(surf, i, v):
        return surf[:i] + [v] + surf[i + 1:]
    bad = [dict(border=2), dict(border=-1), dict(matrix=2), dict(range_=2), dict(fill=-1), dict(fill=0x1000000), dict(F=-1), dict(h=0),
           dict(w=0), dict(h=8193), dict(w=8193), dict(coef=None),
           dict(s_surf=with_(good_s, 1, 2 * w - 2 if fmt in WIDE else w - 1)), dict(d_surf=with_(good_d, 4, 2)),      # a pitch below a row
           dict(s_surf=with_(good_s, 2, good_s[1] * (h - 1))), dict(d_surf=with_(good_d, 5, 8)),                    # a step below its rows
           dict(s_surf=with_(good_s, 0, None)), dict(d_surf=with_(good_d, 3, None)),                               # a NULL plane
           dict(d_surf=good_s),                                                                                    # the same tensor
           # dst starts inside the last src frame
           dict(d_surf=with_(good_d, 0, C.c_void_p(good_s[0].value + (F - 1) * good_s[2] + 2 * good_s[1]))),
           dict(s_surf=with_(good_s, 3, C.c_void_p(good_d[0].value + 4)))]                                         # src chroma inside dst luma
    if fmt in WIDE:
        bad += [dict(s_surf=with_(good_s, 0, C.c_void_p(good_s[0].value + 1))), dict(d_surf=with_(good_d, 1, good_d[1] + 1)),
                dict(d_surf=with_(good_d, 5, good_d[5] + 1))]
    for kw in bad:
        kw = dict(kw)
        c = kw.pop("coef", coef)
        assert _raw(fmt, src, dst, c, **kw) == E_ARG, kw
        assert lib.pips_last_error().decode().startswith("frames_warp:"), kw
        torch.cuda.synchronize()
        assert all(torch.equal(a.cpu(), b) for a, b in zip(d_dev, d_flats)) and all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats))
    for bad_fmt in (9, -1, 42):
        head = (bad_fmt, 1, 0, 0, 0, F, h, w)
        assert lib.pips_frames_warp(*head, *good_s, *good_d, _lib.ptr(coef), None) == E_ARG
        assert lib.pips_last_error().decode().startswith("frames_warp:")
    assert _raw(fmt, src, dst, coef, F=0) == 0 and _raw(fmt, src, dst, None, F=0) == 0      # F = 0 launches nothing
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(d_dev, d_flats))
    assert _raw(fmt, src, dst, coef) == 0                                                  # the same call with good arguments writes
    torch.cuda.synchronize()
    assert all(not torch.equal(a.cpu(), b) for a, b in zip(d_dev, d_flats)) and untouched_outside([f.cpu() for f in d_dev], d_views)
    # the wrapper's own checks
    with pytest.raises(ValueError):
        ops.warp_frames(src, fmt, coef[:2])
    with pytest.raises(ValueError):
        ops.warp_frames(src, fmt, coef, out=[p[:2] for p in dst])
    with pytest.raises(_lib.PipsHipError):
        ops.warp_frames(src, fmt, coef, out=src)
