"""GPU: pips_frames_warp_fill in the library.  Each case is one library call on pitched, offset, poisoned views -- ops.warp_frames_fill
or drivers.warp_frames_fill -- held byte for byte to the torch twin run on the CPU (drivers.warp_frames_fill_torch, itself held to
plain loops over the rule in tests/test_warp_fill.py, which also makes the candidate tables used here and shows that they are not
vacuous).  Checked: the bytes of every plane, the source map, the poison and the 256-byte guard bands around the destination and
the map, and the source surfaces, cand and coef unchanged."""
import ctypes as C

import pytest
import torch

from test_motion import _f64_bits, _life_video
from test_seams import FRAME_COUNTS, FRAME_SIZE, WARP_BORDER, WARP_FILL, periodic, periodic_index
from test_warp import BORDERS, FORMATS, IDENTITY, ONE, POISON, WIDE, coefficient_sets, make_surfaces, untouched_outside, views_like
from test_warp_fill import (BIG, CROP, GPU_FD, GPU_FS, GPU_SHAPES, NONE, SEAM_FS, big_tables, fill_seam_inputs, fill_seam_reference,
                            gpu_tables, mosaic)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
I32 = torch.int32
RULES = (("bt709", "limited"), ("bt601", "full"), ("bt601", "limited"), ("bt709", "full"))
_cache = {}


def _once(key, make):
    """a reference made once, on the CPU, shared by the cases that need it and never written to"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


def make_map(Fd, h, w, off, pad, gap):
    """a poisoned (Fd,h,w) uint8 view behind a guard band of 256 bytes and ``off`` more, rows ``pad`` longer than w, frames ``gap``
    apart beyond their rows -> (allocation, view)"""
    pitch = w + pad
    step = pitch * h + gap
    flat = torch.full((256 + off + step * Fd + 256,), POISON, dtype=torch.uint8)
    return flat, flat.as_strided((Fd, h, w), (step, pitch, 1), 256 + off)


def _check(fmt, Fs, Fd, h, w, cand, coef, border, offs, pad, gap, seed, source=True, fill=(200, 40, 90), matrix="bt709", range_="limited",
           want=None, at=None):
    """one library call on pitched views against the twin on the CPU.  offs = the offsets of src, dst and the map off the dword grid
    (bytes; words of a 16-bit format for src and dst).  want / at: a reference made elsewhere and the index of each frame in it"""
    from pips_amd import drivers, ops
    s_flats, s_views = make_surfaces(fmt, Fs, h, w, seed=seed, off=offs[0], pad=pad, gap=gap)
    d_flats, d_views = make_surfaces(fmt, Fd, h, w, seed=None, off=offs[1], pad=pad + (2 if fmt in WIDE else 1), gap=gap + 4)
    m_flat, m_view = make_map(Fd, h, w, offs[2], pad + 2, gap + 3)
    cand, coef = torch.as_tensor(cand, dtype=torch.int64), torch.as_tensor(coef, dtype=torch.int64)
    if want is None:
        want, wmap = drivers.warp_frames_fill_torch(s_views, fmt, cand, coef, border, fill=fill, matrix=matrix, range=range_, source=True)
        want = _list(want)
    else:
        want, wmap = [p[at] for p in want[0]], want[1][at]
    s_dev, s_planes = views_like(s_flats, s_views, DEV)
    d_dev, d_planes = views_like(d_flats, d_views, DEV)
    (m_dev,), (m_plane,) = views_like([m_flat], [m_view], DEV)
    assert s_planes[0].data_ptr() % 4 == (offs[0] * (2 if fmt in WIDE else 1)) % 4 and m_plane.data_ptr() % 4 == offs[2] % 4
    d_cand, d_coef = cand.to(DEV, I32), coef.to(DEV, I32)
    got = ops.warp_frames_fill(s_planes, fmt, d_cand, d_coef, border, fill, matrix, range_, out=d_planes, source=m_plane if source else None)
    torch.cuda.synchronize()
    got, gmap = got if source else (got, None)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, d_planes)) and (gmap is None or gmap.data_ptr() == m_plane.data_ptr())
    for k, (a, b) in enumerate(zip(d_planes, want)):
        a = a.cpu()
        assert torch.equal(a, b), (fmt, h, w, border, k, int((a != b).sum()), torch.nonzero(a != b)[:4].tolist())
    assert untouched_outside([f.cpu() for f in d_dev], d_views)
    if source:
        a = m_plane.cpu()
        assert torch.equal(a, wmap), (fmt, h, w, border, int((a != wmap).sum()), torch.nonzero(a != wmap)[:4].tolist())
        assert untouched_outside([m_dev.cpu()], [m_view])
    else:
        assert torch.equal(m_dev.cpu(), m_flat)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats))
    assert torch.equal(d_cand.cpu(), cand.to(I32)) and torch.equal(d_coef.cpu(), coef.to(I32))
    return wmap


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_on_shapes_around_the_tile(fmt, shape):
    """Fs = 5 source frames into Fd = 3, both borders, K = 1, 2 and 4 slots of test_warp_fill.gpu_tables; src, dst and the map at
    different offsets of a dword, pitches that are no multiple of 4, the map asked for and not"""
    h, w = shape
    i = GPU_SHAPES.index(shape)
    cand, coef = gpu_tables(h, w)
    wide = fmt in WIDE
    n = 2 if wide else 4
    for b, border in enumerate(BORDERS):
        for q, K in enumerate((1, 2, 4)):
            offs = ((i + b) % n, (i + b + 1 + q) % n, (i + 2 * b + q + 3) % 4)
            pad = 2 * ((i + q) % 3) if wide else (1, 3, 0, 2)[(i + q) % 4]
            matrix, range_ = RULES[(i + q) % 4]
            wmap = _check(fmt, GPU_FS, GPU_FD, h, w, [r[:K] for r in cand], [r[:K] for r in coef], border, offs, pad, 6 + 2 * i,
                          seed=700 + 10 * i + b, source=(b + q) % 2 == 0, matrix=matrix, range_=range_)
            if K == 4 and min(h, w) > 1:
                assert {0, 1, 2, 3, NONE} == set(wmap.unique().tolist())


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_candidate_per_frame_is_the_bytes_of_frames_warp(fmt, border):
    """K = 1 with cand = arange(F) at 17 x 65: the bytes of ops.warp_frames from the same session, both tap paths"""
    from pips_amd import ops
    h, w = 17, 65
    sets = coefficient_sets(h, w)
    coef = torch.tensor([sets[k] for k in ("identity", "rot2", "scale4", "shear", "extreme_a", "quarter")], dtype=I32)
    F = coef.shape[0]
    s_flats, s_views = make_surfaces(fmt, F, h, w, seed=720, off=1, pad=2, gap=6)
    _, planes = views_like(s_flats, s_views, DEV)
    want = ops.warp_frames(planes, fmt, coef, border, (200, 40, 90))
    got, smap = ops.warp_frames_fill(planes, fmt, torch.arange(F).view(F, 1), coef.view(F, 1, 6), border, (200, 40, 90), source=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert bool((smap[0] == 0).all()) and bool((smap[4] == NONE).all()) and set(smap.unique().tolist()) == {0, NONE}


@pytest.mark.parametrize("fmt", FORMATS)
def test_fast_path_tiles_beside_tiles_that_walk_the_list(fmt):
    """80 x 300 with test_warp_fill.big_tables: interior tiles whose candidate-0 box lies inside every plane (the staged pass, and
    the direct one under four source pixels a pixel) beside edge tiles that walk to the later candidates, one of which taps four
    source pixels a pixel"""
    h, w = BIG
    cand, coef = big_tables()
    for b, border in enumerate(BORDERS):
        wmap = _check(fmt, GPU_FS, GPU_FD, h, w, cand, coef, border, (b, 1 - b, 2 + b), 0 if fmt in WIDE else 1, 4, seed=730 + b, source=True)
        assert all({0, 1, 2} <= set(wmap[j].unique().tolist()) for j in range(3))


@pytest.mark.parametrize("fmt", ("nv12", "rgba32"))
def test_sixteen_candidates_with_only_the_last_covering(fmt):
    """K = 16 at 17 x 65: empty slots, indices past Fs and rows at the int32 extremes in front of a shift in the last slot; what it
    leaves is candidate 0 (an extreme row) under the border rule on frame 0 and the fill on frame 1, whose candidate 0 is invalid"""
    h, w = 17, 65
    sets = coefficient_sets(h, w)
    shift = [ONE, 0, int(2.5 * 65536), 0, ONE, -int(1.25 * 65536)]
    cand = [[1] + [-1, 7, 2, 0] * 3 + [-1, 5, 3], [-3] + [4, -1, 9, 0] * 3 + [7, -1, 2]]
    rows = [sets["extreme_a"], IDENTITY, IDENTITY, sets["extreme_b"], sets["extreme_a"]]
    coef = [[rows[0]] + rows[1:] * 3 + [IDENTITY, IDENTITY, shift], [IDENTITY] + [sets["extreme_b"], IDENTITY, IDENTITY, sets["extreme_a"]] * 3 + [IDENTITY, IDENTITY, shift]]
    assert all(len(c) == 16 for c in cand) and all(len(m) == 16 for m in coef)
    for b, border in enumerate(BORDERS):
        wmap = _check(fmt, GPU_FS, 2, h, w, cand, coef, border, (1, 2, 3), 3, 6, seed=740 + b)
        assert set(wmap.unique().tolist()) == {15, NONE}


@pytest.mark.parametrize("Fd", FRAME_COUNTS)
@pytest.mark.parametrize("fmt", sorted(WARP_BORDER))
def test_frames_warp_fill_past_the_frames_of_a_launch(fmt, Fd):
    """warp_fill_kernel's rows of cand and coef, its dst surfaces and its map at f_base + blockIdx.y: 65535 and 65537 output frames of
    3 x 5 from 4 source frames, the lists periodic with 7, against the twin's period (test_warp_fill holds that expectation to the
    twin over every frame)"""
    from pips_amd import ops
    h, w = FRAME_SIZE
    cand, coef, (s_flats, s_views) = fill_seam_inputs(fmt)
    want, wmap = _once(("seam", fmt), lambda: fill_seam_reference(fmt))
    d_flats, d_views = make_surfaces(fmt, Fd, h, w, seed=None, off=1 if fmt in WIDE else 2, pad=4, gap=10)
    m_flat, m_view = make_map(Fd, h, w, 3, 2, 5)
    s_dev, s_planes = views_like(s_flats, s_views, DEV)
    d_dev, d_planes = views_like(d_flats, d_views, DEV)
    (m_dev,), (m_plane,) = views_like([m_flat], [m_view], DEV)
    d_cand, d_coef = periodic(cand, Fd).to(DEV, I32), periodic(coef, Fd).to(DEV, I32)
    got, gmap = ops.warp_frames_fill(s_planes, fmt, d_cand, d_coef, WARP_BORDER[fmt], WARP_FILL, out=d_planes, source=m_plane)
    torch.cuda.synchronize()
    at = periodic_index(Fd)
    for k, (a, b) in enumerate(zip(d_planes, want)):
        a, b = a.cpu(), b[at]
        assert torch.equal(a, b), (fmt, Fd, k, int((a != b).sum()), torch.nonzero((a != b).flatten(1).any(dim=1)).flatten()[:4].tolist())
    assert torch.equal(m_plane.cpu(), wmap[at])
    assert untouched_outside([f.cpu() for f in d_dev], d_views) and untouched_outside([m_dev.cpu()], [m_view])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats))


# ------------------------------------------------------------------ the drivers
def _mosaic_surfaces(fmt, frames, scale):
    """the planar mosaic frames as surfaces of ``fmt`` at ``scale`` times the size (pixels repeated): content only has to differ"""
    big = frames.repeat_interleave(scale, dim=2).repeat_interleave(scale, dim=3)
    if fmt == "bgra32":
        return [torch.cat([big.flip(1), torch.full_like(big[:, :1], 7)], dim=1).permute(0, 2, 3, 1).contiguous()]
    chroma = torch.stack([big[:, 1, ::2, ::2] // 2 + 60, 200 - big[:, 2, ::2, ::2] // 2], dim=-1)
    return [big[:, 0].contiguous(), chroma.contiguous()]


@pytest.mark.parametrize("scale,zoom", [(1, 1.0), (2, 1.05)])
def test_driver_fills_the_planted_mosaic(scale, zoom):
    """drivers.warp_frames_fill on test_warp_fill's mosaic, as NV12 and BGRA32 surfaces of the model's size and at twice it with
    zoom 1.05: warp_coefficients per slot and one library call, the twin's bytes and map"""
    from pips_amd import drivers
    frames, path = mosaic()
    cand, tr = drivers.fill_candidates(path, drivers.motion_smooth(path, None), (3, 1))
    h, w = CROP[0] * scale, CROP[1] * scale
    coef = drivers.warp_coefficients(tr.reshape(-1, 4), CROP, (h, w), zoom).reshape(6, 5, 6)
    for fmt in ("nv12", "bgra32"):
        planes = _mosaic_surfaces(fmt, frames, scale)
        want, wmap = drivers.warp_frames_fill_torch(planes, fmt, cand, coef, "replicate", source=True)
        got, gmap = drivers.warp_frames_fill([p.to(DEV) for p in planes], fmt, cand, tr, size=CROP, zoom=zoom, border="replicate", source=True)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(_list(got), _list(want))) and torch.equal(gmap.cpu(), wmap)
        assert len(set(wmap.unique().tolist()) - {NONE}) >= 4
        plain = drivers.warp_frames_fill([p.to(DEV) for p in planes], fmt, cand, tr, size=CROP, zoom=zoom, border="replicate")
        assert all(torch.equal(a, b) for a, b in zip(_list(plain), _list(got)))


def test_stabilizer_candidates_across_engines_and_a_held_window():
    """the pushes of tests/test_warp_fill.py's stabiliser test on the device: Stabilizer(engine="library", neighbors=(3, 1)) hands
    back the candidates of engine="torch" push by push in every bit, and the NV12 frames warped from the held window of surfaces
    that those candidates name (first > 0 once the video runs) are the twin's"""
    from pips_amd import drivers
    T, K, H, W = 19, 40, 64, 96
    trajs, vis, born, last = _life_video(T, K, 21)
    kw = dict(thr=1.5, hypotheses=48, vis_thr=0.6, seed=5, radius=2, neighbors=(3, 1))
    _, views = make_surfaces("nv12", T, H, W, seed=750, pad=4, gap=8)
    planes = [v.to(DEV) for v in views]
    lib, ref = drivers.Stabilizer(engine="library", **kw), drivers.Stabilizer(engine="torch", **kw)
    done, windows = 0, 0
    for f0 in list(range(0, T, 3)) + [None]:
        if f0 is None:
            (g0, rows), (r0, want_rows) = lib.finish(), ref.finish()
        else:
            f1 = min(f0 + 3, T)
            ids = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
            t, v = trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids]
            (g0, rows), (r0, want_rows) = lib.step(f0, t.to(DEV), v.to(DEV), ids=ids), ref.step(f0, t, v, ids=ids)
        k = rows.shape[0]
        assert g0 == r0 == done and _f64_bits(rows) == _f64_bits(want_rows)
        (fr, tr), (wfr, wtr) = lib.candidates(g0, k), ref.candidates(g0, k)
        assert torch.equal(fr, wfr) and _f64_bits(tr) == _f64_bits(wtr)
        if k:
            lo, hi = int(fr[fr >= 0].min()), int(fr.max()) + 1                             # the surfaces a caller still holds
            windows += lo > 0
            got = _list(drivers.warp_frames_fill([p[lo:hi] for p in planes], "nv12", fr, tr, first=lo, size=(480, 640), zoom=1.05))
            cand, coef = drivers._fill_setup([p[lo:hi] for p in views], "nv12", wfr, wtr, lo, (480, 640), 1.05)
            want = _list(drivers.warp_frames_fill_torch([p[lo:hi] for p in views], "nv12", cand, coef))
            assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
        done += k
    assert done == T and windows >= 3


# ------------------------------------------------------------------ the entry point itself
def _raw(fmt, src, dst, cand, coef, smap, Fs=None, Fd=None, K=None, h=None, w=None, border=0, fill=0, matrix=1, range_=0, s_surf=None,
         d_surf=None, m_surf=None):
    from pips_amd import _lib, ops
    lib = _lib.load()
    src, fs, hs, ws = ops.draw_planes(src, fmt)
    dst, fd, _, _ = ops.draw_planes(dst, fmt)
    head = (ops.DRAW_FORMATS_EX[fmt], matrix, range_, border, fill, fs if Fs is None else Fs, fd if Fd is None else Fd,
            (2 if cand is None else cand.shape[1]) if K is None else K, hs if h is None else h, ws if w is None else w)
    m = m_surf or [_lib.ptr(smap), smap.stride(1), smap.stride(0)]
    return lib.pips_frames_warp_fill(*head, *(s_surf or ops.draw_surfaces(src, fmt)), *(d_surf or ops.draw_surfaces(dst, fmt)),
                                     None if cand is None else _lib.ptr(cand), None if coef is None else _lib.ptr(coef), *m,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("fmt", ("nv12", "p010"))
def test_bad_arguments_with_device_pointers_write_nothing(fmt):
    from pips_amd import _lib, ops
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    Fs, Fd, K, h, w = 4, 3, 2, 17, 33
    s_flats, s_views = make_surfaces(fmt, Fs, h, w, seed=760, pad=2, gap=4)
    d_flats, d_views = make_surfaces(fmt, Fd, h, w, seed=None, pad=2, gap=4)
    m_flat, m_view = make_map(Fd, h, w, 0, 3, 5)
    s_dev, src = views_like(s_flats, s_views, DEV)
    d_dev, dst = views_like(d_flats, d_views, DEV)
    (m_dev,), (smap,) = views_like([m_flat], [m_view], DEV)
    cand = torch.tensor([[0, 1], [3, -1], [2, 2]], dtype=I32, device=DEV)
    coef = torch.tensor([[coefficient_sets(h, w)["rot2"], IDENTITY]] * Fd, dtype=I32, device=DEV)
    good_s, good_d = ops.draw_surfaces(src, fmt), ops.draw_surfaces(dst, fmt)
    good_m = [_lib.ptr(smap), smap.stride(1), smap.stride(0)]

    def with_(surf, i, v):
        return surf[:i] + [v] + surf[i + 1:]

    def clean():
        torch.cuda.synchronize()
        return (all(torch.equal(a.cpu(), b) for a, b in zip(d_dev, d_flats)) and all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats))
                and torch.equal(m_dev.cpu(), m_flat))
    bad = [dict(border=2), dict(border=-1), dict(matrix=2), dict(range_=2), dict(fill=-1), dict(fill=0x1000000), dict(Fs=-1), dict(Fd=-1),
           dict(K=0), dict(K=17), dict(K=-1), dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(cand=None), dict(coef=None),
           dict(s_surf=with_(good_s, 1, 2 * w - 2 if fmt in WIDE else w - 1)), dict(d_surf=with_(good_d, 4, 2)),      # a pitch below a row
           dict(s_surf=with_(good_s, 2, good_s[1] * (h - 1))), dict(d_surf=with_(good_d, 5, 8)),                    # a step below its rows
           dict(s_surf=with_(good_s, 0, None)), dict(d_surf=with_(good_d, 3, None)),                               # a NULL plane
           dict(m_surf=with_(good_m, 1, w - 1)), dict(m_surf=with_(good_m, 2, good_m[1] * h - 1)),                  # the map's pitch and step
           dict(d_surf=good_s, Fd=Fs),                                                                             # the same tensor
           dict(d_surf=with_(good_d, 0, C.c_void_p(good_s[0].value + (Fs - 1) * good_s[2] + 2 * good_s[1]))),      # dst inside the last src frame
           dict(s_surf=with_(good_s, 3, C.c_void_p(good_d[0].value + 4))),                                         # src chroma inside dst luma
           dict(m_surf=with_(good_m, 0, C.c_void_p(good_d[3].value + 2))),                                         # the map inside dst chroma
           dict(m_surf=with_(good_m, 0, C.c_void_p(good_s[0].value + (Fs - 1) * good_s[2])))]                      # the map inside the last src frame
    if fmt in WIDE:
        bad += [dict(s_surf=with_(good_s, 0, C.c_void_p(good_s[0].value + 1))), dict(d_surf=with_(good_d, 1, good_d[1] + 1)),
                dict(d_surf=with_(good_d, 5, good_d[5] + 1))]
    for kw in bad:
        kw = dict(kw)
        c, m = kw.pop("cand", cand), kw.pop("coef", coef)
        assert _raw(fmt, src, dst, c, m, smap, **kw) == E_ARG, kw
        assert lib.pips_last_error().decode().startswith("frames_warp_fill:"), kw
        assert clean(), kw
    assert _raw(fmt, src, dst, cand, coef, smap, Fd=0) == 0 and _raw(fmt, src, dst, None, None, smap, Fd=0) == 0     # Fd = 0 launches nothing
    assert clean()
    assert _raw(fmt, src, dst, cand, coef, smap) == 0                                      # the same call with good arguments writes
    torch.cuda.synchronize()
    assert all(not torch.equal(a.cpu(), b) for a, b in zip(d_dev, d_flats)) and untouched_outside([f.cpu() for f in d_dev], d_views)
    assert untouched_outside([m_dev.cpu()], [m_view]) and set(smap.cpu().unique().tolist()) == {0, 1, NONE}
    # the wrapper's own checks
    with pytest.raises(ValueError):
        ops.warp_frames_fill(src, fmt, cand, coef[:2])
    with pytest.raises(ValueError):
        ops.warp_frames_fill(src, fmt, cand, coef, out=[p[:2] for p in dst])
    with pytest.raises(ValueError):
        ops.warp_frames_fill(src, fmt, cand, coef, source=smap[:2])
    with pytest.raises(_lib.PipsHipError):
        ops.warp_frames_fill([p[:Fd] for p in src], fmt, cand.clamp(max=2), coef, out=[p[:Fd] for p in src])
