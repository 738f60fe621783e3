"""GPU: pips_tracks_draw_ex in the library.  drivers.draw_tracks on P010 / I010 surfaces and with fade tables is held, word for
word and byte for byte, to the torch twin (drivers.draw_tracks_torch, itself held to plain loops in tests/test_draw_ex.py) on the
cases made there: both 16-bit formats under the four matrix / range rows at one tile, at a one-pixel row and column of tiles and at
a size odd both ways, without a fade and with the linear one; 0 / 1 / 5 / 300 tracks with trails of 0 / 1 / 4 / 32 rows on P010 and
on faded BGRA and NV12.  The surfaces are views of larger allocations whose sentinel must survive -- pitches of +0, +2 and +64
bytes, stepped frames, a base two bytes off the 16-byte grid, junk in the six unused bits of every word -- and each case first
asserts on the twin's output that it is not vacuous.  The collapse clause (no table, or one of 256s, gives pips_tracks_draw's bytes)
is held on the device on the seven 8-bit formats; return codes with device pointers leave a poisoned surface alone.  End to end a
TrackPainter paints a CoverTracker's pushes on the P010 surfaces the frames were imported from."""
import ctypes as C

import pytest
import torch

from test_draw import FORMATS, STYLE, buffers, case_inputs, views
from test_draw_ex import (SENTINEL16, WIDE, case_id_ex, case_inputs_ex, format_cases_ex, grid_cases_ex, not_vacuous_ex,
                          untouched_outside)
from test_stream_rounds_gpu import _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


def _dev(b):
    """a host allocation on the device; a 16-bit one with its base two bytes off the 16-byte grid"""
    if b.dtype != torch.int16:
        return b.to(DEV)
    flat = torch.full((b.numel() + 1,), SENTINEL16, dtype=torch.int16, device=DEV)
    out = flat[1:].view(b.shape)
    out.copy_(b)
    assert out.data_ptr() % 16 == 2
    return out


def _run_case(case, with_vis):
    from pips_amd import drivers
    fmt, h, w = case[0], case[3], case[4]
    bufs, trajs, vis, kw = case_inputs_ex(case, with_vis)
    before = [b.clone() for b in bufs]
    dev_bufs = [_dev(b) for b in bufs]
    planes = views(dev_bufs, fmt, h, w)
    trajs, vis = trajs.to(DEV), None if vis is None else vis.to(DEV)
    want = _list(drivers.draw_tracks_torch(planes, fmt, trajs, vis, **kw))
    ok, what = not_vacuous_ex(case, planes, want, trajs, kw)
    assert ok, what
    got = _list(drivers.draw_tracks(planes, fmt, trajs, vis, inplace=True, **kw))
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, planes))                 # drawn where they lie, no copy
    for k, (a, b) in enumerate(zip(planes, want)):
        assert torch.equal(a, b), (case_id_ex(case), k, int((a != b).sum()))
    assert untouched_outside([b.cpu() for b in dev_bufs], before, fmt, h, w)
    if fmt in WIDE and case[6] > 0:                                  # words no track covers kept their junk: not all were rewritten
        low = 63 if fmt == "p010" else 0xFC00
        assert bool(((planes[0].to(torch.int64) & low) != 0).any())
    return what


@pytest.mark.parametrize("case", format_cases_ex(), ids=case_id_ex)
def test_p010_and_i010_at_the_tile_edges(case):
    """2 formats x 4 matrix / range rows x 16x16 (pitch +0), 17x33 (+2 bytes), 37x51 (+64 bytes) x no fade / linear; F = 3, five
    tracks with the named positions, trail 4; at 17x33 without visibilities"""
    _run_case(case, with_vis=(case[3], case[4]) != (17, 33))


@pytest.mark.parametrize("case", grid_cases_ex(), ids=case_id_ex)
def test_track_counts_trails_and_fade_tables(case):
    """n in {0, 1, 5, 300} (300: a full chunk of 256 and a ragged one) x trail in {0, 1, 4, 32} on the 37x51 surface, positions in its
    own pixels and in those of a 24x32 model frame; P010 without a fade, BGRA and NV12 with linear, non-monotone and all-zero tables"""
    _run_case(case, with_vis=True)


# ------------------------------------------------------------------ the entry points themselves
def _raw(entry, fmt, planes, trajs, vis, colors, first, trail, fade=None, ws=None, surf=None, style=(6, 16, 230, 102, 0.0),
         matrix="bt709", range_="limited"):
    """one call of pips_tracks_draw or pips_tracks_draw_ex on device tensors -> its return code; ``surf``: the nine surface
    arguments when they are not the planes' own"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    planes, F, h, w = ops.draw_planes(planes, fmt)
    G, n = vis.shape
    if ws is None:
        ws = torch.empty(max(ops.draw_workspace_bytes(F, n, trail) // 4, 4), dtype=torch.int32, device=DEV)
    line8, dot8, a_vis, a_occ, logit = style
    head = (ops.DRAW_FORMATS_EX[fmt], ops.IMPORT_MATRICES[matrix], ops.IMPORT_RANGES[range_], F, h, w,
            *(surf or ops.draw_surfaces(planes, fmt)), _lib.ptr(trajs), _lib.ptr(vis), G, n, first, h, w, _lib.ptr(colors), trail, line8,
            dot8, a_vis, a_occ, logit)
    tail = (_lib.ptr(ws), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if entry == "pips_tracks_draw":
        return lib.pips_tracks_draw(*head, *tail)
    table = None if fade is None else (C.c_int * max(len(fade), 1))(*fade)
    return lib.pips_tracks_draw_ex(*head, table, *tail)


@pytest.mark.parametrize("fmt", FORMATS)
def test_without_a_table_the_bytes_are_pips_tracks_draws(fmt):
    """the collapse clause on the device: pips_tracks_draw_ex with fade = NULL, and with a table of 256s (the faded kernel), gives
    the bytes of pips_tracks_draw on each of the seven 8-bit formats"""
    from pips_amd import drivers
    case = (fmt, "bt709", "limited", 37, 51, 3, 5, 4, None, STYLE)
    bufs, trajs, vis, kw = case_inputs(case)
    trajs, vis = trajs[0].to(DEV), vis[0].to(DEV)
    colors = drivers.track_colors(torch.arange(5)).to(DEV)
    outs = []
    for entry, fade in (("pips_tracks_draw", None), ("pips_tracks_draw_ex", None), ("pips_tracks_draw_ex", [256] * 4),
                        ("pips_tracks_draw_ex", [256, 128, 64, 0])):
        planes = views([b.to(DEV) for b in bufs], fmt, 37, 51)
        assert _raw(entry, fmt, planes, trajs, vis, colors, kw["first"], 4, fade) == 0
        torch.cuda.synchronize()
        outs.append(planes)
    assert any(not torch.equal(a.cpu(), b) for a, b in zip(outs[0], views(bufs, fmt, 37, 51)))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])) and all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))
    assert any(not torch.equal(a, b) for a, b in zip(outs[0], outs[3]))                   # (a table that fades is seen)


def test_another_stream_and_a_reused_workspace_ex():
    from pips_amd import drivers, ops
    case = ("p010", "bt709", "limited", 37, 51, 3, 300, 4, None, dict(width=1.0, dot=1.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5),
            "linear", (5, 2))
    bufs, trajs, vis, kw = case_inputs_ex(case)
    trajs, vis = trajs.to(DEV), vis.to(DEV)
    want = _list(drivers.draw_tracks(views([_dev(b) for b in bufs], "p010", 37, 51), "p010", trajs, vis, **kw))
    colors = drivers.track_colors(torch.arange(300)).to(DEV)
    logit = float(torch.logit(torch.tensor(0.5, dtype=torch.float32)))
    ws = torch.full((ops.draw_workspace_bytes(3, 300, 4) // 4 + 16,), -77, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(side):
        for _ in range(2):                                           # the second call finds the first one's records in the workspace
            planes = views([_dev(b) for b in bufs], "p010", 37, 51)
            ops.draw_tracks(planes, "p010", trajs[0], vis[0], colors, kw["first"], None, 4, 4, 8, 230, 102, logit, "bt709", "limited",
                            workspace=ws, fade=[256, 192, 128, 64])
            outs.append(planes)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for planes in outs:
        assert all(torch.equal(a, b) for a, b in zip(planes, want))
    assert bool((ws[-16:] == -77).all())                             # nothing behind pips_draw_workspace_bytes is written
    assert drivers._draw_fade("linear", 4) == [256, 192, 128, 64]


def test_bad_arguments_with_device_pointers_leave_the_surface_alone():
    """an odd pitch, an odd base and a fade entry of 257: PIPS_E_ARG, and the poisoned surfaces are what they were; the same call
    with good arguments draws"""
    from pips_amd import _lib, drivers, ops
    case = ("p010", "bt709", "limited", 37, 51, 3, 5, 4, None, STYLE, None, (5, 2))
    bufs, trajs, vis, kw = case_inputs_ex(case)
    trajs, vis = trajs[0].to(DEV), vis[0].to(DEV)
    colors = drivers.track_colors(torch.arange(5)).to(DEV)
    dev_bufs = [torch.full_like(b, 0x5EED).to(DEV) for b in bufs]
    poison = [b.clone() for b in dev_bufs]
    planes = views(dev_bufs, "p010", 37, 51)
    good = ops.draw_surfaces(planes, "p010")
    odd_pitch = good[:1] + [good[1] + 1, good[2] + 3] + good[3:]
    odd_base = [C.c_void_p(good[0].value + 1)] + good[1:]
    odd_chroma = good[:3] + [C.c_void_p(good[3].value + 1)] + good[4:]
    lib = _lib.load()
    for surf, fade in ((odd_pitch, None), (odd_base, None), (odd_chroma, None), (good, [256, 257, 0, 0]), (good, [-1, 0, 0, 0])):
        assert _raw("pips_tracks_draw_ex", "p010", planes, trajs, vis, colors, kw["first"], 4, fade, surf=surf) == E_ARG
        assert lib.pips_last_error().decode().startswith("tracks_draw_ex:")
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(dev_bufs, poison))
    assert _raw("pips_tracks_draw", "p010", planes, trajs, vis, colors, kw["first"], 4) == E_ARG      # (formats 6 and 7 stay illegal there)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev_bufs, poison))
    assert _raw("pips_tracks_draw_ex", "p010", planes, trajs, vis, colors, kw["first"], 4, [256, 128, 64, 32], surf=good) == 0
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(dev_bufs, poison))


# ------------------------------------------------------------------ end to end on the device
EH, EW, MH, MW, ET = 64, 96, 128, 192, 24


def _p010_surfaces(video, seed):
    """the frames of ``video`` (1,T,3,MH,MW) at half size as pitched P010 surfaces with junk in the low six bits -> (allocations,
    views), on the device"""
    from pips_amd import drivers
    g = torch.Generator().manual_seed(seed)
    rgb = video[0, :, :, ::2, ::2].permute(0, 2, 3, 1).to(torch.int64)                     # (T,EH,EW,3)
    yuv = drivers.rgb_to_yuv_torch(rgb, "bt709", "limited", bits=10)
    word = lambda v: ((v << 6) | torch.randint(0, 64, v.shape, generator=g)).to(torch.int32).to(torch.int16)       # (wraps: the bits)
    bufs = [torch.full((ET, EH + 4, EW + 32), SENTINEL16, dtype=torch.int16),
            torch.full((ET, EH // 2 + 2, EW // 2 + 16, 2), SENTINEL16, dtype=torch.int16)]
    bufs[0][:, :EH, :EW] = word(yuv[..., 0])
    bufs[1][:, :EH // 2, :EW // 2] = word(yuv[:, ::2, ::2, 1:])
    return bufs, views([_dev(b) for b in bufs], "p010", EH, EW)


def test_painter_on_a_cover_tracker_paints_the_p010_surfaces_it_imported(weights_tamed):
    """24 P010 surfaces of 64 x 96 are imported to the model's 128 x 192 and pushed to a CoverTracker in three chunks; a TrackPainter
    with a linear fade paints the same surfaces in place, push by push.  Their words are those of draw_tracks_torch over
    track_cover's whole-video result by identity, and importing them again gives frames that differ from the first import only where
    a sample was drawn"""
    from pips_amd import drivers, ops
    m = _model(weights_tamed)
    bufs, surfaces = _p010_surfaces(_video(ET, MH, MW, seed=70), 71)
    before = [b.clone() for b in bufs]
    untouched = [p.clone() for p in surfaces]
    chunks = [drivers.import_frames([p[a:b] for p in surfaces], "p010", size=(MH, MW)) for a, b in ((0, 8), (8, 16), (16, 24))]
    first_import = ops.import_frames(surfaces, "p010")
    cover = lambda: drivers.Cover(cell=32, vis_thr=0.9, lost_after=2, scan="library")
    style = dict(width=1.5, dot=2.0, alpha=0.85, alpha_occ=0.35, vis_thr=0.7)
    trail = 6

    ct = drivers.CoverTracker(m, cover(), None, iters=6, slots=24, rounds="library")
    painter = drivers.TrackPainter((MH, MW), trail=trail, fade="linear", **style)
    painted = 0
    for part in [ct.push(c) for c in chunks] + [ct.finish()]:
        f0, trajs, vis, ids = part
        assert f0 == painted
        painter.paint([p[f0:f0 + trajs.shape[1]] for p in surfaces], "p010", f0, trajs, vis, ids=ids)
        painted += trajs.shape[1]
    assert painted == ET
    torch.cuda.synchronize()

    trajs, vis, born, retired = drivers.track_cover(m, chunks, cover(), iters=6, slots=24, rounds="library")
    K = trajs.shape[2]
    assert K >= 24
    want = drivers.draw_tracks_torch(untouched, "p010", trajs, vis, colors=drivers.track_colors(torch.arange(K)), size=(MH, MW),
                                     trail=trail, fade="linear", **style)
    for a, b in zip(surfaces, want):
        assert torch.equal(a, b), int((a != b).sum())
    drawn = (surfaces[0] != untouched[0]) | (surfaces[1] != untouched[1]).any(dim=-1).repeat_interleave(2, 1).repeat_interleave(2, 2)
    share = float(drawn.float().mean())
    print(f"painter e2e on p010: {K} identities, {share:.1%} of the pixels drawn on")
    assert 0.01 < share < 0.9
    assert untouched_outside([b.cpu() for b in bufs], before, "p010", EH, EW)
    differs = (ops.import_frames(surfaces, "p010") != first_import).any(dim=1)             # (ET,EH,EW)
    assert bool(differs.any()) and not bool((differs & ~drawn).any())
    tiles = drawn.view(ET, EH // 16, 16, EW // 16, 16).any(dim=4).any(dim=2)               # the 16 x 16 tiles that hold a drawn sample
    inside = tiles.repeat_interleave(16, 1).repeat_interleave(16, 2)
    assert not bool((differs & ~inside).any())                                             # (what the line above says, tile by tile)
