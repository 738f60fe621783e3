"""GPU: tracks out in the library.  pips_tracks_draw (drivers.draw_tracks) is held, byte for byte, to the torch twin
(drivers.draw_tracks_torch, itself held to plain loops in tests/test_draw.py) on the cases made there: every format and matrix /
range row at one tile, at a one-pixel row and column of tiles and at a size odd both ways; 0 / 1 / 5 / 300 tracks with trails of 0
/ 1 / 4 / 32 rows, with and without the mapping from the model's size.  The surfaces are views of larger allocations whose
sentinel must survive; each case first asserts on the twin's output that it is not vacuous.  End to end a TrackPainter paints a
CoverTracker's pushes on NV12 surfaces to the bytes of one whole-video call."""
import pytest
import torch

from test_draw import case_id, case_inputs, format_cases, grid_cases, not_vacuous, outside_untouched, views, buffers
from test_stream_rounds_gpu import _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


def _run_case(case, with_vis):
    from pips_amd import drivers
    fmt, h, w = case[0], case[3], case[4]
    bufs, trajs, vis, kw = case_inputs(case, with_vis)
    before = [b.clone() for b in bufs]
    dev_bufs = [b.to(DEV) for b in bufs]
    planes = views(dev_bufs, fmt, h, w)
    trajs, vis = trajs.to(DEV), None if vis is None else vis.to(DEV)
    want = _list(drivers.draw_tracks_torch(planes, fmt, trajs, vis, **kw))
    ok, what = not_vacuous(case, planes, want, trajs, kw)
    assert ok, what
    got = _list(drivers.draw_tracks(planes, fmt, trajs, vis, inplace=True, **kw))
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, planes))                 # drawn where they lie, no copy
    for k, (a, b) in enumerate(zip(planes, want)):
        assert torch.equal(a, b), (case_id(case), k, int((a != b).sum()))
    assert outside_untouched([b.cpu() for b in dev_bufs], before, fmt, h, w)
    return what


@pytest.mark.parametrize("case", format_cases(), ids=case_id)
def test_every_format_at_the_tile_edges(case):
    """7 formats (NV12 and I420 under the four matrix / range rows) x 16x16, 17x33, 37x51; F = 3, five tracks with the named
    positions, trail 4; at 17x33 without visibilities"""
    _run_case(case, with_vis=(case[3], case[4]) != (17, 33))


@pytest.mark.parametrize("case", grid_cases(), ids=case_id)
def test_track_counts_trails_and_the_mapping(case):
    """n in {0, 1, 5, 300} (300: a full chunk of 256 and a ragged one) x trail in {0, 1, 4, 32} on the 37x51 surface, positions in
    its own pixels and in those of a 24x32 model frame; NV12 and BGRA"""
    _run_case(case, with_vis=True)


def test_another_stream_and_a_reused_workspace():
    from pips_amd import drivers, ops
    case = ("nv12", "bt709", "limited", 37, 51, 3, 300, 4, None, dict(width=1.0, dot=1.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5))
    bufs, trajs, vis, kw = case_inputs(case)
    trajs, vis = trajs.to(DEV), vis.to(DEV)
    want = _list(drivers.draw_tracks(views([b.to(DEV) for b in bufs], "nv12", 37, 51), "nv12", trajs, vis, **kw))
    colors = drivers.track_colors(torch.arange(300)).to(DEV)
    logit = float(torch.logit(torch.tensor(0.5, dtype=torch.float32)))
    ws = torch.full((ops.draw_workspace_bytes(3, 300, 4) // 4 + 16,), -77, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(side):
        for _ in range(2):                                           # the second call finds the first one's records in the workspace
            planes = views([b.to(DEV) for b in bufs], "nv12", 37, 51)
            ops.draw_tracks(planes, "nv12", trajs[0], vis[0], colors, kw["first"], None, 4, 4, 8, 230, 102, logit, "bt709", "limited",
                            workspace=ws)
            outs.append(planes)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for planes in outs:
        assert all(torch.equal(a, b) for a, b in zip(planes, want))
    assert bool((ws[-16:] == -77).all())                             # nothing behind pips_draw_workspace_bytes is written


# ------------------------------------------------------------------ end to end on the device
EH, EW, ET = 128, 192, 24


def test_painter_on_a_cover_tracker_is_one_whole_video_call(weights_tamed):
    """the cover tests' 128 x 192 video of 24 frames, cells of 32 px, pushed in three chunks: a TrackPainter paints pitched NV12
    surfaces push by push on the device (the rows of a push belong to frames given earlier: the surfaces are kept until then); the
    bytes are those of draw_tracks_torch over track_cover's whole-video result by identity"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    chunks = [video[:, a:b] for a, b in ((0, 8), (8, 16), (16, 24))]
    cover = lambda: drivers.Cover(cell=32, vis_thr=0.9, lost_after=2, scan="library")
    style = dict(width=2.0, dot=2.5, alpha=0.85, alpha_occ=0.35, vis_thr=0.7)
    trail = 6
    bufs = [b.to(DEV) for b in buffers("nv12", ET, EH, EW, 5, pad=(64, 8))]
    before = [b.cpu() for b in bufs]
    surfaces = views(bufs, "nv12", EH, EW)
    untouched = [p.clone() for p in surfaces]

    ct = drivers.CoverTracker(m, cover(), None, iters=6, slots=24, rounds="library")
    painter = drivers.TrackPainter((EH, EW), trail=trail, **style)
    painted = 0
    for part in [ct.push(c) for c in chunks] + [ct.finish()]:
        f0, trajs, vis, ids = part
        assert f0 == painted
        painter.paint([p[f0:f0 + trajs.shape[1]] for p in surfaces], "nv12", f0, trajs, vis, ids=ids)
        painted += trajs.shape[1]
    assert painted == ET
    torch.cuda.synchronize()

    trajs, vis, born, retired = drivers.track_cover(m, chunks, cover(), iters=6, slots=24, rounds="library")
    K = trajs.shape[2]
    assert K >= 24 and int((retired >= 0).sum()) + int((born > 0).sum()) > 0              # identities come and go between the pushes
    want = drivers.draw_tracks_torch(untouched, "nv12", trajs, vis, colors=drivers.track_colors(torch.arange(K)), trail=trail, **style)
    for a, b in zip(surfaces, want):
        assert torch.equal(a, b), int((a != b).sum())
    changed = float((surfaces[0] != untouched[0]).float().mean())
    print(f"painter e2e: {K} identities, {changed:.1%} of the luma samples changed")
    assert 0.01 < changed < 0.9
    assert outside_untouched([b.cpu() for b in bufs], before, "nv12", EH, EW)
