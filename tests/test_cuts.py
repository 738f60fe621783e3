"""CPU: scene cuts -- drivers.cut_table_torch / find_cuts (the regional luma histogram rule of pips_cut_table, include/pips_hip.h),
StreamTracker.cut() on the fake model of tests/test_stream.py, and Cover(cut_thr=) / CoverTracker on the fake model of
tests/test_cover.py with ``scan="torch"``.  The rule is restated here as a plain-Python loop over the pixels.  The two-scene video
is noise in [0, 100) followed by noise in [150, 255]: 21 + 19 frames, the cut before frame 21.  (The kernel and ``scan="library"``:
tests/test_cuts_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers

from test_cover import CELL, H, USER, W, _cover
from test_multistream import _FakeModel, _bits
from test_stream import _FakeModel as _StreamModel
from test_stream import _queries
from test_stream import _video as _small_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TA, TB = 21, 19
EDGE = [-3.0, -0.0, 254.5, 255.49, 300.0]


def _scenes(h, w, seed, dtype=torch.float32):
    """(1, 21 + 19, 3, h, w): noise uniform in [0, 100), then in [150, 255]"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(1, TA, 3, h, w, generator=g) * 100.0
    b = 150.0 + torch.rand(1, TB, 3, h, w, generator=g) * 105.0
    return torch.cat([a, b], dim=1).to(dtype)


def _frames(F, h, w, dtype, seed):
    """random frames with the float edge values sprinkled over the first of them and a flat last frame (F >= 2)"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        fr = torch.randint(0, 256, (F, 3, h, w), generator=g, dtype=torch.uint8)
    else:
        fr = torch.rand(F, 3, h, w, generator=g) * 255.0
        if F > 0:
            flat = fr[0].reshape(-1)
            at = torch.randperm(flat.numel(), generator=g)[:len(EDGE) * 3]
            flat[at] = torch.tensor(EDGE * 3)[:at.numel()]
    if F >= 2:
        fr[F - 1] = 200                                                    # every pixel of a region in one bin
    return fr


def _rule(frames, prev):
    """the rule, pixel by pixel -> (hist as nested lists, dist as a list)"""
    F, _, h, w = frames.shape
    a = frames.numpy()
    hists = []
    for f in range(F):
        hist = [[0] * 32 for _ in range(16)]
        for y in range(h):
            for x in range(w):
                ch = []
                for k in range(3):
                    v = a[f, k, y, x]
                    if a.dtype == np.uint8:
                        ch.append(int(v))
                    else:                                                  # fp32 throughout, as the kernel computes it
                        ch.append(int(np.floor(np.minimum(np.maximum(v, np.float32(0)), np.float32(255)) + np.float32(0.5))))
                Y = (77 * ch[0] + 150 * ch[1] + 29 * ch[2] + 128) >> 8
                hist[4 * ((4 * y) // h) + (4 * x) // w][Y >> 3] += 1
        hists.append(hist)
    dist = []
    for f in range(F):
        old = hists[f - 1] if f > 0 else (prev.tolist() if prev is not None else hists[0])
        dist.append(sum(abs(hists[f][r][b] - old[r][b]) for r in range(16) for b in range(32)))
    return hists, dist


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 53), (40, 60)])
def test_torch_form_is_the_rule_restated(h, w, dtype):
    """hist and dist at F = 0 / 1 / 5, with and without prev_hist, over the float edge values and a flat frame"""
    g = torch.Generator().manual_seed(h * w)
    prev = torch.randint(0, h * w + 1, (16, 32), generator=g, dtype=torch.int32)
    for F in (0, 1, 5):
        fr = _frames(F, h, w, dtype, 10 * F + h)
        for p in (None, prev):
            hist, dist = drivers.cut_table_torch(fr, p)
            ref_h, ref_d = _rule(fr, p)
            assert tuple(hist.shape) == (F, 16, 32) and tuple(dist.shape) == (F,)
            assert not hist.is_floating_point() and not dist.is_floating_point()
            assert hist.tolist() == ref_h and dist.tolist() == ref_d
            assert hist.sum(dim=(1, 2)).tolist() == [h * w] * F
    if dtype == torch.float32:                                             # the edge values themselves: 0, 0, 255, 255, 255
        fr = torch.tensor(EDGE).view(5, 1, 1, 1).expand(5, 3, 1, 1).contiguous()
        hist, _ = drivers.cut_table_torch(fr)
        assert [int(torch.nonzero(hist[f].sum(0))[0, 0]) for f in range(5)] == [0, 0, 31, 31, 31]


def test_distance_properties():
    fr = _frames(3, 37, 53, torch.uint8, 3)
    hist, dist = drivers.cut_table_torch(torch.cat([fr, fr[2:]]))
    assert dist[0] == 0 and dist[3] == 0 and dist[1] > 0                  # the first frame, and a frame against itself
    assert int(hist[2].max()) >= (37 // 4) * (53 // 4)                   # the flat frame: a region in one bin
    again, d2 = drivers.cut_table_torch(fr[1:], hist[0])                   # carried from call to call
    assert torch.equal(again, hist[1:3]) and d2.tolist() == dist[1:3].tolist()
    for h, w in ((1, 1), (3, 5), (40, 60)):
        bw = torch.stack([torch.zeros(3, h, w), torch.full((3, h, w), 255.0)])
        assert drivers.cut_table_torch(bw)[1].tolist() == [0, 2 * h * w]
    assert drivers.cut_limit(0.5, 40, 60) == 2400 and drivers.cut_limit(0.25, 3, 5) == 7
    with pytest.raises(ValueError):
        drivers.cut_table_torch(torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError):
        drivers.cut_table_torch(torch.zeros(2, 3, 8, 8), torch.zeros(16, 32))
    with pytest.raises(ValueError):
        drivers.cut_table_torch(torch.zeros(2, 3, 8, 8), torch.zeros(16, 31, dtype=torch.int32))


@pytest.mark.parametrize("h,w", [(40, 60), (64, 96)])
def test_scene_videos_have_one_clear_cut(h, w):
    """the condition the end-to-end tests rest on: within a scene dist / 2hw <= 0.3, across the cut >= 0.7 (measured: 0.16 / 0.10
    within a scene at the two sizes, 1.0 across); find_cuts, sliced or not, uint8 or float, finds frame 21 alone"""
    video = _scenes(h, w, 11)
    d = drivers.cut_table_torch(video[0])[1].double() / (2 * h * w)
    print(f"{h}x{w}: within a scene {max(float(d[1:TA].max()), float(d[TA + 1:].max())):.3f}, across the cut {float(d[TA]):.3f}")
    assert float(d[1:TA].max()) <= 0.3 and float(d[TA + 1:].max()) <= 0.3 and float(d[TA]) >= 0.7
    assert drivers.find_cuts(video) == [TA] and drivers.find_cuts(video, 0.5, slice_frames=7) == [TA]
    assert drivers.find_cuts(video.to(torch.uint8), slice_frames=21) == [TA]
    assert drivers.find_cuts(video[:, :TA]) == [] and drivers.find_cuts(video[:, TA - 1:TA + 1], 0.69) == [1]
    for bad in (dict(cut_thr=0.0), dict(cut_thr=None), dict(scan="cpu"), dict(slice_frames=0)):
        with pytest.raises(ValueError):
            drivers.find_cuts(video, **bad)
    with pytest.raises(ValueError):
        drivers.find_cuts(video[0])


# ---------------------------------------------------------------------------------------------- StreamTracker.cut()
def _pieces(video, chunk, c, lo, hi):
    """the frames [lo, hi) of the video as a caller pushes them who feeds chunks of ``chunk`` frames and splits them at ``c``"""
    out = []
    for i in range(0, video.shape[1], chunk):
        for a, b in ((i, min(i + chunk, c)), (max(i, c), i + chunk)):
            a, b = max(a, lo), min(b, hi, video.shape[1])
            if b > a:
                out.append(video[:, a:b])
    return out


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7, 8])
def test_stream_cut_ends_the_started_and_keeps_the_waiting(chunk, slots):
    """T = 21 + 19: the columns of the queries before the cut, over all pushes and the cut, are track_stream on the first 21 frames
    in bits and hops; a query waiting on frame 25 survives the cut, and it and the queries added after the cut are track_stream on
    the video that starts at frame 21; the state shrinks to the survivors"""
    video = _small_video(TA + TB, 21)
    q1 = _queries([0, 20, 5, 5, 13, 25, 17], 22)                         # column 5 waits on a frame behind the cut
    q2 = _queries([21, 30, 24, 39], 23)
    m = _StreamModel()
    st = drivers.StreamTracker(m, q1, iters=3, slots=slots, record_hops=True)
    first = [st.push(p) for p in _pieces(video, chunk, TA, 0, TA)]
    n_state = st.trajs.shape[1]
    f0, trajs, vis, keep = st.cut()
    assert n_state == 7 and keep.tolist() == [5] and keep.dtype == torch.int64
    assert f0 + trajs.shape[1] == TA == st.emitted and tuple(trajs.shape[2:]) == (7, 2) and tuple(vis.shape[2:]) == (7,)
    assert f0 < TA                                                         # the cut returned frames that windows held back
    assert st.N == 1 and st.tq_host.tolist() == [25] and st.trajs.shape[1] == 1 and st.vis.shape[1] == 1 and st.cur.shape[0] == 1
    assert len(st.hops) == 1 and st.hops[0] == [] and len(st.cut_hops) == 7
    got_t = torch.cat([p[1] for p in first] + [trajs], dim=1)
    got_v = torch.cat([p[2] for p in first] + [vis], dim=1)
    assert [p[0] for p in first] == np.cumsum([0] + [p[1].shape[1] for p in first])[:-1].tolist() and got_t.shape[1] == TA
    ref_t, ref_v, ref_h = drivers.track_stream(_StreamModel(), _pieces(video, chunk, TA, 0, TA), q1[:, [0, 1, 2, 3, 4, 6]], iters=3,
                                               slots=slots, return_hops=True)
    ended = [0, 1, 2, 3, 4, 6]
    assert _same(got_t[:, :, ended], ref_t) and _same(got_v[:, :, ended], ref_v)
    assert [st.cut_hops[k] for k in ended] == ref_h and any(len(h) > 1 for h in ref_h)
    assert bool(got_t[:, :, 5].isnan().all()) and bool(got_v[:, :, 5].isnan().all())
    # the second part: the waiting query and four new ones, one of them on the first frame behind the cut
    cols = st.add_queries(q2)
    assert cols.tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        st.add_queries(_queries([20], 1))                                  # frame 20 was returned
    second = [st.push(p) for p in _pieces(video, chunk, TA, TA, TA + TB)] + [st.finish()]
    got_t, got_v = torch.cat([p[1] for p in second], dim=1), torch.cat([p[2] for p in second], dim=1)
    assert second[0][0] == TA and got_t.shape[1] == TB
    q = torch.cat([q1[:, 5:6], q2], dim=1) - torch.tensor([float(TA), 0.0, 0.0])
    ref_t, ref_v, ref_h = drivers.track_stream(_StreamModel(), _pieces(video, chunk, TA, TA, TA + TB), q, iters=3, slots=slots,
                                               return_hops=True)
    assert _same(got_t, ref_t) and _same(got_v, ref_v) and st.hops == ref_h
    assert 1 <= m.max_pass <= slots


def test_stream_cut_before_the_first_push_and_after_finish():
    video = _small_video(12, 31)
    q = _queries([0, 3], 32)
    st = drivers.StreamTracker(_StreamModel(), q, iters=3, slots=9)
    f0, trajs, vis, keep = st.cut()
    assert f0 == 0 and tuple(trajs.shape) == (1, 0, 2, 2) and tuple(vis.shape) == (1, 0, 2) and keep.tolist() == [0, 1] and st.N == 2
    parts = [st.push(video[:, :12]), st.finish()]
    ref = drivers.track_stream(_StreamModel(), [video], q, iters=3, slots=9)
    assert _same(torch.cat([p[1] for p in parts], dim=1), ref[0])
    with pytest.raises(ValueError):
        st.cut()
    assert st.finished and st.N == 2 and st.emitted == 12
    # two cuts in a row: the second has nothing to return and nobody to end
    st = drivers.StreamTracker(_StreamModel(), q, iters=3, slots=9)
    st.push(video[:, :5])
    assert st.cut()[3].tolist() == [] and st.N == 0
    f0, trajs, vis, keep = st.cut()
    assert f0 == 5 and trajs.shape[1] == 0 and keep.tolist() == []


# ---------------------------------------------------------------------------------------------- Cover(cut_thr=)
VIDEO2 = _scenes(H, W, 12)


def _track(chunks, cover, queries, slots):
    ct = drivers.CoverTracker(_FakeModel(), cover, queries, iters=3, slots=slots, record_hops=True)
    heads = []
    for c in chunks:
        alive, n = ct.ids.tolist(), len(ct.born)
        heads.append((alive, n, ct.push(c)))
    parts = [h[2] for h in heads] + [ct.finish()]
    trajs, vis, born, retired = drivers._by_identity(parts, ct.book)
    return ct, trajs, vis, born.tolist(), heads


@pytest.mark.parametrize("kw", [dict(), dict(max_queries=20), dict(per_cell=1, crowd_after=2), dict(seed="corners")],
                         ids=["plain", "max_queries", "per_cell", "corners"])
@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [3, 7, 8])
def test_cover_with_a_cut_is_the_two_scenes_tracked_apart(chunk, slots, kw):
    """track_cover on A || B with cut_thr: the identities born before the cut are track_cover on A pushed in the same pieces --
    except that those alive at A's end are retired as "cut" on A's last frame --, those born from the cut on are track_cover on B
    pushed in B's pieces, shifted by 21 frames and by A's identity count; chunk 8 has the cut inside a push, 3 and 7 at its start"""
    c, T = TA, TA + TB
    whole = [VIDEO2[:, i:i + chunk] for i in range(0, T, chunk)]
    ct, trajs, vis, born, heads = _track(whole, _cover(cut_thr=0.5, **kw), USER, slots)
    assert ct.cuts == [c]
    a, ta, va, born_a, _ = _track(_pieces(VIDEO2, chunk, c, 0, c), _cover(**kw), USER, slots)
    b, tb, vb, born_b, _ = _track(_pieces(VIDEO2, chunk, c, c, T), _cover(**kw), None, slots)
    KA, KB = len(born_a), len(born_b)
    assert KA > USER.shape[1] and KB >= 20 and len(born) == KA + KB
    assert born[:KA] == born_a and born[KA:] == [t + c for t in born_b] and born[KA:KA + 20] == [c] * 20
    assert _same(trajs[:, :c, :KA], ta) and _same(vis[:, :c, :KA], va) and bool(trajs[:, c:, :KA].isnan().all())
    assert _same(trajs[:, c:, KA:], tb) and _same(vis[:, c:, KA:], vb) and bool(trajs[:, :c, KA:].isnan().all())
    assert bool(vis[:, c:, :KA].isnan().all()) and bool(vis[:, :c, KA:].isnan().all())
    alive_a = [i for i in range(KA) if i not in a.retired]
    assert alive_a and any(r != "cut" for _, r in ct.retired.values())
    assert {i: r for i, r in ct.retired.items() if i < KA} == {**a.retired, **{i: (c - 1, "cut") for i in alive_a}}
    assert {i - KA: (f - c, r) for i, (f, r) in ct.retired.items() if i >= KA} == b.retired
    assert ct.hops[:KA] == a.hops and ct.hops[KA:] == b.hops and any(len(h) > 1 for h in ct.hops[KA:])
    # the push that holds the cut: the identities alive at its start, then those created in it, NaN outside each life
    for k, (alive, n, (f0, t, v, ids)) in enumerate(heads):
        ids = ids.tolist()                                                 # (the first step and held corner seeds add columns too)
        assert ids[:len(alive)] == alive and ids[len(alive):] == list(range(n, n + len(ids) - len(alive)))
        if k != c // chunk:
            assert all(born[i] < c for i in ids) or all(born[i] >= c for i in ids)
            continue
        assert f0 < c <= f0 + t.shape[1]                                   # the cut returned the old scene's last frames
        assert all(born[i] <= c for i in ids) and sum(born[i] == c for i in ids) >= 20
        assert tuple(t.shape) == (1, t.shape[1], len(ids), 2) and tuple(v.shape) == (1, t.shape[1], len(ids))
        for j, i in enumerate(ids):
            life = torch.arange(f0, f0 + t.shape[1])
            life = (life >= born[i]) & (life <= ct.retired.get(i, (T,))[0]) & ((life < c) == (i < KA))
            assert torch.equal(~t[0, :, j, 0].isnan(), life) and torch.equal(~v[0, :, j].isnan(), life)


@pytest.mark.parametrize("kw", [dict(), dict(seed="corners")], ids=["centre", "corners"])
def test_two_cuts_in_one_push_and_a_cut_at_the_start_of_the_next(kw):
    """scenes of 5, 4, 6 and 9 frames, the first three in ONE push (cuts before frames 5 and 9, shorter than a window), the fourth
    in a push of its own (the cut before its first frame): every scene is track_cover on that scene alone"""
    v = VIDEO2
    scenes = [v[:, :5], v[:, TA:TA + 4], v[:, 5:11], v[:, TA + 4:TA + 13]]
    starts = [0, 5, 9, 15]
    ct, trajs, vis, born, heads = _track([torch.cat(scenes[:3], dim=1), scenes[3]], _cover(cut_thr=0.5, **kw), None, 24)
    assert ct.cuts == starts[1:] and len(heads[0][2][3]) == 3 * 24 and heads[0][2][1].shape[1] == 9
    k0 = 0
    for s, f0 in zip(scenes, starts):
        one, t1, v1, born1, _ = _track([s], _cover(**kw), None, 24)
        k1, T1 = k0 + len(born1), f0 + s.shape[1]
        assert born[k0:k1] == [b + f0 for b in born1] and born1[:24] == [0] * 24
        assert _same(trajs[:, f0:T1, k0:k1], t1) and _same(vis[:, f0:T1, k0:k1], v1) and ct.hops[k0:k1] == one.hops
        assert bool(trajs[:, :f0, k0:k1].isnan().all()) and bool(trajs[:, T1:, k0:k1].isnan().all())
        mine = {i - k0: (f - f0, r) for i, (f, r) in ct.retired.items() if k0 <= i < k1}
        ends = {} if f0 == starts[-1] else {i: (s.shape[1] - 1, "cut") for i in range(k1 - k0) if i not in one.retired}
        assert mine == {**one.retired, **ends}
        k0 = k1
    assert k0 == len(born)


def test_cut_thr_none_changes_nothing_and_bad_values_are_rejected():
    chunks = [VIDEO2[:, i:i + 7] for i in range(0, TA + TB, 7)]
    x, y = _track(chunks, _cover(cut_thr=None), USER, 9), _track(chunks, _cover(), USER, 9)
    assert x[0].cuts == [] and x[0].book.prev_hist is None                # no frame was looked at
    assert _same(x[1], y[1]) and _same(x[2], y[2]) and x[3] == y[3] and x[0].retired == y[0].retired and x[0].hops == y[0].hops
    assert not any(r == "cut" for _, r in x[0].retired.values())
    assert all(torch.equal(p[2][3], q[2][3]) and _same(p[2][1], q[2][1]) for p, q in zip(x[4], y[4]))
    # a threshold nothing reaches: the frames are looked at and nothing else changes
    one = [VIDEO2[:, i:i + 7] for i in range(0, TA, 7)]
    z, y = _track(one, _cover(cut_thr=0.5), USER, 9), _track(one, _cover(), USER, 9)
    assert z[0].cuts == [] and z[0].book.prev_hist is not None and _same(z[1], y[1]) and z[3] == y[3]
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, True, "0.5", float("nan")):
        with pytest.raises(ValueError):
            drivers.Cover(cut_thr=bad)
    assert drivers.Cover(cut_thr=0.25).cut_thr == 0.25 and drivers.Cover().cut_thr is None
    q = [_queries([0], 1)]
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(_FakeModel(), q, cover=_cover(cut_thr=0.5))
    drivers.MultiStreamTracker(_FakeModel(), q, cover=_cover(cut_thr=None))


def test_cut_table_is_declared_bound_and_exported():
    from pips_amd import _build, _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_cut_table" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)       # the history comment
    assert "Y >> 3" in hdr and "(4 y) / h" in hdr                          # the rule stands in the header
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_cut_table\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 11
    proto = re.search(r"\bsize_t\s+pips_cut_workspace_bytes\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 3
    assert len(_lib.SIGNATURES["pips_cut_table"][1]) == 11 and _lib.SIGNATURES["pips_cut_table"][0] is ctypes.c_int
    assert _lib.SIGNATURES["pips_cut_table"][1][9] is ctypes.c_size_t
    assert _lib.SIGNATURES["pips_cut_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert "cuts.hip" in _build.SOURCES and any(h.endswith("luma.h") for h in _build.headers())
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_cut_table") and hasattr(raw, "pips_cut_workspace_bytes") and callable(ops.cut_table)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the sizing query is a host function: 4 region rows of S strips per frame, 128 counters each
    assert lib.pips_cut_workspace_bytes(2, 360, 640) == 2 * 4 * 12 * 512
    assert lib.pips_cut_workspace_bytes(5, 1, 1) == 5 * 4 * 512 and lib.pips_cut_workspace_bytes(1, 4096, 8) == 4 * 16 * 512
    assert lib.pips_cut_workspace_bytes(0, 8, 8) == 0 and lib.pips_cut_workspace_bytes(-1, 8, 8) == 0
    assert lib.pips_cut_workspace_bytes(1, 0, 8) == 0 and lib.pips_cut_workspace_bytes(1, 8, 0) == 0
    assert lib.pips_cut_workspace_bytes(1, 1 << 15, 1 << 15) > 0 and lib.pips_cut_workspace_bytes(1, (1 << 15) + 1, 1 << 15) == 0
    # the host-side rejections need no device: nothing is launched
    for args in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, (1 << 15) + 1, 1 << 15)):
        assert lib.pips_cut_table(None, 1, args[0], args[1], args[2], None, None, None, None, 0, None) == -1
    assert lib.pips_cut_table(None, 1, 0, 8, 8, None, None, None, None, 0, None) == 0
    assert lib.pips_cut_table(None, 1, 1, 8, 8, None, None, None, None, 0, None) == -1
