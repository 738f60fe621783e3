"""CPU: the stream drivers pinned to a recorded trace.  ``StreamTracker`` and ``MultiStreamTracker`` share one core, so the tests
that compare a stream of the one with the other compare that core with itself; here every ``encode`` / ``track`` call the drivers
make on the fake model of tests/test_multistream.py, everything ``push`` / ``finish`` / ``cut`` return and the hop lists are held
against tests/golden/stream_core_trace.json, which this file wrote -- run as a script -- on the drivers as they were BEFORE the
two trackers were merged (two trackers, four state classes).  It uses the public drivers API only, so it runs on either side.
The ``CoverTracker`` scenarios (f) - (i) -- centre and corner seeds, held seeds, the thin step, scene cuts -- were written the same
way on the drivers as they were while ``CoverTracker`` still drove a plain ``StreamTracker`` and a book of its own from outside.

    python tests/test_stream_core.py          # (re)writes the fixture from the drivers it imports
"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from pips_amd import drivers
from test_cover import USER, _cover
from test_cover import VIDEO as TEXTURED
from test_cuts import TA, VIDEO2
from test_multistream import QUERIES, TQS, TS, VIDEOS, _FakeModel, _bits, _chunks, _queries

GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_core_trace.json")


class _Recorder(_FakeModel):
    """the fake model, keeping a line per ``encode`` / ``track`` call"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def encode(self, rgbs, frames_per_pass=16, into=None, clip=None):
        self.calls.append({"name": "encode", "clip": clip, "count": int(rgbs.shape[1])})
        return super().encode(rgbs, frames_per_pass, into=into, clip=clip)

    def track(self, cache, xys, coords_init=None, feat_init=None, iters=3, win_start=None, return_feat=False, win_dir=None,
              win_clip=None):
        self.calls.append({"name": "track", "clip": None, "count": int(xys.shape[1]), "win_start": win_start.reshape(-1).tolist(),
                           "win_clip": None if win_clip is None else win_clip.reshape(-1).tolist(),
                           "feat_init_none": feat_init is None, "iters": int(iters)})
        return super().track(cache, xys, coords_init=coords_init, feat_init=feat_init, iters=iters, win_start=win_start,
                             return_feat=return_feat, win_dir=win_dir, win_clip=win_clip)


class _Outputs:
    """the int32 bit patterns of everything the tracker's calls returned, in order"""

    def __init__(self):
        self.parts = []

    def take(self, res):
        for x in res:
            if x is None:
                self.parts.append(torch.tensor([-1], dtype=torch.int32))
            elif isinstance(x, (tuple, list)):
                self.take(x)
            elif torch.is_tensor(x):
                self.parts.append((_bits(x) if x.is_floating_point() else x.to(torch.int32)).reshape(-1))
            else:
                self.parts.append(torch.tensor([int(x)], dtype=torch.int32))
        return res

    def digest(self):
        return hashlib.sha256(torch.cat(self.parts).numpy().tobytes()).hexdigest()


def _result(model, outs, hops):
    trace = json.dumps(model.calls, sort_keys=True, separators=(",", ":"))
    return {"calls": len(model.calls), "trace": hashlib.sha256(trace.encode()).hexdigest(), "outputs": outs.digest(), "hops": hops}


def _one_stream(chunk, slots, churn):
    """(a) one stream of 37 frames in chunks; (b) ``churn``: queries added after the second push, two columns removed after the
    third, and a cut once 14 frames are in, with queries waiting on frames 20, 29 and 36"""
    m, outs = _Recorder(), _Outputs()
    st = drivers.StreamTracker(m, QUERIES[0], iters=3, slots=slots, record_hops=True)
    cut_hops = None
    for i, c in enumerate(_chunks(VIDEOS[0], chunk), 1):
        outs.take(st.push(c))
        if churn and i == 2:
            outs.take([st.add_queries(_queries([st.emitted, 20], 70))])
        if churn and i == 3:
            outs.take([st.remove_queries([0, 2])])
        if churn and st.cache.T == 14:
            assert bool((st.tq_host == 20).any())
            outs.take(st.cut())
            cut_hops = st.cut_hops
            assert st.tq_host.tolist() and bool((st.tq_host >= 14).all())
    outs.take(st.finish())
    assert st.emitted == TS[0] and (cut_hops is not None) == churn
    return _result(m, outs, {"hops": st.hops, "cut_hops": cut_hops})


SCHED = [(5, 4, None), (None, 3, 2), (9, None, 7), (None, None, None), (12, 14, None), (11, None, None)]      # frames per push


def _streams(slots, cover):
    """(c) three streams of 37 / 21 / 9 frames pushed by ``SCHED``: stream 2 is finished while the others run; queries are added
    to stream 1 after the second push and two columns of stream 0 removed after the fourth; (e) ``cover``: the same pushes of a
    covered tracker, which adds and removes by itself"""
    m, outs = _Recorder(), _Outputs()
    qs = QUERIES if cover is None else [_queries(tq, 50 + v, W=5.0, H=5.0) for v, tq in enumerate(TQS)]
    mt = drivers.MultiStreamTracker(m, qs, iters=3, slots=slots, record_hops=True, cover=cover)
    pos = [0, 0, 0]
    for i, wave in enumerate(SCHED, 1):
        chunks = [None if k is None else VIDEOS[v][:, pos[v]:pos[v] + k] for v, k in enumerate(wave)]
        pos = [p + (k or 0) for p, k in zip(pos, wave)]
        outs.take(mt.push(chunks))
        if cover is None and i == 2:
            outs.take([mt.add_queries(1, _queries([mt.emitted[1], 18], 71))])
        if i == 3:
            outs.take(mt.finish(2))
            assert mt.finished == [False, False, True]
        if cover is None and i == 4:
            outs.take([mt.remove_queries(0, [1, 3])])
    outs.take(mt.finish())
    assert pos == list(TS) == mt.emitted
    hops = [mt.stream_hops(v) if cover is None else mt.cover_hops(v) for v in range(3)]
    return _result(m, outs, hops)


def _single_multi():
    """(d) a MultiStreamTracker of ONE stream: it keeps the clip table"""
    m, outs = _Recorder(), _Outputs()
    mt = drivers.MultiStreamTracker(m, QUERIES[:1], iters=3, slots=9, record_hops=True)
    for c in _chunks(VIDEOS[0], 7):
        outs.take(mt.push([c]))
    outs.take(mt.finish())
    assert all(c["clip"] == 0 for c in m.calls if c["name"] == "encode")
    assert all(c["win_clip"] == [0] * c["count"] for c in m.calls if c["name"] == "track")
    return _result(m, outs, mt.stream_hops(0))


def _covered(chunks, cover, queries, slots, check=None):
    """(f) - (i) a ``CoverTracker`` over ``chunks``: what every ``push`` and ``finish`` return, with ``ids`` after every call, and
    the attributes a caller reads beside them at the end; ``check(ct, parts)`` asserts what the scenario is there for"""
    m, outs = _Recorder(), _Outputs()
    ct = drivers.CoverTracker(m, cover, queries, iters=3, slots=slots, record_hops=True)
    parts = []
    for c in chunks:
        parts.append(outs.take(ct.push(c)))
        outs.take([ct.ids])
    parts.append(outs.take(ct.finish()))
    outs.take([ct.ids])
    assert ct.finished and ct.emitted == sum(c.shape[1] for c in chunks) == sum(p[1].shape[1] for p in parts)
    if check is not None:
        check(ct, parts)
    retired = [[i, f, r] for i, (f, r) in sorted(ct.retired.items())]
    return _result(m, outs, {"hops": ct.hops, "born": ct.born, "retired": retired, "cuts": ct.cuts})


def _held_first(ct, parts):
    """(g) the first push brought no frame: the seeds of the first step waited for the first frames"""
    assert parts[0][1].shape[1] == 0 and len(parts[1][3]) > len(parts[0][3]) and ct.born.count(0) >= 20


def _seeds_moved(ct, parts):
    """(g) the video is textured: seeds of later frames stand off their cells' centres"""
    centres = {(10.0 * j + 5.0, 10.0 * i + 5.0) for i in range(4) for j in range(6)}
    assert any(f > 0 for f in ct.born) and any(tuple(p) not in centres for p in ct.st.xy_in.tolist())


def _book_without_queries():
    """(g) the held seeds no push can reach while a stream has a query, on the book itself as tests/test_corners.py drives it: the
    first seeds are held, join with frames 0..2, all leave the frame on frame 2, and the seeds of that step lie on frame 3,
    which was not pushed yet: held until it comes"""
    H, W = TEXTURED.shape[3:]
    outs, log = _Outputs(), []
    add = lambda q: log.append(outs.take([q.clone()]))
    remove = lambda cols: log.append(outs.take([torch.tensor(list(cols), dtype=torch.int64)]))
    book = drivers._CoverBook(_cover(seed="corners"), torch.zeros(0, dtype=torch.int64), True)

    def state():
        held = None if book.held is None else [book.held[0], book.held[1]]
        outs.take([torch.tensor(book.ids, dtype=torch.int64), torch.tensor(book.born, dtype=torch.int64), held, book.table,
                   book.table0, book.T])
        return book.held

    book.start(H, W, torch.device("cpu"), torch.zeros(0, dtype=torch.int64), torch.zeros(0, 2), add, remove)
    assert state() is not None
    book.see(TEXTURED[0, :3], 0, add)
    assert state() is None and len(book.ids) == 24
    book.step(0, torch.full((3, 24, 2), -5.0), torch.zeros(3, 24), add, remove, [[3]] * 24)
    assert state()[0] == 3 and book.ids == []
    book.see(TEXTURED[0, 3:8], 3, add)
    assert state() is None and book.born == [0] * 24 + [3] * 24 and len(log) == 3
    retired = [[i, f, r] for i, (f, r) in sorted(book.retired.items())]
    return {"calls": len(log), "trace": "", "outputs": outs.digest(), "hops": {"hops": book.all_hops([[]] * 24), "retired": retired}}


# (h) on the 40 x 60 video: on the 6 x 6 frames of ``VIDEOS`` a track leaves the frame before it has stood in a cell for two frames.
# The caller's queries and three more in the cells of the first two, one of them younger
SHARED = torch.cat([USER, torch.tensor([[[0.0, 4.0, 5.0], [0.0, 56.0, 36.0], [3.0, 5.5, 3.25]]])], dim=1)


def _crowded(ct, parts):
    assert any(r == "crowded" for _, r in ct.retired.values())


def _cut_in_scenes(ct, parts):
    """(i) the two scenes of tests/test_cuts.py: one cut -- on the first frame of a push, 21 being a multiple of 1 and of 7 --
    and, in chunks of one frame, pushes behind it that return no frame"""
    silent = any(p[0] == TA and p[1].shape[1] == 0 for p in parts[1:-1])
    assert ct.cuts == [TA] and silent == (len(parts) == VIDEO2.shape[1] + 1)
    assert any(r == (TA - 1, "cut") for r in ct.retired.values())


SCENES = [VIDEO2[:, :5], VIDEO2[:, TA:TA + 4], VIDEO2[:, 5:11], VIDEO2[:, TA + 4:TA + 13]]      # 5, 4, 6 and 9 frames


def _three_cuts(ct, parts):
    """(i) ONE push that holds two cuts, and a cut that falls on the first frame of the next push"""
    assert ct.cuts == [5, 9, 15] and parts[0][1].shape[1] == 9 and len(parts[0][3]) == 3 * 24


SCENARIOS = {}
for _slots in (9, 24):
    for _chunk in (1, 7):
        SCENARIOS[f"a-chunk{_chunk}-slots{_slots}"] = lambda c=_chunk, s=_slots: _one_stream(c, s, False)
        SCENARIOS[f"b-chunk{_chunk}-slots{_slots}"] = lambda c=_chunk, s=_slots: _one_stream(c, s, True)
    SCENARIOS[f"c-slots{_slots}"] = lambda s=_slots: _streams(s, None)
    SCENARIOS[f"e-slots{_slots}"] = lambda s=_slots: _streams(s, drivers.Cover(cell=16))
SCENARIOS["d"] = _single_multi
for _slots in (9, 24):
    for _kw in (dict(), dict(seed="corners")):
        SCENARIOS[f"i-three-cuts-{_kw.get('seed', 'centre')}-slots{_slots}"] = lambda s=_slots, kw=_kw: _covered(
            [torch.cat(SCENES[:3], dim=1), SCENES[3]], _cover(cut_thr=0.5, **kw), None, s, _three_cuts)
    for _chunk in (1, 7):
        _tag = f"chunk{_chunk}-slots{_slots}"
        for _q in ("user", "none"):
            SCENARIOS[f"f-centre-{_q}-{_tag}"] = lambda c=_chunk, s=_slots, q=_q: _covered(
                _chunks(VIDEOS[0], c), drivers.Cover(cell=16), _queries(TQS[0], 50, W=5.0, H=5.0) if q == "user" else None, s)
            SCENARIOS[f"g-corners-held-{_q}-{_tag}"] = lambda c=_chunk, s=_slots, q=_q: _covered(
                [TEXTURED[:, :0]] + _chunks(TEXTURED, c), _cover(seed="corners"), USER if q == "user" else None, s, _held_first)
        SCENARIOS[f"g-corners-{_tag}"] = lambda c=_chunk, s=_slots: _covered(
            _chunks(TEXTURED, c), _cover(seed="corners"), USER, s, _seeds_moved)
        SCENARIOS[f"h-thin-{_tag}"] = lambda c=_chunk, s=_slots: _covered(
            _chunks(TEXTURED[:, :37], c), _cover(per_cell=1, crowd_after=2), SHARED, s, _crowded)
        for _kw in (dict(), dict(seed="corners"), dict(per_cell=1, crowd_after=2)):
            _name = "-".join(f"{k}-{v}" for k, v in _kw.items()) or "centre"
            SCENARIOS[f"i-cut-{_name}-{_tag}"] = lambda c=_chunk, s=_slots, kw=_kw: _covered(
                _chunks(VIDEO2, c), _cover(cut_thr=0.5, **kw), SHARED if "per_cell" in kw else USER, s, _cut_in_scenes)
SCENARIOS["g-book-without-queries"] = _book_without_queries


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_calls_outputs_and_hops_are_the_recorded_ones(name):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(SCENARIOS)
    got = SCENARIOS[name]()
    assert got["calls"] == want[name]["calls"] > 0
    assert got["hops"] == want[name]["hops"]
    assert got["trace"] == want[name]["trace"]
    assert got["outputs"] == want[name]["outputs"]


if __name__ == "__main__":
    results = {k: SCENARIOS[k]() for k in sorted(SCENARIOS)}                     # (a scenario that fails leaves the fixture alone)
    with open(GOLDEN, "w") as f:
        json.dump(results, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
