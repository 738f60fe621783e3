"""CPU: drivers.Cover / CoverTracker / track_cover and MultiStreamTracker(cover=) -- a stream that retires the queries that left
the frame or stayed invisible and seeds the empty cells of a grid over the frame -- on the fake model of
tests/test_multistream.py with ``scan="torch"``.  The video has a real frame size (40 x 60, cells of 10 px: a 4 x 6 grid), the fake
tracker drifts every point towards the lower right by about a pixel per frame and gives visibility logits of both signs, so
queries leave the frame, get lost and are replaced.  The rule is restated here as a plain-Python loop over the returned rows.
(``scan="library"`` needs the library's kernels: tests/test_cover_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers

from test_multistream import _FakeModel, _bits, _chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CELL, T = 40, 60, 10, 45
GH, GW = 4, 6
LOST_AFTER = 3


def _video(T_, seed, H_=H, W_=W):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, T_, 3, H_, W_, generator=g) * 255


VIDEO = _video(T, 7)
# the caller's own queries: frame 0, a late one (pending for a while: it holds its cell), one that starts outside the frame
USER = torch.tensor([[[0.0, 3.0, 4.0], [0.0, 55.5, 35.25], [12.0, 25.0, 15.0], [5.0, 58.0, 38.5], [20.0, 70.0, 10.0]]])


def _cover(**kw):
    return drivers.Cover(**{**dict(cell=CELL, vis_thr=0.5, lost_after=LOST_AFTER), **kw})


class _Sim:
    """the cover rule restated: plain Python over the rows a push returned (fp32 only where the rule says fp32: the quotient)"""

    def __init__(self, queries, max_queries=None, Hs=H, Ws=W):
        self.H, self.W, self.gh, self.gw = Hs, Ws, -(-Hs // CELL), -(-Ws // CELL)
        self.max = max_queries
        self.live = [dict(id=i, tq=int(q[0]), xy=(float(q[1]), float(q[2])), lost=0) for i, q in enumerate(queries[0].tolist())]
        self.born = [q["tq"] for q in self.live]
        self.xy = {q["id"]: q["xy"] for q in self.live}
        self.retired, self.steps = {}, []

    def inside(self, x, y):
        return x >= 0 and x <= self.W - 1 and y >= 0 and y <= self.H - 1

    def cell(self, x, y):
        q = lambda a: int(np.floor(np.float32(a) / np.float32(CELL)))
        return min(q(y), self.gh - 1), min(q(x), self.gw - 1)

    def step(self, f1, trajs, vis):
        m, f = vis.shape[0], f1 - 1
        keep, occupied, pending = [], set(), []
        for c, q in enumerate(self.live):
            if m == 0 or q["tq"] > f:
                q["lost"] = 0
                keep.append(q)
                pending.append(q["id"])
                if self.inside(*q["xy"]):
                    occupied.add(self.cell(*q["xy"]))
                continue
            for g in range(m):
                if f1 - m + g >= q["tq"]:
                    q["lost"] = q["lost"] + 1 if float(vis[g, c]) < 0.0 else 0          # logit(0.5) = 0
            x, y = (float(v) for v in trajs[m - 1, c])
            if not self.inside(x, y):
                self.retired[q["id"]] = (f, "outside")
            elif q["lost"] >= LOST_AFTER:
                self.retired[q["id"]] = (f, "lost")
            else:
                keep.append(q)
                occupied.add(self.cell(x, y))
        room = len(occupied) + self.gh * self.gw if self.max is None else max(0, self.max - len(keep))
        empty = [(i, j) for i in range(self.gh) for j in range(self.gw) if (i, j) not in occupied]
        seeds = [(f1, min((j + 0.5) * CELL, self.W - 1), min((i + 0.5) * CELL, self.H - 1)) for i, j in empty[:room]]
        self.steps.append(dict(f1=f1, n_before=len(self.live), n_keep=len(keep), seeds=seeds, cut=len(empty) > room,
                               occupied=occupied, pending=pending))
        self.live = keep
        for t, x, y in seeds:
            i = len(self.born)
            self.live.append(dict(id=i, tq=t, xy=(x, y), lost=0))
            self.born.append(t)
            self.xy[i] = (x, y)


def _run(chunk, slots, cover, queries=USER, video=VIDEO, record_hops=False):
    """a CoverTracker over the video in chunks, the restated rule run beside it on the returned rows, ids checked at every push
    -> (tracker, sim, parts, the number of pushes that returned no frame)"""
    ct = drivers.CoverTracker(_FakeModel(), cover, queries, iters=3, slots=slots, record_hops=record_hops)
    sim = _Sim(torch.zeros(1, 0, 3) if queries is None else queries, cover.max_queries, *video.shape[3:])
    parts, silent = [], 0
    sim.step(0, None, torch.zeros(0, len(sim.live)))                   # the first step: inside the first push, no rows
    for c in _chunks(video, chunk):
        f0, trajs, vis, ids = ct.push(c)
        assert ids.dtype == torch.int64 and ids.tolist() == [q["id"] for q in sim.live]
        assert len({(q["tq"], q["xy"]) for q in sim.live}) == len(sim.live)       # nobody is seeded twice
        assert tuple(trajs.shape) == (1, trajs.shape[1], len(sim.live), 2) and tuple(vis.shape) == tuple(trajs.shape[:3])
        parts.append((f0, trajs, vis, ids))
        if trajs.shape[1] == 0:
            silent += 1                                                  # no frame returned: no step
            continue
        sim.step(f0 + trajs.shape[1], trajs[0], vis[0])
    n_steps = len(sim.steps)
    f0, trajs, vis, ids = ct.finish()
    assert ids.tolist() == [q["id"] for q in sim.live] and len(sim.steps) == n_steps      # finish() runs no step
    parts.append((f0, trajs, vis, ids))
    assert sum(p[1].shape[1] for p in parts) == video.shape[1]
    return ct, sim, parts, silent


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_the_rule_restated_independently(chunk, slots):
    """ids at every push, .born and .retired (frame and reason) are those of the plain-Python rule on the returned rows; the run
    has retirements of both reasons, re-seeds after frame 0 and pushes without a step"""
    ct, sim, parts, silent = _run(chunk, slots, _cover())
    assert ct.born == sim.born and ct.retired == sim.retired
    reasons = [r for _, r in sim.retired.values()]
    assert reasons.count("outside") >= 1 and reasons.count("lost") >= 1
    assert any(t > 0 for t in sim.born[USER.shape[1]:]) and silent >= 1
    assert sim.born[USER.shape[1]] == 0                                  # the first step seeded frame 0
    # the outside query of the caller was never tracked into a cell and retired on its first returned frame
    assert sim.retired[4][1] == "outside" and sim.retired[4][0] >= 20


def test_each_identity_is_the_stream_given_it_alone():
    """over its life every identity is, bit for bit with the hop list, track_stream given only that query up front; the frames
    behind its retirement are absent (NaN), and its hop list stops where the retirement cut it"""
    chunks = _chunks(VIDEO, 3)
    trajs, vis, born, retired, hops = drivers.track_cover(_FakeModel(), chunks, _cover(), USER, iters=3, slots=9, return_hops=True)
    ct, sim, _, _ = _run(3, 9, _cover())
    K = len(sim.born)
    assert tuple(trajs.shape) == (1, T, K, 2) and tuple(vis.shape) == (1, T, K)
    assert born.tolist() == sim.born and retired.tolist() == [sim.retired.get(i, (-1,))[0] for i in range(K)]
    cut = 0
    for i in range(K):
        q = torch.tensor([[[float(sim.born[i]), *sim.xy[i]]]])
        ref_t, ref_v, ref_h = drivers.track_stream(_FakeModel(), chunks, q, iters=3, slots=9, return_hops=True)
        end = T if int(retired[i]) < 0 else int(retired[i]) + 1
        assert torch.equal(_bits(trajs[0, :end, i]), _bits(ref_t[0, :end, 0])), i
        assert torch.equal(_bits(vis[0, :end, i]), _bits(ref_v[0, :end, 0])), i
        assert bool(torch.isnan(trajs[0, end:, i]).all()) and bool(torch.isnan(vis[0, end:, i]).all())
        assert bool(torch.isnan(trajs[0, :sim.born[i], i]).all())
        if int(retired[i]) < 0:
            assert hops[i] == ref_h[0], i
        else:
            assert hops[i] == ref_h[0][:len(hops[i])], i
            cut += len(hops[i]) < len(ref_h[0])
    assert cut >= 1 and K > USER.shape[1] + GH * GW - 4


@pytest.mark.parametrize("max_queries", [None, 20, 26])
def test_invariants_after_every_step(max_queries):
    """every cell holds a kept or pending query unless the cap cut the seeds; seeding never lifts the live count above the cap;
    a cell that a pending query holds is not seeded"""
    ct, sim, parts, _ = _run(3, 9, _cover(max_queries=max_queries))
    assert ct.born == sim.born and ct.retired == sim.retired
    cuts = 0
    for s in sim.steps:
        cells = set(s["occupied"]) | {(int(y // CELL), int(x // CELL)) for _, x, y in s["seeds"]}
        if s["cut"]:
            cuts += 1
            assert s["n_keep"] + len(s["seeds"]) == max(max_queries, s["n_keep"])
        else:
            assert cells == {(i, j) for i in range(GH) for j in range(GW)}
        if max_queries is not None:
            assert s["n_keep"] + len(s["seeds"]) <= max(max_queries, s["n_keep"])
    assert (cuts >= 1) == (max_queries is not None)
    # the caller's query 2 waits for frame 12 in cell (1, 2): no seed lands there while it is pending (nor while it is tracked)
    centre = (25.0, 15.0)
    for s in sim.steps:
        if 2 in s["pending"]:
            assert all((x, y) != centre for _, x, y in s["seeds"])
    assert any(2 in s["pending"] for s in sim.steps[1:])


def test_a_cap_below_the_survivors_seeds_nothing_and_changes_nothing_else():
    """max_queries = 2 under five queries of the caller: no seed while two or more survive (only once fewer do), and the
    survivors stay as they are"""
    ct, sim, parts, _ = _run(3, 9, _cover(max_queries=2))
    assert ct.born == sim.born and ct.retired == sim.retired
    above = [s for s in sim.steps if s["n_keep"] >= 2]
    assert len(above) >= 4 and above[0]["n_keep"] == 5 and all(len(s["seeds"]) == 0 for s in above)
    assert all(s["n_keep"] + len(s["seeds"]) == 2 for s in sim.steps if s["n_keep"] < 2)
    # nothing else changes: the survivors keep their columns and identities (checked at every push by _run against the rule)
    first = sim.steps[1]
    after = next(i for i, p in enumerate(parts) if p[1].shape[1] > 0) + 1       # the push behind the first step with rows
    gone = [i for i, r in sim.retired.items() if r[0] < first["f1"]]
    assert first["n_keep"] > 2 and parts[after][3].tolist() == [q for q in range(5) if q not in gone]


def test_no_queries_of_the_caller():
    """queries=None: the tracker starts from the seeds of the first step alone"""
    ct, sim, parts, _ = _run(7, 24, _cover(), queries=None)
    assert ct.born == sim.born and ct.retired == sim.retired and ct.born[:GH * GW] == [0] * (GH * GW)
    assert parts[1][3].tolist()[:GH * GW] == list(range(GH * GW))


TS = (37, 21, 9)
MULTI_Q = [USER, USER[:, :2], torch.zeros(1, 0, 3)]


@pytest.mark.parametrize("rounds_chunk", [3, (7, 3, 1)])
def test_every_covered_stream_is_its_own_cover_tracker(rounds_chunk):
    """MultiStreamTracker(cover=): three streams of 37 / 21 / 9 frames, each pushed part equal to the part its own CoverTracker
    returns on the same chunks -- f0, bits, ids -- with born, retired and the hop lists; track_streams(cover=) is track_cover"""
    sizes = rounds_chunk if isinstance(rounds_chunk, tuple) else (rounds_chunk,) * 3
    videos = [_video(t, 60 + v) for v, t in enumerate(TS)]
    lists = [_chunks(v, s) for v, s in zip(videos, sizes)]
    cover = _cover()
    mt = drivers.MultiStreamTracker(_FakeModel(), MULTI_Q, iters=3, slots=9, record_hops=True, cover=cover)
    parts = [[] for _ in TS]
    for i in range(max(len(c) for c in lists) + 1):
        for v, c in enumerate(lists):
            if len(c) == i:
                parts[v].append(mt.finish(v))
        wave = [c[i] if i < len(c) else None for c in lists]
        if any(w is not None for w in wave):
            for v, p in enumerate(mt.push(wave)):
                if wave[v] is not None:
                    parts[v].append(p)
                else:
                    assert p[1].shape[1] == 0
    for v in range(3):
        ct = drivers.CoverTracker(_FakeModel(), cover, MULTI_Q[v], iters=3, slots=9, record_hops=True)
        own = [ct.push(c) for c in lists[v]] + [ct.finish()]
        assert len(own) == len(parts[v])
        for (f0, t, vi, ids), (g0, gt, gv, gids) in zip(parts[v], own):
            assert f0 == g0 and torch.equal(ids, gids) and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(vi), _bits(gv))
        assert mt.books[v].born == ct.born and mt.books[v].retired == ct.retired and mt.cover_hops(v) == ct.hops
        assert len(ct.retired) >= 1 or TS[v] < 16
    got = drivers.track_streams(_FakeModel(), lists, MULTI_Q, iters=3, slots=9, return_hops=True, cover=cover)
    for v in range(3):
        ref = drivers.track_cover(_FakeModel(), lists[v], cover, MULTI_Q[v], iters=3, slots=9, return_hops=True)
        for a, b in zip(got[v][:4], ref[:4]):
            assert a.shape == b.shape and torch.equal(_bits(a.float()), _bits(b.float()))
        assert got[v][4] == ref[4]
    with pytest.raises(ValueError):
        mt.add_queries(0, USER)
    with pytest.raises(ValueError):
        mt.remove_queries(0, [0])


def test_cover_none_leaves_the_multi_tracker_as_it_was():
    lists = [_chunks(_video(t, 60 + v), 3) for v, t in enumerate(TS)]
    mt = drivers.MultiStreamTracker(_FakeModel(), [USER[:, :2], USER[:, :2], USER[:, :1]], iters=3, slots=9)
    res = mt.push([c[0] for c in lists])
    assert all(len(r) == 3 for r in res) and mt.books is None
    assert mt.add_queries(0, USER[:, :1]).tolist() == [2] and mt.remove_queries(0, [0]).tolist() == [1, 2]
    assert all(len(r) == 3 for r in mt.finish())


@pytest.mark.parametrize("kw", [dict(cell=7), dict(cell=8.5), dict(cell="32"), dict(cell=True), dict(vis_thr=0.0), dict(vis_thr=1.0),
                                dict(vis_thr=float("nan")), dict(lost_after=0), dict(lost_after=1.5), dict(max_queries=-1),
                                dict(scan="hip"), dict(scan=None)])
def test_cover_rejects_bad_arguments(kw):
    with pytest.raises(ValueError):
        drivers.Cover(**kw)


def test_cover_accepts_its_documented_values():
    c = drivers.Cover()
    assert (c.cell, c.vis_thr, c.lost_after, c.max_queries, c.scan, c.vis_logit) == (32, 0.5, 4, None, "torch", 0.0)
    c = drivers.Cover(cell=8, vis_thr=0.75, lost_after=None, max_queries=0, scan="library")
    assert c.lost_after is None and c.max_queries == 0 and c.grid(45, 70) == (6, 9)
    assert c.vis_logit == float(torch.logit(torch.tensor(0.75, dtype=torch.float32)))


def test_cover_tracker_rejects_bad_arguments_and_stays_as_it_was():
    m = _FakeModel()
    with pytest.raises(ValueError):
        drivers.CoverTracker(m, "cover")
    with pytest.raises(ValueError):
        drivers.CoverTracker(m, _cover(), torch.zeros(1, 3, 2))
    with pytest.raises(ValueError):
        drivers.CoverTracker(m, _cover(), USER, slots=8)
    with pytest.raises(ValueError):
        drivers.CoverTracker(m, _cover(), USER, rounds="hip")
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(m, [USER], cover="cover")
    ct = drivers.CoverTracker(m, _cover(), USER, iters=3, slots=9)
    with pytest.raises(ValueError):
        ct.push(torch.zeros(1, 2, 1, H, W))                               # before the first step: nothing was seeded
    assert ct.st.cache is None and ct.book.size is None and ct.ids.tolist() == list(range(USER.shape[1])) and ct.st.N == USER.shape[1]
    ct.push(VIDEO[:, :9])
    before = (ct.ids.tolist(), list(ct.born), dict(ct.retired), ct.st.N, ct.emitted)
    with pytest.raises(ValueError):
        ct.push(torch.zeros(1, 2, 3, H + 8, W))                           # another frame size
    with pytest.raises(ValueError):
        ct.push(torch.zeros(2, 3, H, W))
    assert before == (ct.ids.tolist(), list(ct.born), dict(ct.retired), ct.st.N, ct.emitted)
    # finish() with a query of the caller beyond the last frame: the stream's own error, the tracker left running
    with pytest.raises(ValueError):
        ct.finish()
    assert not ct.finished
    ct.push(VIDEO[:, 9:30])
    ct.finish()
    with pytest.raises(ValueError):
        ct.push(VIDEO[:, :1])
    with pytest.raises(ValueError):
        ct.finish()


def test_cover_step_is_declared_bound_and_exported():
    from pips_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_cover_step" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)      # the history comment
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_cover_step\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 21
    proto = re.search(r"\bsize_t\s+pips_cover_workspace_bytes\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 3
    assert len(_lib.SIGNATURES["pips_cover_step"][1]) == 21 and _lib.SIGNATURES["pips_cover_step"][0] is ctypes.c_int
    assert _lib.SIGNATURES["pips_cover_step"][1][11] is ctypes.c_float
    assert _lib.SIGNATURES["pips_cover_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_cover_step") and hasattr(raw, "pips_cover_workspace_bytes") and callable(ops.cover_step)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the sizing query is a host function: flag and run per query, one int per cell
    assert lib.pips_cover_workspace_bytes(1000, 33, 41) == 4 * (2 * 1000 + 33 * 41)
    assert lib.pips_cover_workspace_bytes(0, 1, 1) == 4
    assert lib.pips_cover_workspace_bytes(-1, 4, 6) == 0 and lib.pips_cover_workspace_bytes(5, 0, 6) == 0
    assert lib.pips_cover_workspace_bytes(5, 1 << 13, 1 << 12) == 0
