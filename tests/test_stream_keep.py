"""CPU: ``StreamTracker.remove_queries`` / ``MultiStreamTracker.remove_queries`` under ``rounds="torch"`` on the fake model and the
fake rings of tests/test_multistream.py (every read is asserted to land on a frame its ring still holds), and the presence of
pips_stream_keep in the header and the binding table.  The definition: a stream given queries Q that has the subset D removed
after some push returns, for every frame and in the kept columns, the bits -- hop lists included -- of a stream given Q minus D
from the start.  (``rounds="library"`` needs the library's kernels: tests/test_stream_keep_gpu.py.)"""
import os
import re

import pytest
import torch

from pips_amd import drivers
from test_multistream import _FakeModel, _bits, _chunks, _queries, _video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_ = 29
TQ = [0, 0, 3, 8, 8, 11, 16, 16, 20, 20, 25, 28]
DROP = [1, 4, 5, 9]                                  # column 9 (frame 20) is still waiting for its frame after 12 frames
KEPT = [c for c in range(len(TQ)) if c not in DROP]
VIDEO = _video(T_, 70)
Q = _queries(TQ, 71)


class _Log:
    """the parts a tracker returned, with the identity of the column behind each output column at that call"""

    def __init__(self, st, ids):
        self.st, self.ids, self.parts, self.next = st, list(ids), [], 0

    def take(self, part):
        f0, tr, vi = part
        assert f0 == self.next and tr.shape[1] == vi.shape[1], "every frame once, in order"
        assert tuple(tr.shape[2:]) == (len(self.ids), 2) and vi.shape[2] == len(self.ids)
        self.next += tr.shape[1]
        self.parts.append((f0, tr, vi, list(self.ids)))

    def push(self, video, chunk):
        for c in _chunks(video, chunk):
            self.take(self.st.push(c))

    def remove(self, cols):
        keep = self.st.remove_queries(cols)
        assert keep.dtype == torch.int64 and keep.device.type == "cpu"
        assert keep.tolist() == [k for k in range(len(self.ids)) if k not in list(cols)]
        self.ids = [self.ids[k] for k in keep.tolist()]
        assert self.st.N == len(self.ids) == self.st.tq_host.numel() == self.st.xy_in.shape[0]
        assert self.st.hops is None or len(self.st.hops) == self.st.N
        return keep

    def add(self, q, ids):
        got = self.st.add_queries(q)
        assert got.tolist() == list(range(len(self.ids), len(self.ids) + len(ids))), "new columns go behind the kept ones"
        self.ids += list(ids)

    def full(self, T, n):
        """(T,n,2) / (T,n) by identity, NaN where a frame was not returned for that identity, and the mask of what was"""
        tr, vi, seen = torch.full((1, T, n, 2), float("nan")), torch.full((1, T, n), float("nan")), torch.zeros(T, n, dtype=torch.bool)
        for f0, t, v, ids in self.parts:
            tr[:, f0:f0 + t.shape[1], ids], vi[:, f0:f0 + v.shape[1], ids] = t, v
            seen[f0:f0 + t.shape[1], ids] = True
        return tr, vi, seen


def _up_front(q, pushes, slots, iters=3):
    """the stream given the queries q from the start, fed the chunks ``pushes``"""
    return drivers.track_stream(_FakeModel(), pushes, q, iters=iters, slots=slots, return_hops=True)


@pytest.mark.parametrize("chunk,slots", [(1, 24), (3, 24), (7, 24), (1, 9)])
def test_kept_columns_are_the_stream_given_them_up_front(chunk, slots):
    """T = 29, twelve queries, columns {1, 4, 5, 9} removed once 12 frames were pushed: the kept columns are, bit for bit with the
    hop lists, the stream given the other eight from the start -- the frames returned before the removal and the ones the
    removed queries held back alike; the frames of the removed columns returned before the removal are those of the stream
    given all twelve; no window of a later round reads a frame that left the ring (asserted by the fake ring).  chunk = 1 at
    slots = 9 and chunks of at most 16 at slots = 24 are never split, so both streams encode every frame in the same pass."""
    st = drivers.StreamTracker(_FakeModel(), Q, iters=3, slots=slots, record_hops=True)
    log = _Log(st, range(12))
    log.push(VIDEO[:, :12], chunk)
    emitted = st.emitted
    keep = log.remove(DROP)
    assert keep.tolist() == KEPT and st.trajs.shape == (slots + 8, 8, 2) and st.vis.shape == (slots + 8, 8)
    assert st.cur.shape[0] == 8 and st.tq_host.tolist() == [TQ[k] for k in KEPT]
    log.push(VIDEO[:, 12:], chunk)
    log.take(st.finish())
    assert log.next == T_
    tr, vi, seen = log.full(T_, 12)
    assert bool(seen[:, KEPT].all()) and bool((seen[:, DROP].sum(0) == emitted).all())
    pushes = _chunks(VIDEO[:, :12], chunk) + _chunks(VIDEO[:, 12:], chunk)
    ref_t, ref_v, ref_h = _up_front(Q[:, KEPT], pushes, slots)
    assert torch.equal(_bits(tr[:, :, KEPT]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, KEPT]), _bits(ref_v))
    assert st.hops == ref_h and any(len(h) > 2 for h in st.hops)
    all_t, all_v, _ = _up_front(Q, pushes, slots)
    assert torch.equal(_bits(tr[:, :emitted, DROP]), _bits(all_t[:, :emitted, DROP]))
    assert torch.equal(_bits(vi[:, :emitted, DROP]), _bits(all_v[:, :emitted, DROP]))


@pytest.mark.parametrize("engine", drivers.ENGINES)
def test_removing_before_the_first_push_under_either_engine(engine):
    """removing before the first push only shrinks the host lists (there is no device state yet), under either engine value"""
    st = drivers.StreamTracker(_FakeModel(), Q, iters=2, slots=12, engine=engine)
    assert st.remove_queries(torch.tensor(DROP)).tolist() == KEPT and st.N == 8 and st.cache is None


def test_removal_then_add_queries_puts_new_columns_behind_the_kept_ones():
    """columns {1, 4, 5, 9} removed after 12 frames, then two queries added (the oldest frame not returned yet, and frame 22): they
    take columns 8 and 9, and all ten columns equal the stream given the eight kept and the two new queries up front"""
    st = drivers.StreamTracker(_FakeModel(), Q, iters=3, slots=24, record_hops=True)
    log = _Log(st, range(12))
    log.push(VIDEO[:, :12], 3)
    log.remove(DROP)
    late = _queries([st.emitted, 22], 72)
    log.add(late, [12, 13])
    log.push(VIDEO[:, 12:], 3)
    log.take(st.finish())
    tr, vi, seen = log.full(T_, 14)
    ids = KEPT + [12, 13]
    tq = [TQ[k] for k in KEPT] + late[0, :, 0].long().tolist()
    for c, t in zip(ids, tq):                                   # a column added later lacks only frames before its query
        assert bool(seen[t:, c].all())
    ref_t, ref_v, ref_h = _up_front(torch.cat([Q[:, KEPT], late], dim=1), _chunks(VIDEO[:, :12], 3) + _chunks(VIDEO[:, 12:], 3), 24)
    assert torch.equal(_bits(tr[:, :, ids]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, ids]), _bits(ref_v))
    assert st.hops == ref_h


def test_removing_every_query_then_pushing_on_then_adding_one():
    """a tracker whose queries are all removed keeps running as one constructed with none: frames come back with no column, and a
    query added afterwards is the stream given that query alone"""
    st = drivers.StreamTracker(_FakeModel(), Q[:, :3], iters=3, slots=12, record_hops=True)
    log = _Log(st, range(3))
    log.push(VIDEO[:, :10], 5)
    assert log.remove([0, 1, 2]).numel() == 0 and st.N == 0 and st.hops == [] and st.trajs.shape == (20, 0, 2)
    assert st.remove_queries([]).tolist() == []
    log.push(VIDEO[:, 10:15], 5)
    assert st.emitted == 15 and log.parts[-1][1].shape == (1, 15 - log.parts[-1][0], 0, 2)
    one = _queries([st.emitted + 1], 73)
    log.add(one, [3])
    log.push(VIDEO[:, 15:], 5)
    log.take(st.finish())
    tr, vi, _ = log.full(T_, 4)
    ref_t, ref_v, ref_h = _up_front(one, _chunks(VIDEO, 5), 12)
    assert torch.equal(_bits(tr[:, :, 3:]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, 3:]), _bits(ref_v)) and st.hops == ref_h


def test_removing_before_the_first_push():
    st = drivers.StreamTracker(_FakeModel(), Q, iters=3, slots=12, record_hops=True)
    log = _Log(st, range(12))
    assert log.remove([]).tolist() == list(range(12))
    log.remove(DROP)
    assert st.cache is None
    log.push(VIDEO, 7)
    log.take(st.finish())
    tr, vi, seen = log.full(T_, 12)
    assert not bool(seen[:, DROP].any())
    ref_t, ref_v, ref_h = _up_front(Q[:, KEPT], _chunks(VIDEO, 7), 12)
    assert torch.equal(_bits(tr[:, :, KEPT]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, KEPT]), _bits(ref_v)) and st.hops == ref_h


def test_removing_a_query_on_a_frame_that_never_comes_lets_finish_succeed():
    q = torch.cat([Q[:, :4], _queries([T_ + 5], 74)], dim=1)
    st = drivers.StreamTracker(_FakeModel(), q, iters=3, slots=12, record_hops=True)
    log = _Log(st, range(5))
    log.push(VIDEO, 7)
    with pytest.raises(ValueError):
        st.finish()
    assert not st.finished
    assert log.remove([4]).tolist() == [0, 1, 2, 3]
    log.take(st.finish())
    assert log.next == T_
    tr, vi, _ = log.full(T_, 5)
    ref_t, ref_v, ref_h = _up_front(Q[:, :4], _chunks(VIDEO, 7), 12)
    assert torch.equal(_bits(tr[:, :, :4]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, :4]), _bits(ref_v)) and st.hops == ref_h


def test_bad_columns_raise_and_leave_the_tracker_as_its_untouched_twin():
    st, twin = (drivers.StreamTracker(_FakeModel(), Q, iters=3, slots=12, record_hops=True) for _ in range(2))
    for bad in ([12], [-1], [0, 0], [3, 11, 3], torch.tensor([0, 12]), [1.5]):
        with pytest.raises(ValueError):
            st.remove_queries(bad)
    a, b = st.push(VIDEO[:, :12]), twin.push(VIDEO[:, :12])
    assert a[0] == b[0] and torch.equal(_bits(a[1]), _bits(b[1]))
    for bad in ([12], [-1], [0, 0], [3, 11, 3], torch.tensor([0, 12]), [1.5]):
        before = (st.N, st.emitted, st.tq_host.clone(), st.xy_in.clone(), st.trajs.clone(), st.cur.clone(), [list(h) for h in st.hops])
        with pytest.raises(ValueError):
            st.remove_queries(bad)
        assert (st.N, st.emitted) == before[:2] and torch.equal(st.tq_host, before[2]) and torch.equal(st.xy_in, before[3])
        assert torch.equal(_bits(st.trajs), _bits(before[4])) and torch.equal(st.cur, before[5]) and st.hops == before[6]
    for x, y in ((st.push(VIDEO[:, 12:]), twin.push(VIDEO[:, 12:])), (st.finish(), twin.finish())):
        assert x[0] == y[0] and torch.equal(_bits(x[1]), _bits(y[1])) and torch.equal(_bits(x[2]), _bits(y[2]))
    assert st.hops == twin.hops
    with pytest.raises(ValueError):
        st.remove_queries([0])                                   # after finish()
    assert st.N == 12


# ---------------------------------------------------------------------------------------------- several streams
TS = (37, 21, 9)
TQS = ([0, 36, 29, 5, 5, 13], [0, 20, 7, 7], [0, 3, 8])
VIDEOS = [_video(T, 80 + v) for v, T in enumerate(TS)]
QUERIES = [_queries(tq, 90 + v) for v, tq in enumerate(TQS)]


@pytest.mark.parametrize("slots", [9, 24])
def test_every_stream_of_several_is_its_own_tracker_with_the_same_removals(slots):
    """three streams of 37 / 21 / 9 frames in chunks of 6 / 4 / 3: position 1 of stream 2 removed after the first wave, positions 1
    (a query waiting for frame 36) and 4 of stream 0 after the second, stream 2 finished after the third while the others go on --
    every call hands each stream what its own StreamTracker with the same removals hands out, bit for bit, hop lists included;
    stream 1 never notices"""
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=3, slots=slots, record_hops=True)
    singles = [drivers.StreamTracker(_FakeModel(), q, iters=3, slots=slots, record_hops=True) for q in QUERIES]
    sizes = (6, 4, 3)

    def same(got, want):
        assert got[0] == want[0] and torch.equal(_bits(got[1]), _bits(want[1])) and torch.equal(_bits(got[2]), _bits(want[2]))

    for i in range(7):
        chunks = [v[:, i * s:(i + 1) * s] for v, s in zip(VIDEOS, sizes)]
        chunks = [c if c.shape[1] > 0 and not mt.finished[v] else None for v, c in enumerate(chunks)]
        got = mt.push(chunks)
        for v, c in enumerate(chunks):
            if c is not None:
                same(got[v], singles[v].push(c))
        if i == 0:
            assert mt.remove_queries(2, [1]).tolist() == singles[2].remove_queries([1]).tolist() == [0, 2]
            assert mt.columns(2).tolist() == [10, 11] and mt.N == 12 and mt.clip_host.tolist() == [0] * 6 + [1] * 4 + [2] * 2
        if i == 1:
            assert mt.remove_queries(0, torch.tensor([4, 1])).tolist() == singles[0].remove_queries([1, 4]).tolist() == [0, 2, 3, 5]
            assert mt.columns(0).tolist() == [0, 1, 2, 3] and mt.columns(1).tolist() == [4, 5, 6, 7] and mt.N == 10
            assert mt.trajs.shape == (slots + 8, 10, 2) and mt.cur.shape[0] == 10 and len(mt.hops) == 10
            assert mt.add_queries(0, _queries([30], 95)).tolist() == singles[0].add_queries(_queries([30], 95)).tolist() == [4]
        if i == 2:
            same(mt.finish(2), singles[2].finish())
            with pytest.raises(ValueError):
                mt.remove_queries(2, [0])                        # a finished stream
    for bad in (lambda: mt.remove_queries(3, [0]), lambda: mt.remove_queries(0, [5]), lambda: mt.remove_queries(1, [0, 0]),
                lambda: mt.remove_queries(1, [-1])):
        n, cur = mt.N, mt.cur.clone()
        with pytest.raises(ValueError):
            bad()
        assert mt.N == n and torch.equal(mt.cur, cur)
    rest = mt.finish()
    assert rest[2] is None
    for v in (0, 1):
        same(rest[v], singles[v].finish())
    for v in range(3):
        assert mt.emitted[v] == TS[v] and mt.stream_hops(v) == singles[v].hops
    assert any(len(h) > 2 for h in mt.stream_hops(0))


def test_multi_removal_before_the_first_push():
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=2, slots=12)
    assert mt.remove_queries(1, [0, 3]).tolist() == [1, 2] and mt.cache is None and mt.N == 11
    outs = [mt.push([v[:, :9] for v in VIDEOS]), mt.push([VIDEOS[0][:, 9:], VIDEOS[1][:, 9:], None]), mt.finish()]
    ref_t, ref_v = drivers.track_stream(_FakeModel(), [VIDEOS[1][:, :9], VIDEOS[1][:, 9:]], QUERIES[1][:, 1:3], iters=2, slots=12)
    assert torch.equal(_bits(torch.cat([o[1][1] for o in outs], dim=1)), _bits(ref_t))
    assert torch.equal(_bits(torch.cat([o[1][2] for o in outs], dim=1)), _bits(ref_v))


# ---------------------------------------------------------------------------------------------- plumbing
def test_stream_keep_is_declared_bound_and_exported():
    import ctypes
    from pips_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert "pips_stream_keep" in re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)      # the history comment
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_stream_keep\s*\(([^)]*)\)\s*;", hdr)
    assert proto and len(proto.group(1).split(",")) == 23
    assert len(_lib.SIGNATURES["pips_stream_keep"][1]) == 23 and _lib.SIGNATURES["pips_stream_keep"][0] is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pips_stream_keep") and callable(ops.stream_keep)
    assert _lib.load().pips_abi_version() == 3
    for cls in (drivers._TorchRounds, drivers._LibraryRounds):
        assert callable(cls.keep)
