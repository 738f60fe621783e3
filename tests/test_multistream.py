"""CPU: drivers.MultiStreamTracker / track_streams -- V videos fed in chunks through V rings on one flat cache and ONE state -- on
the fake model of tests/test_stream.py extended to V rings: every ring records which logical frame each slot holds, and ``track``
asserts on every read that the frame is still held by the ring of the particle's OWN stream.  Each stream must be what a
``StreamTracker`` given that stream alone returns, bit for bit with the hop lists.  (``rounds="library"`` needs the library's
kernels: tests/test_multistream_gpu.py.)"""
import os
import re

import pytest
import torch

from pips_amd import drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Cache:
    """one ring (``rings`` None: the cache of tests/test_stream.py) or ``rings`` rings of ``slots`` slots on one flat buffer"""

    def __init__(self, slots, rings=None):
        V = 1 if rings is None else rings
        self.B, self.slots, self.rings = 1, slots, rings
        self.m = torch.zeros(V * slots)                                    # per-slot content
        self.frame = torch.full((V * slots,), -1, dtype=torch.long)       # logical frame in each slot
        self.T = 0 if rings is None else V * slots
        self.device = torch.device("cpu")
        self.clip_lengths = None if rings is None else [0] * V
        self.clip_frames = None if rings is None else torch.zeros(V, dtype=torch.int32)
        self.clip_first = None if rings is None else torch.arange(V, dtype=torch.int32) * slots

    def frames(self, clip):
        return torch.full_like(clip, self.T) if self.rings is None else self.clip_frames.long()[clip]

    def read(self, t, clip):
        """content of logical frames t of the streams clip (same shape), already clamped to the streams' own frames"""
        assert bool((t >= 0).all()) and bool((t < self.frames(clip)).all())
        slot = t % self.slots + (0 if self.rings is None else clip * self.slots)
        assert torch.equal(self.frame[slot], t), "a window read a frame that has left its ring (or a neighbour's slot)"
        return self.m[slot]


class _FakeModel:
    """encode / ring_cache / ring_cache_videos / encode_streams / track with the real signatures.  A particle's result depends on
    its start, its window start, its carried features and the frames its window reads in its own stream (row s reads
    clamp(win_start + s, 0, T_v - 1)); features of feat_init=None are the content of the window's first frame.  Only exactly
    rounded float ops, so a particle computes the same bits in any batch."""
    S = 8

    def __init__(self):
        self.max_pass, self.joint_calls = 0, 0

    def ring_cache(self, H, W, slots):
        return _Cache(slots)

    def ring_cache_videos(self, H, W, slots, V):
        return _Cache(slots, rings=V)

    def encode(self, rgbs, frames_per_pass=16, into=None, clip=None):
        assert into is not None and (clip is None) == (into.rings is None)
        m = rgbs.float().mean(dim=(2, 3, 4))[0]
        assert rgbs.shape[1] <= into.slots
        self.max_pass = max(self.max_pass, rgbs.shape[1])
        for f in range(rgbs.shape[1]):
            T = into.T if clip is None else into.clip_lengths[clip]
            s = T % into.slots + (0 if clip is None else clip * into.slots)
            into.m[s], into.frame[s] = m[f], T
            if clip is None:
                into.T += 1
            else:
                into.clip_lengths[clip] += 1
                into.clip_frames[clip] += 1
        return into

    def encode_streams(self, cache, chunks, frames_per_pass=16, joint=False):
        self.joint_calls += int(joint)
        for v, c in chunks:
            self.encode(c, into=cache, clip=v)
        return cache

    def track(self, cache, xys, coords_init=None, feat_init=None, iters=3, win_start=None, return_feat=False, win_dir=None,
              win_clip=None):
        B, N, _ = xys.shape
        assert (win_clip is None) == (cache.rings is None) and win_dir is None
        ws = win_start.long()
        clip = torch.zeros(B, N, dtype=torch.long) if win_clip is None else win_clip.long()
        last = cache.frames(clip) - 1                                                                   # (B,N)
        t = torch.minimum((ws.unsqueeze(1) + torch.arange(8).view(1, 8, 1)).clamp(min=0), last.unsqueeze(1))   # (B,8,N)
        fm = cache.read(t, clip.unsqueeze(1).expand(B, 8, N))
        ff = cache.read(torch.minimum(ws.clamp(min=0), last), clip).unsqueeze(-1).expand(B, N, 128).clone() \
            if feat_init is None else feat_init
        base = xys.reshape(B, 1, N, 2) + 0.01 * fm.unsqueeze(-1) * torch.arange(8).view(1, 8, 1, 1) \
            + 0.001 * ff[:, :, 0].reshape(B, 1, N, 1)
        lock = (torch.arange(8) > 0).float().view(1, 8, 1, 1)                                       # row 0 stays the start
        preds = [base + 0.1 * i * lock for i in range(iters)]
        vis = torch.remainder(base.sum(-1) * 7.3, 8.0) - 4.0                                         # logits of both signs
        out = (preds, [base, base] + preds + [base] * 2, vis)
        return out + ((ff, None) if return_feat else (None,))


def _video(T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, T, 3, 6, 6, generator=g) * 255


def _queries(tq, seed, W=60.0, H=40.0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(len(tq), 2, generator=g) * torch.tensor([W, H])
    return torch.cat([torch.tensor(tq, dtype=torch.float32).view(-1, 1), xy], dim=1).unsqueeze(0)


def _chunks(video, size):
    return [video[:, i:i + size] for i in range(0, video.shape[1], size)]


def _bits(t):
    return t.contiguous().view(torch.int32)


TS = (37, 21, 9)
TQS = ([0, 36, 29, 5, 5, 13], [0, 20, 7, 7], [0, 3, 8])          # first and last frames, late, duplicated
VIDEOS = [_video(T, 40 + v) for v, T in enumerate(TS)]
QUERIES = [_queries(tq, 50 + v) for v, tq in enumerate(TQS)]


def _assert_stream_is_alone(v, got, chunks, slots, iters=3):
    """got = (trajs, vis, hops) of stream v out of the multi tracker against track_stream on that stream alone"""
    ref_t, ref_v, ref_h = drivers.track_stream(_FakeModel(), chunks, QUERIES[v], iters=iters, slots=slots, return_hops=True)
    assert tuple(got[0].shape) == (1, TS[v], len(TQS[v]), 2) and tuple(got[1].shape) == (1, TS[v], len(TQS[v]))
    assert torch.equal(_bits(got[0]), _bits(ref_t)) and torch.equal(_bits(got[1]), _bits(ref_v))
    assert got[2] == ref_h


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7, (7, 3, 1)])
def test_every_stream_is_its_own_stream_tracker(chunk, slots):
    """V = 3 streams of 37 / 21 / 9 frames in equal chunks, or a chunk size per stream: each stream is track_stream on it alone,
    bit for bit (NaN before the query frames included) with the hop lists; the short streams finish while the long one goes on;
    no read of an evicted or of a neighbour's slot (asserted by the fake rings); no pass larger than a ring."""
    sizes = chunk if isinstance(chunk, tuple) else (chunk,) * 3
    lists = [_chunks(v, s) for v, s in zip(VIDEOS, sizes)]
    m = _FakeModel()
    outs = drivers.track_streams(m, lists, QUERIES, iters=3, slots=slots, return_hops=True)
    assert len(outs) == 3 and 1 <= m.max_pass <= slots
    assert any(len(h) > 2 for h in outs[0][2])
    for v in range(3):
        _assert_stream_is_alone(v, outs[v], lists[v], slots)


@pytest.mark.parametrize("slots", [9, 24])
def test_push_with_idle_streams_returns_every_frame_once(slots):
    """pushes in which one or two streams deliver nothing (None), with unequal chunk sizes, one stream finished early while the
    others go on and frames pushed to them afterwards: every frame of every stream comes back exactly once, in order, and the
    concatenation is the stream alone with the chunks it was given."""
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=3, slots=slots, record_hops=True)
    sched = [(5, 4, None), (None, 3, 2), (9, None, 7), (None, None, None), (12, 14, None), (11, None, None)]   # frames per push
    pos, given, parts = [0, 0, 0], [[], [], []], [[], [], []]
    for i, wave in enumerate(sched):
        chunks = []
        for v, k in enumerate(wave):
            c = None if k is None else VIDEOS[v][:, pos[v]:pos[v] + k]
            chunks.append(c)
            if c is not None:
                given[v].append(c)
                pos[v] += k
        for v, p in enumerate(mt.push(chunks)):
            parts[v].append(p)
        if i == 2:                                                # stream 2 has its 9 frames: it ends, the others go on
            assert pos[2] == TS[2]
            parts[2].append(mt.finish(2))
            assert mt.finished == [False, False, True]
    assert pos == list(TS)
    rest = mt.finish()
    assert rest[2] is None
    for v in (0, 1):
        parts[v].append(rest[v])
    for v in range(3):
        nxt = 0
        for f0, tr, vi in parts[v]:
            assert f0 == nxt and tr.shape[1] == vi.shape[1] and tuple(tr.shape[2:]) == (len(TQS[v]), 2)
            nxt += tr.shape[1]
        assert nxt == TS[v] == mt.emitted[v]
        got = (torch.cat([p[1] for p in parts[v]], dim=1), torch.cat([p[2] for p in parts[v]], dim=1), mt.stream_hops(v))
        _assert_stream_is_alone(v, got, given[v], slots)
    assert mt.trajs.shape[0] == slots + 8 and mt.cache.slots == slots and mt.cache.rings == 3


def test_push_returns_what_the_single_tracker_returns_per_call():
    """not only the concatenation: every push() hands stream v the frames its own StreamTracker hands out in that call"""
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=2, slots=12)
    singles = [drivers.StreamTracker(_FakeModel(), q, iters=2, slots=12) for q in QUERIES]
    sizes = (10, 6, 4)
    for i in range(4):
        chunks = [v[:, i * s:(i + 1) * s] for v, s in zip(VIDEOS, sizes)]
        chunks = [c if c.shape[1] > 0 else None for c in chunks]
        got = mt.push(chunks)
        for v, c in enumerate(chunks):
            if c is not None:
                f0, tr, vi = singles[v].push(c)
                assert got[v][0] == f0 and torch.equal(_bits(got[v][1]), _bits(tr)) and torch.equal(_bits(got[v][2]), _bits(vi))
            else:
                assert got[v][1].shape[1] == 0
    for v, g in enumerate(mt.finish()):
        f0, tr, vi = singles[v].finish()
        assert g[0] == f0 and torch.equal(_bits(g[1]), _bits(tr)) and torch.equal(_bits(g[2]), _bits(vi))


@pytest.mark.parametrize("slots", [9, 24])
def test_add_queries_on_the_oldest_frame_not_returned(slots):
    """queries added to ONE stream while all run -- at the oldest frame of that stream not yet returned and at a frame not pushed
    yet: that stream is the stream given all its queries up front, the other streams are untouched"""
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=3, slots=slots, record_hops=True)
    parts = [[], [], []]
    lists = [_chunks(v, 5) for v in VIDEOS]

    def push(i):
        for v, p in enumerate(mt.push([l[i] if i < len(l) else None for l in lists])):
            parts[v].append(p)

    push(0), push(1)
    oldest = mt.emitted[1]
    assert 0 <= oldest <= 10
    late = _queries([oldest, 18], 60)
    assert mt.add_queries(1, late).tolist() == [4, 5] and mt.N == 15
    assert mt.columns(1).tolist() == [6, 7, 8, 9, 13, 14]
    for i in range(2, 8):
        push(i)
    for v, p in enumerate(mt.finish()):
        parts[v].append(p)
    # stream 1: the columns a part lacks are frames before the added queries (NaN in the full stream)
    q1 = torch.cat([QUERIES[1], late], dim=1)
    full_t, full_v = torch.full((1, TS[1], 6, 2), float("nan")), torch.full((1, TS[1], 6), float("nan"))
    for f0, tr, vi in parts[1]:
        full_t[:, f0:f0 + tr.shape[1], :tr.shape[2]] = tr
        full_v[:, f0:f0 + vi.shape[1], :vi.shape[2]] = vi
    ref_t, ref_v, ref_h = drivers.track_stream(_FakeModel(), lists[1], q1, iters=3, slots=slots, return_hops=True)
    assert torch.equal(_bits(full_t), _bits(ref_t)) and torch.equal(_bits(full_v), _bits(ref_v)) and mt.stream_hops(1) == ref_h
    for v in (0, 2):
        got = (torch.cat([p[1] for p in parts[v]], dim=1), torch.cat([p[2] for p in parts[v]], dim=1), mt.stream_hops(v))
        _assert_stream_is_alone(v, got, lists[v], slots)


def test_queries_added_before_the_first_push_and_streams_without_queries():
    qs = [QUERIES[0][:, :0], QUERIES[1][:, :2], QUERIES[2]]
    mt = drivers.MultiStreamTracker(_FakeModel(), qs, iters=2, slots=12)
    assert mt.add_queries(1, QUERIES[1][:, 2:]).tolist() == [2, 3]
    parts = [mt.push([v[:, :6] for v in VIDEOS]), mt.push([VIDEOS[0][:, 6:], VIDEOS[1][:, 6:], VIDEOS[2][:, 6:]]), mt.finish()]
    assert sum(p[0][1].shape[1] for p in parts) == TS[0] and parts[0][0][1].shape[2] == 0      # no query: frames, no column
    for v in (1, 2):
        chunks = [VIDEOS[v][:, :6], VIDEOS[v][:, 6:]]
        ref_t, ref_v = drivers.track_stream(_FakeModel(), chunks, QUERIES[v], iters=2, slots=12)
        assert torch.equal(_bits(torch.cat([p[v][1] for p in parts], dim=1)), _bits(ref_t))
        assert torch.equal(_bits(torch.cat([p[v][2] for p in parts], dim=1)), _bits(ref_v))


def test_errors_leave_the_tracker_usable():
    """bad arguments raise ValueError ahead of any change of state: the streams go on and end as if the calls had not been made"""
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, iters=3, slots=12, record_hops=True)
    lists = [_chunks(v, 6) for v in VIDEOS]
    parts = [[], [], []]

    def push(chunks):
        for v, p in enumerate(mt.push(chunks)):
            parts[v].append(p)

    def snapshot():
        return (mt.N, list(mt.emitted), list(mt.finished), mt.tq_host.clone(), mt.trajs.clone(), mt.cur.clone(),
                [list(h) for h in mt.hops], list(mt.cache.clip_lengths), mt.cache.frame.clone())

    def same(a, b):
        return a[:3] == b[:3] and torch.equal(a[3], b[3]) and torch.equal(_bits(a[4]), _bits(b[4])) and torch.equal(a[5], b[5]) \
            and a[6] == b[6] and a[7] == b[7] and torch.equal(a[8], b[8])

    push([l[0] for l in lists])
    push([l[1] for l in lists])                                   # stream 2 has its 9 frames
    parts[2].append(mt.finish(2))
    assert mt.emitted[0] > 0
    bad_calls = [
        lambda: mt.push([lists[0][2], lists[1][2]]),                              # one chunk per stream
        lambda: mt.push([lists[0][2], torch.zeros(1, 2, 3, 5, 6), None]),       # another frame size (after a valid chunk)
        lambda: mt.push([lists[0][2], torch.zeros(1, 4, 3, 6), None]),          # not (1,k,3,H,W)
        lambda: mt.push([lists[0][2], None, VIDEOS[2][:, :1]]),                  # a finished stream
        lambda: mt.finish(2),                                                     # twice
        lambda: mt.finish(3),
        lambda: mt.add_queries(0, _queries([mt.emitted[0] - 1], 61)),             # returned already
        lambda: mt.add_queries(0, _queries([mt.emitted[0] + 0.5], 61)),
        lambda: mt.add_queries(2, _queries([8], 61)),                             # finished
        lambda: mt.add_queries(5, _queries([8], 61)),
        lambda: mt.add_queries(0, torch.zeros(1, 2, 2)),
    ]
    for call in bad_calls:
        before = snapshot()
        with pytest.raises(ValueError):
            call()
        assert same(before, snapshot())
    for i in range(2, 7):
        push([l[i] if i < len(l) else None for l in lists])
    before = snapshot()
    mt.add_queries(1, _queries([TS[1]], 62))                      # beyond the frames pushed: accepted, an error only at the end
    with pytest.raises(ValueError):
        mt.finish(1)
    with pytest.raises(ValueError):
        mt.finish()
    assert mt.finished == [False, False, True] and mt.emitted == before[1]
    parts[0].append(mt.finish(0))
    got = (torch.cat([p[1] for p in parts[0]], dim=1), torch.cat([p[2] for p in parts[0]], dim=1), mt.stream_hops(0))
    _assert_stream_is_alone(0, got, lists[0], 12)
    got = (torch.cat([p[1] for p in parts[2]], dim=1), torch.cat([p[2] for p in parts[2]], dim=1), mt.stream_hops(2))
    _assert_stream_is_alone(2, got, lists[2], 12)


def test_constructor_checks_and_keywords():
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(_FakeModel(), QUERIES, rounds="bogus")
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(_FakeModel(), QUERIES, slots=8)
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(_FakeModel(), [])
    with pytest.raises(ValueError):
        drivers.MultiStreamTracker(_FakeModel(), [QUERIES[0], torch.zeros(1, 2, 2)])
    with pytest.raises(ValueError):
        drivers.track_streams(_FakeModel(), [[VIDEOS[0]]], QUERIES)
    assert drivers.MultiStreamTracker(_FakeModel(), QUERIES).rounds == "torch"
    mt = drivers.MultiStreamTracker(_FakeModel(), QUERIES, rounds="library", joint_encode=True)
    assert mt.rounds == "library" and mt.joint_encode and mt.V == 3 and mt.N == 13


def test_joint_encode_goes_through_encode_streams():
    """joint_encode=True hands each wave of appends to Pips.encode_streams(joint=True) in one call; on the fake (whose frames do
    not depend on the pass they were encoded in) the outputs stay those of the streams alone"""
    m = _FakeModel()
    lists = [_chunks(v, 7) for v in VIDEOS]
    outs = drivers.track_streams(m, lists, QUERIES, iters=3, slots=9, return_hops=True, joint_encode=True)
    assert m.joint_calls > 0
    for v in range(3):
        _assert_stream_is_alone(v, outs[v], lists[v], 9)


NEW_SYMBOLS = {"pips_track_rings": 32, "pips_mixer_input_build_rings": 20, "pips_pyramid_append_at": 13,
               "pips_stream_workspace_bytes_clips": 3, "pips_stream_select_clips": 15, "pips_stream_round_clips": 33,
               "pips_stream_emit_cols": 11}


def test_new_entry_points_are_declared_bound_and_exported():
    import ctypes
    from pips_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert re.search(r"#define\s+PIPS_STREAM_V_MAX\s+64\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW_SYMBOLS.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        proto = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert proto and len(proto.group(1).split(",")) == nargs, name
        assert hasattr(raw, name), name
    # the _rings forms take the arguments of the _clips forms
    for a, b in (("pips_track_rings", "pips_track_clips"), ("pips_mixer_input_build_rings", "pips_mixer_input_build_clips")):
        assert _lib.SIGNATURES[a] == _lib.SIGNATURES[b]
    for name in ("mixer_input_build_rings", "pyramid_append_at", "stream_select_clips", "stream_round_clips", "stream_emit_cols",
                 "stream_workspace_bytes_clips"):
        assert callable(getattr(ops, name))
    lib = _lib.load()                                          # sizing queries are pure host functions
    assert lib.pips_abi_version() == 3
    assert lib.pips_stream_workspace_bytes_clips(64, 6, 3) == lib.pips_stream_workspace_bytes(64, 6) + 64 * 4
    assert lib.pips_stream_workspace_bytes_clips(64, 6, 64) > 0
    for bad in ((0, 6, 3), (64, -1, 3), (64, 6, 0), (64, 6, 65)):
        assert lib.pips_stream_workspace_bytes_clips(*bad) == 0
    from pips_amd import Pips
    for name in ("ring_cache_videos", "encode_streams"):
        assert callable(getattr(Pips, name))
    assert callable(drivers.track_streams) and drivers.MultiStreamTracker.S == 8
