"""CPU: ``StreamTracker.add_queries`` and the ``rounds`` keyword of drivers.StreamTracker / track_stream on a fake model (the kind
tests/test_stream.py builds: a ring cache that records which logical frame each slot holds and a ``track`` that asserts every
frame it reads is still held), and the presence of the pips_stream_* entry points in the header and the binding table."""
import os
import re

import pytest
import torch

from pips_amd import drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Cache:
    def __init__(self, m, slots=None):
        self.m = m                                                     # (T or slots,) per-frame content
        self.B, self.T = 1, (m.shape[0] if slots is None else 0)
        self.slots = self.T if slots is None else slots
        self.frame = None if slots is None else torch.full((slots,), -1, dtype=torch.long)   # logical frame in each slot
        self.device = torch.device("cpu")

    def read(self, t):
        assert bool((t >= 0).all()) and bool((t < self.T).all())
        if self.frame is None:
            return self.m[t]
        slot = t % self.slots
        assert torch.equal(self.frame[slot], t), "a window read a frame that has left the ring"
        return self.m[slot]


class _FakeModel:
    """encode / ring_cache / track with the real signatures.  A particle's result depends on its start, its window start, its
    carried features and the frames its window reads; features of feat_init=None are the content of the window's first frame.
    Only exactly rounded float ops, so a particle computes the same bits in any batch."""
    S = 8

    def encode(self, rgbs, frames_per_pass=16, into=None):
        m = rgbs.float().mean(dim=(2, 3, 4))[0]
        if into is None:
            return _Cache(m)
        assert rgbs.shape[1] <= into.slots
        for f in range(rgbs.shape[1]):
            s = into.T % into.slots
            into.m[s], into.frame[s] = m[f], into.T
            into.T += 1
        return into

    def ring_cache(self, H, W, slots):
        return _Cache(torch.zeros(slots), slots=slots)

    def track(self, cache, xys, coords_init=None, feat_init=None, iters=3, win_start=None, return_feat=False, win_dir=None):
        B, N, _ = xys.shape
        ws = torch.zeros(B, N, dtype=torch.long) if win_start is None else win_start.long()
        d = torch.ones(B, N, dtype=torch.long) if win_dir is None else torch.where(win_dir < 0, -1, 1).long()
        t = (ws.unsqueeze(1) + d.unsqueeze(1) * torch.arange(8).view(1, 8, 1)).clamp(0, cache.T - 1)   # (B,8,N)
        fm = cache.read(t)
        ff = cache.read(ws.clamp(0, cache.T - 1)).unsqueeze(-1).expand(B, N, 128).clone() if feat_init is None else feat_init
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


T_ = 29


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_added_queries_are_the_stream_given_them_up_front(chunk, slots):
    """Queries at frames 0 and 5 at construction, 9 and 20 added once 8 frames were pushed, and -- once 16 were -- one at a frame
    not pushed yet (25) and one at the oldest frame not returned yet (pushed and still in the ring): the outputs are those of a
    stream given all six up front, bit for bit with the hop lists, and track_queries' forward frames; every frame comes back
    exactly once, with the columns of the queries known at that call."""
    m = _FakeModel()
    video = _video(T_, 21)
    st = drivers.StreamTracker(m, _queries([0, 5], 22), iters=3, slots=slots, record_hops=True)
    parts = [st.push(c) for c in _chunks(video[:, :8], chunk)]
    early = _queries([9, 20], 23)
    assert st.add_queries(early).tolist() == [2, 3]
    parts += [st.push(c) for c in _chunks(video[:, 8:16], chunk)]
    oldest = st.emitted
    assert 0 <= oldest <= 16
    late = _queries([25, oldest], 24)
    assert st.add_queries(late).tolist() == [4, 5] and st.N == 6
    parts += [st.push(c) for c in _chunks(video[:, 16:], chunk)] + [st.finish()]
    # every frame once, in order; the columns of a part are the queries known when it was returned
    nxt, widths = 0, []
    for f0, tr, vi in parts:
        assert f0 == nxt and tr.shape[1] == vi.shape[1] and tr.shape[2] == vi.shape[2]
        nxt += tr.shape[1]
        widths.append(tr.shape[2])
    assert nxt == T_ and widths == sorted(widths) and widths[0] == 2 and widths[-1] == 6
    # the columns a part lacks are frames before the query (NaN in the full stream)
    full_t = torch.full((1, T_, 6, 2), float("nan"))
    full_v = torch.full((1, T_, 6), float("nan"))
    for f0, tr, vi in parts:
        full_t[:, f0:f0 + tr.shape[1], :tr.shape[2]] = tr
        full_v[:, f0:f0 + vi.shape[1], :vi.shape[2]] = vi
    q = torch.cat([_queries([0, 5], 22), early, late], dim=1)
    tq = q[0, :, 0].long().tolist()
    ref_t, ref_v, ref_h = drivers.track_stream(_FakeModel(), _chunks(video, chunk), q, iters=3, slots=slots, return_hops=True)
    assert torch.equal(_bits(full_t), _bits(ref_t)) and torch.equal(_bits(full_v), _bits(ref_v))
    assert st.hops == ref_h and any(len(h) > 2 for h in st.hops)
    qt, qv, (qh, _) = drivers.track_queries(_FakeModel(), video, q, iters=3, return_hops=True)
    for n, t in enumerate(tq):
        assert torch.equal(full_t[:, t:, n], qt[:, t:, n]) and torch.equal(full_v[:, t:, n], qv[:, t:, n])
        assert bool(full_t[:, :t, n].isnan().all()) and bool(full_v[:, :t, n].isnan().all())
        assert st.hops[n] == qh[n]


def test_add_queries_before_the_first_push_and_of_none():
    """queries added before any frame arrived are queries given at construction; an empty set adds no column"""
    m = _FakeModel()
    video = _video(T_, 25)
    q = _queries([0, 5, 9], 26)
    st = drivers.StreamTracker(m, q[:, :1], iters=2, slots=12)
    assert st.add_queries(q[:, 1:]).tolist() == [1, 2]
    parts = [st.push(video[:, :10])]
    assert st.add_queries(q[:, :0]).tolist() == [] and st.N == 3
    parts += [st.push(video[:, 10:]), st.finish()]
    ref_t, ref_v = drivers.track_stream(_FakeModel(), [video[:, :10], video[:, 10:]], q, iters=2, slots=12)
    assert torch.equal(_bits(torch.cat([p[1] for p in parts], dim=1)), _bits(ref_t))
    assert torch.equal(_bits(torch.cat([p[2] for p in parts], dim=1)), _bits(ref_v))


def test_add_queries_rejects_bad_frames_and_leaves_the_tracker_usable():
    """a frame already returned, a non-integer frame, a call after finish(): ValueError and no change of state -- the stream
    goes on and ends as if the call had not been made"""
    m = _FakeModel()
    video = _video(T_, 27)
    q = _queries([0, 0], 28)
    st = drivers.StreamTracker(m, q, iters=2, slots=12, record_hops=True)
    parts = [st.push(video[:, :20])]
    assert st.emitted > 0
    for bad in ([st.emitted - 1], [25, 0], [st.emitted + 0.5], [float("nan")], [-1]):
        before = (st.N, st.emitted, st.tq_host.clone(), st.trajs.clone(), st.cur.clone(), [list(h) for h in st.hops])
        with pytest.raises(ValueError):
            st.add_queries(_queries(bad, 29))
        assert (st.N, st.emitted) == before[:2] and torch.equal(st.tq_host, before[2]) and st.hops == before[5]
        assert torch.equal(_bits(st.trajs), _bits(before[3])) and torch.equal(st.cur, before[4])
    with pytest.raises(ValueError):
        st.add_queries(torch.zeros(1, 2, 2))                     # not (1,m,3)
    assert st.add_queries(_queries([st.emitted], 30)).tolist() == [2]        # the oldest frame not returned yet is accepted
    parts += [st.push(video[:, 20:]), st.finish()]
    assert sum(p[1].shape[1] for p in parts) == T_
    with pytest.raises(ValueError):
        st.add_queries(_queries([T_ - 1], 31))
    assert st.N == 3


def test_unknown_rounds_value_raises():
    q = _queries([0], 32)
    for rounds in ("bogus", None, "native"):
        with pytest.raises(ValueError):
            drivers.StreamTracker(_FakeModel(), q, rounds=rounds)
    with pytest.raises(ValueError):
        drivers.track_stream(_FakeModel(), [_video(9, 33)], q, rounds="bogus")
    assert drivers.StreamTracker(_FakeModel(), q).rounds == "torch"
    assert drivers.StreamTracker(_FakeModel(), q, rounds="library").rounds == "library"


def test_stream_entry_points_are_declared_and_bound():
    from pips_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pips_stream_workspace_bytes", "pips_stream_select", "pips_stream_round", "pips_stream_emit"):
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(_lib.SIGNATURES["pips_stream_round"][1]) == 29 and len(_lib.SIGNATURES["pips_stream_select"][1]) == 13
    lib = _lib.load()                                          # sizing queries are pure host functions
    assert lib.pips_stream_workspace_bytes(64, 6) > lib.pips_chain_workspace_bytes(64, 6) > 0
    assert lib.pips_stream_workspace_bytes(0, 6) == 0 and lib.pips_stream_workspace_bytes(64, -1) == 0
