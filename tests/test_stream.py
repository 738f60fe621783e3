"""CPU: drivers.StreamTracker / track_stream -- a video fed in chunks through a ring of encoded frames -- on a fake model whose
ring cache records which logical frame each slot holds, and whose ``track`` asserts that every frame a window (or the point
sample of a first window) reads is still in the ring.  The stream must be track_queries' forward chains, bit for bit."""
import pytest
import torch

from pips_amd import drivers


class _Cache:
    def __init__(self, m, slots=None):
        self.m = m                                                     # (T or slots,) per-frame content
        self.B, self.T = 1, (m.shape[0] if slots is None else 0)
        self.slots = self.T if slots is None else slots
        self.frame = None if slots is None else torch.full((slots,), -1, dtype=torch.long)   # logical frame in each slot
        self.device = torch.device("cpu")

    def read(self, t):
        """content of logical frames t (any shape, already clamped to [0, T-1])"""
        assert bool((t >= 0).all()) and bool((t < self.T).all())
        if self.frame is None:
            return self.m[t]
        slot = t % self.slots
        assert torch.equal(self.frame[slot], t), "a window read a frame that has left the ring"
        return self.m[slot]


class _FakeModel:
    """encode / ring_cache / track stand-in with the real signatures: a particle's result depends on its start, its window
    start and direction, its carried features and the frames its window reads (row s reads clamp(win_start + dir*s, 0, T-1)).
    Features of feat_init=None are the content of the window's first frame, as the point sample reads it.  Only exactly
    rounded float ops, so a particle computes the same bits in any batch."""
    S = 8

    def __init__(self):
        self.max_pass = 0

    def encode(self, rgbs, frames_per_pass=16, into=None):
        m = rgbs.float().mean(dim=(2, 3, 4))[0]
        if into is None:
            return _Cache(m)
        assert rgbs.shape[1] <= into.slots
        self.max_pass = max(self.max_pass, rgbs.shape[1])
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
    T = video.shape[1]
    size = T if size is None else size
    return [video[:, i:i + size] for i in range(0, T, size)]


T_ = 37
TQ = [0, T_ - 1, 29, 5, 5, 13, 0, T_ - 8, 22]                    # first and last frame, late, duplicated


@pytest.mark.parametrize("slots", [9, 12, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7, 16, None])
def test_stream_is_forward_queries(chunk, slots):
    """(a) frames t >= t_q: track_queries' forward chain bit for bit (positions and visibility), the same hop sequence; frames
    before t_q are NaN; no read of an evicted slot (asserted by the fake ring); the ring never takes more than `slots` frames
    per pass."""
    m = _FakeModel()
    video = _video(T_, 1)
    q = _queries(TQ, 2)
    trajs, vis, hops = drivers.track_stream(m, _chunks(video, chunk), q, iters=3, slots=slots, return_hops=True)
    ref_t, ref_v, (ref_fh, _) = drivers.track_queries(m, video, q, iters=3, return_hops=True)
    assert tuple(trajs.shape) == (1, T_, len(TQ), 2) and tuple(vis.shape) == (1, T_, len(TQ))
    assert any(len(h) > 2 for h in hops)
    for n, tq in enumerate(TQ):
        assert torch.equal(trajs[:, tq:, n], ref_t[:, tq:, n]) and torch.equal(vis[:, tq:, n], ref_v[:, tq:, n])
        assert bool(trajs[:, :tq, n].isnan().all()) and bool(vis[:, :tq, n].isnan().all())
        assert hops[n] == ref_fh[n]
    assert 1 <= m.max_pass <= slots


def test_stream_from_frame_zero_is_track_chained():
    """(b) one chunk, all queries at t = 0: track_chained, hops included."""
    m = _FakeModel()
    video = _video(21, 3)
    q = _queries([0] * 6, 4)
    trajs, _, hops = drivers.track_stream(m, [video], q, iters=2, slots=30, return_hops=True)
    ref, ref_h = drivers.track_chained(m, video, q[:, :, 1:], iters=2, return_hops=True)
    assert torch.equal(trajs, ref) and hops == ref_h


@pytest.mark.parametrize("chunk,slots", [(1, 9), (5, 12), (16, 24), (40, 9)])
def test_push_finish_outputs_are_the_stream(chunk, slots):
    """(c) push() / finish() hand out every frame exactly once, in order, and their concatenation is track_stream; device state
    is (slots + 8) output rows and a ring of `slots` frames whatever the video length."""
    m = _FakeModel()
    T = 45
    video = _video(T, 5)
    q = _queries([3, 0, 40, 17, 17], 6)
    st = drivers.StreamTracker(m, q, iters=2, slots=slots)
    parts = [st.push(c) for c in _chunks(video, chunk)] + [st.finish()]
    nxt = 0
    for f0, tr, vi in parts:
        assert f0 == nxt and tr.shape[1] == vi.shape[1] and tuple(tr.shape[2:]) == (5, 2)
        nxt += tr.shape[1]
    assert nxt == T
    ref_t, ref_v = drivers.track_stream(m, _chunks(video, chunk), q, iters=2, slots=slots)
    got_t = torch.cat([p[1] for p in parts], dim=1)
    got_v = torch.cat([p[2] for p in parts], dim=1)
    assert torch.equal(got_t.nan_to_num(-1.0), ref_t.nan_to_num(-1.0)) and torch.equal(got_v.nan_to_num(-1.0), ref_v.nan_to_num(-1.0))
    assert st.trajs.shape[0] == slots + 8 and st.vis.shape[0] == slots + 8 and st.cache.slots == slots


def test_frames_become_final_while_streaming():
    """(d) trajectories come back before the end of the video: with queries at frame 0, a push of 16 frames after the first
    ones already returns frames."""
    m = _FakeModel()
    video = _video(64, 7)
    st = drivers.StreamTracker(m, _queries([0, 0, 0], 8), iters=2, slots=24)
    emitted = [st.push(c)[1].shape[1] for c in _chunks(video, 16)]
    assert sum(emitted[:-1]) > 0 and sum(emitted) < 64
    assert sum(emitted) + st.finish()[1].shape[1] == 64


@pytest.mark.parametrize("slots", [8, 1, 0])
def test_stream_rejects_small_rings(slots):
    with pytest.raises(ValueError):
        drivers.StreamTracker(_FakeModel(), _queries([0], 9), slots=slots)


@pytest.mark.parametrize("t", [-1, 2.5, float("nan"), float("inf")])
def test_stream_rejects_bad_query_frames(t):
    q = _queries([0, 3], 10)
    q[0, 1, 0] = t
    with pytest.raises(ValueError):
        drivers.StreamTracker(_FakeModel(), q)


def test_stream_rejects_query_beyond_the_video():
    """a query frame the video never reached is an error at finish(); a frame beyond the pushed ones is not an error before"""
    st = drivers.StreamTracker(_FakeModel(), _queries([0, 12], 11), iters=2, slots=12)
    st.push(_video(10, 12))
    with pytest.raises(ValueError):
        st.finish()
    with pytest.raises(ValueError):
        drivers.track_stream(_FakeModel(), [_video(12, 13)], _queries([0, 12], 14), iters=2)


def test_stream_rejects_bad_frames_and_use_after_finish():
    st = drivers.StreamTracker(_FakeModel(), _queries([0], 15), iters=2, slots=12)
    with pytest.raises(ValueError):
        st.push(torch.zeros(1, 4, 3, 6))
    st.push(_video(9, 16))
    with pytest.raises(ValueError):
        st.push(torch.zeros(1, 2, 3, 5, 6))
    st.finish()
    with pytest.raises(ValueError):
        st.push(_video(2, 17))
