"""CPU: drivers.track_chained_batch / track_queries_batch -- several videos of different lengths chained in one set of hop
launches on one flat cache -- on a fake model whose ``track`` asserts that every frame a window (or the point sample of a
first window) reads lies inside the particle's own video.  Each video must get what its single-video driver returns on the
same fake: trajectories, visibilities and hop logs, bit for bit."""
import pytest
import torch

from pips_amd import drivers

LENGTHS = (13, 9, 21)


class _Cache:
    def __init__(self, m, lengths=None):
        self.m = m                                                     # (T,) per-frame content, the videos one after the other
        self.B, self.T = 1, m.shape[0]
        self.slots = self.T
        self.clip_lengths = None if lengths is None else list(lengths)
        self.clip_frames = None if lengths is None else torch.tensor(lengths)
        self.clip_first = None if lengths is None else torch.cumsum(self.clip_frames, 0) - self.clip_frames
        self.device = torch.device("cpu")


class _FakeModel:
    """tests/test_stream.py's stand-in plus ``encode_videos`` and ``track(..., win_clip=)``: a particle's result depends on
    its start, its window start and direction, its carried features and the content of the frames its window reads, row s =
    frame clamp(win_start + dir*s, 0, T_v - 1) of ITS video.  Only exactly rounded float ops: the same bits in any batch."""
    S = 8

    def __init__(self):
        self.track_calls = 0

    def encode(self, rgbs, frames_per_pass=16, into=None):
        assert into is None
        return _Cache(rgbs.float().mean(dim=(2, 3, 4))[0])

    def encode_videos(self, videos, frames_per_pass=16):
        return _Cache(torch.cat([v.float().mean(dim=(2, 3, 4))[0] for v in videos]), [v.shape[1] for v in videos])

    def track(self, cache, xys, coords_init=None, feat_init=None, iters=3, win_start=None, return_feat=False, win_dir=None,
              win_clip=None):
        self.track_calls += 1
        B, N, _ = xys.shape
        ws = torch.zeros(B, N, dtype=torch.long) if win_start is None else win_start.long()
        d = torch.ones(B, N, dtype=torch.long) if win_dir is None else torch.where(win_dir < 0, -1, 1).long()
        if win_clip is None:
            assert cache.clip_first is None, "a cache of several videos is read through win_clip"
            first, frames = torch.zeros(B, N, dtype=torch.long), torch.full((B, N), cache.T)
        else:
            assert B == 1 and win_start is not None
            v = win_clip.long()
            assert bool((v >= 0).all()) and bool((v < len(cache.clip_lengths)).all())
            first, frames = cache.clip_first[v], cache.clip_frames[v]
        own = (ws.unsqueeze(1) + d.unsqueeze(1) * torch.arange(8).view(1, 8, 1)).clamp(min=0)
        own = torch.minimum(own, (frames - 1).unsqueeze(1))                                        # (B,8,N) frames of the own video
        t = first.unsqueeze(1) + own
        # every frame read lies inside the particle's own video
        assert bool((t >= first.unsqueeze(1)).all()) and bool((t < (first + frames).unsqueeze(1)).all())
        assert bool((ws >= 0).all()) and bool((ws < frames).all()), "a window starts outside its own video"
        fm = cache.m[t]
        ff = cache.m[first + ws].unsqueeze(-1).expand(B, N, 128).clone() if feat_init is None else feat_init
        base = xys.reshape(B, 1, N, 2) + 0.01 * fm.unsqueeze(-1) * torch.arange(8).view(1, 8, 1, 1) \
            + 0.001 * ff[:, :, 0].reshape(B, 1, N, 1)
        lock = (torch.arange(8) > 0).float().view(1, 8, 1, 1)                                       # row 0 stays the start
        preds = [base + 0.1 * i * lock for i in range(iters)]
        vis = torch.remainder(base.sum(-1) * 7.3, 8.0) - 4.0                                         # logits of both signs
        out = (preds, [base, base] + preds + [base] * 2, vis)
        return out + ((ff, None) if return_feat else (None,))


def _video(T, seed, size=6):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, T, 3, size, size, generator=g) * 255


def _points(n, seed, W=60.0, H=40.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 2, generator=g) * torch.tensor([W, H])).unsqueeze(0)


def _queries(tq, seed):
    return torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), _points(len(tq), seed)], dim=-1)


VIDEOS = [_video(T, 10 + i) for i, T in enumerate(LENGTHS)]
XY0S = [_points(n, 20 + i) for i, n in enumerate((5, 11, 7))]
QUERIES = [_queries([0, 12, 5, 5, 8], 30), _queries([8, 0, 3, 8, 1, 4, 7], 31), _queries([20, 0, 13, 7, 19, 9, 9, 2, 16], 32)]


def test_track_chained_batch_is_track_chained_per_video():
    m = _FakeModel()
    got = drivers.track_chained_batch(m, VIDEOS, XY0S, iters=3, return_hops=True)
    batched_calls = m.track_calls
    assert len(got) == 3
    single_calls = 0
    for (tr, hops), video, xy0, T in zip(got, VIDEOS, XY0S, LENGTHS):
        ref = _FakeModel()
        ref_tr, ref_hops = drivers.track_chained(ref, video, xy0, iters=3, return_hops=True)
        single_calls += ref.track_calls
        assert tuple(tr.shape) == (1, T, xy0.shape[1], 2)
        assert torch.equal(tr, ref_tr) and hops == ref_hops
        assert any(len(h) > 1 for h in hops)
    assert batched_calls < single_calls                                # the videos' hops share their launches
    plain = drivers.track_chained_batch(_FakeModel(), VIDEOS, XY0S, iters=3)
    assert all(torch.equal(a, b[0]) for a, b in zip(plain, got))


def test_track_queries_batch_is_track_queries_per_video():
    m = _FakeModel()
    got = drivers.track_queries_batch(m, VIDEOS, QUERIES, iters=3, return_hops=True)
    for (tr, vi, hops), video, q, T in zip(got, VIDEOS, QUERIES, LENGTHS):
        ref_tr, ref_vi, ref_hops = drivers.track_queries(_FakeModel(), video, q, iters=3, return_hops=True)
        assert tuple(tr.shape) == (1, T, q.shape[1], 2) and tuple(vi.shape) == (1, T, q.shape[1])
        assert torch.equal(tr, ref_tr) and torch.equal(vi, ref_vi) and hops == ref_hops
        assert any(len(h) > 1 for h in hops[0]) and any(len(h) > 0 for h in hops[1])
    plain = drivers.track_queries_batch(_FakeModel(), VIDEOS, QUERIES, iters=3)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain, got))


def test_one_video_batch_is_track_chained_itself():
    video, xy0 = VIDEOS[2], XY0S[2]
    (tr, hops), = drivers.track_chained_batch(_FakeModel(), [video], [xy0], iters=2, return_hops=True)
    ref_tr, ref_hops = drivers.track_chained(_FakeModel(), video, xy0, iters=2, return_hops=True)
    assert torch.equal(tr, ref_tr) and hops == ref_hops


def test_batch_drivers_reject_bad_arguments():
    m = _FakeModel()
    with pytest.raises(ValueError, match="frame size"):
        drivers.track_chained_batch(m, [VIDEOS[0], _video(9, 1, size=8)], XY0S[:2])
    with pytest.raises(ValueError, match="frame size"):
        drivers.track_queries_batch(m, [VIDEOS[0], _video(9, 1, size=8)], QUERIES[:2])
    with pytest.raises(ValueError, match="3 videos but 2"):
        drivers.track_chained_batch(m, VIDEOS, XY0S[:2])
    with pytest.raises(ValueError, match="3 videos but 2"):
        drivers.track_queries_batch(m, VIDEOS, QUERIES[:2])
    # frame 10 does not exist in video 1 (9 frames) although the flat axis (43 frames) holds a frame 13 + 10
    with pytest.raises(ValueError, match=r"\[0, 8\]"):
        drivers.track_queries_batch(m, VIDEOS, [QUERIES[0], _queries([3, 10], 5), QUERIES[2]])
    for fn, per_video in ((drivers.track_chained_batch, XY0S), (drivers.track_queries_batch, QUERIES)):
        with pytest.raises(ValueError, match="engine"):
            fn(m, VIDEOS, per_video, engine="hip")
    assert m.track_calls == 0


def test_clip_entry_points_check_their_arguments_before_anything_else():
    """The PIPS_E_ARG cases of the clip forms are decided on the host ahead of the first launch, so they answer without a GPU:
    V < 1, a NULL table, win_clip without win_start, B != 1, a ring (R != T), the score-map block."""
    import ctypes as C
    from pips_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))                       # stands for every buffer: never read
    F, N = 5, 4
    good = dict(B=1, T=F, R=F, ws=p, wc=p, first=p, frames=p, V=2, ce=None)
    bad = [dict(V=0), dict(first=None), dict(frames=None), dict(ws=None), dict(B=2), dict(R=F + 1)]

    def gather(**o):
        a = dict(good, **o)
        return lib.pips_mixer_input_build_clips(p, a["B"], a["T"], a["R"], 16, 20, p, p, p, N, a["ws"], p, a["wc"], a["first"],
                                                a["frames"], a["V"], 0, 8, p, None)

    def track(**o):
        a = dict(good, **o)
        return lib.pips_track_clips(p, p, a["B"], a["T"], a["R"], 16, 20, p, None, None, a["ws"], p, a["wc"], a["first"], a["frames"],
                                    a["V"], p, N, 8, 1, 0, 8, p, 1 << 40, p, p, p, a["ce"], a["ce"], a["ce"], 1 << 40, None)

    def hop(**o):
        a = dict(good, **o)
        return lib.pips_chain_hop_clips(p, p, a["T"], a["R"], 16, 20, p, 8, 1, 0, N, p, N, 1, p, p, 24, 7, p, None, a["wc"], a["first"],
                                        a["frames"], a["V"], p, p, C.c_void_p(C.addressof(buf) + 64), p, p, 1 << 40, None)
    for o in bad:
        assert gather(**o) == -1 and lib.pips_last_error(), o
        assert track(**o) == -1 and lib.pips_last_error(), o
    assert track(ce=p) == -1 and b"score-map" in lib.pips_last_error()
    for o in (dict(V=0), dict(first=None), dict(frames=None), dict(R=F + 1)):
        assert hop(**o) == -1 and lib.pips_last_error(), o
    assert lib.pips_chain_step_clips(p, p, p, F, N, p, N, 1, p, p, 24, 7, p, None, p, None, 2, p, p,
                                     C.c_void_p(C.addressof(buf) + 64), p, None) == -1
    assert lib.pips_chain_step_clips(p, p, p, F, N, p, N, 1, p, p, 24, 7, p, None, p, p, 0, p, p,
                                     C.c_void_p(C.addressof(buf) + 64), p, None) == -1
    assert lib.pips_chain_gather_clips(p, 24, 7, N, p, None, p, p, p, N, 0, p, p, p, None, p, None) == -1
