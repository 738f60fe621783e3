"""CPU: drivers.track_queries / dist.track_queries_sharded -- queries from any frame, tracked forwards and backwards -- on a
fake model whose ``track`` honours ``win_start`` and ``win_dir`` (the frames a window reads, as the HIP gather reads them)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pips_amd import dist as pd
from pips_amd import drivers


class _FakeCache:
    def __init__(self, rgbs):
        self.m = rgbs.float().mean(dim=(2, 3, 4))                      # (B,T) per-frame content
        self.B, self.T = self.m.shape


class _FakeModel:
    """encode / track stand-in with the real signatures: a particle's result depends on its own start, its window start and
    direction, and the content of the frames its window reads -- row s reads frame clamp(win_start + dir * s, 0, T-1).
    Only exactly rounded float ops (no transcendental functions), so a particle computes the same bits in any batch."""
    S = 8

    def encode(self, rgbs):
        return _FakeCache(rgbs)

    def track(self, cache, xys, coords_init=None, feat_init=None, iters=3, win_start=None, return_feat=False, win_dir=None):
        B, N, _ = xys.shape
        ws = torch.zeros(B, N, dtype=torch.long) if win_start is None else win_start.long()
        d = torch.ones(B, N, dtype=torch.long) if win_dir is None else torch.where(win_dir < 0, -1, 1).long()
        t = (ws.unsqueeze(1) + d.unsqueeze(1) * torch.arange(8).view(1, 8, 1)).clamp(0, cache.T - 1)   # (B,8,N)
        fm = torch.gather(cache.m.unsqueeze(2).expand(B, cache.T, N), 1, t)                          # (B,8,N)
        base = xys.reshape(B, 1, N, 2) + 0.01 * fm.unsqueeze(-1) * torch.arange(8).view(1, 8, 1, 1)
        lock = (torch.arange(8) > 0).float().view(1, 8, 1, 1)                                       # row 0 stays the start
        preds = [base + 0.1 * i * lock for i in range(iters)]
        vis = torch.remainder(base.sum(-1) * 7.3, 8.0) - 4.0                                         # logits of both signs
        out = (preds, [base, base] + preds + [preds[-1]] * 2, vis)
        ff = xys.new_zeros(B, N, 128) if feat_init is None else feat_init
        return out + ((ff, None) if return_feat else (None,))


def _video(T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, T, 3, 6, 6, generator=g) * 255


def _queries(tq, seed, W=60.0, H=40.0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(len(tq), 2, generator=g) * torch.tensor([W, H])
    return torch.cat([torch.tensor(tq, dtype=torch.float32).view(-1, 1), xy], dim=1).unsqueeze(0)


def _replay_vis(m, video, trajs, tq, hops, n, d):
    """Visibility of every frame of one chain of query n, recomputed from the window that last wrote the frame (hop log
    replayed; the window's start position is the chain's own output at its start frame, which no later window rewrites)."""
    T = video.shape[1]
    cache = m.encode(video)
    out = {}
    cur = tq
    for si in hops:
        xy = trajs[0, cur, n].view(1, 1, 2)
        vis = m.track(cache, xy, iters=2, win_start=torch.tensor([[cur]]), win_dir=torch.tensor([[d]]))[2]
        for s in range(8):
            f = cur + d * s
            if 0 <= f < T:
                out[f] = vis[0, s, 0]
        cur += d * si
    return out


def test_queries_equal_chains_on_sliced_and_flipped_videos():
    """(a) per query frame: frames >= t_q are track_chained on rgbs[:, t_q:], frames < t_q are track_chained on
    rgbs[:, :t_q+1].flip(1) flipped back -- positions bit for bit, hop logs equal -- and every frame's visibility is the
    row of the window that last wrote it."""
    m = _FakeModel()
    T = 23
    video = _video(T, 1)
    tqs = [0, 3, T - 8, T - 2, T - 1, 3, T - 1, 0, 9]                    # both ends, duplicates
    q = _queries(tqs, 2)
    trajs, vis, (fh, bh) = drivers.track_queries(m, video, q, iters=3, return_hops=True)
    assert tuple(trajs.shape) == (1, T, len(tqs), 2) and tuple(vis.shape) == (1, T, len(tqs))
    assert any(len(h) > 2 for h in fh) and any(len(h) > 2 for h in bh)
    for n, tq in enumerate(tqs):
        xy = q[:, n:n + 1, 1:]
        fwd, fwd_h = drivers.track_chained(m, video[:, tq:], xy, iters=3, return_hops=True)
        assert torch.equal(trajs[:, tq:, n], fwd[:, :, 0]) and fh[n] == fwd_h[0]
        if tq > 0:
            bwd, bwd_h = drivers.track_chained(m, video[:, :tq + 1].flip(1), xy, iters=3, return_hops=True)
            assert torch.equal(trajs[:, :tq, n], bwd.flip(1)[:, :tq, 0]) and bh[n] == bwd_h[0]
            assert torch.equal(bwd[0, 0, 0], q[0, n, 1:])
        else:
            assert bh[n] == []
        assert torch.equal(trajs[0, tq, n], q[0, n, 1:])                 # the frame-0 lock: the query frame is the query
        ref = _replay_vis(m, video, trajs, tq, fh[n], n, 1)
        ref.update({f: v for f, v in _replay_vis(m, video, trajs, tq, bh[n], n, -1).items() if f < tq})
        assert sorted(ref) == list(range(T))
        assert torch.equal(vis[0, :, n], torch.stack([ref[f] for f in range(T)]))


def test_queries_at_frame_zero_are_track_chained():
    """(b) all queries at t = 0: exactly track_chained (positions and hop logs)."""
    m = _FakeModel()
    video = _video(21, 3)
    q = _queries([0] * 7, 4)
    trajs, vis, (fh, bh) = drivers.track_queries(m, video, q, iters=2, return_hops=True)
    ref, ref_h = drivers.track_chained(m, video, q[:, :, 1:], iters=2, return_hops=True)
    assert torch.equal(trajs, ref) and fh == ref_h and bh == [[]] * 7


@pytest.mark.parametrize("t", [-1, 12, 2.5, float("nan")])
def test_queries_reject_bad_frames(t):
    """(c) a query frame outside [0, T-1] or not an integer is an error."""
    q = _queries([0, 3], 5)
    q[0, 1, 0] = t
    with pytest.raises(ValueError):
        drivers.track_queries(_FakeModel(), _video(12, 5), q)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _FakeModel()
    video = _video(19, 6)
    qs = _queries([0, 5, 18, 11, 5, 1, 17], 7)                            # N = 7: padded to 8, cut back after the gather
    trajs, vis = pd.track_queries_sharded(m, video, qs, iters=2)
    ref_t, ref_v = drivers.track_queries(m, video, qs, iters=2)
    q.put((rank, bool(torch.equal(trajs, ref_t) and torch.equal(vis, ref_v) and tuple(trajs.shape) == (1, 19, 7, 2))))
    dist.barrier()
    dist.destroy_process_group()


def test_track_queries_sharded_world2():
    """(d) two ranks over gloo with an odd query count equal the single-process call."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
