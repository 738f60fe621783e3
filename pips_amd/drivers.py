"""Caller-side loops of the reference re-built on cached maps.

* ``track_dense``   -- test_on_davis.py:103-130: many query points on one clip.  The reference
  re-runs the encoder for every chunk of 256 points; here the clip is encoded once.
* ``track_chained`` -- chain_demo.py:40-83 / test_on_badja.py:64-112: visibility-aware
  chaining of 8-frame windows over a long video.  The reference re-encodes 8 frames per particle
  and per hop; here every video frame is encoded once and all live particles advance together,
  each with its own window start.
* ``track_queries`` -- the same chaining from a query frame ``t`` per point, forwards to the end and
  backwards to frame 0 (the reference's loop on ``rgbs[:, t:]`` and on ``rgbs[:, :t+1].flip(1)``):
  one encoder pass, both directions in the same hop launches (per-particle ``win_dir``).
* ``StreamTracker`` / ``track_stream`` -- ``track_queries``' forward chains on a video fed in chunks: frames are
  encoded into a ring of ``slots`` frames (``Pips.ring_cache``) and trajectories come back as frames become final,
  so device memory does not grow with the length of the video.
* ``track_chained_batch`` / ``track_queries_batch`` -- the same two drivers over a LIST of videos (equal frame size, any
  lengths) in one set of hop launches: the videos share one flat cache (``Pips.encode_videos``), every particle carries the
  index of its video (``Pips.track``'s ``win_clip``), and each video gets what its single-video driver returns, bit for bit.
* ``MultiStreamTracker`` / ``track_streams`` -- ``StreamTracker`` for a LIST of streams (equal frame size; own lengths, chunking,
  queries and ends) on one cache of rings (``Pips.ring_cache_videos``) and one state: a round hops the ready queries of every
  stream together, and each stream gets what its own ``StreamTracker`` returns, bit for bit.
* ``CoverTracker`` / ``track_cover`` (and ``MultiStreamTracker(cover=)``) -- a stream that decides which queries it tracks:
  a ``Cover`` policy retires the queries that left the frame or stayed invisible and seeds the empty cells of a grid over the
  frame after every push, in torch ops or as one ``pips_cover_step`` call (``scan``); ``Cover(per_cell=k)`` also retires the youngest
  of more than k tracks that share a cell (``cover_scan_thin`` / ``pips_cover_step_thin``).  ``Cover(seed="corners")`` puts each seed on
  the most trackable pixel of its cell (``corner_table_torch`` / ``pips_corner_table``); ``corner_queries`` is the offline form.
* ``import_frames`` / ``import_frames_torch`` -- a decoder's frames (pitched NV12, I420, 10-bit P010 and I010, packed RGB / BGR with
  or without alpha) as the planar ``(1,F,3,H,W)`` frames every driver above takes, resized to the model's size in the same
  ``pips_frames_import_ex`` launch when asked -- two-tap bilinear, or antialiased with ``antialias=True``; the second is the same
  rule in torch ops, bit for bit.
* ``draw_tracks`` / ``draw_tracks_torch`` / ``TrackPainter`` -- the way out: the trails of a tracker's output drawn onto the decoder's
  surfaces on the device, in place -- the 8-bit ones by one ``pips_tracks_draw`` call, the 10-bit P010 / I010 and trails that fade
  with age (``fade=``) by ``pips_tracks_draw_ex``; the second is the same integer rule in torch ops, byte for byte; ``TrackPainter``
  paints the pushes of a streamed tracker one by one, keeping the last rows by identity; ``track_colors``
  gives each identity its colour.
* ``motion_fit`` / ``motion_fit_torch`` / ``MotionEstimator`` / ``motion_path`` -- what the tracks mean together: the frame-to-frame
  camera motion as a consensus similarity between consecutive rows, by one ``pips_motion_fit`` call; the second is the same exact
  rule in torch ops, equal in every bit; ``MotionEstimator`` fits the pushes of a streamed tracker one by one, keeping the last row
  by identity; ``motion_path`` composes the pairs into frame -> frame-0 transforms.
* ``motion_layers`` / ``motion_layers_torch`` / ``link_layers`` / ``MotionLayers`` -- what moves, beside the camera: the consensus
  of ``motion_fit`` peeled into motion layers on the columns left over, by one ``pips_motion_layers`` call, and the layers linked
  from pair to pair into object ids on the host; the torch form is the same exact rule, equal in every bit; ``MotionLayers`` does
  it for the pushes of a streamed tracker, keeping the last pair's labels, ids and counts by identity.
* ``fill_candidates`` / ``warp_frames_fill`` / ``warp_frames_fill_torch`` / ``crop_zoom`` / ``Stabilizer(neighbors=)`` -- the border of
  a stabilised frame filled from its neighbouring frames by one ``pips_frames_warp_fill`` call, with a byte-exact torch twin, and
  the crop zoom at which no border shows at all.
* ``motion_smooth`` / ``warp_coefficients`` / ``warp_frames`` / ``warp_frames_torch`` / ``Stabilizer`` -- frames out, stabilised: the
  camera path smoothed on the host, the corrections turned into fixed-point affine rows, and the decoder's surfaces resampled
  through them by one ``pips_frames_warp`` call, in every format import and draw speak; the torch form is the same integer rule,
  byte for byte; ``Stabilizer`` does it for the pushes of a streamed tracker, handing a frame's correction back once the frames
  its window needs have been seen.

Host logic only (a few tiny torch ops on (8,N) tensors); all model arithmetic is in
libpips_hip.so through ``Pips.encode`` / ``Pips.track``.

The chaining drivers take ``engine="torch" | "native"``: one hop loop (``_chain``) on one of two engine classes that hold the chain
state.  ``_TorchEngine`` (the default) keeps the hop's bookkeeping -- the indexed read of the start positions, the scatters into
the trajectory, the sigmoid, ``skip_scan``, the index update -- as the torch ops of ``_hop``; ``_NativeEngine`` runs the whole hop as
ONE library call (``Pips.chain_hop``: the same bookkeeping as HIP kernels around the same tracker launches, state held as int32)
and reads the live count back, one host sync per hop either way.  Both give the same hops and the same bits.

The streamed trackers are ONE core, ``_StreamCore``, whose docstring states their rules -- when a query is ready, how it joins, when
a frame is final, how much room a push has, and what a covered stream does when: ``StreamTracker`` is its one-stream form on one
ring, ``CoverTracker`` that form with a cover, ``MultiStreamTracker`` its form on V rings behind a clip table, covered or not.
All take ``rounds="torch" | "library"`` and keep the device state in one object per value, for one stream or V:
``_TorchRounds`` decides who is ready, who joins and which frames are final in torch ops and hops on the chosen engine;
for ``_LibraryRounds`` the round itself is one ``pips_stream_round`` / ``pips_stream_round_clips`` call on int32 state.  The clip table
is optional in both, as it is in the library (a NULL table is the one-video form): it decides which entry points are called,
nothing else.  Queries can be added while a video runs (``add_queries``, either value) and taken away again (``remove_queries``: the
state's ``keep`` copies the remaining columns into narrower arrays -- ``pips_stream_keep`` under ``rounds="library"``), so the device
state follows the number of queries being tracked, not the number ever given.
"""
from __future__ import annotations

import cmath
import math
import weakref

import torch

from . import ops


@torch.no_grad()
def track_dense(model, rgbs, xys, iters=6, chunk=None):
    """rgbs (B,8,3,H,W), xys (B,N,2) -> (trajs_e (B,8,N,2), vis_e (B,8,N) logits)."""
    cache = model.encode(rgbs)
    N = xys.shape[1]
    chunk = N if chunk is None else chunk
    trajs, viss = [], []
    for n0 in range(0, N, chunk):
        preds, _, vis, _ = model.track(cache, xys[:, n0:n0 + chunk], iters=iters)
        trajs.append(preds[-1])
        viss.append(vis)
    return torch.cat(trajs, dim=2), torch.cat(viss, dim=2)


def _threshold_table(n=64):
    """thr after k decrements exactly as chain_demo.py:64,75 computes it (python doubles),
    rounded to float32 as the tensor comparison ``vis[0,si] > thr`` does."""
    thr, out = 0.9, []
    for _ in range(n):
        out.append(thr)
        thr -= 0.02
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def skip_scan(vis):
    """vis (8,n) sigmoid confidences -> si (n,) int64: chain_demo.py:63-77.  Frames 7..2 are
    tested against thr (0.9, lowered by 0.02 whenever the scan reaches frame 1); the LATEST
    frame above the threshold wins."""
    thr = _threshold_table().to(vis.device)
    cand = vis[2:8].unsqueeze(0) > thr.view(-1, 1, 1)                 # (K,6,n)
    anyk = cand.any(dim=1)                                            # (K,n)
    kfirst = torch.argmax(anyk.to(torch.int32), dim=0)                # first threshold that admits a frame
    n = vis.shape[1]
    sel = cand[kfirst, :, torch.arange(n, device=vis.device)]         # (n,6)
    last = 5 - torch.argmax(sel.flip(1).to(torch.int32), dim=1)       # latest admitted frame
    return last + 2


def _hop(model, cache, trajs, vis_p, base, cur, active, feat, d=None, iters=6, clip=None):
    """One window of chain_demo.py:40-83 for each particle in ``active``: its start position is its trajectory at its window
    start ``cur[active]`` (logical frames), its rows are written back and ``skip_scan`` gives the step.  trajs (L,n,2) and
    vis_p (L,n) (or None) hold frame f in row (f + base) mod L.  feat: (n,128) features carried from the first window, or
    None (the track call samples them); d: the active particles' directions (+1 / -1) or None (all forward); clip: the active
    particles' videos on a cache of several (``cur`` then counts frames of the particle's own video) or None.
    -> (the new window starts of ``active``, their steps si, the features of this call (n_active,128))."""
    S = 8
    L = trajs.shape[0]
    c = cur[active]
    start_xy = trajs[(c + base) % L, active].unsqueeze(0)                        # traj_e[:,cur_frame]
    fi = None if feat is None else feat[active].unsqueeze(0)
    rows = torch.arange(S, device=c.device).unsqueeze(1)                         # (S,1)
    kw = {}
    if d is not None:
        kw["win_dir"] = d.to(torch.int32).unsqueeze(0)
        rows = rows * d.unsqueeze(0)                                              # row s of a window is frame c + d * s
    if clip is not None:
        kw["win_clip"] = clip.to(torch.int32).unsqueeze(0)
    preds, _, vis, ffeat, _ = model.track(cache, start_xy, iters=iters, feat_init=fi,
                                          win_start=c.to(torch.int32).unsqueeze(0), return_feat=True, **kw)
    rows = (c.unsqueeze(0) + rows + base) % L                                     # (S,n)
    cols = active.unsqueeze(0).expand(S, -1)
    trajs[rows, cols] = preds[-1][0]                                              # traj_e[cur:cur+8] = xys[:S_local]
    if vis_p is not None:
        vis_p[rows, cols] = vis[0]
    si = skip_scan(torch.sigmoid(vis[0]))
    return c + (si if d is None else si * d), si, ffeat[0]


class _TorchEngine:
    """The chain state of ``engine="torch"``: int64 window starts ``cur`` and the shrinking list ``active`` of live particles.
    trajs (L,n,2) / vis_p (L,n) or None hold frame f in row (f + base) % L; ``cur0`` (n,) the first window starts, ``dirs`` (n,)
    +1 / -1 or None (all forward), ``clip`` (n,) the particles' videos or None, ``end`` the frames of the video (or (n,), of each
    particle's own).  ``feat`` (n,128): the features carried from the first window; while None, the next window samples them.
    The log is made of the tensors a hop produced anyway, so it is kept whether or not ``want_log`` is set."""

    def __init__(self, model, cache, trajs, vis_p, base, cur0, dirs, clip, end, iters, want_log):
        self.model, self.cache, self.trajs, self.vis_p, self.base, self.iters = model, cache, trajs, vis_p, base, iters
        self.dirs, self.clip, self.end = dirs, clip, end
        self.cur, self.active = cur0.clone(), torch.arange(cur0.shape[0], device=cur0.device)
        self.feat, self.log = None, []

    def window(self, active):
        """``_hop`` for the particles ``active`` (int64) -> (their new window starts, their steps)"""
        c, si, ffeat = _hop(self.model, self.cache, self.trajs, self.vis_p, self.base, self.cur, active, self.feat,
                            None if self.dirs is None else self.dirs[active], self.iters, None if self.clip is None else self.clip[active])
        if self.feat is None:
            self.feat = ffeat.clone()                                              # carried forever (:57)
        self.cur[active] = c
        return c, si

    def hop(self):
        """every live particle advances by one window -> the number still live (one host sync: the live count)"""
        active = self.active
        c, si = self.window(active)
        self.log.append((active, si))
        end = self.end[active] if torch.is_tensor(self.end) else self.end        # the end of each particle's own video
        self.active = active[c < end if self.dirs is None else (c < end) & (c >= 0)]
        return self.active.numel()


class _NativeEngine:
    """The chain state of ``engine="native"``, a window being one ``Pips.chain_hop`` call: int32 ``cur`` / ``dirs`` / ``clip``, the
    ping-pong lists ``active`` / ``next`` of live particles, their ``count`` and the ``steps``.  Arguments as ``_TorchEngine``; the
    library takes the videos' lengths from the cache, so ``end`` is not looked at.  ``want_log=False`` spares the two copies per
    hop that keep ``active`` / ``steps`` for the log (the buffers are reused by the next hop): the log then stays empty."""

    def __init__(self, model, cache, trajs, vis_p, base, cur0, dirs, clip, end, iters, want_log):
        self.model, self.cache, self.trajs, self.vis_p, self.base, self.iters = model, cache, trajs, vis_p, base, iters
        i32, dev, n = torch.int32, cur0.device, cur0.shape[0]
        self.cur = cur0.to(i32).contiguous()
        self.dirs, self.clip = (None if x is None else x.to(i32).contiguous() for x in (dirs, clip))
        self.active, self.next, self.n_act = torch.arange(n, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev), n
        self.count, self.steps = torch.zeros(1, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev)
        self.feat, self.want_log, self.log = None, want_log, []

    def _launch(self, act):
        sample = self.feat is None
        if sample:                                                                  # written by this window (sample_feat)
            self.feat = torch.empty(self.cur.shape[0], 128, dtype=torch.float32, device=self.cur.device)
        self.model.chain_hop(self.cache, act, act.numel(), self.trajs, self.vis_p, self.base, self.cur, self.dirs, self.feat, self.next,
                             self.count, self.steps, iters=self.iters, sample_feat=sample, clip=self.clip)

    def window(self, active):
        """one library hop for the particles ``active`` (ascending) -> (their new window starts, their steps)"""
        act = active.to(torch.int32)
        self._launch(act)
        return self.cur[active], self.steps[:act.numel()]

    def hop(self):
        """every live particle advances by one window -> the number still live (one host sync: the live count)"""
        act = self.active[:self.n_act]
        self._launch(act)
        if self.want_log:
            self.log.append((act.clone(), self.steps[:self.n_act].clone()))
        self.n_act = int(self.count.item())
        self.active, self.next = self.next, self.active
        return self.n_act


_ENGINES = {"torch": _TorchEngine, "native": _NativeEngine}
ENGINES = tuple(_ENGINES)


def _check_engine(engine):
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {ENGINES}, not {engine!r}")


def _chain(model, cache, T, xy, f0, dirs=None, iters=6, with_vis=True, engine="torch", want_log=True, clip=None):
    """The hop loop of chain_demo.py:40-83 for all particles at once, on the chosen engine.  xy (n,2) px at frames f0 (n,) int64;
    dirs (n,) +1 / -1 per particle or None (all forward).  A backward particle runs the loop on the time-reversed video: its
    window rows read f, f-1, ... (``Pips.track``'s ``win_dir``) and it is finished when its start passes frame 0.
    ``clip`` (n,) int64: the video of each particle, for several videos on one cache (``Pips.encode_videos``); ``T`` is then (n,)
    int64, the frames of each particle's video, and trajs / vis come back with max(T) rows.  -> trajs (T,n,2), vis (T,n) logits
    (None without ``with_vis``), each frame from the last window that wrote it, and the engine's hop log [(active, si)]."""
    dev, pad, n = xy.device, 7, xy.shape[0]
    rows = int(T.max()) if torch.is_tensor(T) else T                              # the frames the output buffer holds
    # S - 1 frames of padding on both sides of the video: a window that runs past either end is written whole and cut off
    # on return (no per-row masks, no host round trips inside a hop)
    trajs = torch.zeros(rows + 2 * pad, n, 2, dtype=torch.float32, device=dev)
    vis_p = torch.zeros(rows + 2 * pad, n, dtype=torch.float32, device=dev) if with_vis else None
    trajs[f0 + pad, torch.arange(n, device=dev)] = xy.to(torch.float32)
    eng = _ENGINES[engine](model, cache, trajs, vis_p, pad, f0, dirs, clip, T, iters, want_log)
    live = n
    while live > 0:
        live = eng.hop()
    return trajs[pad:pad + rows], None if vis_p is None else vis_p[pad:pad + rows], eng.log


def _hops(log, n):
    hops = [[] for _ in range(n)]
    for act, si in log:
        for k, s in zip(act.tolist(), si.tolist()):
            hops[k].append(s)
    return hops


@torch.no_grad()
def track_chained(model, rgbs, xy0, iters=6, return_hops=False, engine="torch"):
    """rgbs (1,T,3,H,W), xy0 (1,N,2) px at frame 0 -> trajs_e (1,T,N,2) (chain_demo.run_model).
    ``return_hops=True``: also the list, per particle, of the frame steps ``si`` its windows advanced by
    (chain_demo.py:63-79) -- what a parity test compares hop for hop.  ``engine``: see the module docstring."""
    _check_engine(engine)
    assert rgbs.shape[0] == 1, "the reference chains one video at a time (chain_demo.py:24)"
    assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
    dev = rgbs.device
    T, N = rgbs.shape[1], xy0.shape[1]
    cache = model.encode(rgbs)
    trajs, _, log = _chain(model, cache, T, xy0[0].to(dev), torch.zeros(N, dtype=torch.int64, device=dev), iters=iters,
                           with_vis=False, engine=engine, want_log=return_hops)
    out = trajs.unsqueeze(0).contiguous()
    if not return_hops:
        return out
    return out, _hops(log, N)


def _query_frames(queries, T=None):
    """queries (1,N,3) = (t, x, y) -> t as int64 on the host; ValueError unless every t is an integer in [0, T-1] (T = None:
    no upper bound)."""
    if queries.dim() != 3 or queries.shape[0] != 1 or queries.shape[2] != 3:
        raise ValueError(f"queries must be (1,N,3) = (t, x, y), not {tuple(queries.shape)}")
    t = queries[0, :, 0].detach().to("cpu", torch.float64)
    hi = float("inf") if T is None else T - 1
    if not bool(torch.isfinite(t).all()) or not torch.equal(t, t.round()) or bool(((t < 0) | (t > hi)).any()):
        raise ValueError("query frames must be non-negative integers" if T is None else
                         f"query frames must be integers in [0, {T - 1}]")
    return t.to(torch.int64)


@torch.no_grad()
def track_queries(model, rgbs, queries, iters=6, return_hops=False, engine="torch"):
    """Track query points from any frame over the whole video, forwards and backwards in time.

    rgbs (1,T,3,H,W), queries (1,N,3) = (t, x, y): ``t`` an integer frame index, ``x, y`` in pixels -- PIPs' xy order, not
    TAP-Vid's (t, y, x).  -> trajs_e (1,T,N,2) px and vis_e (1,T,N) logits (the units of ``forward``'s vis_e).

    Frames t >= t_q come from the reference's chaining loop (chain_demo.py:40-83) run on ``rgbs[:, t_q:]``, frames t < t_q
    from the same loop on the time-reversed ``rgbs[:, :t_q+1].flip(1)``, flipped back; within each chain the last window
    that wrote a frame gives its position and visibility.  The video is encoded once; every query is a forward particle,
    plus a backward one when t_q > 0, and all of them advance together, one ``model.track`` call per hop.
    ``return_hops=True``: also ``(forward, backward)``, per query the frame steps of each chain's windows (backward: [] when
    t_q = 0).  ``engine``: see the module docstring."""
    _check_engine(engine)
    assert rgbs.shape[0] == 1 and queries.shape[0] == 1, "one video at a time, as track_chained"
    assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
    dev = rgbs.device
    T, N = rgbs.shape[1], queries.shape[1]
    xy, f0, dirs, tq_d, back = _query_particles(queries, T, dev)
    cache = model.encode(rgbs)
    tr, vi, log = _chain(model, cache, T, xy, f0, dirs, iters=iters, engine=engine, want_log=return_hops)
    trajs, vis = _join_directions(tr, vi, N, tq_d, back.to(dev))
    if not return_hops:
        return trajs, vis
    return trajs, vis, _query_hops(_hops(log, N + back.numel()), N, back)


def _query_particles(queries, T, dev):
    """The particles of one video's queries (1,N,3): the N forward ones, then a backward one for every query with t > 0.
    -> (xy (n,2), f0 (n,), dirs (n,), the query frames on the device, the queries that have a backward particle (host))."""
    N = queries.shape[1]
    tq = _query_frames(queries, T)
    back = torch.nonzero(tq > 0).squeeze(1)
    nb = back.numel()
    xy = queries[0, :, 1:3].to(dev, torch.float32)
    tq_d, back_d = tq.to(dev), back.to(dev)
    f0 = torch.cat([tq_d, tq_d[back_d]])
    dirs = torch.cat([torch.ones(N, dtype=torch.int64, device=dev), torch.full((nb,), -1, dtype=torch.int64, device=dev)])
    return torch.cat([xy, xy[back_d]]), f0, dirs, tq_d, back


def _join_directions(tr, vi, N, tq_d, back_d):
    """tr (T,N+nb,2), vi (T,N+nb) of ``_query_particles``' particles -> trajs (1,T,N,2), vis (1,T,N): frames before a query's
    frame come from its backward chain."""
    T = tr.shape[0]
    trajs, vis = tr[:, :N].clone(), vi[:, :N].clone()
    before = torch.arange(T, device=tr.device).unsqueeze(1) < tq_d[back_d].unsqueeze(0)     # (T,nb): frames of the backward chain
    trajs[:, back_d] = torch.where(before.unsqueeze(-1), tr[:, N:], trajs[:, back_d])
    vis[:, back_d] = torch.where(before, vi[:, N:], vis[:, back_d])
    return trajs.unsqueeze(0), vis.unsqueeze(0)


def _query_hops(hops, N, back):
    """the hop lists of ``_query_particles``' particles -> (forward, backward) per query"""
    bwd = [[] for _ in range(N)]
    for j, q in enumerate(back.tolist()):
        bwd[q] = hops[N + j]
    return hops[:N], bwd


def _check_videos(model, videos, per_video, what):
    """The argument checks of the batch drivers -> the videos' lengths."""
    assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
    videos, per_video = list(videos), list(per_video)
    if not videos or len(videos) != len(per_video):
        raise ValueError(f"{len(videos)} videos but {len(per_video)} {what}")
    for v in videos:
        if v.dim() != 5 or v.shape[0] != 1:
            raise ValueError(f"every video must be (1,T,3,H,W), not {tuple(v.shape)}")
        if tuple(v.shape[2:]) != tuple(videos[0].shape[2:]):
            raise ValueError(f"the videos of one call share a frame size: {tuple(v.shape[2:])} against {tuple(videos[0].shape[2:])}")
    return [int(v.shape[1]) for v in videos]


@torch.no_grad()
def track_chained_batch(model, videos, xy0s, iters=6, return_hops=False, engine="torch"):
    """``track_chained`` over several videos in one set of hop launches.  videos: list of (1,T_v,3,H,W) of one frame size,
    xy0s: list of (1,N_v,2) px at frame 0 of each -> the list, per video, of what ``track_chained(model, video, xy0)`` returns
    (bit for bit while the mixer's GEMMs take the same route at the batched and at the single-video row counts)."""
    _check_engine(engine)
    lengths = _check_videos(model, videos, xy0s, "start point sets")
    dev = videos[0].device
    counts = [int(x.shape[1]) for x in xy0s]
    n = sum(counts)
    clip = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(counts)).to(dev)
    Tq = torch.tensor(lengths)[clip.cpu()].to(dev)
    cache = model.encode_videos(videos)
    trajs, _, log = _chain(model, cache, Tq, torch.cat([x[0].to(dev) for x in xy0s]), torch.zeros(n, dtype=torch.int64, device=dev),
                           iters=iters, with_vis=False, engine=engine, want_log=return_hops, clip=clip)
    hops = _hops(log, n) if return_hops else None
    out, p0 = [], 0
    for T, N in zip(lengths, counts):
        tr = trajs[:T, p0:p0 + N].unsqueeze(0).contiguous()
        out.append((tr, hops[p0:p0 + N]) if return_hops else tr)
        p0 += N
    return out


@torch.no_grad()
def track_queries_batch(model, videos, queries, iters=6, return_hops=False, engine="torch"):
    """``track_queries`` over several videos in one set of hop launches.  videos: list of (1,T_v,3,H,W) of one frame size,
    queries: list of (1,N_v,3) = (t, x, y) with ``t`` a frame of ITS video -> the list, per video, of the ``(trajs, vis[, hops])``
    of ``track_queries(model, video, queries_v)`` (bit for bit, as ``track_chained_batch``)."""
    _check_engine(engine)
    lengths = _check_videos(model, videos, queries, "query sets")
    dev = videos[0].device
    parts = [_query_particles(q, T, dev) for q, T in zip(queries, lengths)]        # (a query frame past its OWN video raises here)
    counts = [p[0].shape[0] for p in parts]
    clip = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(counts)).to(dev)
    Tq = torch.tensor(lengths)[clip.cpu()].to(dev)
    cache = model.encode_videos(videos)
    tr, vi, log = _chain(model, cache, Tq, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]),
                         torch.cat([p[2] for p in parts]), iters=iters, engine=engine, want_log=return_hops, clip=clip)
    hops = _hops(log, sum(counts)) if return_hops else None
    out, p0 = [], 0
    for T, n, q, (_, _, _, tq_d, back) in zip(lengths, counts, queries, parts):
        N = q.shape[1]
        res = _join_directions(tr[:T, p0:p0 + n], vi[:T, p0:p0 + n], N, tq_d, back.to(dev))
        out.append(res + (_query_hops(hops[p0:p0 + n], N, back),) if return_hops else res)
        p0 += n
    return out


def _wider(old, m):                                       # the row ring (L,n[,2]) with m more NaN columns
    return torch.cat([old, old.new_full((old.shape[0], m) + tuple(old.shape[2:]), float("nan"))], dim=1)


def _longer(old, new):                                    # the per-query array (n[,k]) with the rows ``new`` behind it, in its type
    return torch.cat([old, new.to(old.device, old.dtype).reshape((-1,) + tuple(old.shape[1:]))])


_INT_MAX = 2 ** 31 - 1                                       # the int32 "nothing pending" / "no limit" of the library's counts and rules


class _Rounds:
    """The device state of a stream tracker (``_StreamCore``), in the form its ``rounds`` value takes, for the queries of V >= 1
    streams.  Both forms hold the output rows -- trajs (L,N,2) and vis (L,N), frame f in row f % L, NaN where nothing was written
    -- the queries ``tq`` / ``xy``, the stream ``clip`` (N) of each query, and the host list ``final`` (V) of the streams that ended.
      start(dev) / grow(t, xy, m, v)   the state of the tracker's N queries, none joined / m more columns for stream v
      keep(idx)      only the columns idx (host int64, ascending) remain, in narrower arrays; the others are forgotten
      end(v, final=True)   stream v has ended: its unfinished queries are ready, their windows repeat its last frame (False: a
                     cut takes the mark back)
      lows()         per stream, the lowest window start of its unfinished queries (None: it has none)
      run()          hop rounds until no query of any stream is ready (the core's readiness rule); yields (active indices,
                     steps) per round ((None, None) when a library round keeps no steps)
      emit(f0, f1, cols)   the rows of frames [f0, f1) of one stream's columns ``cols`` (host int64) moved out of the ring (NaN
                     is left behind for reuse)
    ``table`` says whether the cache has a clip table (``Pips.ring_cache_videos``: V rings) or is the one ring of one video
    (``Pips.ring_cache``: then V = 1 and ``clip`` is all zero).  It decides only what the model and the library are handed --
    ``_handed`` and the entry points next to it: the clip-table forms, or the NULL-table forms the one-video tracker always used."""

    def __init__(self, tracker, engine):
        # (a weak reference: no cycle, so a dropped tracker gives its ring and its rows back at once, not at some later collection)
        self.t, self.engine = weakref.proxy(tracker), engine

    def start(self, dev):
        t = self.t
        L = t.slots + t.S                                                         # output rows: frames f live in row f % L
        self.table = t.table
        self.trajs = torch.full((L, t.N, 2), float("nan"), dtype=torch.float32, device=dev)
        self.vis = torch.full((L, t.N), float("nan"), dtype=torch.float32, device=dev)
        self.tq, self.xy, self.clip = t.tq_host.to(dev), t.xy_in.to(dev, torch.float32), t.clip_host.to(dev)
        self.final = [False] * t.V
        self.final_d = torch.zeros(t.V, dtype=torch.bool, device=dev) if self.table else None      # ``final`` as the table form reads it

    def grow(self, t, xy, m, v):
        self.trajs, self.vis = _wider(self.trajs, m), _wider(self.vis, m)
        self.tq, self.xy = _longer(self.tq, t), _longer(self.xy, xy)
        self.clip = _longer(self.clip, torch.full((m,), v)) if self.t.V > 1 else self.clip.new_zeros(self.clip.shape[0] + m)

    def _keep_torch(self, idx, names):
        """the torch form of ``keep``: the arrays ``names`` indexed on their query axis -> idx on the device"""
        i = idx.to(self.tq.device)
        self.trajs, self.vis = self.trajs.index_select(1, i), self.vis.index_select(1, i)       # (new, contiguous tensors)
        for k in names:
            setattr(self, k, getattr(self, k)[i])
        self.clip = self.clip[i] if self.t.V > 1 else self.clip[:i.numel()]
        return i

    def end(self, v, final=True):
        self.final[v] = final
        if self.table:
            self.final_d[v:v + 1].fill_(int(final))

    def _handed(self):
        """(final, clip) as the model and the library take them: the tables, or the one stream's bool and no clip"""
        return (self.final_d, self.clip) if self.table else (self.final[0], None)


class _TorchRounds(_Rounds):
    """``rounds="torch"``: which queries are ready, which join (``joined``) and which are finished (``done``) is decided here in
    torch ops; the hop is a window of the chosen hop engine on the row ring (base 0) -- ``_hop(..., clip=)`` on a cache of rings --
    which holds the window starts ``cur`` (= t_q until a query joins) and the first-window features."""

    def _engine(self, cur0, feat=None):
        t = self.t
        self.eng = _ENGINES[self.engine](t.model, t.cache, self.trajs, self.vis, 0, cur0, None, self._handed()[1], None, t.iters, False)
        self.eng.feat = feat

    cur = property(lambda self: self.eng.cur)

    def start(self, dev):
        super().start(dev)
        self.joined, self.done = (torch.zeros(self.t.N, dtype=torch.bool, device=dev) for _ in range(2))
        self._engine(self.tq)

    def grow(self, t, xy, m, v):
        super().grow(t, xy, m, v)
        self.joined, self.done = _longer(self.joined, torch.zeros(m)), _longer(self.done, torch.zeros(m))
        feat = self.eng.feat
        self._engine(_longer(self.eng.cur, t), None if feat is None else _longer(feat, torch.zeros(m, feat.shape[1])))

    def keep(self, idx):
        cur, feat = self.eng.cur, self.eng.feat
        i = self._keep_torch(idx, ("tq", "xy", "joined", "done"))
        self._engine(cur[i], None if feat is None else feat[i])                    # (the engine is rebuilt as ``grow`` rebuilds it)

    def lows(self):
        live, cur = ~self.done, self.eng.cur                                      # (int64, or the native engine's int32)
        if self.t.V == 1:                                                         # one stream: a plain minimum, no scatter
            live = cur[live]
            return [None if live.numel() == 0 else int(live.min())]
        low = torch.full((self.t.V,), _INT_MAX, dtype=cur.dtype, device=cur.device)      # (one host read)
        low = low.scatter_reduce(0, self.clip[live], cur[live], "amin")
        return [None if x == _INT_MAX else x for x in low.tolist()]

    def _ends(self):
        """-> (the queries whose window can run now, ``ended(active, c)``: which of the hopped ones are finished, or None: none is),
        by the frames T and the end ``fin`` of each query's OWN stream -- (n) tensors through the table, two scalars without one"""
        cur, S = self.eng.cur, self.t.S
        if self.table:
            T, fin = self.t.cache.clip_frames.to(torch.int64)[self.clip], self.final_d[self.clip]
            return ~self.done & torch.where(fin, cur < T, cur + S <= T), lambda active, c: fin[active] & (c >= T[active])
        T, fin = self.t.cache.T, self.final[0]
        return ~self.done & ((cur < T) if fin else (cur + S <= T)), (lambda active, c: c >= T) if fin else None

    def run(self):
        t, eng, L, clip = self.t, self.eng, self.trajs.shape[0], self._handed()[1]
        while True:
            ready, ended = self._ends()
            active = torch.nonzero(ready).squeeze(1)
            if active.numel() == 0:
                return
            new = active[~self.joined[active]]
            if new.numel() > 0:
                # first window: the start is the query and the features are its point sample at t_q (feat_init=None)
                self.trajs[self.tq[new] % L, new] = self.xy[new]
                ring = {} if clip is None else {"win_clip": clip[new].to(torch.int32).unsqueeze(0)}
                ff = t.model.track(t.cache, self.xy[new].unsqueeze(0), iters=0, return_feat=True,
                                   win_start=self.tq[new].to(torch.int32).unsqueeze(0), **ring)[3]
                if eng.feat is None:
                    eng.feat = ff.new_zeros(self.tq.shape[0], ff.shape[-1])
                eng.feat[new] = ff[0]
                self.joined[new] = True
            c, si = eng.window(active)
            if ended is not None:
                self.done[active] = ended(active, c)
            yield active, si

    def emit(self, f0, f1, cols):
        rows = torch.arange(f0, f1, device=self.trajs.device) % self.trajs.shape[0]
        at = (rows.unsqueeze(1), cols.to(rows.device).unsqueeze(0)) if self.table else rows      # one stream: its columns are the rows
        out = (self.trajs[at], self.vis[at])
        self.trajs[at] = float("nan")
        self.vis[at] = float("nan")
        return out


class _LibraryRounds(_Rounds):
    """``rounds="library"``: the int32 / float arrays of ``pips_stream_round`` / ``pips_stream_round_clips`` (include/pips_hip.h) --
    ``status`` (0 waiting, 1 joined, 2 done), ``cur``, ``feat``, ``clip``, the lists ``active`` / ``new_list`` / ``steps`` a round writes
    and its ``counts``: four, the low in counts[2], or with a table 4 + V, the streams' lows behind the four -- and ``low`` (V), the
    host copy of those lows.  The hop is the library's, so the engine is not looked at."""

    def _lists(self):
        """the lists a round writes, for the queries there are now (their contents do not outlive a push)"""
        n, dev = self.tq.shape[0], self.tq.device
        self.active, self.new_list = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        self.steps = torch.empty(n, dtype=torch.int32, device=dev) if self.t.hops is not None else None

    def _lows(self, counts):
        self.low = [None if x == _INT_MAX else x for x in (counts[4:] if self.table else counts[2:3])]

    def start(self, dev):
        super().start(dev)
        t, i32 = self.t, torch.int32
        self.tq, self.xy, self.clip = self.tq.to(i32), self.xy.contiguous(), self.clip.to(i32)
        self.cur = self.tq.clone()                                                # window start (= t_q until it joins)
        self.status = torch.zeros(t.N, dtype=i32, device=dev)
        self.feat = torch.zeros(t.N, 128, dtype=torch.float32, device=dev)
        if self.table:
            self.counts, self.final_d = torch.zeros(4 + t.V, dtype=i32, device=dev), self.final_d.to(i32)
        else:
            self.counts = torch.zeros(4, dtype=i32, device=dev)
        self._lists()
        self.low = [None] * t.V
        for v, tq in zip(t.clip_host.tolist(), t.tq_host.tolist()):
            self.low[v] = tq if self.low[v] is None else min(self.low[v], tq)

    def grow(self, t, xy, m, v):
        super().grow(t, xy, m, v)
        self.cur, self.status = _longer(self.cur, t), _longer(self.status, torch.zeros(m))
        self.feat = _longer(self.feat, torch.zeros(m, self.feat.shape[1]))
        self._lists()
        self.low[v] = int(t.min()) if self.low[v] is None else min(self.low[v], int(t.min()))

    def keep(self, idx):
        # one pips_stream_keep call; its counts are what a select over the kept queries would report (the one host read)
        table = dict(clip=self.clip, V=self.t.V) if self.table else {}
        *arrays, counts = ops.stream_keep(idx.to(self.tq.device, torch.int32), self.tq, self.xy, self.cur, self.status, self.feat,
                                          self.trajs, self.vis, **table)
        self.tq, self.xy, self.cur, self.status, self.feat, self.trajs, self.vis = arrays[:7]
        self.clip = arrays[7] if self.table else self.clip[:idx.numel()]          # (one stream: all zero)
        self._lists()
        self._lows(counts.tolist())

    def lows(self):
        return list(self.low)

    def _select(self):
        c = self.t.cache
        if self.table:
            ops.stream_select_clips(self.tq, self.xy, self.cur, self.status, self.clip, c.clip_frames, self.final_d, self.trajs,
                                    self.active, self.new_list, self.counts)
        else:
            ops.stream_select(c.T, self.final[0], self.tq, self.xy, self.cur, self.status, self.trajs, self.active, self.new_list,
                              self.counts)

    def run(self):
        # select, then one round call per round while any query of any stream is ready (one host read per round: the counts)
        t = self.t
        if self.tq.shape[0] == 0:
            return
        final, clip = self._handed()
        self._select()
        counts = self.counts.tolist()
        while counts[0] > 0:
            n_act, n_new = counts[:2]
            act = self.active[:n_act].clone() if self.steps is not None else None      # the round rewrites the list
            t.model.stream_round(t.cache, final, n_act, n_new, self.tq, self.xy, self.cur, self.status, self.feat, self.trajs,
                                 self.vis, self.active, self.new_list, self.counts, self.steps, iters=t.iters, clip=clip)
            yield act, None if act is None else self.steps[:n_act]
            counts = self.counts.tolist()
        self._lows(counts)

    def emit(self, f0, f1, cols):
        if self.table:
            return ops.stream_emit_cols(self.trajs, self.vis, f0, f1, cols.to(self.trajs.device, torch.int32))
        if self.tq.shape[0] == 0:                                                 # (the library takes no empty state)
            return self.trajs.new_empty(f1 - f0, 0, 2), self.vis.new_empty(f1 - f0, 0)
        return ops.stream_emit(self.trajs, self.vis, f0, f1)


def _kept(cols, n, what):
    """``cols``: a tensor or a sequence of columns to remove out of ``n`` -> (cols as host int64, the columns that remain, ascending);
    ValueError for a column outside [0, n), one that is no integer and a duplicate"""
    c = torch.as_tensor(cols).detach().to("cpu").reshape(-1)
    if c.numel() > 0 and (c.is_floating_point() or c.is_complex() or c.dtype == torch.bool):
        raise ValueError(f"{what} must be integers, not {c.dtype}")
    c = c.to(torch.int64)
    if bool(((c < 0) | (c >= n)).any()):
        raise ValueError(f"{what} must lie in [0, {n}): {c.tolist()}")
    mask = torch.ones(n, dtype=torch.bool)
    mask[c] = False
    if int(mask.sum()) != n - c.numel():
        raise ValueError(f"{what} holds a column twice: {c.tolist()}")
    return c, torch.nonzero(mask).squeeze(1)


_ROUNDS = {"torch": _TorchRounds, "library": _LibraryRounds}
ROUNDS = tuple(_ROUNDS)


def _check_frames(frames):
    if frames.dim() != 5 or frames.shape[0] != 1 or frames.shape[2] != 3:
        raise ValueError(f"frames must be (1,k,3,H,W), not {tuple(frames.shape)}")


class _StreamCore:
    """``track_queries``' forward chains on V >= 1 videos of one frame size that arrive in chunks, in bounded device memory: what
    ``StreamTracker`` (one video, ``table=False``) and ``MultiStreamTracker`` (``table=True``) are facades of.  Every stream has its own
    length, chunking, queries and end.  The rules, stated here once:

    Frames.  Each stream's frames are encoded once into its ring of ``slots`` frames -- the one ring of ``Pips.ring_cache`` without a
      clip table, V rings on one flat cache (``Pips.ring_cache_videos``) with one.  ``T_v`` is the number of frames stream v has got.
    Readiness.  A query is READY once the 8 frames of its window have arrived, ``cur + 8 <= T_v``; after the end of its stream
      (``finish``) every unfinished query is ready, and a window past the last frame repeats it (chain_demo.py:50-52).
    Rounds and joining.  A round is ONE hop over the ready queries of every stream (V cameras fill the mixer's rows together).  A
      query JOINS in its first round: its start is the query position and its features are the point sample at ``t_q`` (the
      sample of ``feat_init=None``), carried from then on.  After each wave of appended frames the rounds run until no query is ready.
    Final frames.  A frame of stream v is FINAL, and handed out, when it lies below ``low_v``, the lowest window start of the
      stream's unfinished queries: ``push`` / ``finish`` return the frames ``[emitted_v, min(low_v, T_v))``.  Frame ``t >= t_q`` of a
      query is the reference's chaining loop (chain_demo.py:40-83) on ``rgbs[:, t_q:]``; frames before ``t_q`` are NaN.
    Room.  ``push`` splits a stream's chunk so that no slot is overwritten while a pending window can still read it: a wave appends
      at most ``min(slots, low_v + slots - T_v)`` frames to stream v; ``slots >= 9`` keeps a window plus one new frame per split.

    The state has one column per query -- those of stream 0, then of stream 1, ..., then the ones ``add_queries`` brought, in
    ``tq_host`` / ``xy_in`` / ``clip_host`` / ``hops`` on the host and in ``self.state`` on the device (``_TorchRounds`` or ``_LibraryRounds`` by
    ``rounds``: (slots + 8) output rows per query being tracked); ``columns(v)`` are the columns of stream v, in the order of its
    outputs.  ``engine="native"`` (``rounds="torch"``) needs the one-ring cache.  Same hops and the same bits under every value.

    Cover.  With ``cover`` (a ``Cover``) the queries are the cover's: every stream has a book (``books[v]``, a ``_CoverBook``) that acts
      through ``_add_queries`` / ``_remove_queries``, a caller's ``add_queries`` / ``remove_queries`` raise, and ``push`` / ``finish`` put
      ``ids``, the identity of each returned column, behind each stream's tuple.  The FIRST STEP of every stream runs inside the
      first ``push``, after every check and once the ring is made (the frame size is known then), before anything is encoded: it
      seeds frame 0.  A ``push`` then, in this order: hands each book the frames it brings (``see``, under ``seed="corners"``: their
      corner tables, one call per chunk and stream); takes ``ids``; encodes and hops; and runs a cover step (``step``) on the
      frames each stream returned, if any -- it retires and seeds for the pushes that follow.  ``finish`` runs no step.
      HELD SEEDS (``seed="corners"``): seeds whose frame was not pushed yet -- the first step's, and those of a stream that lost
      every query at once -- have no column and no identity; the ``see`` that brings their frame places them on its corners and
      adds them, with the columns and identities they would have had; ``finish`` drops them.
      CUTS (``Cover(cut_thr=)``, ONE stream: ``MultiStreamTracker`` refuses it).  After the checks and the first step the book
      looks at the pushed frames (``look``: one table call per chunk); a refused push leaves its ``prev_hist`` alone.  A push that
      holds a cut before frame ``c`` is split there: between two pieces every started query is ended on frame ``c - 1`` as the end
      of a video ends it (``_cut``: ALL its frames are returned) and retired as ``(c - 1, "cut")``, and every cell without a pending
      query is seeded on frame ``c`` (the book's ``cut``); each piece is a push of its own, tables and closing step included.  Such
      a push returns the identities alive at its start followed by those created during it (before its last piece's closing
      step), NaN where an identity had not started or was retired."""

    S = 8

    def __init__(self, model, queries_list, iters, slots, record_hops, engine, rounds, table, joint_encode=False, cover=None):
        _check_engine(engine)
        if table and engine != "torch":
            raise ValueError('engine="native" hops on one ring: pips_chain_hop_clips takes no ring size beside its clip table')
        if rounds not in ROUNDS:
            raise ValueError(f"rounds must be one of {ROUNDS}, not {rounds!r}")
        assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
        if int(slots) < self.S + 1:
            raise ValueError(f"slots must be at least {self.S + 1} (one window and a new frame), not {slots}")
        queries_list = list(queries_list)
        if not queries_list or not (table or len(queries_list) == 1):
            raise ValueError("a stream tracker needs at least one stream, and a clip table for more than one")
        self.model, self.iters, self.slots, self.engine, self.rounds = model, iters, int(slots), engine, rounds
        self.table, self.joint_encode, self.V = table, bool(joint_encode), len(queries_list)
        self._of = (lambda v: f" of stream {v}") if table else (lambda v: "")      # (for the messages)
        tqs = [_query_frames(q) for q in queries_list]
        self.tq_host = torch.cat(tqs)
        self.xy_in = torch.cat([q[0, :, 1:3] for q in queries_list])
        self.clip_host = torch.cat([torch.full((t.numel(),), v, dtype=torch.int64) for v, t in enumerate(tqs)])
        self.N = self.tq_host.numel()
        self.cache = self.size = None                                             # made by the first push: it brings the frame size
        self.finished, self.emitted = [False] * self.V, [0] * self.V                # per stream; frames [0, emitted[v]) returned
        self.hops = [[] for _ in range(self.N)] if record_hops else None          # frame steps per column (grows with T)
        self.cut_hops = None                                                      # the hop lists of a stream's columns at its last cut
        self.state = _ROUNDS[rounds](self, engine)                                # the device state, started by the first push
        self.cover = cover
        self.books = None if cover is None else [_CoverBook(cover, t, record_hops) for t in tqs]

    # the state's output rows (slots + 8, N, 2) / (slots + 8, N) and window starts (N,)
    trajs, vis, cur = (property(lambda self, k=k: getattr(self.state, k)) for k in ("trajs", "vis", "cur"))

    def stream_ids(self, v):
        """the identity of each output column of stream ``v`` of a covered tracker (host int64)"""
        return torch.tensor(self.books[v].ids, dtype=torch.int64)

    def cover_hops(self, v):
        """the hop list of each identity of stream ``v`` of a covered tracker (``record_hops=True``)"""
        return self.books[v].all_hops(self.stream_hops(v))

    def _uncovered(self, what):
        if self.cover is not None:
            raise ValueError(f"{what}() on a covered tracker: its cover adds and removes the queries")

    def columns(self, v):
        """the columns of the state that hold stream ``v``'s queries, in the order of its outputs (host int64)"""
        return torch.arange(self.N) if self.V == 1 else torch.nonzero(self.clip_host == v).squeeze(1)

    def count(self, v):
        """the number of stream ``v``'s queries"""
        return self.N if self.V == 1 else int((self.clip_host == v).sum())

    def stream_hops(self, v):
        """the frame steps of each query of stream ``v`` (``record_hops=True``)"""
        return [self.hops[c] for c in self.columns(v).tolist()]

    def frames(self, v):
        """T_v: the frames stream ``v`` has got"""
        if self.cache is None:
            return 0
        return self.cache.clip_lengths[v] if self.table else self.cache.T

    def _stream(self, v):
        if not (isinstance(v, int) and 0 <= v < self.V):
            raise ValueError(f"stream must be an int in [0, {self.V - 1}], not {v!r}")
        return v

    def add_queries(self, v, queries):
        """Further queries (1,m,3) = (t, x, y) for stream ``v`` while it runs -> the positions (m,) they take among stream ``v``'s
        output columns in the ``push`` / ``finish`` calls from now on, behind the queries already there.  ``t`` is an integer frame of
        that stream that was not returned yet (``t >= emitted[v]``; it may lie beyond the frames pushed so far): such a frame is
        still in the ring, so the new column is what a stream given the query up front returns -- NaN before ``t``, the forward
        chain from ``t`` on.  ValueError, with the tracker left as it was, for any other ``t`` and after the stream's ``finish``."""
        self._uncovered("add_queries")
        return self._add_queries(v, queries)

    def _add_queries(self, v, queries):
        v = self._stream(v)
        if self.finished[v]:
            raise ValueError(f"add_queries() after finish(){self._of(v)}")
        t = _query_frames(queries)
        if bool((t < self.emitted[v]).any()):
            raise ValueError(f"a query frame lies before frame {self.emitted[v]}{self._of(v)}: those frames were returned already")
        m, n_v = t.numel(), self.count(v)
        xy = queries[0, :, 1:3]
        self.tq_host = torch.cat([self.tq_host, t])
        self.xy_in = torch.cat([self.xy_in, xy.to(self.xy_in.device, self.xy_in.dtype)])
        self.clip_host = torch.cat([self.clip_host, torch.full((m,), v, dtype=torch.int64)])
        self.N += m
        if self.hops is not None:
            self.hops += [[] for _ in range(m)]
        if self.cache is not None and m > 0:
            self.state.grow(t, xy, m, v)
        return torch.arange(n_v, n_v + m)

    @torch.no_grad()
    def remove_queries(self, v, cols):
        """Stop tracking the queries at the positions ``cols`` (a tensor or a sequence) among stream ``v``'s output columns -> ``keep``,
        a host int64 tensor with the former position of each of that stream's columns that remains, ascending.  From this call on
        the removed queries are not hopped, do not hold back the frames of the others or the room for new frames, and have no
        column in what ``push`` / ``finish`` return: the remaining columns keep their order, ``add_queries`` puts new ones behind them,
        and ``tq_host``, ``xy_in``, ``clip_host``, ``N``, ``hops`` and the device state shrink (the state's ``keep``); the other streams are
        untouched.  ``finish`` no longer looks at a removed query: this is how one on a frame that will never come is cancelled.
        Frames of a removed query that were not returned yet are DISCARDED; frames of the remaining queries that the removed ones
        held back become final and are returned by the stream's next ``push`` / ``finish``.  Each remaining column stays what a stream
        given only the remaining queries up front returns (the clause of ``add_queries``).  Works before the first ``push``, with no
        column and with every column.  ValueError, with the tracker left as it was, for a bad stream, a position outside the
        stream's columns, a duplicate and after the stream's ``finish``."""
        self._uncovered("remove_queries")
        return self._remove_queries(v, cols)

    def _remove_queries(self, v, cols):
        v = self._stream(v)
        if self.finished[v]:
            raise ValueError(f"remove_queries() after finish(){self._of(v)}")
        mine = self.columns(v)
        cols, keep_v = _kept(cols, mine.numel(), f"the columns to remove{self._of(v)}")
        if cols.numel() == 0:
            return keep_v
        keep = keep_v if self.V == 1 else _kept(mine[cols], self.N, "the columns to remove")[1]
        self.tq_host, self.xy_in = self.tq_host[keep], self.xy_in[keep.to(self.xy_in.device)]
        self.clip_host = self.clip_host[keep]
        self.N = keep.numel()
        if self.hops is not None:
            self.hops = [self.hops[k] for k in keep.tolist()]
        if self.cache is not None:
            self.state.keep(keep)
        return keep_v

    @torch.no_grad()
    def push(self, chunks):
        """``chunks``: one ``(1,k_v,3,H,W)`` tensor (host or device, uint8 or float, 0..255; ``k_v`` may be 0) or ``None`` per stream
        -> per stream ``(f0, trajs (1,m,N_v,2), vis (1,m,N_v))``, its frames ``[f0, f0 + m)`` that became final (``m`` may be 0),
        with ``ids (N_v,)`` behind them on a covered tracker.  ValueError, ahead of the first append, for a chunk that is not
        such a tensor, another frame size and a finished stream."""
        chunks = list(chunks)
        if len(chunks) != self.V:
            raise ValueError(f"push() takes one chunk (or None) per stream: {self.V}, not {len(chunks)}")
        size = self.size
        for v, c in enumerate(chunks):                                             # every check ahead of the first append
            if c is None:
                continue
            if self.finished[v]:
                raise ValueError(f"push() after finish(){self._of(v)}")
            _check_frames(c)
            size = tuple(c.shape[3:]) if size is None else size
            if tuple(c.shape[3:]) != size:
                raise ValueError(f"frames of {tuple(c.shape[3:])} pushed to a stream of {size}")
        if self.cache is None and size is not None:
            self.size = size
            self.cache = self.model.ring_cache_videos(*size, self.slots, self.V) if self.table else self.model.ring_cache(*size, self.slots)
            self.state.start(self.cache.device)
            for v in range(self.V if self.cover is not None else 0):            # the first cover step of every stream
                cols = self.columns(v)
                self.books[v].start(*size, self.cache.device, self.tq_host[cols], self.xy_in[cols.to(self.xy_in.device)],
                                    *self._cover_acts(v))
        if self.cover is None or self.cover.cut_thr is None:
            return self._piece(chunks)
        # scene cuts.  ONE stream from here on (MultiStreamTracker takes no Cover(cut_thr=)): the frames are looked at after every
        # check and after the first step, the push is split at the cuts, and between two pieces every started query is ended
        # (``_cut``) and the book retires them and seeds the new scene (``cut``)
        assert self.V == 1
        (frames,), book = chunks, self.books[0]
        at = [] if frames is None else book.look(frames[0])
        if not at:
            return self._piece(chunks)
        parts, T0 = [], self.frames(0)
        for j, (a, b) in enumerate(zip([0] + at, at + [frames.shape[1]])):
            if j > 0:
                ids = self.stream_ids(0)
                f0, trajs, vis, keep = self._cut(0)
                parts.append((f0, trajs, vis, ids))
                book.cut(T0 + a, keep, self.cut_hops, self._cover_acts(0)[0])
            if b > a:
                parts.append(self._piece([frames[:, a:b]])[0])
        # the columns: the identities alive at the start of the push, then those created before the last piece's closing step --
        # every identity is in the part that follows its creation, and the new ones are numbered upwards
        first = parts[0][3].tolist()
        out = first + sorted({i for p in parts[1:] for i in p[3].tolist()} - set(first))
        col = torch.zeros(max(out) + 1 if out else 0, dtype=torch.int64)
        col[torch.tensor(out, dtype=torch.int64)] = torch.arange(len(out))
        return [(parts[0][0],) + _scatter(parts, col, len(out), parts[0][0]) + (torch.tensor(out, dtype=torch.int64),)]

    def _piece(self, chunks):
        """``push`` for a run of frames with no cut inside: under ``seed="corners"`` the books' tables of what it brings, the waves
        and their rounds and, on a covered tracker, the cover step on what each stream returned"""
        for v, c in enumerate(chunks if self.cover is not None and self.cover.seed == "corners" else []):
            if c is not None:
                self.books[v].see(c[0], self.emitted[v], self._cover_acts(v)[0])
        ids = None if self.cover is None else [self.stream_ids(v) for v in range(self.V)]      # (none is made before the step)
        f0, outs = list(self.emitted), [[] for _ in range(self.V)]
        left = [0 if c is None else c.shape[1] for c in chunks]
        while any(left):
            lows, wave = self.state.lows(), []
            for v, c in enumerate(chunks):
                if left[v] == 0:
                    continue
                # the room rule: the slot of frame T + j holds frame T + j - slots until then
                room = self.slots if lows[v] is None else min(self.slots, lows[v] + self.slots - self.frames(v))
                n, i = min(left[v], room), c.shape[1] - left[v]
                wave.append((v, c[:, i:i + n]))
                left[v] -= n
            if self.joint_encode:
                self.model.encode_streams(self.cache, wave, joint=True)
            else:
                for v, c in wave:
                    self.model.encode(c, into=self.cache, **({"clip": v} if self.table else {}))
            for v, rows in self._rounds(range(self.V)).items():
                outs[v].append(rows)
        res = [self._cat(v, f0[v], outs[v]) for v in range(self.V)]
        if self.cover is None:
            return res
        for v, (f, t, vi) in enumerate(res):                                       # a cover step on what each stream returned
            if t.shape[1] > 0:
                self.books[v].step(f, t[0], vi[0], *self._cover_acts(v), None if self.hops is None else self.stream_hops(v))
        return [r + (i,) for r, i in zip(res, ids)]

    def _cover_acts(self, v):
        return (lambda q: self._add_queries(v, q)), (lambda cols: self._remove_queries(v, cols))

    @torch.no_grad()
    def finish(self, v=None):
        """End stream ``v`` (-> its tuple, as ``push`` returns it: the rest of its frames) or every stream still running (-> the
        list; None for one ended before).  ValueError, ahead of any change, for a stream ended before and for a query on a frame
        beyond the stream's last."""
        which = [u for u in range(self.V) if not self.finished[u]] if v is None else [self._stream(v)]
        for u in which:                                                             # every check ahead of the first change
            if self.finished[u]:
                raise ValueError(f"finish(){self._of(u)} called twice")
            T = self.frames(u)
            if bool((self.tq_host[self.clip_host == u] > T - 1).any()):
                raise ValueError(f"a query frame lies beyond the last frame{self._of(u)} ({T - 1})")
        f0, outs = list(self.emitted), {}
        for u in which:
            self.finished[u] = True
            if self.cover is not None:
                self.books[u].held = None          # (seeds held for a frame that never comes)
            if self.cache is not None:
                self.state.end(u)
        if self.cache is not None and which:
            outs = self._rounds(which)
        res = [self._cat(u, f0[u], [outs[u]] if u in outs else []) if u in which else None for u in range(self.V)]
        if self.cover is not None:                                                  # (no cover step at the end of a stream)
            res = [None if r is None else r + (self.stream_ids(u),) for u, r in enumerate(res)]
        return res if v is None else res[v]

    @torch.no_grad()
    def _cut(self, v):
        """End every query of stream ``v`` that has started, at the ``T_v`` frames pushed so far, and keep the stream open -> ``(f0,
        trajs (1,m,N_v,2), vis (1,m,N_v), keep)``: the rounds run with the stream marked as ended (windows that reach past frame
        ``T_v - 1`` repeat it), ALL its frames ``[f0, T_v)`` not returned yet come back in the columns as they were at the call, the
        queries with ``t < T_v`` are removed (``remove_queries``: state, rows and hop lists shrink) and the mark is taken back.
        ``keep`` holds the former position of each column that remains -- the queries with ``t >= T_v``, which stay waiting,
        untouched: on later pushes such a query is what a stream that starts at frame ``T_v`` returns for it, since a forward
        window never reads below its start.  ``cut_hops`` is, with ``record_hops``, the hop list of each of the stream's columns as
        it was at the last cut (None otherwise).  Before the first push no frame is returned and nothing is removed.  ValueError,
        with the tracker left as it was, after the stream's ``finish``."""
        if self.finished[v]:
            raise ValueError(f"cut() after finish(){self._of(v)}")
        self.cut_hops = None if self.hops is None else self.stream_hops(v)
        mine, f0 = self.columns(v), self.emitted[v]
        if self.cache is None:
            return self._cat(v, f0, []) + (torch.arange(mine.numel()),)
        self.state.end(v)
        outs = self._rounds([v])
        self.state.end(v, False)
        started = torch.nonzero(self.tq_host[mine] < self.frames(v)).squeeze(1)
        return self._cat(v, f0, list(outs.values())) + (self._remove_queries(v, started),)

    def _rounds(self, which):
        """the state's hop rounds over every stream, their steps recorded per column -> {v: the rows of the frames of stream v that
        became final} for the streams ``which`` that had any (another stream's stay in the ring until it is asked)"""
        for active, steps in self.state.run():
            if self.hops is not None:
                for q, h in zip(active.tolist(), steps.tolist()):
                    self.hops[q].append(h)
        lows, outs = self.state.lows(), {}
        for v in which:
            T = self.frames(v)
            f1 = T if lows[v] is None else min(lows[v], T)
            if f1 > self.emitted[v]:
                outs[v] = self.state.emit(self.emitted[v], f1, self.columns(v))
                self.emitted[v] = f1
        return outs

    def _cat(self, v, f0, outs):
        if not outs:
            dev = self.cache.device if self.cache is not None else self.xy_in.device
            return f0, torch.empty(1, 0, self.count(v), 2, device=dev), torch.empty(1, 0, self.count(v), device=dev)
        return f0, torch.cat([o[0] for o in outs]).unsqueeze(0), torch.cat([o[1] for o in outs]).unsqueeze(0)


class StreamTracker:
    """One video that arrives in chunks: the one-stream form of ``_StreamCore`` on the one ring of ``Pips.ring_cache`` (no clip table),
    whose docstring states the rules -- readiness, joining, when a frame is final, the room of a push.

    queries (1,N,3) = (t, x, y) as for ``track_queries``; ``t`` may lie beyond the frames pushed so far.  ``push(frames)`` takes the
    next ``(1,k,3,H,W)`` frames and returns ``(f0, trajs (1,m,N,2), vis (1,m,N))`` for the frames ``[f0, f0+m)`` that became final;
    ``finish()`` ends the video and returns the rest; ``add_queries(queries)`` / ``remove_queries(cols)`` / ``cut()`` are the core's
    ``add_queries`` / ``remove_queries`` / ``_cut`` for stream 0, in columns of the outputs.  ``rounds="torch"`` (the default) makes a
    ``model.track`` call per round or, with ``engine="native"``, one ``pips_chain_hop`` call; under ``rounds="library"`` a round is ONE
    ``pips_stream_round`` call and ``engine`` is not looked at."""

    S = 8

    def __init__(self, model, queries, iters=6, slots=24, record_hops=False, engine="torch", rounds="torch", _cover=None):
        self.core = _StreamCore(model, [queries], iters, slots, record_hops, engine, rounds, table=False, cover=_cover)

    model, iters, slots, engine, rounds, tq_host, xy_in, N, hops, cut_hops, cache, size, state, trajs, vis, cur = (
        property(lambda self, k=k: getattr(self.core, k)) for k in (
            "model", "iters", "slots", "engine", "rounds", "tq_host", "xy_in", "N", "hops", "cut_hops", "cache", "size", "state", "trajs",
            "vis", "cur"))
    emitted, finished = (property(lambda self, k=k: getattr(self.core, k)[0]) for k in ("emitted", "finished"))

    def add_queries(self, queries):
        return self.core.add_queries(0, queries)

    def remove_queries(self, cols):
        return self.core.remove_queries(0, cols)

    def push(self, frames):
        return self.core.push([frames])[0]

    def finish(self):
        return self.core.finish(0)

    def cut(self):
        self.core._uncovered("cut")
        return self.core._cut(0)


@torch.no_grad()
def track_stream(model, chunks, queries, iters=6, slots=24, return_hops=False, engine="torch", rounds="torch"):
    """``StreamTracker`` over an iterable of ``(1,k,3,H,W)`` chunks -> trajs_e (1,T,N,2) px and vis_e (1,T,N) logits, NaN
    before each query's frame.  ``return_hops=True``: also, per query, the frame steps of its windows.  ``engine`` / ``rounds``:
    see ``StreamTracker``."""
    st = StreamTracker(model, queries, iters=iters, slots=slots, record_hops=return_hops, engine=engine, rounds=rounds)
    return _joined([st.push(c) for c in chunks] + [st.finish()], None, st.hops, return_hops)


def _joined(parts, book, hops, return_hops):
    """the parts one stream's pushes and its ``finish`` returned as ONE result: their rows behind one another -> (trajs, vis), or
    with the ``book`` of a covered stream by identity (``_by_identity``) -> (trajs, vis, born, retired); ``hops`` behind them when asked"""
    out = (torch.cat([p[1] for p in parts], dim=1), torch.cat([p[2] for p in parts], dim=1)) if book is None else _by_identity(parts, book)
    return out + (hops,) if return_hops else out


# ---------------------------------------------------------------------------------------------- keeping the frame covered
COVER_SCANS = ("torch", "library")
COVER_SEEDS = ("centre", "corners")


def _whole(x, what, low):
    """x as an int; ValueError unless it is a whole number >= low (a bool is not a number here)"""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x or x in (float("inf"), float("-inf")) or int(x) != x \
            or int(x) < low:
        raise ValueError(f"{what} must be an integer >= {low}, not {x!r}")
    if int(x) > _INT_MAX:
        raise ValueError(f"{what} must fit an int32, not {x!r}")
    return int(x)


class Cover:
    """The policy of a tracker that decides itself which queries it tracks (``CoverTracker``, ``MultiStreamTracker(cover=)``): a grid
    of ``cell`` x ``cell`` pixel cells lies over the frame, and after every push that returned frames a COVER STEP
      * retires a started query as "outside" unless its position on the last returned frame has 0 <= x <= W-1 and 0 <= y <= H-1
        (NaN and infinities retire), and otherwise as "lost" when its visibility logit stayed below ``logit(vis_thr)`` for
        ``lost_after`` returned frames in a row (``None``: never) -- the run is carried from push to push;
      * keeps every other query, and every query whose frame was not returned yet (pending) on its query position;
      * seeds one new query on the next frame at the centre of every cell that holds no kept or pending query, in row-major
        order, as long as the stream has fewer than ``max_queries`` (``None``: no cap).
    The full rule is pips_cover_step's in include/pips_hip.h.  ``scan="torch"`` performs the step as torch ops (``cover_scan``; it
    also runs on CPU tensors); ``scan="library"`` makes one ``pips_cover_step`` call and reads its four counts -- the kept list and
    the seeds come to the host only when the counts say that something changed.  Both give the same queries and the same bits.
    ``seed="corners"`` moves each seed from the centre of its cell to the most trackable pixel of that cell on the seed's own frame
    -- the largest smaller eigenvalue of the 7x7 structure tensor of the 8-bit luma, the integer rule of pips_corner_table in
    include/pips_hip.h -- where that score is above ``min_corner`` (a whole number >= 0); a cell that is flat by that measure keeps
    the centre, so which cells are seeded, how many and in which order stay what ``seed="centre"`` (the default) gives.  The table
    of best corners comes from ``corner_table_torch`` / ``cover_place_torch`` under ``scan="torch"`` and from one ``pips_corner_table``
    call per pushed chunk and one ``pips_cover_place`` call per step under ``scan="library"``: the same bits again.  With an
    unweighted window the chosen pixel of a sharp corner lies about 2 px inside it.
    ``per_cell=k`` (``None``, the default: no cap, the step described so far and its calls) caps the tracks of a cell: tracks that
    lose their surface slide onto a neighbour and ride along with it, and a query that, on ``crowd_after`` returned frames in a
    row, stood in a cell with at least ``k`` older started queries is retired as "crowded" -- the youngest go, the run is carried
    from push to push, and the step is ``cover_scan_thin`` / one ``pips_cover_step_thin`` call (the THIN step; its full rule is in
    include/pips_hip.h).  The cap is per cell, not per distance: two tracks 1 px apart on either side of a cell border both stay.
    ``cut_thr=x`` (``None``, the default: no frame is looked at and every path is the one described so far) ends the tracks at scene
    cuts: a cut lies before a pushed frame whose regional luma histogram differs from that of the frame before by more than
    ``cut_limit(x, H, W)`` (``cut_table_torch`` / one ``pips_cut_table`` call per pushed chunk, by ``scan``: the same integers).  A
    ``CoverTracker`` splits a push there, ends every started query as "cut" on the last frame of the old scene (the core's ``_cut``)
    and seeds every cell of the new scene's first frame.  0.5 is a reasonable value, not a tuned one: on one 640 x 360 video with fast
    motion consecutive frames stayed below 0.15 and frames 64 apart below 0.45, a frame against its negative reached 0.6."""

    def __init__(self, cell=32, vis_thr=0.5, lost_after=4, max_queries=None, scan="torch", seed="centre", min_corner=0, per_cell=None,
                 crowd_after=4, cut_thr=None):
        self.cell = _whole(cell, "cell", 8)
        if isinstance(vis_thr, bool) or not isinstance(vis_thr, (int, float)) or not 0.0 < vis_thr < 1.0:
            raise ValueError(f"vis_thr must lie in (0, 1), not {vis_thr!r}")
        self.vis_thr = float(vis_thr)
        # computed once, on the host, as fp32: no exp on the device, and both scans compare against the same bits
        self.vis_logit = float(torch.logit(torch.tensor(self.vis_thr, dtype=torch.float32)))
        self.lost_after = None if lost_after is None else _whole(lost_after, "lost_after", 1)
        self.max_queries = None if max_queries is None else _whole(max_queries, "max_queries", 0)
        if scan not in COVER_SCANS:
            raise ValueError(f"scan must be one of {COVER_SCANS}, not {scan!r}")
        self.scan = scan
        if not isinstance(seed, str) or seed not in COVER_SEEDS:
            raise ValueError(f"seed must be one of {COVER_SEEDS}, not {seed!r}")
        self.seed = seed
        self.min_corner = _whole(min_corner, "min_corner", 0)
        self.per_cell = None if per_cell is None else _whole(per_cell, "per_cell", 1)
        self.crowd_after = _whole(crowd_after, "crowd_after", 1)
        if cut_thr is not None and (isinstance(cut_thr, bool) or not isinstance(cut_thr, (int, float)) or not 0.0 < cut_thr < 1.0):
            raise ValueError(f"cut_thr must be None or lie in (0, 1), not {cut_thr!r}")
        self.cut_thr = None if cut_thr is None else float(cut_thr)

    def cut_table(self, frames, prev_hist=None, dev=None):
        """the regional luma histograms of the frames (F,3,H,W) and their distances (``cut_table_torch``'s rule) by the chosen scan
        -> (hist (F,16,32), dist (F,)) on ``dev`` (None: where the frames lie; the GPU under ``scan="library"``)"""
        if self.scan == "library":
            return ops.cut_table(frames if frames.is_cuda else frames.to("cuda" if dev is None else dev), prev_hist)
        return cut_table_torch(frames if dev is None else frames.to(dev), prev_hist)

    def grid(self, H, W):
        """(rows, columns) of the cells over an H x W frame"""
        return (H - 1) // self.cell + 1, (W - 1) // self.cell + 1

    def table(self, frames, dev=None):
        """the best corner of each cell of each of the frames (F,3,H,W), uint8 or float 0..255, by the chosen scan -> (F,gh,gw,3) =
        (x, y, score) on ``dev`` (None: where the frames lie; the GPU under ``scan="library"``).  Host frames are copied to ``dev`` once"""
        if self.scan == "library":
            return ops.corner_table(frames if frames.is_cuda else frames.to("cuda" if dev is None else dev), self.cell)
        return corner_table_torch(frames if dev is None else frames.to(dev), self.cell)

    def place(self, seeds, table, H, W):
        """the seeds (k,3) of a cover step on the frame whose table (gh,gw,3) this is, by the chosen scan -> the seeds on their
        corners (``scan="library"`` moves them in place)"""
        if self.scan == "library":
            return ops.cover_place(seeds.contiguous(), table, H, W, self.cell, self.min_corner)
        return cover_place_torch(seeds, table, H, W, self.cell, self.min_corner)

    def step(self, trajs, vis, f1, tq, xy, lost, crowd, H, W):
        """one cover step by the chosen scan and policy -> (keep (n_keep) ints, lost_out (n_keep) int32, crowd_out (n_keep) int32 or
        None, seeds (n_seed,3), gone, why, counts): ``gone`` are the retired columns, ascending, and ``why`` their reasons ("outside" /
        "lost" / "crowded"), both host lists; ``counts`` [n_keep, n_seed, n_outside, n_lost(, n_crowded)] on the host.  trajs (m,n,2) /
        vis (m,n) are the rows of frames [f1 - m, f1), tq / lost (n) int32, xy (n,2).  Without ``per_cell`` it is ``cover_scan`` or one
        ``pips_cover_step`` call and ``crowd`` is not looked at; with it, ``crowd`` (n) int32 is the second run and the step is
        ``cover_scan_thin`` or one ``pips_cover_step_thin`` call.  The counts are the one host read; who went and why comes over only
        when they say that somebody did -- the thin step's own lists, or the kept list and the goners' last row, which tell
        "outside" from "lost" by the step's inside test"""
        n, thin, library = tq.numel(), self.per_cell is not None, self.scan == "library"
        caps = (_INT_MAX if self.lost_after is None else self.lost_after, _INT_MAX if self.max_queries is None else self.max_queries)
        if thin:
            keep, lost_out, crowd_out, seeds, gone, reason, counts = (ops.cover_step_thin if library else cover_scan_thin)(
                trajs, vis, f1, tq, xy, lost, crowd, H, W, self.cell, self.vis_logit, *caps, self.per_cell, self.crowd_after)
        else:
            keep, lost_out, seeds, counts = (ops.cover_step if library else cover_scan)(
                trajs, vis, f1, tq, xy, lost, H, W, self.cell, self.vis_logit, *caps)
        if library:
            counts = counts.tolist()                                              # the one host read
        k, went, why = counts[0], [], []
        if k < n and thin:
            went, why = gone[:n - k].tolist(), [COVER_REASONS[r] for r in reason[:n - k].tolist()]
        elif k < n:
            went = sorted(set(range(n)) - set(keep[:k].tolist()))
            x, y = trajs[-1][torch.tensor(went, device=trajs.device)].to("cpu").unbind(1)
            why = ["lost" if ok else "outside" for ok in ((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)).tolist()]
        assert len(went) == n - k and [why.count(r) for r in COVER_REASONS[1:len(counts) - 1]] == counts[2:]
        return keep[:k], lost_out[:k], crowd_out[:k] if thin else None, seeds[:counts[1]], went, why, counts


def cover_scan(trajs, vis, f1, tq, xy, lost, H, W, cell, vis_logit, lost_after, max_queries):
    """The cover step (pips_cover_step, include/pips_hip.h) as torch ops, on any device -> (keep (n_keep) int32 ascending, lost_out
    (n_keep) int32, seeds (n_seed,3) = (t, x, y), [n_keep, n_seed, n_outside, n_lost]).  trajs (m,n,2) / vis (m,n): the rows of
    frames [f1 - m, f1); tq / lost (n) int32; xy (n,2); the inputs are left as they were."""
    n, m, dev = tq.numel(), vis.shape[0], xy.device
    gh, gw = (H - 1) // cell + 1, (W - 1) // cell + 1
    pending = (tq > f1 - 1) if m > 0 else torch.ones(n, dtype=torch.bool, device=dev)
    run, zero = lost.to(torch.int32), torch.zeros(n, dtype=torch.int32, device=dev)
    for g in range(m):                                                            # the run over the frames from t_q on, in order
        on = ~pending & (tq <= f1 - m + g)
        run = torch.where(on, torch.where(vis[g] < vis_logit, run + 1, zero), run)      # (a NaN compares false: the run restarts)
    run = torch.where(pending, zero, run)
    pos = torch.where(pending.unsqueeze(1), xy, trajs[m - 1]) if m > 0 else xy
    x, y = pos[:, 0], pos[:, 1]
    inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)                    # written so that NaN and +-inf fail it
    outside = ~pending & ~inside
    gone = ~pending & inside & (run >= lost_after)
    kept = ~(outside | gone)
    keep = torch.nonzero(kept).squeeze(1)
    stand = kept & inside                                                         # (a pending query outside the frame: no cell)
    i = torch.div(torch.where(stand, y, torch.zeros_like(y)), float(cell)).floor().to(torch.int64).clamp(max=gh - 1)
    j = torch.div(torch.where(stand, x, torch.zeros_like(x)), float(cell)).floor().to(torch.int64).clamp(max=gw - 1)
    occ = torch.zeros(gh * gw, dtype=torch.bool, device=dev)
    occ[(i * gw + j)[stand]] = True
    empty = torch.nonzero(~occ).squeeze(1)[:max(max_queries - keep.numel(), 0)]
    sx = ((empty % gw).to(torch.float32) + 0.5) * cell
    sy = (torch.div(empty, gw, rounding_mode="floor").to(torch.float32) + 0.5) * cell
    seeds = torch.stack([torch.full_like(sx, float(f1)), sx.clamp(max=float(W - 1)), sy.clamp(max=float(H - 1))], dim=1)
    return keep.to(torch.int32), run[keep], seeds, [keep.numel(), empty.numel(), int(outside.sum()), int(gone.sum())]


COVER_REASONS = ("kept", "outside", "lost", "crowded")                           # pips_cover_step_thin's `reason` values


def cover_scan_thin(trajs, vis, f1, tq, xy, lost, crowd, H, W, cell, vis_logit, lost_after, max_queries, per_cell, crowd_after):
    """The thin cover step (pips_cover_step_thin, include/pips_hip.h) as torch ops, on any device -> (keep (n_keep) int32 ascending,
    lost_out, crowd_out (n_keep) int32, seeds (n_seed,3) = (t, x, y), gone (n - n_keep) int32 ascending, reason (n - n_keep) int32 =
    1 outside / 2 lost / 3 crowded, [n_keep, n_seed, n_outside, n_lost, n_crowded]).  ``crowd`` (n) int32 is the second run; the
    other arguments are ``cover_scan``'s; the inputs are left as they were.  Not greedy: an elder counts in its cell even when it
    is itself retired as crowded in this step.  (A row is ranked through an n x n comparison.)"""
    n, m, dev = tq.numel(), vis.shape[0], xy.device
    gh, gw = (H - 1) // cell + 1, (W - 1) // cell + 1
    pending = (tq > f1 - 1) if m > 0 else torch.ones(n, dtype=torch.bool, device=dev)
    run, zero = lost.to(torch.int32), torch.zeros(n, dtype=torch.int32, device=dev)
    for g in range(m):                                                            # the run `lost`: cover_scan's
        on = ~pending & (tq <= f1 - m + g)
        run = torch.where(on, torch.where(vis[g] < vis_logit, run + 1, zero), run)
    run = torch.where(pending, zero, run)
    pos = torch.where(pending.unsqueeze(1), xy, trajs[m - 1]) if m > 0 else xy

    def judge(p):                                                                 # the inside test and the cell where it passes
        x, y = p[:, 0], p[:, 1]
        ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)                    # written so that NaN and +-inf fail it
        i = torch.div(torch.where(ok, y, torch.zeros_like(y)), float(cell)).floor().to(torch.int64).clamp(max=gh - 1)
        j = torch.div(torch.where(ok, x, torch.zeros_like(x)), float(cell)).floor().to(torch.int64).clamp(max=gw - 1)
        return ok, i * gw + j

    inside, at = judge(pos)
    outside = ~pending & ~inside
    lostq = ~pending & inside & (run >= lost_after)
    col = torch.arange(n, device=dev)
    elder = col.unsqueeze(0) < col.unsqueeze(1)                                   # [j, i]: i is older than j
    crun = crowd.to(torch.int32)
    for g in range(m):                                                            # the second run: surplus on each returned frame
        on = ~pending & (tq <= f1 - m + g)
        ok, cid = judge(trajs[g])
        counts_here = on & ~outside & ~lostq & ok
        cid = torch.where(counts_here, cid, torch.full_like(cid, -1))
        older = ((cid.unsqueeze(1) == cid.unsqueeze(0)) & elder & counts_here.unsqueeze(0)).sum(dim=1)
        surplus = counts_here & (older >= per_cell)
        crun = torch.where(on, torch.where(surplus, crun + 1, zero), crun)
    crun = torch.where(pending, zero, crun)
    crowded = ~pending & ~outside & ~lostq & (crun >= crowd_after)
    kept = ~(outside | lostq | crowded)
    keep, gone = torch.nonzero(kept).squeeze(1), torch.nonzero(~kept).squeeze(1)
    stand = kept & inside                                                         # (a pending query outside the frame: no cell)
    occ = torch.zeros(gh * gw, dtype=torch.bool, device=dev)
    occ[at[stand]] = True
    empty = torch.nonzero(~occ).squeeze(1)[:max(max_queries - keep.numel(), 0)]
    sx = ((empty % gw).to(torch.float32) + 0.5) * cell
    sy = (torch.div(empty, gw, rounding_mode="floor").to(torch.float32) + 0.5) * cell
    seeds = torch.stack([torch.full_like(sx, float(f1)), sx.clamp(max=float(W - 1)), sy.clamp(max=float(H - 1))], dim=1)
    reason = (outside.to(torch.int32) + 2 * lostq.to(torch.int32) + 3 * crowded.to(torch.int32))[gone]
    return (keep.to(torch.int32), run[keep], crun[keep], seeds, gone.to(torch.int32), reason,
            [keep.numel(), empty.numel(), int(outside.sum()), int(lostq.sum()), int(crowded.sum())])


def corner_table_torch(frames, cell):
    """pips_corner_table (include/pips_hip.h) as int64 torch ops, on any device: frames (F,3,h,w), uint8 or float 0..255 -> table
    (F,gh,gw,3) float32 = (x, y, S), the candidate with the largest S of each cell -- the lowest y, then the lowest x among equals --
    or the cell's centre and -1 where a cell has no candidate.  Integer arithmetic up to the argmax: the same bits as the kernel."""
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames must be (F,3,h,w), not {tuple(frames.shape)}")
    cell = int(cell)
    F, _, h, w = frames.shape
    gh, gw, dev = (h - 1) // cell + 1, (w - 1) // cell + 1, frames.device
    key = torch.full((F, gh * cell, gw * cell), -1, dtype=torch.int64, device=dev)      # -1: no candidate
    if F > 0 and h >= 9 and w >= 9:
        if frames.dtype == torch.uint8:
            u = frames.to(torch.int64)
        else:                                           # (as ops.corner_table: anything but uint8 goes through float32)
            u = (frames.to(torch.float32).clamp(0.0, 255.0) + 0.5).floor().to(torch.int64)
        Y = (77 * u[:, 0] + 150 * u[:, 1] + 29 * u[:, 2] + 128) >> 8
        gx = Y[:, 1:-1, 2:] - Y[:, 1:-1, :-2]                                          # pixel (y, x) at [y - 1, x - 1]
        gy = Y[:, 2:, 1:-1] - Y[:, :-2, 1:-1]

        def window(p):                                                                # 7x7 sums: pixel (y, x) at [y - 4, x - 4]
            p = sum(p[:, :, k:k + w - 8] for k in range(7))
            return sum(p[:, k:k + h - 8] for k in range(7))

        a, b, c = window(gx * gx), window(gx * gy), window(gy * gy)
        d = (a - c) ** 2 + 4 * b * b                                                   # < 2^53: exact as a double
        r = d.to(torch.float64).sqrt().to(torch.int64)
        r = torch.where(r * r > d, r - 1, r)
        r = torch.where((r + 1) * (r + 1) <= d, r + 1, r)                             # floor(sqrt(d)), exactly
        S = a + c - (r + (r * r < d).to(torch.int64))
        ys = torch.arange(4, h - 4, device=dev).unsqueeze(1)
        xs = torch.arange(4, w - 4, device=dev).unsqueeze(0)
        # S above the complement of the pixel's index: one max per cell picks the largest S, then the lowest y, then the lowest x
        key[:, 4:h - 4, 4:w - 4] = (S << 32) | (0xFFFFFFFF - (ys * w + xs))
    best = key.view(F, gh, cell, gw, cell).permute(0, 1, 3, 2, 4).reshape(F, gh, gw, cell * cell).amax(dim=3)
    at = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    i = torch.arange(gh, device=dev, dtype=torch.float32).view(1, gh, 1).expand(F, gh, gw)
    j = torch.arange(gw, device=dev, dtype=torch.float32).view(1, 1, gw).expand(F, gh, gw)
    none = best < 0
    x = torch.where(none, ((j + 0.5) * cell).clamp(max=float(w - 1)), (at % w).to(torch.float32))
    y = torch.where(none, ((i + 0.5) * cell).clamp(max=float(h - 1)), torch.div(at, w, rounding_mode="floor").to(torch.float32))
    return torch.stack([x, y, torch.where(none, torch.full_like(x, -1.0), (best >> 32).to(torch.float32))], dim=3)


def cut_limit(cut_thr, h, w):
    """the largest distance that is no cut: floor(cut_thr * 2 h w), computed once on the host in double"""
    return int(math.floor(float(cut_thr) * (2 * int(h) * int(w))))


def cut_table_torch(frames, prev_hist=None):
    """pips_cut_table (include/pips_hip.h) as int64 torch ops, on any device: frames (F,3,h,w), uint8 or float 0..255 -> (hist
    (F,16,32), dist (F,)) int64.  hist[f][r][b] counts the pixels of frame f in region r = 4 ((4y)/h) + (4x)/w whose 8-bit luma Y
    (``corner_table_torch``'s) has Y >> 3 == b; dist[f] is the sum of |hist[f] - hist[f-1]|, frame 0 against ``prev_hist`` (16,32)
    or 0 without it.  Integers throughout: equal to the kernel's."""
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames must be (F,3,h,w), not {tuple(frames.shape)}")
    F, _, h, w = frames.shape
    dev = frames.device
    if h < 1 or w < 1 or h * w > 2 ** 30:
        raise ValueError(f"frames of {h} x {w}: need at least 1 x 1 and at most 2^30 pixels")
    if prev_hist is not None and (tuple(prev_hist.shape) != (16, 32) or prev_hist.is_floating_point()):
        raise ValueError(f"prev_hist must be a (16,32) integer tensor, not {tuple(prev_hist.shape)} {prev_hist.dtype}")
    if frames.dtype == torch.uint8:
        u = frames.to(torch.int64)
    else:                                               # (as ops.cut_table: anything but uint8 goes through float32)
        u = (frames.to(torch.float32).clamp(0.0, 255.0) + 0.5).floor().to(torch.int64)
    Y = (77 * u[:, 0] + 150 * u[:, 1] + 29 * u[:, 2] + 128) >> 8
    ry = torch.div(4 * torch.arange(h, device=dev), h, rounding_mode="floor")
    rx = torch.div(4 * torch.arange(w, device=dev), w, rounding_mode="floor")
    key = 512 * torch.arange(F, device=dev).view(F, 1, 1) + 32 * (4 * ry.view(1, h, 1) + rx.view(1, 1, w)) + (Y >> 3)
    hist = torch.bincount(key.reshape(-1), minlength=512 * F).view(F, 16, 32)
    if F == 0:
        return hist, hist.new_zeros(0)
    first = hist[:1] if prev_hist is None else prev_hist.to(dev, torch.int64).view(1, 16, 32)
    return hist, (hist - torch.cat([first, hist[:-1]])).abs().sum(dim=(1, 2))


# pips_frames_import's constants (include/pips_hip.h; pips_amd/csrc/yuv.h): (y0, ky, rv, gu, gv, bu) by (matrix, range)
YUV_RULES = {
    ("bt601", "limited"): (16, 76309, 104597, -25675, -53279, 132201),
    ("bt601", "full"): (0, 65536, 91881, -22553, -46802, 116130),
    ("bt709", "limited"): (16, 76309, 117489, -13975, -34925, 138438),
    ("bt709", "full"): (0, 65536, 103206, -12276, -30679, 121609),
}


# the 10-bit formats' (P010, I010: samples 0..1023, y0 = 64, chroma centred on 512, constants scaled by 2^18)
YUV10_RULES = {
    ("bt601", "limited"): (64, 76309, 104597, -25675, -53279, 132201),
    ("bt601", "full"): (0, 65344, 91612, -22487, -46664, 115789),
    ("bt709", "limited"): (64, 76309, 117489, -13975, -34925, 138438),
    ("bt709", "full"): (0, 65344, 102903, -12240, -30589, 121252),
}


def triangle_taps(n, N, device=None):
    """PIPS_FILTER_TRIANGLE along one axis of ``n`` source and ``N`` output samples -> (idx, wgt) int64 (N, T): output i sums
    ``wgt[i, t] * p[idx[i, t]]`` and divides by ``wgt[i].sum()``.  The raw weight of source j is
    max(0, 2 m - |(2 j + 1) N - (2 i + 1) n|), m = max(n, N), 0 <= j < n; T is the most positive weights of any output, and the
    entries behind an output's last tap have weight 0 (and a clamped index)."""
    m2 = 2 * max(n, N)
    i = torch.arange(N, dtype=torch.int64, device=device)
    lo = (torch.div((2 * i + 1) * n - m2 - N, 2 * N, rounding_mode="floor") + 1).clamp(min=0)
    T = 2 * (max(n, N) // N) + 2
    idx = lo.view(N, 1) + torch.arange(T, dtype=torch.int64, device=device).view(1, T)
    wgt = (m2 - ((2 * idx + 1) * N - (2 * i.view(N, 1) + 1) * n).abs()).clamp(min=0)
    wgt = torch.where(idx < n, wgt, torch.zeros_like(wgt))
    keep = int((wgt > 0).any(dim=0).sum())                                       # (the positive weights of a row are its first ones)
    return idx.clamp(max=n - 1)[:, :keep], wgt[:, :keep]


def import_frames_torch(planes, fmt, size=None, matrix="bt709", range="limited", dtype=torch.uint8, antialias=False):
    """pips_frames_import_ex (include/pips_hip.h) as torch ops, on any device: ``ops.import_frames``' arguments -> planar frames
    (F,3,H,W), uint8 or float32.  The conversion is int64 arithmetic -- packed formats pick their bytes, the YCbCr formats replicate
    a chroma sample to its 2 x 2 pixels and apply the fixed-point matrix of ``YUV_RULES`` (``YUV10_RULES`` for p010 and i010) -- and
    the resize to ``size`` is the kernel's fp32 arithmetic as elementwise ops in its order (the source index one fused multiply-add,
    every product and sum of the blend a separate, single-rounded op), or with ``antialias=True`` the triangle filter in integers:
    two contractions with ``triangle_taps``' weights and one division.  Equal to the kernels bit for bit."""
    planes, F, h, w = ops.import_planes(planes, fmt)
    if matrix not in ops.IMPORT_MATRICES or range not in ops.IMPORT_RANGES:
        raise ValueError(f"matrix must be one of {sorted(ops.IMPORT_MATRICES)} and range one of {sorted(ops.IMPORT_RANGES)}, "
                         f"not {matrix!r}, {range!r}")
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"dtype must be torch.uint8 or torch.float32, not {dtype}")
    H, W = ops.import_size(size, h, w, antialias)
    dev = planes[0].device
    if fmt in ("nv12", "i420", "p010", "i010"):
        if fmt in ("nv12", "p010"):
            cb, cr = planes[1][..., 0], planes[1][..., 1]
        else:
            cb, cr = planes[1], planes[2]
        Y, cb, cr = (c.to(torch.int64) for c in (planes[0], cb, cr))
        if fmt == "p010":                               # the high ten bits of the word (planes: int16 views of the bits)
            Y, cb, cr = ((c & 0xFFFF) >> 6 for c in (Y, cb, cr))
        elif fmt == "i010":                             # the low ten
            Y, cb, cr = (c & 1023 for c in (Y, cb, cr))
        iy, ix = torch.arange(h, device=dev) >> 1, torch.arange(w, device=dev) >> 1
        cb, cr = (c[:, iy][:, :, ix] for c in (cb, cr))
        if fmt in ops.IMPORT_16BIT:
            (y0, ky, rv, gu, gv, bu), mid, shift = YUV10_RULES[(matrix, range)], 512, 18
        else:
            (y0, ky, rv, gu, gv, bu), mid, shift = YUV_RULES[(matrix, range)], 128, 16
        c, d, e = ky * (Y - y0) + (1 << (shift - 1)), cb - mid, cr - mid
        rgb = torch.stack([(c + rv * e) >> shift, (c + gu * d + gv * e) >> shift, (c + bu * d) >> shift], dim=1).clamp(0, 255)
    else:
        order = [2, 1, 0] if fmt in ("bgr24", "bgra32") else [0, 1, 2]
        rgb = planes[0][..., order].permute(0, 3, 1, 2).to(torch.int64)
    if (H, W) == (h, w):
        return rgb.to(dtype)
    if antialias:
        (jx, wx), (jy, wy) = triangle_taps(w, W, dev), triangle_taps(h, H, dev)
        rows = sum(rgb[..., j] * r for j, r in zip(jx.unbind(1), wx.unbind(1)))                        # (F,3,h,W): sum_x rx p < 2^27
        num = sum(rows[:, :, j] * r.view(H, 1) for j, r in zip(jy.unbind(1), wy.unbind(1)))            # (F,3,H,W): < 2^46
        den = wy.sum(dim=1).view(H, 1) * wx.sum(dim=1).view(1, W)
        q = torch.div(512 * num + den, 2 * den, rounding_mode="floor")                                 # 8.8 fixed point, half up
        return q.to(torch.float32) / 256.0 if dtype == torch.float32 else ((q + 128) >> 8).to(torch.uint8)

    def taps(n, N):                                     # resize_frames_kernel's source index, second tap and weights along one axis
        s = torch.tensor(float(n), dtype=torch.float32, device=dev) / torch.tensor(float(N), dtype=torch.float32, device=dev)
        # the kernel's one fused multiply-add: in float64 the product of a float32 and of i + 0.5 (i < 2^24) and its difference to
        # 0.5 are exact, so the one rounding to float32 is the fused one
        f = (s.double() * (torch.arange(N, device=dev).double() + 0.5) - 0.5).to(torch.float32).clamp(min=0.0)
        i0 = f.to(torch.int64).clamp(max=n - 1)
        i1 = i0 + (i0 < n - 1).to(torch.int64)
        l1 = f - i0.to(torch.float32)
        return i0, i1, 1.0 - l1, l1

    y0, y1, ly0, ly1 = taps(h, H)
    x0, x1, lx0, lx1 = taps(w, W)
    p = rgb.to(torch.float32)
    ly0, ly1 = ly0.view(H, 1), ly1.view(H, 1)
    r0, r1 = p[:, :, y0], p[:, :, y1]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    v = ly0 * top + ly1 * bot
    return v if dtype == torch.float32 else (v + 0.5).floor().to(torch.uint8)


def import_frames(planes, fmt, size=None, matrix="bt709", range="limited", dtype=torch.uint8, device=None, antialias=False):
    """A decoder's frames -> rgbs (1,F,3,H,W), ready for ``Pips.encode``, ``StreamTracker.push``, ``CoverTracker.push`` and
    ``MultiStreamTracker.push``: ``ops.import_frames`` (one ``pips_frames_import_ex`` launch; its docstring has the formats) on planes
    that may still lie on the host.  Host planes are copied to ``device`` (default "cuda") in their SOURCE format and converted
    there: an NV12 chunk crosses the bus at 1.5 bytes per pixel, where frames converted on the CPU cost 3.  ``size`` = (H, W)
    resizes to the model's size in the same launch, with ``antialias=True`` through the triangle filter instead of the two-tap
    bilinear rule."""
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    if not all(torch.is_tensor(p) for p in planes):
        raise ValueError("planes must be a tensor or a sequence of tensors")
    if device is None:
        device = next((p.device for p in planes if p.is_cuda), "cuda")
    planes = [p.to(device) for p in planes]
    return ops.import_frames(planes, fmt, size, matrix, range, dtype, antialias).unsqueeze(0)


_range = range                                     # (several functions below name an argument ``range``, as import does)


# pips_tracks_draw's constants (include/pips_hip.h; pips_amd/csrc/yuv.h): (y0, yr, yg, yb, ur, ug, ub, vr, vg, vb) by (matrix, range)
RGB_RULES = {
    ("bt601", "limited"): (16, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681),
    ("bt601", "full"): (0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329),
    ("bt709", "limited"): (16, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639),
    ("bt709", "full"): (0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
}


# pips_tracks_draw_ex's constants for P010 and I010: (y0, sh, yr, yg, yb, ur, ug, ub, vr, vg, vb) by (matrix, range)
RGB10_RULES = {
    ("bt601", "limited"): (64, 14, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681),
    ("bt601", "full"): (0, 16, 78612, 154331, 29972, -44363, -87095, 131458, 131458, -110079, -21379),
    ("bt709", "limited"): (64, 14, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639),
    ("bt709", "full"): (0, 16, 55896, 188037, 18982, -30123, -101335, 131458, 131458, -119404, -12054),
}


def rgb_to_yuv_torch(rgb, matrix="bt709", range="limited", bits=8):
    """the colour conversion of pips_tracks_draw (``bits=8``) and of pips_tracks_draw_ex on the 10-bit surfaces (``bits=10``): rgb
    (...,3) integers 0..255 -> (...,3) int64 Y, Cb, Cr"""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, not {bits!r}")
    R, G, B = rgb.to(torch.int64).unbind(-1)
    if bits == 10:
        y0, sh, yr, yg, yb, ur, ug, ub, vr, vg, vb = RGB10_RULES[(matrix, range)]
        half = 1 << (sh - 1)
        Y = y0 + ((yr * R + yg * G + yb * B + half) >> sh)
        Cb = (512 + ((ur * R + ug * G + ub * B + half) >> sh)).clamp(0, 1023)
        Cr = (512 + ((vr * R + vg * G + vb * B + half) >> sh)).clamp(0, 1023)
        return torch.stack([Y, Cb, Cr], dim=-1)
    y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = RGB_RULES[(matrix, range)]
    Y = y0 + ((yr * R + yg * G + yb * B + 32768) >> 16)
    Cb = (128 + ((ur * R + ug * G + ub * B + 32768) >> 16)).clamp(0, 255)
    Cr = (128 + ((vr * R + vg * G + vb * B + 32768) >> 16)).clamp(0, 255)
    return torch.stack([Y, Cb, Cr], dim=-1)


def track_colors(ids):
    """The colour of each identity, ids (n,) integers -> (n,3) uint8 RGB: the hue h = ((id * 2654435769) mod 2^32) >> 24 on a
    six-segment wheel -- seg = (6 h) >> 8, up = (6 h) & 255, down = 255 - up, and (255,up,0), (down,255,0), (0,255,up), (0,down,255),
    (up,0,255), (255,0,down) for seg 0..5.  Integers only, on the device of ``ids``: an identity keeps its colour for life."""
    ids = torch.as_tensor(ids).to(torch.int64).reshape(-1)
    h = (((ids & 0xFFFFFFFF) * 2654435769) & 0xFFFFFFFF) >> 24               # (int64 products wrap: the low 32 bits are exact)
    seg, up = (6 * h) >> 8, (6 * h) & 255
    down, full, none = 255 - up, torch.full_like(up, 255), torch.zeros_like(up)
    wheel = torch.stack([torch.stack(c, dim=1) for c in ((full, up, none), (down, full, none), (none, full, up), (none, down, full),
                                                         (up, none, full), (full, none, down))])               # (6,n,3)
    return wheel[seg, torch.arange(ids.numel(), device=ids.device)].to(torch.uint8)


def _round_half_up(v, scale):
    return int(math.floor(scale * float(v) + 0.5))


def _draw_setup(planes, trajs, vis, colors, ids, width, dot, alpha, alpha_occ, vis_thr):
    """what ``draw_tracks`` and ``draw_tracks_torch`` make of their arguments: trajs (1,G,n,2) / vis (1,G,n) without the batch
    dimension, the colours, and the rule's integers -> (trajs, vis, colors, line8, dot8, alpha_vis, alpha_occ, vis_logit)"""
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    if not planes or not all(torch.is_tensor(p) for p in planes):
        raise ValueError("planes must be a tensor or a sequence of tensors")
    dev = planes[0].device
    if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
        raise ValueError(f"trajs must be (1,G,n,2), not {tuple(trajs.shape)}")
    trajs = trajs[0].to(dev, torch.float32)
    G, n = trajs.shape[:2]
    if vis is not None:
        if tuple(vis.shape) != (1, G, n):
            raise ValueError(f"vis must be (1,G,n) = {(1, G, n)}, not {tuple(vis.shape)}")
        vis = vis[0].to(dev, torch.float32)
    if colors is None:
        if ids is not None and torch.as_tensor(ids).numel() != n:
            raise ValueError(f"{torch.as_tensor(ids).numel()} ids for {n} columns")
        colors = track_colors(torch.arange(n) if ids is None else ids)
    colors = colors.to(dev)
    if isinstance(vis_thr, bool) or not isinstance(vis_thr, (int, float)) or not 0.0 < vis_thr < 1.0:
        raise ValueError(f"vis_thr must lie in (0, 1), not {vis_thr!r}")
    vis_logit = float(torch.logit(torch.tensor(float(vis_thr), dtype=torch.float32)))              # (as Cover: fp32, on the host)
    return (planes, trajs, vis, colors, _round_half_up(width, 4.0), _round_half_up(dot, 8.0), _round_half_up(alpha, 256.0),
            _round_half_up(alpha_occ, 256.0), vis_logit)


def _draw_fade(fade, trail):
    """``fade`` of ``draw_tracks``: None, "linear" or ``trail`` floats in 0..1 -> None or the rule's ``trail`` ints 0..256 by age"""
    if fade is None:
        return None
    if isinstance(fade, str):
        if fade != "linear":
            raise ValueError(f"fade must be None, 'linear' or a sequence of {trail} floats in 0..1, not {fade!r}")
        return [(512 * (trail - a) + trail) // (2 * trail) for a in _range(trail)]       # round_half_up(256 (trail - a) / trail)
    fade = fade.tolist() if torch.is_tensor(fade) else list(fade)
    if len(fade) != trail:
        raise ValueError(f"fade must have trail = {trail} entries, not {len(fade)}")
    for v in fade:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError(f"a fade entry must lie in 0..1, not {v!r}")
    return [_round_half_up(v, 256.0) for v in fade]


def _draw_quantise(v, n_src, n_dst):
    """a coordinate column (…) float32 of an ``n_src`` wide axis -> (Q int64 eighths of a pixel of the ``n_dst`` wide axis, present)"""
    if n_src != n_dst:
        s = torch.tensor(float(n_dst), dtype=torch.float32, device=v.device) / torch.tensor(float(n_src), dtype=torch.float32, device=v.device)
        v = ((v + 0.5) * s) - 0.5                                  # three elementwise ops: each rounded once, none fused
    ok = v.abs() <= 32768.0                                        # (false for NaN and the infinities)
    q = torch.floor(torch.where(ok, v, torch.zeros_like(v)) * 8.0 + 0.5).to(torch.int64)
    return q, ok


def _draw_inside(cx, cy, p0, p1, R):
    """the inside test of the rule in int64: subsample coordinates cx (1,1,X), cy (1,Y,1), the ends p0, p1 (n,2) and the radius ->
    bool (n,Y,X)"""
    x0, y0, x1, y1 = (t.view(-1, 1, 1) for t in (p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]))
    ax, ay = x1 - x0, y1 - y0
    bx, by = cx - x0, cy - y0
    L, t = ax * ax + ay * ay, ax * bx + ay * by
    R2 = R * R
    at_p0 = bx * bx + by * by <= R2
    at_p1 = (cx - x1) ** 2 + (cy - y1) ** 2 <= R2
    along = (ax * by - ay * bx) ** 2 <= R2 * L
    return torch.where((L == 0) | (t <= 0), at_p0, torch.where(t >= L, at_p1, along))


def draw_coverage_torch(trajs, r, h, w, src_size, trail, line8, dot8, fade=None):
    """The coverage of the rule for the frame that takes row ``r`` of trajs (G,n,2): k (n,h,w) int64 in 0..4, the subsamples of
    each pixel inside the union of each track's primitives.  Subsample (j, i) of the 2h x 2w grid lies at (4 i - 2, 4 j - 2)
    eighths: pixel x owns columns 2 x and 2 x + 1.  With ``fade`` (``trail`` ints 0..256 by age) the result is Wp (n,h,w) in
    0..1024 instead: per subsample the largest factor among the primitives that hold it -- 256 for the head's disc, fade[a] for the
    segment of age a -- summed over the pixel's four."""
    dev, n = trajs.device, trajs.shape[1]
    src_h, src_w = src_size
    cx = (4 * torch.arange(2 * w, device=dev) - 2).view(1, 1, -1)
    cy = (4 * torch.arange(2 * h, device=dev) - 2).view(1, -1, 1)
    rows = trajs[max(r - trail, 0):r + 1]
    qx, okx = _draw_quantise(rows[..., 0], src_w, w)
    qy, oky = _draw_quantise(rows[..., 1], src_h, h)
    pts, ok = torch.stack([qx, qy], dim=-1), okx & oky             # (m,n,2), (m,n): the head is the last row
    live = torch.nonzero(ok[-1]).squeeze(1)                        # an absent head hides the whole trail: only these tracks draw
    pts, ok = pts[:, live], ok[:, live]
    faded = fade is not None
    inside = torch.zeros(live.numel(), 2 * h, 2 * w, dtype=torch.int64 if faded else torch.bool, device=dev)     # phi when faded
    if dot8 >= 0:
        head = _draw_inside(cx, cy, pts[-1], pts[-1], dot8)
        inside = torch.where(head, 256, inside) if faded else inside | head
    if line8 >= 0:
        for g in range(1, pts.shape[0]):
            d = (pts[g] - pts[g - 1]).abs()
            drawn = ok[g] & ok[g - 1] & (d[:, 0] <= ops.DRAW_JUMP8_MAX) & (d[:, 1] <= ops.DRAW_JUMP8_MAX)
            if bool(drawn.any()):
                seg = _draw_inside(cx, cy, pts[g - 1], pts[g], line8) & drawn.view(-1, 1, 1)
                if faded:                                              # the segment that ends on row g has age (rows - 1) - g
                    inside = torch.maximum(inside, seg.to(torch.int64) * int(fade[pts.shape[0] - 1 - g]))
                else:
                    inside |= seg
    k = torch.zeros(n, h, w, dtype=torch.int64, device=dev)
    k[live] = inside.view(live.numel(), h, 2, w, 2).sum(dim=(2, 4))
    return k


def draw_tracks_torch(planes, fmt, trajs, vis=None, colors=None, ids=None, size=None, first=0, trail=16, width=2.0, dot=3.0, alpha=1.0,
                      alpha_occ=0.35, vis_thr=0.5, matrix="bt709", range="limited", inplace=False, fade=None):
    """pips_tracks_draw and pips_tracks_draw_ex (include/pips_hip.h) as int64 torch ops, on any device: ``draw_tracks``' arguments and
    result.  Per frame the coverage of every track (``draw_coverage_torch``), then the tracks one after the other in column order:
    the blend of the full-resolution samples with 1024 - k A, and for the 4:2:0 formats of the chroma samples with K summed over
    each 2 x 2 block of the zero-padded coverage; with ``fade`` the weights are (Wp A + 128) >> 8 and (K A + 128) >> 8 of the faded
    coverage.  On "p010" / "i010" the blend runs on the 10-bit values and only the words that got a weight are written, their six
    other bits zero.  Equal to the kernels bit for bit; written to be read, not to be fast."""
    planes, trajs, vis, colors, line8, dot8, a_vis, a_occ, vis_logit = _draw_setup(planes, trajs, vis, colors, ids, width, dot, alpha,
                                                                                  alpha_occ, vis_thr)
    trail, first = _whole(trail, "trail", 0), _whole(first, "first", 0)
    if not 0 <= trail <= ops.DRAW_TRAIL_MAX:
        raise ValueError(f"trail must lie in 0..{ops.DRAW_TRAIL_MAX}, not {trail}")
    fade = _draw_fade(fade, trail)
    dtypes = [p.dtype for p in planes]                                                             # (uint16 planes are worked on as int16)
    planes, F, h, w, G, n, src_h, src_w = ops.draw_check(planes, fmt, trajs, vis, colors, first, size, trail, line8, dot8, a_vis, a_occ,
                                                         matrix, range)
    if not inplace:
        planes = [p.clone() for p in planes]
    wide, shift = fmt in ops.IMPORT_16BIT, 6 if fmt == "p010" else 0
    yuv = fmt in ("nv12", "i420") or wide
    comp = rgb_to_yuv_torch(colors, matrix, range, 10 if wide else 8) if yuv else colors.to(torch.int64)     # (n,3) in the surface's components

    def value(p):                                                                                  # a plane of one frame -> its samples' values
        return ((p.to(torch.int64) & 0xFFFF) >> shift) & 1023 if wide else p.to(torch.int64)

    def put(p, f, v, hit):
        """the blended values ``v`` into frame f of plane p: every byte of an 8-bit plane (an untouched one is its old value), of a
        16-bit plane the words that got a weight (``hit``) alone, as int16 bit patterns"""
        if not wide:
            p[f] = v.to(torch.uint8)
            return
        word = v << shift
        p[f] = torch.where(hit, word - ((word & 0x8000) << 1), p[f].to(torch.int64)).to(torch.int16)
    if fmt == "planar8":
        full = [planes[0][:, c] for c in (0, 1, 2)]                                                # views (F,h,w) the blend writes into
    elif yuv:
        full = [planes[0]]
        chroma = [planes[1][..., 0], planes[1][..., 1]] if fmt in ("nv12", "p010") else [planes[1], planes[2]]
    else:
        full = [planes[0][..., c] for c in ((2, 1, 0) if fmt in ("bgr24", "bgra32") else (0, 1, 2))]
    for f in _range(F):
        r = first + f
        k = draw_coverage_torch(trajs, r, h, w, (src_h, src_w), trail, line8, dot8, fade)          # (n,h,w): k, or Wp when faded
        seen = torch.ones(n, dtype=torch.bool, device=k.device) if vis is None else vis[r] > vis_logit      # (NaN compares false)
        A = torch.where(seen, a_vis, a_occ).to(torch.int64).view(n, 1, 1)
        wgt = k * A if fade is None else (k * A + 128) >> 8
        cur = [value(p[f]) for p in full]
        if yuv:
            K = torch.nn.functional.pad(k, (0, w % 2, 0, h % 2)).view(n, (h + 1) // 2, 2, (w + 1) // 2, 2).sum(dim=(2, 4))
            K = K * A if fade is None else (K * A + 128) >> 8
            cur_c = [value(p[f]) for p in chroma]
        for i in _range(n):                                                                # column order is part of the rule
            cur = [(p * (1024 - wgt[i]) + comp[i, c] * wgt[i] + 512) >> 10 for c, p in enumerate(cur)]
            if yuv:
                cur_c = [(p * (4096 - K[i]) + comp[i, 1 + c] * K[i] + 2048) >> 12 for c, p in enumerate(cur_c)]
        for p, v in zip(full, cur):
            put(p, f, v, (wgt > 0).any(dim=0))
        if yuv:
            for p, v in zip(chroma, cur_c):
                put(p, f, v, (K > 0).any(dim=0))
    planes = [p.view(t) for p, t in zip(planes, dtypes)]
    return planes[0] if len(planes) == 1 else planes


def draw_tracks(planes, fmt, trajs, vis=None, colors=None, ids=None, size=None, first=0, trail=16, width=2.0, dot=3.0, alpha=1.0,
                alpha_occ=0.35, vis_thr=0.5, matrix="bt709", range="limited", inplace=False, fade=None):
    """Tracks drawn onto frames on the device, one ``pips_tracks_draw`` call (``ops.draw_tracks``; include/pips_hip.h has the rule):
    lines along the last ``trail`` rows with a dot at the head, as the reference's demos end (chain_demo.py:92-108).  ``planes`` /
    ``fmt`` are F surfaces in one of ``ops.import_frames``' six 8-bit layouts, or ``fmt="planar8"`` with one (F,3,h,w) uint8 tensor
    (``import_frames``' own output, without the batch dimension).  trajs (1,G,n,2) and vis (1,G,n) logits (or None) are a tracker's
    output; frame k of the surfaces takes row ``first + k``.  ``size`` = the model's (H, W) when the surfaces are larger (positions
    are mapped back through the import's resize).  ``width`` is the full line width and ``dot`` the head's radius in surface pixels
    (a negative value draws none), ``alpha`` / ``alpha_occ`` the opacity of a track whose visibility is above / not above
    ``vis_thr`` (a probability; ``vis=None``: all visible).  ``colors`` (n,3) uint8 RGB, default ``track_colors(ids)``
    (``track_colors(arange(n))`` without ``ids``); ``matrix`` / ``range`` as for import.  ``inplace=False`` draws on clones and
    returns them (a tensor for one plane, a list otherwise); ``inplace=True`` draws on the given tensors -- pitched views included
    -- and returns them.  Later columns are drawn over earlier ones.  ``fmt`` "p010" / "i010" draws on the decoder's 10-bit
    surfaces (uint16 or int16 planes of ``import_frames``' shapes).  ``fade``: None for one opacity from head to tail, "linear" for
    a trail that fades towards nothing with age (factor (trail - a) / trail on the segment of age a, the one that ends on the head
    being age 0), or ``trail`` factors in 0..1 by age; the head's dot is never faded.  A 10-bit format or a fade goes through
    ``pips_tracks_draw_ex``."""
    planes, trajs, vis, colors, line8, dot8, a_vis, a_occ, vis_logit = _draw_setup(planes, trajs, vis, colors, ids, width, dot, alpha,
                                                                                  alpha_occ, vis_thr)
    trail, first = _whole(trail, "trail", 0), _whole(first, "first", 0)
    if not 0 <= trail <= ops.DRAW_TRAIL_MAX:
        raise ValueError(f"trail must lie in 0..{ops.DRAW_TRAIL_MAX}, not {trail}")
    fade = _draw_fade(fade, trail)
    if not inplace:
        planes = [p.clone() for p in planes]
    ops.draw_tracks(planes, fmt, trajs, vis, colors, first, size, trail, line8, dot8, a_vis, a_occ, vis_logit, matrix, range, fade=fade)
    return planes[0] if len(planes) == 1 else planes


PAINT_ENGINES = ("library", "torch")


class TrackPainter:
    """Draws what a streamed tracker returns, push by push: ``paint(planes, fmt, f0, trajs, vis, ids)`` takes the ``(f0, trajs
    (1,m,n,2), vis (1,m,n)[, ids (n,)])`` of ``StreamTracker.push``, ``CoverTracker.push`` or one stream of
    ``MultiStreamTracker.push`` (one painter per stream) and the m surfaces of the frames ``[f0, f0 + m)``, and draws them as
    ``draw_tracks`` does.  It keeps the last ``trail`` rows BY IDENTITY on the device between calls, so a trail runs across pushes:
    painting push by push gives the bytes of one ``draw_tracks`` call over the whole video (trajs by identity, NaN outside each
    life, ``colors=track_colors(arange(K))``).  An identity it has not seen gets NaN history, one that is no longer among ``ids`` is
    dropped; ``ids=None`` means the columns are stable (their number may not change).  ``size`` is the model's (H, W); ``style`` are
    ``draw_tracks``' width, dot, alpha, alpha_occ, vis_thr, matrix and range; ``fade`` is ``draw_tracks``' (None, "linear" or
    ``trail`` factors in 0..1).
    The painter does not hold frames.  A push returns rows of frames it was given EARLIER (a frame is returned once every query is
    past it), so the caller keeps its surfaces -- a decoder's pool, a ring of NV12 buffers -- until their rows come back, paints
    them then and hands them on.  ``engine="torch"`` paints with ``draw_tracks_torch`` (any device) instead of the library."""

    def __init__(self, size, trail=16, engine="library", fade=None, **style):
        self.size = (int(size[0]), int(size[1]))
        self.trail = _whole(trail, "trail", 0)
        if self.trail > ops.DRAW_TRAIL_MAX:
            raise ValueError(f"trail must lie in 0..{ops.DRAW_TRAIL_MAX}, not {trail}")
        if engine not in PAINT_ENGINES:
            raise ValueError(f"engine must be one of {PAINT_ENGINES}, not {engine!r}")
        unknown = set(style) - {"width", "dot", "alpha", "alpha_occ", "vis_thr", "matrix", "range"}
        if unknown:
            raise ValueError(f"unknown style arguments {sorted(unknown)}")
        _draw_fade(fade, self.trail)                                  # (a ValueError here, not at the first paint)
        self.engine, self.style, self.fade = engine, style, fade
        self.ids, self.rows, self.T = None, None, None              # the columns of ``rows`` (trail,n,2), the next frame

    @torch.no_grad()
    def paint(self, planes, fmt, f0, trajs, vis=None, ids=None, inplace=True):
        if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
            raise ValueError(f"trajs must be (1,m,n,2), not {tuple(trajs.shape)}")
        if self.T is not None and int(f0) != self.T:
            raise ValueError(f"rows of frame {int(f0)} painted after frame {self.T - 1}")
        m, n = trajs.shape[1:3]
        now = trajs[0].to(torch.float32)
        if ids is not None:
            ids = [int(i) for i in torch.as_tensor(ids).reshape(-1).tolist()]
            if len(ids) != n or len(set(ids)) != n:
                raise ValueError(f"ids must name the {n} columns, each once")
        elif self.rows is not None and self.rows.shape[1] != n:
            raise ValueError(f"{n} columns after {self.rows.shape[1]}: pass ids when the columns change")
        hist = torch.full((self.trail, n, 2), float("nan"), dtype=torch.float32, device=now.device)
        if self.rows is not None and self.rows.numel() > 0 and n > 0:
            if ids is None or self.ids is None:
                hist = self.rows.to(now.device)
            else:
                col = {i: j for j, i in enumerate(self.ids)}
                new = [j for j, i in enumerate(ids) if i in col]
                if new:
                    old = torch.tensor([col[ids[j]] for j in new], device=now.device)
                    hist[:, torch.tensor(new, device=now.device)] = self.rows.to(now.device)[:, old]
        rows = torch.cat([hist, now])                                 # (trail + m, n, 2): frame k of the push takes row trail + k
        all_vis = None if vis is None else torch.cat([vis.new_zeros(1, self.trail, n).to(torch.float32), vis.to(torch.float32)], dim=1)
        draw = draw_tracks if self.engine == "library" else draw_tracks_torch
        out = draw(planes, fmt, rows.unsqueeze(0), all_vis, ids=ids, size=self.size, first=self.trail, trail=self.trail,
                   inplace=inplace, fade=self.fade, **self.style)
        self.rows, self.ids, self.T = rows[rows.shape[0] - self.trail:], ids, int(f0) + m
        return out


# ---------------------------------------------------------------------------------------------- global motion from tracks
_M32 = 0xFFFFFFFF


def _mul32(u, c):
    """(u c) mod 2^32 for an int64 tensor 0 <= u < 2^32 and a constant 0 <= c < 2^32; no intermediate passes 2^49"""
    return ((u & 0xFFFF) * c + ((((u >> 16) * c) & 0xFFFF) << 16)) & _M32


def motion_mix(seed, g, k):
    """pips_motion_fit's mix(k) of frame g (include/pips_hip.h), k an int64 tensor (or an int) -> int64 tensor of 32-bit words"""
    k = torch.as_tensor(k, dtype=torch.int64)
    c0 = (int(seed) + 0x9E3779B9 * (int(g) + 1)) & _M32
    u = (c0 + _mul32((k + 1) & _M32, 0x85EBCA6B)) & _M32
    u = u ^ (u >> 16)
    u = _mul32(u, 0x85EBCA6B)
    u = u ^ (u >> 13)
    u = _mul32(u, 0xC2B2AE35)
    return u ^ (u >> 16)


def _motion_inliers(p, q, pi, qi, d, e, thr4):
    """the rule's inlier test of the points p, q (m,2) against the hypotheses (c,2) each of pi, qi, d, e -> (c,m) bool; int64"""
    a, b = p.unsqueeze(0) - pi.unsqueeze(1), q.unsqueeze(0) - qi.unsqueeze(1)                    # (c,m,2)
    ex, ey, dx, dy = (v.unsqueeze(1) for v in (e[:, 0], e[:, 1], d[:, 0], d[:, 1]))
    rre = (ex * a[..., 0] - ey * a[..., 1]) - (dx * b[..., 0] - dy * b[..., 1])
    rim = (ex * a[..., 1] + ey * a[..., 0]) - (dx * b[..., 1] + dy * b[..., 0])
    return (rre * rre + rim * rim <= (thr4 * thr4) * (dx * dx + dy * dy)) & ((dx != 0) | (dy != 0))


def motion_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed):
    """pips_motion_fit (include/pips_hip.h) as int64 / float64 torch ops, on any device: rows trajs (F,n,2) and vis (F,n) logits or
    None -> (head (P,4) int64, sums (P,8) int64, model (P,4) float64, flags (P,n) uint8) for the P = max(F - 1, 0) pairs of
    consecutive rows.  Integers up to the sums, then one float64 operation per rounding of the rule: equal to the kernels' in
    every bit."""
    if trajs.dim() != 3 or trajs.shape[2] != 2:
        raise ValueError(f"trajs must be (F,n,2), not {tuple(trajs.shape)}")
    F, n = trajs.shape[:2]
    if vis is not None and tuple(vis.shape) != (F, n):
        raise ValueError(f"vis must be (F,n) = {(F, n)}, not {tuple(vis.shape)}")
    K, thr4, frame0, seed = int(K), int(thr4), int(frame0), int(seed)
    if n > ops.MOTION_N_MAX:
        raise ValueError(f"{n} columns: the sums are exact up to {ops.MOTION_N_MAX}")
    if not 1 <= K <= ops.MOTION_HYPS_MAX or not 1 <= thr4 <= ops.MOTION_THR4_MAX:
        raise ValueError(f"need 1 <= K <= {ops.MOTION_HYPS_MAX} and 1 <= thr4 <= {ops.MOTION_THR4_MAX} (K={K}, thr4={thr4})")
    if frame0 < 0 or frame0 + F > _INT_MAX or not 0 <= seed <= _M32:
        raise ValueError(f"frame0 + F must fit an int32 and seed a uint32 (frame0={frame0}, seed={seed})")
    dev, I64, P = trajs.device, torch.int64, max(F - 1, 0)
    s = trajs.to(torch.float32) * 4.0                                                            # exact
    usable = (s.abs() <= float(ops.MOTION_QUARTER_MAX)).all(dim=2)                               # (a NaN compares false)
    quarter = torch.where(usable.unsqueeze(2), s, torch.zeros_like(s)).round().to(I64)           # round-half-even
    if vis is not None:
        usable = usable & (vis.to(dev, torch.float32) > float(vis_logit))
    head = torch.zeros(P, 4, dtype=I64, device=dev)
    sums = torch.zeros(P, 8, dtype=I64, device=dev)
    flags = torch.zeros(P, n, dtype=torch.uint8, device=dev)
    hyp = torch.arange(K, device=dev)
    for f in range(1, F):
        ok = usable[f - 1] & usable[f]
        cols = torch.nonzero(ok).squeeze(1)
        m = int(cols.numel())
        flags[f - 1] = ok.to(torch.uint8)
        head[f - 1, 0], head[f - 1, 2] = m, -1
        if m < 2:
            continue
        p, q = quarter[f - 1][cols], quarter[f][cols]
        i = (motion_mix(seed, frame0 + f, 2 * hyp) * m) >> 32
        j = (motion_mix(seed, frame0 + f, 2 * hyp + 1) * (m - 1)) >> 32
        j = j + (j >= i).to(I64)
        d, e = p[j] - p[i], q[j] - q[i]
        step = max(1, (1 << 22) // m)                                                            # hypotheses at a time
        score = torch.cat([_motion_inliers(p, q, p[i[a:a + step]], q[i[a:a + step]], d[a:a + step], e[a:a + step], thr4).sum(dim=1)
                           for a in range(0, K, step)])
        best = int(score.max())
        if best < 2:
            continue
        h = int(torch.nonzero(score == best)[0, 0])                                              # ties: the lowest h
        inl = _motion_inliers(p, q, p[i[h:h + 1]], q[i[h:h + 1]], d[h:h + 1], e[h:h + 1], thr4)[0]
        p, q = p[inl], q[inl]
        flags[f - 1, cols[inl]] = 2
        head[f - 1, 1], head[f - 1, 2] = best, h
        sums[f - 1] = torch.stack([inl.sum(), p[:, 0].sum(), p[:, 1].sum(), q[:, 0].sum(), q[:, 1].sum(), (p * p).sum(),
                                   (p * q).sum(), (p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum()])
    return head, sums, _motion_model(sums, head[:, 2] >= 0), flags


def _motion_model(sums, have):
    """the rule's least-squares similarity on the inliers from their sums (R,8) int64 and ``have`` (R,) bool -> (R,4) float64: int64
    up to D, A, B, then float64, an operation a line"""
    N, spx, spy, sqx, sqy, spp, sdot, scross = sums.unbind(dim=1)
    F64 = torch.float64
    D = torch.where(have, N * spp - (spx * spx + spy * spy), torch.ones_like(N)).to(F64)
    A = (N * sdot - (spx * sqx + spy * sqy)).to(F64)
    B = (N * scross - (spx * sqy - spy * sqx)).to(F64)
    n4 = torch.where(have, 4 * N, torch.ones_like(N)).to(F64)
    spx, spy, sqx, sqy = spx.to(F64), spy.to(F64), sqx.to(F64), sqy.to(F64)
    are, aim = A / D, B / D
    tx = are * spx
    tx = tx - aim * spy
    tx = (sqx - tx) / n4
    ty = aim * spx
    ty = ty + are * spy
    ty = (sqy - ty) / n4
    one, zero = torch.ones_like(are), torch.zeros_like(are)
    return torch.stack([torch.where(have, are, one), torch.where(have, aim, zero), torch.where(have, tx, zero),
                        torch.where(have, ty, zero)], dim=1)


MOTION_LAYER_SEED = 0x632BE5AB                                                                   # seed_l = seed + l * this, mod 2^32
MOTION_NO_LAYER, MOTION_NOT_VALID = 254, 255                                                     # pips_motion_layers' labels


def motion_layers_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer=None):
    """pips_motion_layers (include/pips_hip.h) as int64 / float64 torch ops, on any device: rows trajs (F,n,2), vis (F,n) logits or
    None and prev_layer (n,) uint8 or None -> (head (P,L,4) int64, sums (P,L,8) int64, model (P,L,4) float64, box (P,L,4) int64,
    layer (P,n) uint8, overlap (P,L,L) int64) for the P = max(F - 1, 0) pairs of consecutive rows: ``motion_table_torch``'s consensus
    peeled L times on the columns left over, equal to the kernels' in every bit."""
    if trajs.dim() != 3 or trajs.shape[2] != 2:
        raise ValueError(f"trajs must be (F,n,2), not {tuple(trajs.shape)}")
    F, n = trajs.shape[:2]
    if vis is not None and tuple(vis.shape) != (F, n):
        raise ValueError(f"vis must be (F,n) = {(F, n)}, not {tuple(vis.shape)}")
    if prev_layer is not None and (tuple(prev_layer.shape) != (n,) or prev_layer.dtype != torch.uint8):
        raise ValueError(f"prev_layer must be uint8 (n,) = {(n,)}, not {prev_layer.dtype} {tuple(prev_layer.shape)}")
    K, thr4, frame0, seed, L, min_in = int(K), int(thr4), int(frame0), int(seed), int(L), int(min_in)
    if n > ops.MOTION_N_MAX:
        raise ValueError(f"{n} columns: the sums are exact up to {ops.MOTION_N_MAX}")
    if not 1 <= K <= ops.MOTION_HYPS_MAX or not 1 <= thr4 <= ops.MOTION_THR4_MAX:
        raise ValueError(f"need 1 <= K <= {ops.MOTION_HYPS_MAX} and 1 <= thr4 <= {ops.MOTION_THR4_MAX} (K={K}, thr4={thr4})")
    if frame0 < 0 or frame0 + F > _INT_MAX or not 0 <= seed <= _M32:
        raise ValueError(f"frame0 + F must fit an int32 and seed a uint32 (frame0={frame0}, seed={seed})")
    if not 1 <= L <= ops.MOTION_LAYERS_MAX or not 2 <= min_in <= ops.MOTION_N_MAX:
        raise ValueError(f"need 1 <= L <= {ops.MOTION_LAYERS_MAX} and 2 <= min_in <= {ops.MOTION_N_MAX} (L={L}, min_in={min_in})")
    dev, I64, P = trajs.device, torch.int64, max(F - 1, 0)
    s = trajs.to(torch.float32) * 4.0                                                            # exact
    usable = (s.abs() <= float(ops.MOTION_QUARTER_MAX)).all(dim=2)                               # (a NaN compares false)
    quarter = torch.where(usable.unsqueeze(2), s, torch.zeros_like(s)).round().to(I64)           # round-half-even
    if vis is not None:
        usable = usable & (vis.to(dev, torch.float32) > float(vis_logit))
    head = torch.zeros(P, L, 4, dtype=I64, device=dev)
    head[:, :, 2] = -1
    sums = torch.zeros(P, L, 8, dtype=I64, device=dev)
    box = torch.zeros(P, L, 4, dtype=I64, device=dev)
    layer = torch.full((P, n), MOTION_NOT_VALID, dtype=torch.uint8, device=dev)
    overlap = torch.zeros(P, L, L, dtype=I64, device=dev)
    hyp = torch.arange(K, device=dev)
    for f in range(1, F):
        ok = usable[f - 1] & usable[f]
        cols = torch.nonzero(ok).squeeze(1)                                                      # the list of layer 0
        layer[f - 1, cols] = MOTION_NO_LAYER
        for l in range(L):
            m = int(cols.numel())
            head[f - 1, l, 0] = m
            if m < 2:
                continue
            seed_l = (seed + l * MOTION_LAYER_SEED) & _M32
            p, q = quarter[f - 1][cols], quarter[f][cols]
            i = (motion_mix(seed_l, frame0 + f, 2 * hyp) * m) >> 32
            j = (motion_mix(seed_l, frame0 + f, 2 * hyp + 1) * (m - 1)) >> 32
            j = j + (j >= i).to(I64)
            d, e = p[j] - p[i], q[j] - q[i]
            step = max(1, (1 << 22) // m)                                                        # hypotheses at a time
            score = torch.cat([_motion_inliers(p, q, p[i[a:a + step]], q[i[a:a + step]], d[a:a + step], e[a:a + step], thr4).sum(dim=1)
                               for a in range(0, K, step)])
            best = int(score.max())
            if best < (2 if l == 0 else min_in):
                continue
            h = int(torch.nonzero(score == best)[0, 0])                                          # ties: the lowest h
            inl = _motion_inliers(p, q, p[i[h:h + 1]], q[i[h:h + 1]], d[h:h + 1], e[h:h + 1], thr4)[0]
            p, q = p[inl], q[inl]
            layer[f - 1, cols[inl]] = l
            head[f - 1, l, 1], head[f - 1, l, 2] = best, h
            sums[f - 1, l] = torch.stack([inl.sum(), p[:, 0].sum(), p[:, 1].sum(), q[:, 0].sum(), q[:, 1].sum(), (p * p).sum(),
                                          (p * q).sum(), (p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum()])
            box[f - 1, l] = torch.cat([q.min(dim=0).values, q.max(dim=0).values])
            cols = cols[~inl]                                                                    # the inliers leave, the order stays
        before = layer[f - 2] if f >= 2 else None if prev_layer is None else prev_layer.to(dev)
        if before is not None:
            now, before = layer[f - 1].to(I64), before.to(I64)
            both = (now < L) & (before < L)
            overlap[f - 1] = torch.bincount((now * L + before)[both], minlength=L * L).view(L, L)
    model = _motion_model(sums.view(P * L, 8), head.view(P * L, 4)[:, 2] >= 0).view(P, L, 4)
    return head, sums, model, box, layer, overlap


def link_layers(head, overlap, prev_ids=None, prev_counts=None, next_id=1):
    """Object identities for ``pips_motion_layers``' layers, on the host, from ``head`` (P,L,4) and ``overlap`` (P,L,L) alone ->
    (object_ids (P,L) int64, next_id).  Layer 0 with a model is the camera, id 0; a layer without a model has id -1.  For l = 1..L-1
    in ascending order, with a model: the candidates are the layers b >= 1 of the pair before with an id >= 1 that no lower l of this
    pair has taken; the b with the largest overlap[f][l][b] is taken, ties to the lowest b; its id is inherited iff overlap >= 1 and
    2 overlap >= min(n_in[f][l], n_in[f-1][b]); otherwise the id is ``next_id``, which then goes up by one.  The first pair links
    against ``prev_ids`` (L,) and ``prev_counts`` (L,) = the ids and n_in of the pair before the call when both are given, otherwise
    against nothing.  Known limit: an identity has no memory beyond the previous pair -- an object that loses its layer for one pair
    comes back under a new id."""
    head, overlap = torch.as_tensor(head), torch.as_tensor(overlap)
    if head.dim() != 3 or head.shape[2] != 4 or tuple(overlap.shape) != (head.shape[0], head.shape[1], head.shape[1]):
        raise ValueError(f"head must be (P,L,4) and overlap (P,L,L), not {tuple(head.shape)} and {tuple(overlap.shape)}")
    P, L = head.shape[:2]
    next_id = _whole(next_id, "next_id", 1)
    if (prev_ids is None) != (prev_counts is None):
        raise ValueError("prev_ids and prev_counts are given together or not at all")
    ids_before = counts_before = None
    if prev_ids is not None:
        ids_before = [int(v) for v in torch.as_tensor(prev_ids).reshape(-1).tolist()]
        counts_before = [int(v) for v in torch.as_tensor(prev_counts).reshape(-1).tolist()]
        if len(ids_before) != L or len(counts_before) != L:
            raise ValueError(f"prev_ids and prev_counts must hold {L} entries")
    n_in, have, over = head[:, :, 1].tolist(), (head[:, :, 2] >= 0).tolist(), overlap.tolist()
    out = []
    for f in range(P):
        ids, taken = [-1] * L, set()
        if L and have[f][0]:
            ids[0] = 0
        for l in range(1, L):
            if not have[f][l]:
                continue
            best, best_b = 0, -1
            for b in range(1, L if ids_before is not None else 0):
                if ids_before[b] >= 1 and b not in taken and over[f][l][b] > best:               # (ties: the lowest b stays)
                    best, best_b = over[f][l][b], b
            if best_b >= 0 and 2 * best >= min(n_in[f][l], counts_before[best_b]):
                ids[l] = ids_before[best_b]
                taken.add(best_b)
            else:
                ids[l], next_id = next_id, next_id + 1
        out.append(ids)
        ids_before, counts_before = ids, n_in[f]
    return torch.tensor(out, dtype=torch.int64).view(P, L), next_id


MOTION_ENGINES = ("library", "torch")
_MOTION_PARAMS = ("thr", "hypotheses", "vis_thr", "seed")


def _motion_setup(trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed):
    """what ``motion_fit`` and ``motion_fit_torch`` make of their arguments -> (rows (F,n,2), vis (F,n) or None, order or None,
    the rule's integers (frame0, vis_logit, K, thr4, seed)); with ``ids`` the columns are put in ascending id order (``order``)"""
    if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
        raise ValueError(f"trajs must be (1,F,n,2), not {tuple(trajs.shape)}")
    rows = trajs[0].to(torch.float32)
    F, n = rows.shape[:2]
    if vis is not None:
        if tuple(vis.shape) != (1, F, n):
            raise ValueError(f"vis must be (1,F,n) = {(1, F, n)}, not {tuple(vis.shape)}")
        vis = vis[0].to(rows.device, torch.float32)
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not 0.25 <= thr <= ops.MOTION_THR4_MAX / 4 or \
            float(thr) * 4.0 != int(float(thr) * 4.0):
        raise ValueError(f"thr must be a multiple of 0.25 px in 0.25..{ops.MOTION_THR4_MAX / 4}, not {thr!r}")
    K = _whole(hypotheses, "hypotheses", 1)
    if K > ops.MOTION_HYPS_MAX:
        raise ValueError(f"hypotheses must lie in 1..{ops.MOTION_HYPS_MAX}, not {hypotheses!r}")
    if isinstance(vis_thr, bool) or not isinstance(vis_thr, (int, float)) or not 0.0 < vis_thr < 1.0:
        raise ValueError(f"vis_thr must lie in (0, 1), not {vis_thr!r}")
    vis_logit = float(torch.logit(torch.tensor(float(vis_thr), dtype=torch.float32)))              # (as Cover: fp32, on the host)
    order = None
    if ids is not None:
        ids = torch.as_tensor(ids).reshape(-1).to(torch.int64).cpu()
        if ids.numel() != n or torch.unique(ids).numel() != n:
            raise ValueError(f"ids must name the {n} columns, each once")
        order = torch.argsort(ids).to(rows.device)
        rows, vis = rows[:, order], None if vis is None else vis[:, order]
    return rows, vis, order, (_whole(frame0, "frame0", 0), vis_logit, K, int(float(thr) * 4.0), _whole(seed, "seed", 0))


def _motion_result(head, model, flags, order):
    """the rule's tables -> (models (P,4) float64, inliers (P,n) bool, valid (P,n) bool, counts (P,2) int64 = (m, n_in)), the
    columns back in the caller's order"""
    if order is not None:
        back = torch.empty_like(flags)
        back[:, order] = flags
        flags = back
    return model, flags == 2, flags >= 1, head[:, :2].to(torch.int64)


def motion_fit(trajs, vis=None, ids=None, frame0=0, thr=2.0, hypotheses=256, vis_thr=0.5, seed=0):
    """The camera motion between consecutive frames of a tracker's output, one ``pips_motion_fit`` call (``ops.motion_fit``;
    include/pips_hip.h has the rule): trajs (1,F,n,2) and vis (1,F,n) logits (or None) on the GPU -> ``models`` (F-1,4) float64 =
    (a_re, a_im, tx, ty) with q = a p + t taking the positions of frame f - 1 to those of frame f (the identity where a pair has no
    model), ``inliers`` (F-1,n) bool, ``valid`` (F-1,n) bool and ``counts`` (F-1,2) = (valid columns, inliers).  A column counts
    in a pair when it has a position within +-2047.75 px in both frames and, with ``vis``, a visibility above ``vis_thr`` (a
    probability) in both; a track that is valid but no inlier moves on its own.  ``thr`` is the inlier distance in px at the scale
    of the hypothesis' two points, a multiple of 0.25; ``hypotheses`` two-point samples are scored, drawn from ``seed`` and the
    absolute frame index ``frame0 + f``.  With ``ids`` (n,) the valid columns are taken in ascending id order, so the result does
    not depend on where a tracker put its columns."""
    rows, vis, order, (frame0, vis_logit, K, thr4, seed) = _motion_setup(trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed)
    head, _, model, flags = ops.motion_fit(rows, vis, frame0, vis_logit, K, thr4, seed)
    return _motion_result(head, model, flags, order)


def motion_fit_torch(trajs, vis=None, ids=None, frame0=0, thr=2.0, hypotheses=256, vis_thr=0.5, seed=0):
    """``motion_fit`` by ``motion_table_torch``: the same rule as int64 / float64 torch ops on any device, equal in every bit"""
    rows, vis, order, (frame0, vis_logit, K, thr4, seed) = _motion_setup(trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed)
    head, _, model, flags = motion_table_torch(rows, vis, frame0, vis_logit, K, thr4, seed)
    return _motion_result(head, model, flags, order)


class MotionEstimator:
    """The camera motion of a streamed tracker, push by push: ``step(f0, trajs, vis, ids)`` takes the ``(f0, trajs (1,m,n,2), vis
    (1,m,n)[, ids (n,)])`` of ``StreamTracker.push``, ``CoverTracker.push`` or one stream of ``MultiStreamTracker.push`` and returns
    the models (float64, four a row) of the pairs that END on the frames ``f0 .. f0 + m - 1`` -- the first push with rows has no pair
    for its first row.  It keeps the last row BY IDENTITY between calls, so the pair across two pushes is fitted too: stepping push
    by push gives what one ``motion_fit`` call gives on the whole video laid out by identity (NaN outside each life, ``ids =
    arange(K)``).  An identity it has not seen has no position in the kept row, one that is no longer among ``ids`` is dropped;
    ``ids=None`` means the columns are stable (their number may not change).  ``vis`` is given on every step or on none.
    ``inliers``, ``valid`` and ``counts`` hold ``motion_fit``'s other results for the pairs of the last step, in its column order.
    ``params`` are ``motion_fit``'s thr, hypotheses, vis_thr and seed; ``engine="torch"`` fits with ``motion_fit_torch`` (any
    device) instead of the library."""

    def __init__(self, engine="library", **params):
        if engine not in MOTION_ENGINES:
            raise ValueError(f"engine must be one of {MOTION_ENGINES}, not {engine!r}")
        unknown = set(params) - set(_MOTION_PARAMS)
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}")
        _motion_setup(torch.zeros(1, 0, 0, 2), None, None, 0, **{**dict(thr=2.0, hypotheses=256, vis_thr=0.5, seed=0), **params})
        self.engine, self.params = engine, params
        self.ids, self.row, self.vis_row, self.T = None, None, None, None           # the columns of ``row`` (n,2), the next frame
        self.inliers = self.valid = self.counts = None

    @torch.no_grad()
    def step(self, f0, trajs, vis=None, ids=None):
        if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
            raise ValueError(f"trajs must be (1,m,n,2), not {tuple(trajs.shape)}")
        if self.T is not None and int(f0) != self.T:
            raise ValueError(f"rows of frame {int(f0)} after frame {self.T - 1}")
        m, n = trajs.shape[1:3]
        if vis is not None and tuple(vis.shape) != (1, m, n):
            raise ValueError(f"vis must be (1,m,n) = {(1, m, n)}, not {tuple(vis.shape)}")
        if ids is not None:
            ids = [int(i) for i in torch.as_tensor(ids).reshape(-1).tolist()]
            if len(ids) != n or len(set(ids)) != n:
                raise ValueError(f"ids must name the {n} columns, each once")
        elif self.row is not None and self.row.shape[0] != n:
            raise ValueError(f"{n} columns after {self.row.shape[0]}: pass ids when the columns change")
        if self.row is not None and (vis is None) != (self.vis_row is None):
            raise ValueError("vis must be given on every step or on none")
        self.T = int(f0) + m
        if m == 0:
            return torch.zeros(0, 4, dtype=torch.float64, device=trajs.device)
        now = trajs[0].to(torch.float32)
        now_vis = None if vis is None else vis[0].to(now.device, torch.float32)
        rows, all_vis, frame0 = now, now_vis, int(f0)
        if self.row is not None:
            old = torch.full((1, n, 2), float("nan"), dtype=torch.float32, device=now.device)
            old_vis = None if vis is None else torch.full((1, n), float("nan"), dtype=torch.float32, device=now.device)
            if n > 0 and self.row.shape[0] > 0:
                if ids is None or self.ids is None:
                    old[0] = self.row.to(now.device)
                    if vis is not None:
                        old_vis[0] = self.vis_row.to(now.device)
                else:
                    col = {i: j for j, i in enumerate(self.ids)}
                    new = [j for j, i in enumerate(ids) if i in col]
                    if new:
                        at, src = torch.tensor(new, device=now.device), torch.tensor([col[ids[j]] for j in new], device=now.device)
                        old[0, at] = self.row.to(now.device)[src]
                        if vis is not None:
                            old_vis[0, at] = self.vis_row.to(now.device)[src]
            rows, frame0 = torch.cat([old, now]), int(f0) - 1
            all_vis = None if vis is None else torch.cat([old_vis, now_vis])
        fit = motion_fit if self.engine == "library" else motion_fit_torch
        models, self.inliers, self.valid, self.counts = fit(rows.unsqueeze(0), None if all_vis is None else all_vis.unsqueeze(0),
                                                            ids=ids, frame0=frame0, **self.params)
        self.row, self.vis_row, self.ids = now[m - 1], None if vis is None else now_vis[m - 1], ids
        return models


# ---------------------------------------------------------------------------------------------- moving objects from tracks
_MOTION_LAYER_PARAMS = _MOTION_PARAMS + ("layers", "min_inliers")
_MOTION_LAYER_DEFAULTS = dict(thr=2.0, hypotheses=256, vis_thr=0.5, seed=0, layers=4, min_inliers=8)


def _motion_layers_run(engine, trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed, layers, min_inliers, prev_layer=None,
                       prev_ids=None, prev_counts=None, next_id=1):
    """``motion_layers`` / ``motion_layers_torch`` with the state a stream carries from call to call: ``prev_layer`` (n,) uint8 are
    the library's labels of the pair before the call in the CALLER's column order, ``prev_ids`` / ``prev_counts`` / ``next_id``
    are ``link_layers``' -> (the six results, layer (P,n) uint8 in the caller's order, next_id)"""
    rows, vis, order, (frame0, vis_logit, K, thr4, seed) = _motion_setup(trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed)
    L, min_in = _whole(layers, "layers", 1), _whole(min_inliers, "min_inliers", 2)
    if L > ops.MOTION_LAYERS_MAX or min_in > ops.MOTION_N_MAX:
        raise ValueError(f"layers must lie in 1..{ops.MOTION_LAYERS_MAX} and min_inliers in 2..{ops.MOTION_N_MAX}, not {layers!r} "
                         f"and {min_inliers!r}")
    if prev_layer is not None:
        prev_layer = prev_layer.to(rows.device)
        prev_layer = prev_layer if order is None else prev_layer[order]
    table = ops.motion_layers if engine == "library" else motion_layers_table_torch
    head, _, model, box, layer, overlap = table(rows, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer)
    if order is not None:
        back = torch.empty_like(layer)
        back[:, order] = layer
        layer = back
    head = head.to(torch.int64)
    object_ids, next_id = link_layers(head.cpu(), overlap.cpu(), prev_ids, prev_counts, next_id)
    object_ids = object_ids.to(rows.device)
    at = layer.to(torch.int64)
    labels = torch.where(at == MOTION_NOT_VALID, -2, torch.where(at == MOTION_NO_LAYER, -1, at))
    P = head.shape[0]
    objects = torch.where(labels >= 0, torch.gather(object_ids, 1, labels.clamp(min=0)), labels) if P else labels
    return (model, head[:, :, :2], labels, object_ids, objects, box.to(torch.float64) / 4.0), layer, next_id


def motion_layers(trajs, vis=None, ids=None, frame0=0, thr=2.0, hypotheses=256, vis_thr=0.5, seed=0, layers=4, min_inliers=8):
    """What moves, beside the camera: one ``pips_motion_layers`` call (``ops.motion_layers``; include/pips_hip.h has the rule) and
    ``link_layers`` on its small tables.  For every pair of consecutive frames of trajs (1,F,n,2) (vis (1,F,n) logits or None) the
    consensus similarity of ``motion_fit`` is found -- layer 0, the camera --, then found again on the valid columns left over, up
    to ``layers`` times; a layer above 0 needs ``min_inliers`` columns to count.  The layers are linked from pair to pair into
    objects by the columns they share.  Returns ``models`` (P,L,4) float64 (the identity without a model), ``counts`` (P,L,2) =
    (columns the layer chose from, its inliers), ``labels`` (P,n) int64 with -2 for a column that is not valid, -1 for a valid one
    in no layer and 0..L-1 otherwise, ``object_ids`` (P,L) int64 (0 the camera, >= 1 objects, -1 no model), ``objects`` (P,n) the
    id of each column's layer (-2, -1 as in labels) and ``boxes`` (P,L,4) float64 = (min x, min y, max x, max y) px of each layer's
    columns in the pair's second frame (zeros without a model).  The other arguments are ``motion_fit``'s; with ``ids`` the columns
    are taken in ascending id order and come back in the caller's.  Known limits: similarities only; a layer is a motion, not a
    compact region; no re-scoring after the refit; layers with the same motion are not merged; an identity has no memory beyond
    the previous pair; the labels are per track (``object_masks`` makes per-pixel masks of them)."""
    return _motion_layers_run("library", trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed, layers, min_inliers)[0]


def motion_layers_torch(trajs, vis=None, ids=None, frame0=0, thr=2.0, hypotheses=256, vis_thr=0.5, seed=0, layers=4, min_inliers=8):
    """``motion_layers`` by ``motion_layers_table_torch``: the same rule as int64 / float64 torch ops on any device, equal in every
    bit"""
    return _motion_layers_run("torch", trajs, vis, ids, frame0, thr, hypotheses, vis_thr, seed, layers, min_inliers)[0]


class MotionLayers:
    """The moving objects of a streamed tracker, push by push: ``step(f0, trajs, vis, ids)`` takes the ``(f0, trajs (1,m,n,2), vis
    (1,m,n)[, ids (n,)])`` of ``StreamTracker.push`` or ``CoverTracker.push`` and returns ``motion_layers``' six results for the
    pairs that END on the frames ``f0 .. f0 + m - 1``, in the push's column order.  Like ``MotionEstimator`` it keeps the last row
    and vis BY IDENTITY, and beside them the last pair's labels by identity (an identity it has not seen counts in no overlap),
    the last pair's object ids and inlier counts and the next free id: stepping push by push gives what one ``motion_layers`` call
    gives on the whole video laid out by identity, object ids included.  ``ids=None`` means the columns are stable; ``ids`` and
    ``vis`` are each given on every step or on none.  ``params`` are ``motion_layers``' thr, hypotheses, vis_thr, seed, layers
    and min_inliers; ``engine="torch"`` runs ``motion_layers_torch`` (any device) instead of the library."""

    def __init__(self, engine="library", **params):
        if engine not in MOTION_ENGINES:
            raise ValueError(f"engine must be one of {MOTION_ENGINES}, not {engine!r}")
        unknown = set(params) - set(_MOTION_LAYER_PARAMS)
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}")
        self.engine, self.params = engine, {**_MOTION_LAYER_DEFAULTS, **params}
        _motion_layers_run("torch", torch.zeros(1, 0, 0, 2), None, None, 0, **self.params)
        self.ids, self.row, self.vis_row, self.T = None, None, None, None           # the columns of ``row`` (n,2), the next frame
        self.layer, self.object_ids, self.counts, self.next_id = None, None, None, 1   # of the last pair: labels (n,) uint8, (L,), (L,)

    def _by_identity(self, kept, ids, fill, like):
        """the kept per-column tensor in the columns of this push: ``fill`` for an identity that was not there"""
        n = len(ids) if ids is not None else kept.shape[0]
        out = torch.full((n,) + tuple(kept.shape[1:]), fill, dtype=kept.dtype, device=like.device)
        if n == 0 or kept.shape[0] == 0:
            return out
        if ids is None:                                                             # (stable columns: step checked their number)
            return kept.to(like.device).clone()
        col = {i: j for j, i in enumerate(self.ids)}
        new = [j for j, i in enumerate(ids) if i in col]
        if new:
            at, src = torch.tensor(new, device=like.device), torch.tensor([col[ids[j]] for j in new], device=like.device)
            out[at] = kept.to(like.device)[src]
        return out

    @torch.no_grad()
    def step(self, f0, trajs, vis=None, ids=None):
        if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
            raise ValueError(f"trajs must be (1,m,n,2), not {tuple(trajs.shape)}")
        if self.T is not None and int(f0) != self.T:
            raise ValueError(f"rows of frame {int(f0)} after frame {self.T - 1}")
        m, n = trajs.shape[1:3]
        if vis is not None and tuple(vis.shape) != (1, m, n):
            raise ValueError(f"vis must be (1,m,n) = {(1, m, n)}, not {tuple(vis.shape)}")
        if ids is not None:
            ids = [int(i) for i in torch.as_tensor(ids).reshape(-1).tolist()]
            if len(ids) != n or len(set(ids)) != n:
                raise ValueError(f"ids must name the {n} columns, each once")
        elif self.row is not None and self.row.shape[0] != n:
            raise ValueError(f"{n} columns after {self.row.shape[0]}: pass ids when the columns change")
        if self.row is not None and (vis is None) != (self.vis_row is None):
            raise ValueError("vis must be given on every step or on none")
        if self.row is not None and (ids is None) != (self.ids is None):
            raise ValueError("ids must be given on every step or on none: the kept row and labels are matched by identity")
        self.T = int(f0) + m
        now = trajs[0].to(torch.float32)
        now_vis = None if vis is None else vis[0].to(now.device, torch.float32)
        rows, all_vis, frame0, prev_layer = now, now_vis, int(f0), None
        if m > 0 and self.row is not None:
            nan = float("nan")
            rows, frame0 = torch.cat([self._by_identity(self.row, ids, nan, now).unsqueeze(0), now]), int(f0) - 1
            if vis is not None:
                all_vis = torch.cat([self._by_identity(self.vis_row, ids, nan, now).unsqueeze(0), now_vis])
            if self.layer is not None:
                prev_layer = self._by_identity(self.layer, ids, MOTION_NOT_VALID, now)
        out, layer, self.next_id = _motion_layers_run(self.engine, rows.unsqueeze(0), None if all_vis is None else all_vis.unsqueeze(0),
                                                      ids, frame0, **self.params, prev_layer=prev_layer, prev_ids=self.object_ids,
                                                      prev_counts=self.counts, next_id=self.next_id)
        if m > 0:
            self.row, self.vis_row, self.ids = now[m - 1], None if vis is None else now_vis[m - 1], ids
        if layer.shape[0] > 0:
            self.layer, self.object_ids, self.counts = layer[-1], out[3][-1].cpu(), out[1][-1, :, 1].cpu()
        return out


# ---------------------------------------------------------------------------------------------- object masks from the layers
def _masks_setup(trajs, labels, size, out_size, radius, vote, first):
    """what ``object_masks`` and ``object_masks_torch`` make of their arguments -> (rows (F,n,2) float32, labels (F,n) uint8 with
    255 for every value outside 0..254, (h, w), (src_h, src_w), radius8, vote, first)"""
    if trajs.dim() != 4 or trajs.shape[0] != 1 or trajs.shape[3] != 2:
        raise ValueError(f"trajs must be (1,F,n,2), not {tuple(trajs.shape)}")
    rows = trajs[0].to(torch.float32)
    F, n = rows.shape[:2]
    labels = torch.as_tensor(labels)
    if tuple(labels.shape) != (F, n) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must be integers (F,n) = {(F, n)}, not {labels.dtype} {tuple(labels.shape)}")
    labels = labels.to(rows.device, torch.int64)
    labels = torch.where((labels >= 0) & (labels < ops.MASK_NONE), labels, ops.MASK_NONE).to(torch.uint8)
    src = (int(size[0]), int(size[1]))
    out = src if out_size is None else (int(out_size[0]), int(out_size[1]))
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0.0 <= radius <= ops.MASK_RADIUS8_MAX / 8:
        raise ValueError(f"radius must lie in 0..{ops.MASK_RADIUS8_MAX // 8} px, not {radius!r}")
    return rows, labels, out, src, _round_half_up(radius, 8.0), _whole(vote, "vote", 1), _whole(first, "first", 0)


def object_masks(trajs, labels, size, out_size=None, radius=48.0, vote=1, first=0):
    """A label per pixel from a label per track, one ``pips_object_masks`` call (``ops.object_masks``; include/pips_hip.h has the
    rule): trajs (1,F,n,2) on the GPU are positions in a ``size`` = (H, W) image (the model's frames), labels (F,n) integers of
    any dtype; a value outside 0..254 takes no part -- ``motion_layers``' -1 and -2 among them.  Returns (F - first, h, w) uint8,
    ``out_size`` = (h, w) (default ``size``; a decoder's surface when it is larger: positions are mapped as ``draw_tracks`` maps
    them): frame k is made from row ``first + k`` alone, every pixel taking the label that its ``vote`` nearest participating
    tracks within ``radius`` px OF THE MASK vote for -- ties to the nearest -- and 255 where no track is that near.  With
    ``vote=1`` the mask is the Voronoi diagram of the tracks cut off at ``radius``; a radius of about 1.5 x the track spacing
    closes the cells of a regular cover.  With ``motion_layers``' result the call is ``object_masks(trajs[:, 1:], res_labels, size)``:
    a pair's labels sit on its second frame, as its boxes do.  No stateful class is needed for a stream: a mask depends on one row
    only, so a streaming user calls this per push on the labels ``MotionLayers.step`` returns and the rows the push brought."""
    rows, labels, out, src, radius8, vote, first = _masks_setup(trajs, labels, size, out_size, radius, vote, first)
    return ops.object_masks(rows, labels, out, src, radius8, vote, first)


def object_masks_torch(trajs, labels, size, out_size=None, radius=48.0, vote=1, first=0):
    """``object_masks`` as int64 torch ops on any device, equal in every byte: per frame the keys d2 2^24 + column 2^8 + label of
    the participating columns at every pixel (2^62 outside the radius), the ``vote`` smallest by ``topk``, and the label with the
    most votes among them, the first such in key order.  Rows of pixels are taken in slabs, each against the columns within the
    radius of the slab.  Written to be read, not to be fast."""
    rows, labels, (h, w), (src_h, src_w), radius8, vote, first = _masks_setup(trajs, labels, size, out_size, radius, vote, first)
    G, n, F = ops.object_masks_check(rows, labels, (h, w), (src_h, src_w), radius8, vote, first)[:3]
    dev = rows.device
    out = torch.full((F, h, w), ops.MASK_NONE, dtype=torch.uint8, device=dev)
    far = 1 << 62
    X8 = (8 * torch.arange(w, device=dev)).view(1, 1, w)
    for k in _range(F):
        qx, okx = _draw_quantise(rows[first + k, :, 0], src_w, w)
        qy, oky = _draw_quantise(rows[first + k, :, 1], src_h, h)
        lab = labels[first + k].to(torch.int64)
        part = okx & oky & (lab != ops.MASK_NONE)
        slab = max(1, min(h, (1 << 22) // max(1, w * max(int(part.sum()), 1))))
        for y0 in _range(0, h, slab):
            y1 = min(h, y0 + slab)
            col = torch.nonzero(part & (qy >= 8 * y0 - radius8) & (qy <= 8 * (y1 - 1) + radius8)).squeeze(1)
            if col.numel() == 0:
                continue
            dx = X8 - qx[col].view(-1, 1, 1)
            dy = (8 * torch.arange(y0, y1, device=dev)).view(1, -1, 1) - qy[col].view(-1, 1, 1)
            d2 = dx * dx + dy * dy
            near = (dx.abs() <= radius8) & (dy.abs() <= radius8) & (d2 <= radius8 * radius8)
            key = torch.where(near, (d2 << 24) + (col.view(-1, 1, 1) << 8) + lab[col].view(-1, 1, 1), far)
            top = torch.topk(key, min(vote, col.numel()), dim=0, largest=False).values          # ascending: the nearest first
            took, vlab = top != far, top & 255
            count = ((vlab.unsqueeze(0) == vlab.unsqueeze(1)) & took.unsqueeze(0) & took.unsqueeze(1)).sum(dim=1)   # votes of entry j's label
            best, most = torch.full_like(vlab[0], ops.MASK_NONE), torch.zeros_like(vlab[0])
            for j in _range(top.shape[0]):
                better = took[j] & (count[j] > most)
                best, most = torch.where(better, vlab[j], best), torch.where(better, count[j], most)
            out[k, y0:y1] = best.to(torch.uint8)
    return out


def _guided_setup(trajs, labels, guide, size, out_size, radius, edge, first):
    """what ``object_masks_guided`` and ``object_masks_guided_torch`` make of their arguments -> (rows, labels, guide on the rows'
    device, (h, w), (src_h, src_w), edge, reach, first); reach = floor(5 radius + 0.5), the radius in pixels of the mask"""
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0.0 <= radius <= ops.MASK_REACH_MAX or \
            _round_half_up(radius, 5.0) > ops.MASK_REACH_MAX:
        raise ValueError(f"radius must lie in 0..{ops.MASK_REACH_MAX / 5} px (reach = floor(5 radius + 0.5) <= {ops.MASK_REACH_MAX}), "
                         f"not {radius!r}")
    rows, labels, out, src, _, _, first = _masks_setup(trajs, labels, size, out_size, 0.0, 1, first)
    if guide is not None:
        if not torch.is_tensor(guide) or guide.dtype != torch.uint8 or guide.dim() != 3:
            raise ValueError(f"guide must be a uint8 tensor (F - first, h, w), not {getattr(guide, 'dtype', None)} "
                             f"{tuple(getattr(guide, 'shape', ()))}")
        guide = guide.to(rows.device)
    return rows, labels, guide, out, src, _whole(edge, "edge", 0), _round_half_up(radius, 5.0), first


def object_masks_guided(trajs, labels, guide, size, out_size=None, radius=48.0, edge=4, first=0):
    """``object_masks`` with the image in the decision, one ``pips_object_masks_guided`` call (``ops.object_masks_guided``;
    include/pips_hip.h has the rule): trajs, labels, ``size``, ``out_size`` and ``first`` as there; ``guide`` (F - first, h, w) uint8
    on the GPU is the 8-bit luma of the frames at the mask's size -- ``guide_plane`` of the surfaces; any row and frame strides
    with a unit last stride.  A pixel takes the label of the track that is nearest along a path over the pixel grid whose steps
    cost 1 px (1.4 px diagonally; 5 and 7 in fifths of a pixel) plus ``edge`` / 5 px per grey level that the step changes the
    guide by, within ``radius`` px of cost; 255 where no track is that near.  Crossing a luma edge of 60 levels at ``edge=4``
    costs as much as 48 px of flat ground, so the boundary between two labels runs along such an edge wherever one lies between
    their tracks; ``edge=0`` is the (chamfer) Voronoi diagram of ``object_masks``' ``vote=1``.  A streaming user calls this per
    push on what ``MotionLayers.step`` returns, as ``object_masks``."""
    rows, labels, guide, out, src, edge, reach, first = _guided_setup(trajs, labels, guide, size, out_size, radius, edge, first)
    return ops.object_masks_guided(rows, labels, guide, out, src, edge, reach, first)


def object_masks_guided_torch(trajs, labels, guide, size, out_size=None, radius=48.0, edge=4, first=0):
    """``object_masks_guided`` as int64 torch ops on any device, equal in every byte: per frame the keys cost 2^16 + column of the
    seed pixels, then floor(reach / 5) Jacobi steps -- the keys padded by a ring of none, shifted to each of the eight neighbours,
    the step's cost added and the minimum taken -- leaving early when a step changes nothing.  Written to be read, not to be
    fast."""
    return _guided_keys(trajs, labels, guide, size, out_size, radius, edge, first)[0]


def _guided_keys(trajs, labels, guide, size, out_size, radius, edge, first):
    """the twin's work -> (masks (F,h,w) uint8, keys (F,h,w) int64 with 2^32 - 1 for none, the Jacobi steps each frame took before
    one changed nothing)"""
    rows, labels, guide, (h, w), (src_h, src_w), edge, reach, first = _guided_setup(trajs, labels, guide, size, out_size, radius, edge,
                                                                                    first)
    G, n, F = ops.object_masks_guided_check(rows, labels, guide, (h, w), (src_h, src_w), edge, reach, first)[:3]
    dev = rows.device
    none = (1 << 32) - 1
    masks = torch.full((F, h, w), ops.MASK_NONE, dtype=torch.uint8, device=dev)
    keys = torch.full((F, h, w), none, dtype=torch.int64, device=dev)
    steps = []
    pad = torch.nn.functional.pad
    for k in _range(F):
        qx, okx = _draw_quantise(rows[first + k, :, 0], src_w, w)
        qy, oky = _draw_quantise(rows[first + k, :, 1], src_h, h)
        lab = labels[first + k].to(torch.int64)
        X, Y = (qx + 4) >> 3, (qy + 4) >> 3
        seeds = torch.nonzero(okx & oky & (lab != ops.MASK_NONE) & (X >= 0) & (X < w) & (Y >= 0) & (Y < h)).squeeze(1)
        key = keys[k].view(-1)
        key.scatter_reduce_(0, Y[seeds] * w + X[seeds], seeds, "amin")                      # cost 0: the key is the lowest column
        key = key.view(h, w)
        done = 0
        if seeds.numel() > 0:
            g = pad(guide[k].to(torch.int64), (1, 1, 1, 1))
            for _ in _range(reach // 5):
                kp = pad(key, (1, 1, 1, 1), value=none)
                new = key
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if dx == 0 and dy == 0:
                            continue
                        kq = kp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                        c = (7 if dx != 0 and dy != 0 else 5) + edge * (g[1:1 + h, 1:1 + w] - g[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]).abs()
                        cand = kq + (c << 16)
                        new = torch.minimum(new, torch.where((kq != none) & ((cand >> 16) <= reach), cand, none))
                if torch.equal(new, key):
                    break
                key, done = new, done + 1
        keys[k] = key
        if n > 0:
            masks[k] = torch.where(key != none, lab[(key & 0xFFFF).clamp(max=n - 1)], ops.MASK_NONE).to(torch.uint8)
        steps.append(done)
    return masks, keys, steps


def guide_plane(planes, fmt):
    """The guide of ``object_masks_guided`` from F surfaces on the GPU: their 8-bit luma (F,h,w) uint8.  ``planes`` / ``fmt`` as in
    ``draw_tracks``: for "nv12" and "i420" the Y plane itself, as the view it is -- no copy, no launch; for "rgb24", "bgr24",
    "rgba32", "bgra32" and "planar8" one ``pips_guide_plane`` call (``ops.guide_plane``): (77 R + 150 G + 29 B + 128) >> 8.  The
    16-bit formats are a ValueError."""
    if fmt in ("nv12", "i420"):
        return ops.draw_planes(planes, fmt)[0][0]
    return ops.guide_plane(planes, fmt)


def guide_plane_torch(planes, fmt):
    """``guide_plane`` as int64 torch ops on any device, equal in every byte"""
    if fmt in ("nv12", "i420"):
        return ops.draw_planes(planes, fmt)[0][0]
    planes = ops.guide_check(planes, fmt)[0]
    if fmt == "planar8":
        r, g, b = (planes[0][:, c].to(torch.int64) for c in (0, 1, 2))
    else:
        r, g, b = (planes[0][..., c].to(torch.int64) for c in ((2, 1, 0) if fmt in ("bgr24", "bgra32") else (0, 1, 2)))
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).to(torch.uint8)


def object_colors(object_ids, alpha=0.5, camera_alpha=0.0):
    """The colours and opacities ``tint_masks`` takes, from ``motion_layers``' ``object_ids`` (P,L): -> (colors (P,L,3) uint8,
    alpha (P,L) float64).  A mask holds LAYER indices, which an object may change from pair to pair; the colour of layer l of pair
    f is ``track_colors`` of its OBJECT id, so an object keeps its colour for life.  The opacity is ``alpha`` for an object (id >=
    1), ``camera_alpha`` for the camera (id 0) and 0 for a layer without a model (id -1)."""
    object_ids = torch.as_tensor(object_ids)
    if object_ids.dim() != 2 or object_ids.dtype.is_floating_point or object_ids.dtype == torch.bool:
        raise ValueError(f"object_ids must be integers (P,L), not {object_ids.dtype} {tuple(object_ids.shape)}")
    for v in (alpha, camera_alpha):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError(f"an opacity must lie in 0..1, not {v!r}")
    ids = object_ids.to(torch.int64)
    colors = track_colors(ids.clamp(min=0)).view(ids.shape[0], ids.shape[1], 3)
    a = torch.full(ids.shape, float(alpha), dtype=torch.float64, device=ids.device)
    a[ids == 0], a[ids < 0] = float(camera_alpha), 0.0
    return colors, a


def _tint_setup(planes, masks, colors, alpha):
    """what ``tint_masks`` and ``tint_masks_torch`` make of their arguments -> (planes, masks, colors on the surfaces' device,
    alpha (F,C) int64 0..256 on the host)"""
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    if not planes or not all(torch.is_tensor(p) for p in planes):
        raise ValueError("planes must be a tensor or a sequence of tensors")
    dev = planes[0].device
    alpha = torch.as_tensor(alpha).to("cpu", torch.float64)
    if alpha.numel() and not bool(((alpha >= 0.0) & (alpha <= 1.0)).all()):                      # (false for a NaN)
        raise ValueError("an alpha must lie in 0..1")
    return planes, masks.to(dev), colors.to(dev), torch.floor(alpha * 256.0 + 0.5).to(torch.int64)


def tint_masks(planes, fmt, masks, colors, alpha, matrix="bt709", range="limited", inplace=False):
    """Label planes shown on frames on the device, one ``pips_masks_tint`` call (``ops.masks_tint``; include/pips_hip.h has the
    rule): ``planes`` / ``fmt`` are F surfaces in one of ``draw_tracks``' seven 8-bit layouts, ``masks`` (F,h,w) uint8 of the
    surfaces' size (``object_masks``' result), ``colors`` (F,C,3) uint8 RGB and ``alpha`` (F,C) opacities in 0..1 per (frame,
    label) -- ``object_colors`` makes both.  A pixel with label l < C is blended towards its colour with opacity round(256 alpha)
    / 256; a label >= C, 255 among them, and an opacity of 0 leave the pixel.  ``inplace=False`` tints clones and returns them (a
    tensor for one plane, a list otherwise); ``inplace=True`` tints the given tensors -- pitched views included."""
    planes, masks, colors, alpha = _tint_setup(planes, masks, colors, alpha)
    if not inplace:
        planes = [p.clone() for p in planes]
    ops.masks_tint(planes, fmt, masks, colors, alpha, matrix, range)
    return planes[0] if len(planes) == 1 else planes


def tint_masks_torch(planes, fmt, masks, colors, alpha, matrix="bt709", range="limited", inplace=False):
    """``tint_masks`` as int64 torch ops on any device, equal in every byte: the opacity and the colour of every pixel looked up by
    its label, the full-resolution samples blended with 256 - A, the 4:2:0 chroma samples with 1024 - the sum of A over each 2 x 2
    block of the zero-padded opacities.  Written to be read, not to be fast."""
    planes, masks, colors, alpha = _tint_setup(planes, masks, colors, alpha)
    planes, F, h, w, C, alpha = ops.tint_check(planes, fmt, masks, colors, alpha, matrix, range)
    if not inplace:
        planes = [p.clone() for p in planes]
    dev = planes[0].device
    yuv = fmt in ("nv12", "i420")
    comp = rgb_to_yuv_torch(colors, matrix, range) if yuv else colors.to(torch.int64)             # (F,C,3) in the surface's components
    alpha = alpha.to(dev)
    if fmt == "planar8":
        full = [planes[0][:, c] for c in (0, 1, 2)]
    elif yuv:
        full = [planes[0]]
        chroma = [planes[1][..., 0], planes[1][..., 1]] if fmt == "nv12" else [planes[1], planes[2]]
    else:
        full = [planes[0][..., c] for c in ((2, 1, 0) if fmt in ("bgr24", "bgra32") else (0, 1, 2))]
    for f in _range(F):
        l = masks[f].to(torch.int64)
        known = l < C
        at = l.clamp(max=C - 1)
        A = torch.where(known, alpha[f][at], 0)                                                    # (h,w)
        c = comp[f][at]                                                                            # (h,w,3)
        for k, p in enumerate(full):
            old = p[f].to(torch.int64)
            p[f] = torch.where(A > 0, (old * (256 - A) + c[..., k] * A + 128) >> 8, old).to(torch.uint8)
        if yuv:
            pad = (0, w % 2, 0, h % 2)
            SA = torch.nn.functional.pad(A, pad).view((h + 1) // 2, 2, (w + 1) // 2, 2).sum(dim=(1, 3))
            for k, p in enumerate(chroma):
                S = torch.nn.functional.pad(c[..., 1 + k] * A, pad).view((h + 1) // 2, 2, (w + 1) // 2, 2).sum(dim=(1, 3))
                old = p[f].to(torch.int64)
                p[f] = torch.where(SA > 0, (old * (1024 - SA) + S + 512) >> 10, old).to(torch.uint8)
    return planes[0] if len(planes) == 1 else planes


def motion_path(models):
    """Per-pair similarities ``models`` (P,4) = (a_re, a_im, tx, ty), pair f taking frame f - 1 to frame f -> (P+1,4) float64 on
    the host: row f takes the positions of frame f to those of FRAME 0 (row 0 is the identity) -- the inverses composed,
    path_f = path_{f-1} o model_f^-1, in complex float64.  Warping frame f by row f holds the camera still."""
    models = torch.as_tensor(models).to("cpu", torch.float64)
    if models.dim() != 2 or models.shape[1] != 4:
        raise ValueError(f"models must be (P,4), not {tuple(models.shape)}")
    A, T = complex(1.0, 0.0), complex(0.0, 0.0)
    out = [[1.0, 0.0, 0.0, 0.0]]
    for a_re, a_im, tx, ty in models.tolist():
        a, t = complex(a_re, a_im), complex(tx, ty)
        if a == 0:
            raise ValueError("a model with a = 0 has no inverse")
        A, T = A / a, T - (A / a) * t                                              # x_0 = A ((q - t) / a) + T
        out.append([A.real, A.imag, T.real, T.imag])
    return torch.tensor(out, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------- frames out, stabilised
def _smooth_params(A_prev, theta_prev, A, T):
    """the parameters (log|A|, theta, Re T, Im T) of one path row, theta unwrapped from the row before"""
    if A == 0:
        raise ValueError("a path row with A = 0 has no logarithm")
    theta = cmath.phase(A) if A_prev is None else theta_prev + cmath.phase(A / A_prev)
    return [math.log(abs(A)), theta, T.real, T.imag]


def _smooth_row(g, A, T, f, radius):
    """the correction of frame f: its window of ``g`` summed on its own in ascending frame order, plain float adds"""
    lo, hi = max(0, f - radius), min(len(g) - 1, f + radius)
    mean = []
    for c in _range(4):
        acc = 0.0
        for k in _range(lo, hi + 1):
            acc = acc + g[k][c]
        mean.append(acc / (hi - lo + 1))
    As = math.exp(mean[0]) * complex(math.cos(mean[1]), math.sin(mean[1]))
    Ts = complex(mean[2], mean[3])
    Wa, Wt = A / As, (T - Ts) / As
    return [Wa.real, Wa.imag, Wt.real, Wt.imag]


def _smooth_radius(radius):
    return None if radius is None else _whole(radius, "radius", 0)


def motion_smooth(path, radius=15):
    """The corrections that stabilise a video, on the host in float64: ``path`` (F,4) is ``motion_path``'s output, row f = (A, T)
    taking frame f to frame 0 -> (F,4) rows W_f taking frame f to the STABILISED frame f.  ``radius=None``: W = path, the camera
    held still.  Otherwise the path's parameters g_f = (log|A_f|, theta_f, Re T_f, Im T_f), theta unwrapped (theta_0 = arg A_0,
    theta_f = theta_{f-1} + arg(A_f / A_{f-1})), are replaced by their mean over the frames max(0, f - radius) .. min(F - 1, f +
    radius) -- each window summed on its own in ascending order, so that ``Stabilizer`` reproduces the bits push by push -- and with
    A~ = exp(l~) e^{i theta~}, W_f = (A_f / A~_f, (T_f - T~_f) / A~_f): the smoothed camera keeps the slow motion, the frame loses
    the shake."""
    radius = _smooth_radius(radius)
    path = torch.as_tensor(path).to("cpu", torch.float64)
    if path.dim() != 2 or path.shape[1] != 4:
        raise ValueError(f"path must be (F,4), not {tuple(path.shape)}")
    if not bool(torch.isfinite(path).all()):
        raise ValueError("path has a non-finite entry")
    if radius is None:
        return path.clone()
    rows = [(complex(r[0], r[1]), complex(r[2], r[3])) for r in path.tolist()]
    g = []
    for f, (A, T) in enumerate(rows):
        g.append(_smooth_params(rows[f - 1][0] if f else None, g[f - 1][1] if f else 0.0, A, T))
    out = [_smooth_row(g, A, T, f, radius) for f, (A, T) in enumerate(rows)]
    return torch.tensor(out, dtype=torch.float64).reshape(len(out), 4)


def _warp_maps(transforms, size, surface):
    """the checks of ``warp_coefficients`` on the transforms and the sizes -> (affine rows as a list of six floats each, (h, w) of the
    surface, S1: surface index -> model index, S4: model index -> surface index, both 3 x 3 float64)"""
    t = torch.as_tensor(transforms).to("cpu", torch.float64)
    if t.dim() != 2 or t.shape[1] not in (4, 6):
        raise ValueError(f"transforms must be (F,4) or (F,6), not {tuple(t.shape)}")
    H, W = int(size[0]), int(size[1])
    h, w = (H, W) if surface is None else (int(surface[0]), int(surface[1]))
    if min(H, W, h, w) < 1:
        raise ValueError(f"sizes must be at least 1 x 1, not {H} x {W} and {h} x {w}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError("transforms has a non-finite entry")
    if t.shape[1] == 4:
        t = torch.stack([t[:, 0], -t[:, 1], t[:, 2], t[:, 1], t[:, 0], t[:, 3]], dim=1)
    sx, sy = w / W, h / H
    eye = [0.0, 0.0, 1.0]
    S1 = torch.tensor([[1.0 / sx, 0.0, 0.5 / sx - 0.5], [0.0, 1.0 / sy, 0.5 / sy - 0.5], eye], dtype=torch.float64)
    S4 = torch.tensor([[sx, 0.0, 0.5 * sx - 0.5], [0.0, sy, 0.5 * sy - 0.5], eye], dtype=torch.float64)
    return t.tolist(), (h, w), S1, S4


def _affine_inverse(a, b, c, d, e, f):
    """the inverse of x' = a x + b y + c, y' = d x + e y + f as a 3 x 3 float64 matrix; ValueError for a singular map"""
    det = a * e - b * d
    if det == 0.0 or not math.isfinite(det) or not math.isfinite(1.0 / det):
        raise ValueError(f"the map ({a}, {b}, {c}, {d}, {e}, {f}) is singular")
    ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
    return torch.tensor([[ia, ib, -(ia * c + ib * f)], [id_, ie, -(id_ * c + ie * f)], [0.0, 0.0, 1.0]], dtype=torch.float64)


def warp_coefficients(transforms, size, surface=None, zoom=1.0):
    """Forward transforms -> the (F,6) int32 rows of ``pips_frames_warp`` on the host, in float64.  ``transforms`` is (F,4)
    similarity rows (a_re, a_im, tx, ty) -- ``motion_smooth``'s output; the affine row (a_re, -a_im, tx, a_im, a_re, ty) -- or (F,6)
    affine rows (a, b, c, d, e, f) with x' = a x + b y + c, y' = d x + e y + f: FORWARD maps, taking a position of the frame to
    where it shall be shown, in pixel-index coordinates of the model's ``size`` = (H, W).  ``surface`` = (h, w) of the surfaces that
    are warped (default ``size``).  An output pixel u of the surface goes, as 3 x 3 float64 matrices applied in this order, through
    the zoom about the surface centre ((w-1)/2, (h-1)/2) -- the output pixel shows the stabilised position c + (u - c) / zoom --,
    from surface index to model index, x = (u + 0.5) / s - 0.5 with s = w / W (y with h / H: the inverse of what draw applies),
    through the inverse of the forward map, and from model index back to surface index.  Rows 0 and 1 of the product are quantised
    with floor(v 2^24 + 0.5) for the linear terms and floor(v 2^16 + 0.5) for the offsets.  ValueError for a singular map, zoom <= 0,
    a non-finite entry and a coefficient outside int32 (a linear term needs |v| < 128, an offset |v| < 32768 px)."""
    if isinstance(zoom, bool) or not isinstance(zoom, (int, float)) or not math.isfinite(zoom) or zoom <= 0:
        raise ValueError(f"zoom must be a finite number above 0, not {zoom!r}")
    t, (h, w), S1, S4 = _warp_maps(transforms, size, surface)
    cx, cy, z = (w - 1) / 2, (h - 1) / 2, 1.0 / float(zoom)
    Z = torch.tensor([[z, 0.0, cx - cx * z], [0.0, z, cy - cy * z], [0.0, 0.0, 1.0]], dtype=torch.float64)
    out = []
    for a, b, c, d, e, f in t:
        inv = _affine_inverse(a, b, c, d, e, f)
        M = (S4 @ (inv @ (S1 @ Z))).tolist()
        row = []
        for r in (0, 1):
            for k, (scale, limit) in enumerate(((2.0 ** 24, 128.0), (2.0 ** 24, 128.0), (2.0 ** 16, 32768.0))):
                v = M[r][k]
                q = math.floor(v * scale + 0.5) if math.isfinite(v) and abs(v) < limit else None
                if q is None or not -2 ** 31 <= q <= 2 ** 31 - 1:
                    raise ValueError(f"coefficient {v!r} of the map ({a}, {b}, {c}, {d}, {e}, {f}) does not fit its fixed-point int32")
                row.append(q)
        out.append(row)
    return torch.tensor(out, dtype=torch.int32).reshape(len(out), 6)


def _warp_positions(h, w, m, chroma, dev):
    """U (h,w) and V (h,w) int64: the source position, in 1/256 sample, of every sample of an h x w plane under the six python ints m"""
    x, y = torch.arange(w, dtype=torch.int64, device=dev).view(1, w), torch.arange(h, dtype=torch.int64, device=dev).view(h, 1)
    if chroma:
        U = (m[0] * (4 * x + 1) + m[1] * (4 * y + 1) + 512 * m[2] - 2 ** 24 + 2 ** 17) >> 18
        V = (m[3] * (4 * x + 1) + m[4] * (4 * y + 1) + 512 * m[5] - 2 ** 24 + 2 ** 17) >> 18
    else:
        U = (m[0] * x + m[1] * y + 256 * m[2] + 32768) >> 16
        V = (m[3] * x + m[4] * y + 256 * m[5] + 32768) >> 16
    return U, V


def _warp_plane(src, m, chroma, border, fill):
    """one plane of one frame: src (h,w,C) int64 values, m the frame's six python ints, fill (C,) int64 -> (h,w,C) int64"""
    h, w, _ = src.shape
    U, V = _warp_positions(h, w, m, chroma, src.device)
    x0, fx, y0, fy = U >> 8, (U & 255).unsqueeze(-1), V >> 8, (V & 255).unsqueeze(-1)

    def tap(xi, yi):
        v = src[yi.clamp(0, h - 1), xi.clamp(0, w - 1)]                                           # (h,w,C)
        if border == "replicate":
            return v
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return torch.where(inside.unsqueeze(-1), v, fill.view(1, 1, -1))
    p00, p01, p10, p11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    return ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16


def _warp_covers(h, w, m, chroma, dev="cpu"):
    """(h,w) bool: the samples of an h x w plane that the row m covers -- every tap that has weight lies inside the plane, per axis
    x0 >= 0 and (x0 + 1 <= w - 1, or fx == 0 and x0 <= w - 1)"""
    U, V = _warp_positions(h, w, m, chroma, dev)

    def axis(P, n):
        i, f = P >> 8, P & 255
        return (i >= 0) & ((i + 1 <= n - 1) | ((f == 0) & (i <= n - 1)))
    return axis(U, w) & axis(V, h)


def _fill_plane(get, shape, Fs, cand, rows, chroma, border, fill):
    """one plane of one output frame of pips_frames_warp_fill: get(f) -> the (h,w,C) int64 values of source frame f, shape = (h,w,C),
    cand the K python ints and rows the K rows of the frame -> (values (h,w,C), who (h,w)): candidate 0 under the border rule (the
    fill when it is invalid), then the candidates from the last to the first, each laid over what it covers, so that the first in
    list order is the one that stays.  A covering candidate needs no border rule: "replicate" only moves its taps of weight 0"""
    h, w, C = shape
    dev = fill.device
    if 0 <= cand[0] < Fs:
        value = _warp_plane(get(cand[0]), rows[0], chroma, border, fill)
    else:
        value = fill.view(1, 1, C).expand(h, w, C)
    who = torch.full((h, w), ops.WARP_FILL_NONE, dtype=torch.int64, device=dev)
    for k in reversed(_range(len(cand))):
        if not 0 <= cand[k] < Fs:
            continue
        cov = _warp_covers(h, w, rows[k], chroma, dev)
        value = torch.where(cov.unsqueeze(-1), _warp_plane(get(cand[k]), rows[k], chroma, "replicate", fill), value)
        who = torch.where(cov, k, who)
    return value, who


def warp_frames_torch(planes, fmt, coef, border="constant", fill=(0, 0, 0), matrix="bt709", range="limited"):
    """pips_frames_warp (include/pips_hip.h) as int64 torch ops, on any device: ``ops.warp_frames``' arguments (without ``out``) ->
    new planes of the source's shapes and types, a tensor for one plane and a list otherwise.  Per frame and plane the positions
    U, V of every output sample from the six integers, the four taps under the border rule, the blend with 256 - f and f.  Equal
    to the kernel byte for byte; written to be read, not to be fast."""
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    dtypes = [p.dtype for p in planes]
    planes, F, h, w, coef, fill_rgb = ops.warp_check(planes, fmt, coef, border, fill, matrix, range)
    dev = planes[0].device
    rows = coef.to("cpu", torch.int64).tolist()
    wide, shift = fmt in ops.IMPORT_16BIT, 6 if fmt == "p010" else 0
    yuv = fmt in ("nv12", "i420") or wide
    rgb = torch.tensor([fill_rgb >> 16, (fill_rgb >> 8) & 255, fill_rgb & 255], dtype=torch.int64)
    comp = (rgb_to_yuv_torch(rgb, matrix, range, 10 if wide else 8) if yuv else rgb).to(dev)
    out = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in planes]

    def value(p):                                                                                  # a plane of one frame -> its samples' values
        return ((p.to(torch.int64) & 0xFFFF) >> shift) & 1023 if wide else p.to(torch.int64)

    def word(v):                                                                                   # values -> what is stored
        if not wide:
            return v.to(torch.uint8)
        v = v << shift
        return (v - ((v & 0x8000) << 1)).to(torch.int16)
    for f in _range(F):
        m = rows[f]
        if fmt == "planar8":
            for c in (0, 1, 2):
                out[0][f, c] = word(_warp_plane(value(planes[0][f, c]).unsqueeze(-1), m, False, border, comp[c:c + 1])[..., 0])
        elif yuv:
            out[0][f] = word(_warp_plane(value(planes[0][f]).unsqueeze(-1), m, False, border, comp[:1])[..., 0])
            if fmt in ("nv12", "p010"):
                out[1][f] = word(_warp_plane(value(planes[1][f]), m, True, border, comp[1:]))
            else:
                for k in (1, 2):
                    out[k][f] = word(_warp_plane(value(planes[k][f]).unsqueeze(-1), m, True, border, comp[k:k + 1])[..., 0])
        else:
            order = comp.flip(0) if fmt in ("bgr24", "bgra32") else comp                            # the bytes of a pixel in memory order
            out[0][f, ..., :3] = word(_warp_plane(value(planes[0][f, ..., :3]), m, False, border, order))
            if fmt in ("rgba32", "bgra32"):
                out[0][f, ..., 3] = 255
    out = [p.view(t) for p, t in zip(out, dtypes)]
    return out[0] if len(out) == 1 else out


def warp_frames_fill_torch(planes, fmt, cand, coef, border="constant", fill=(0, 0, 0), matrix="bt709", range="limited", source=False):
    """pips_frames_warp_fill (include/pips_hip.h) as int64 torch ops, on any device: ``ops.warp_frames_fill``'s arguments (without
    ``out``) -> Fd new surfaces of the source's format, a tensor for one plane and a list otherwise, and with ``source=True``
    ``(planes, map)``, the (Fd,h,w) uint8 map of the list position that supplied each sample of plane 0.  Per output frame and
    plane ``_fill_plane``: candidate 0 under the border rule, every covering candidate laid over it.  Equal to the kernel byte for
    byte, the map included; written to be read, not to be fast."""
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    dtypes = [p.dtype for p in planes]
    planes, Fs, Fd, K, h, w, cand, coef, fill_rgb = ops.warp_fill_check(planes, fmt, cand, coef, border, fill, matrix, range)
    dev = planes[0].device
    cands, rows = cand.to("cpu", torch.int64).tolist(), coef.to("cpu", torch.int64).tolist()
    wide, shift = fmt in ops.IMPORT_16BIT, 6 if fmt == "p010" else 0
    yuv = fmt in ("nv12", "i420") or wide
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rgb = torch.tensor([fill_rgb >> 16, (fill_rgb >> 8) & 255, fill_rgb & 255], dtype=torch.int64)
    comp = (rgb_to_yuv_torch(rgb, matrix, range, 10 if wide else 8) if yuv else rgb).to(dev)
    out = [torch.zeros((Fd,) + tuple(p.shape[1:]), dtype=p.dtype, device=dev) for p in planes]
    smap = torch.zeros(Fd, h, w, dtype=torch.uint8, device=dev)

    def value(p):                                                                                  # a plane of one frame -> its samples' values
        return ((p.to(torch.int64) & 0xFFFF) >> shift) & 1023 if wide else p.to(torch.int64)

    def word(v):                                                                                   # values -> what is stored
        if not wide:
            return v.to(torch.uint8)
        v = v << shift
        return (v - ((v & 0x8000) << 1)).to(torch.int16)
    for j in _range(Fd):
        def one(get, shape, chroma, fillc):
            return _fill_plane(get, shape, Fs, cands[j], rows[j], chroma, border, fillc)
        if fmt == "planar8":
            for c in (0, 1, 2):
                v, who = one(lambda f: value(planes[0][f, c]).unsqueeze(-1), (h, w, 1), False, comp[c:c + 1])
                out[0][j, c] = word(v[..., 0])
                if c == 0:
                    smap[j] = who.to(torch.uint8)
        elif yuv:
            v, who = one(lambda f: value(planes[0][f]).unsqueeze(-1), (h, w, 1), False, comp[:1])
            out[0][j], smap[j] = word(v[..., 0]), who.to(torch.uint8)
            if fmt in ("nv12", "p010"):
                out[1][j] = word(one(lambda f: value(planes[1][f]), (ch, cw, 2), True, comp[1:])[0])
            else:
                for k in (1, 2):
                    out[k][j] = word(one(lambda f: value(planes[k][f]).unsqueeze(-1), (ch, cw, 1), True, comp[k:k + 1])[0][..., 0])
        else:
            order = comp.flip(0) if fmt in ("bgr24", "bgra32") else comp                            # the bytes of a pixel in memory order
            v, who = one(lambda f: value(planes[0][f, ..., :3]), (h, w, 3), False, order)
            out[0][j, ..., :3], smap[j] = word(v), who.to(torch.uint8)
            if fmt in ("rgba32", "bgra32"):
                out[0][j, ..., 3] = 255
    out = [p.view(t) for p, t in zip(out, dtypes)]
    out = out[0] if len(out) == 1 else out
    return (out, smap) if source else out


def warp_frames(planes, fmt, transforms, size=None, zoom=1.0, border="constant", fill=(0, 0, 0), matrix="bt709", range="limited",
                out=None):
    """Frames moved by forward transforms on the device: ``warp_coefficients(transforms, size, surface, zoom)`` followed by one
    ``pips_frames_warp`` call (``ops.warp_frames``).  ``planes`` / ``fmt`` are F surfaces in any of ``draw_tracks``' layouts,
    ``transforms`` (F,4) similarities -- ``motion_smooth``'s or ``Stabilizer``'s corrections -- or (F,6) affine rows in the pixels of
    the model's ``size`` = (H, W) (default: the surfaces' own size).  Returns new surfaces (``out`` when given): a tensor for one
    plane, a list otherwise."""
    got, _, h, w = ops.draw_planes(planes, fmt)
    coef = warp_coefficients(transforms, (h, w) if size is None else size, (h, w), zoom)
    res = ops.warp_frames(planes, fmt, coef, border, fill, matrix, range, out=out)
    if out is None:                                                                                # (uint16 planes come back as uint16)
        given = [planes] if torch.is_tensor(planes) else list(planes)
        res = [r.view(p.dtype) for r, p in zip(res, given)]
    else:
        res = [out] if torch.is_tensor(out) else list(out)
    return res[0] if len(res) == 1 else res


def _fill_neighbors(neighbors):
    if isinstance(neighbors, (str, bytes)) or len(tuple(neighbors)) != 2:
        raise ValueError(f"neighbors must be (back, ahead), not {neighbors!r}")
    back, ahead = (_whole(v, "neighbors", 0) for v in neighbors)
    if 1 + back + ahead > ops.WARP_FILL_MAX:
        raise ValueError(f"at most {ops.WARP_FILL_MAX} candidates a frame, not 1 + {back} + {ahead}")
    return back, ahead


def _fill_offsets(back, ahead):
    """the slot order: offset 0, -1, +1, -2, +2, ..., restricted to -back .. +ahead"""
    out = [0]
    for d in _range(1, max(back, ahead) + 1):
        out += ([-d] if d <= back else []) + ([d] if d <= ahead else [])
    return out


def _fill_rows(path, corr, f0, offsets, total):
    """the candidate rows of the frames f0 .. f0 + len(corr) - 1: ``path(g)`` -> (A_g, T_g) complex for a frame 0 <= g < total, corr
    their corrections as lists of four floats -> (frames, transforms) as nested lists.  Slot 0 is the correction itself.  The
    transform of frame g into the stabilised frame f, W_f o P_f^-1 o P_g, is composed in this order of complex operations:
    I = (1 / A_f, -(1 / A_f) T_f); C = (W_a I_a, W_a I_t + W_t); R = (C_a A_g, C_a T_g + C_t)"""
    frames, rows = [], []
    for i, w in enumerate(corr):
        f = f0 + i
        Wa, Wt = complex(w[0], w[1]), complex(w[2], w[3])
        Af, Tf = path(f)
        Ia = 1.0 / Af
        It = -(Ia * Tf)
        Ca, Ct = Wa * Ia, Wa * It + Wt
        fr, tr = [], []
        for off in offsets:
            g = f + off
            if off == 0:
                fr.append(f), tr.append([w[0], w[1], w[2], w[3]])
            elif 0 <= g < total:
                Ag, Tg = path(g)
                Ra, Rt = Ca * Ag, Ca * Tg + Ct
                fr.append(g), tr.append([Ra.real, Ra.imag, Rt.real, Rt.imag])
            else:
                fr.append(-1), tr.append([1.0, 0.0, 0.0, 0.0])
        frames.append(fr), rows.append(tr)
    return frames, rows


def fill_candidates(path, corrections, neighbors=(3, 1), first=0):
    """The candidate lists that fill a stabilised frame's border from its neighbours (``warp_frames_fill``), on the host in float64:
    ``path`` (F,4) is ``motion_path``'s output for the whole video and ``corrections`` (n,4) the rows of ``motion_smooth`` /
    ``Stabilizer`` for the frames ``first .. first + n - 1`` (default: all F) -> ``(frames (n,K) int64, transforms (n,K,4) float64)``
    with K = 1 + back + ahead for ``neighbors`` = (back, ahead).  Slot order: offset 0, -1, +1, -2, +2, ..., restricted to -back ..
    +ahead; ``frames[f][k]`` is the absolute index of the frame in slot k and ``transforms[f][k]`` the similarity that takes its
    positions into the STABILISED frame f: W_f o P_f^-1 o P_g, with P from ``path`` (frame -> frame 0) and W the correction, composed
    in the fixed order of complex operations of ``_fill_rows`` so that ``Stabilizer.candidates`` reproduces the bits; slot 0 is the
    correction itself.  A slot whose frame falls outside [0, F) holds -1 and an identity row -- it is NOT replaced by a farther
    frame, so K is fixed and the streamed form is the one-shot."""
    back, ahead = _fill_neighbors(neighbors)
    path = torch.as_tensor(path).to("cpu", torch.float64)
    corr = torch.as_tensor(corrections).to("cpu", torch.float64)
    first = _whole(first, "first", 0)
    if path.dim() != 2 or path.shape[1] != 4 or corr.dim() != 2 or corr.shape[1] != 4:
        raise ValueError(f"path and corrections must be (F,4) and (n,4), not {tuple(path.shape)} and {tuple(corr.shape)}")
    if first + corr.shape[0] > path.shape[0]:
        raise ValueError(f"corrections of frames [{first}, {first + corr.shape[0]}) of a path with {path.shape[0]} rows")
    if not bool(torch.isfinite(path).all()) or not bool(torch.isfinite(corr).all()):
        raise ValueError("path or corrections has a non-finite entry")
    rows = [(complex(r[0], r[1]), complex(r[2], r[3])) for r in path.tolist()]
    if any(A == 0 for A, _ in rows):
        raise ValueError("a path row with A = 0 has no inverse")
    offsets = _fill_offsets(back, ahead)
    frames, tr = _fill_rows(lambda g: rows[g], corr.tolist(), first, offsets, len(rows))
    return (torch.tensor(frames, dtype=torch.int64).reshape(len(frames), len(offsets)),
            torch.tensor(tr, dtype=torch.float64).reshape(len(tr), len(offsets), 4))


def _fill_setup(planes, fmt, frames, transforms, first, size, zoom):
    """``warp_frames_fill``'s candidate lists -> (cand (F,K) int64 indices into the held surfaces, coef (F,K,6) int32)"""
    _, Fs, h, w = ops.draw_planes(planes, fmt)
    frames = torch.as_tensor(frames).to("cpu")
    t = torch.as_tensor(transforms).to("cpu", torch.float64)
    if frames.dim() != 2 or frames.dtype.is_floating_point or t.dim() != 3 or tuple(t.shape[:2]) != tuple(frames.shape) or t.shape[2] not in (4, 6):
        raise ValueError(f"frames must be integers (F,K) and transforms (F,K,4) or (F,K,6), not {tuple(frames.shape)} and {tuple(t.shape)}")
    frames, first = frames.to(torch.int64), _whole(first, "first", 0)
    held = frames >= 0
    if bool((held & ((frames < first) | (frames >= first + Fs))).any()):
        raise ValueError(f"a candidate frame lies outside the held surfaces [{first}, {first + Fs})")
    F, K = frames.shape
    coef = warp_coefficients(t.reshape(F * K, t.shape[2]), (h, w) if size is None else size, (h, w), zoom).reshape(F, K, 6)
    return torch.where(held, frames - first, torch.full_like(frames, -1)), coef


def warp_frames_fill(planes, fmt, frames, transforms, first=0, size=None, zoom=1.0, border="constant", fill=(0, 0, 0), matrix="bt709",
                     range="limited", out=None, source=None):
    """Stabilised frames whose border is filled from neighbouring frames, on the device: ``warp_coefficients`` on every slot of
    ``fill_candidates``' / ``Stabilizer.candidates``' ``(frames (F,K), transforms (F,K,4))`` followed by one
    ``pips_frames_warp_fill`` call (``ops.warp_frames_fill``).  ``planes`` / ``fmt`` hold the source frames ``first .. first + Fs - 1``
    of the video; ``frames`` are absolute indices, -1 for an empty slot; a non-negative index outside the held range is a
    ValueError.  ``size``, ``zoom``, ``border``, ``fill``, ``matrix``, ``range`` as in ``warp_frames``; ``out`` / ``source`` as in
    ``ops.warp_frames_fill``.  Returns F new surfaces (``out`` when given), a tensor for one plane and a list otherwise, and
    ``(surfaces, map)`` when a source map was asked for.  Known limits: a moving object is shown where the neighbour saw it, no
    feathering or exposure matching at the seam, luma and chroma choose independently, nothing comes from frames outside the list."""
    cand, coef = _fill_setup(planes, fmt, frames, transforms, first, size, zoom)
    res = ops.warp_frames_fill(planes, fmt, cand, coef, border, fill, matrix, range, out=out, source=source)
    res, smap = res if isinstance(res, tuple) else (res, None)
    if out is None:                                                                                # (uint16 planes come back as uint16)
        given = [planes] if torch.is_tensor(planes) else list(planes)
        res = [r.view(p.dtype) for r, p in zip(res, given)]
    else:
        res = [out] if torch.is_tensor(out) else list(out)
    res = res[0] if len(res) == 1 else res
    return res if smap is None else (res, smap)


def crop_zoom(transforms, size, surface=None, margin=1.0 / 128):
    """The automatic crop: the smallest ``zoom`` of ``warp_frames`` / ``warp_frames_fill`` at which every output pixel of every frame
    lands inside its own source frame, so that no border shows.  A closed form on the host, in float64: ``transforms`` (F,4) or
    (F,6), ``size`` and ``surface`` are ``warp_coefficients``'.  With N_f the product that function forms without the zoom (model
    index <- surface index, the inverse forward map, surface index <- model index), L_f its linear part and c the surface centre,
    the corner u of the output lands at N_f c + L_f (u - c) / z.  Per frame, corner and axis, with d the component of L_f (u - c)
    and the slack that of N_f c to the end of [margin, extent - 1 - margin] that d points to: z >= |d| / slack; the maximum over all
    of them is returned (corners suffice: the map is affine).  The identity gives exactly 1.0 at ``margin=0``.  The fixed-point rows of
    ``warp_coefficients`` stand within about 0.003 px of the float map at sides up to 8192 (2^-24 of a linear term times 8192, twice,
    and 2^-17 of the offset): the default margin of 1/128 px keeps the quantised rows inside too.  ValueError when a frame's centre
    lies outside that interval (no zoom can help), for a singular map and for a negative or non-finite margin."""
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin) or margin < 0:
        raise ValueError(f"margin must be a finite number of at least 0, not {margin!r}")
    t, (h, w), S1, S4 = _warp_maps(transforms, size, surface)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    zoom = 0.0
    for a, b, c, d, e, f in t:
        N = (S4 @ (_affine_inverse(a, b, c, d, e, f) @ S1)).tolist()
        for r, extent in ((0, w), (1, h)):
            at = N[r][0] * cx + N[r][1] * cy + N[r][2]
            lo, hi = float(margin), extent - 1 - float(margin)
            if not lo <= at <= hi:
                raise ValueError(f"the centre of a frame under ({a}, {b}, {c}, {d}, {e}, {f}) lands at {at} outside [{lo}, {hi}]")
            for ux in (-cx, cx):
                for uy in (-cy, cy):
                    dist = N[r][0] * ux + N[r][1] * uy
                    slack = hi - at if dist > 0 else at - lo
                    if dist != 0.0:
                        if slack <= 0.0:
                            raise ValueError(f"the centre of a frame under ({a}, {b}, {c}, {d}, {e}, {f}) lies on the margin")
                        zoom = max(zoom, abs(dist) / slack)
    return zoom


class Stabilizer:
    """The corrections that stabilise a streamed video, push by push: ``step(f0, trajs, vis, ids)`` takes the ``(f0, trajs
    (1,m,n,2), vis (1,m,n)[, ids (n,)])`` of a tracker's push, fits the camera motion of its pairs with an internal
    ``MotionEstimator`` (``motion_params``: thr, hypotheses, vis_thr, seed; ``engine`` "library" or "torch"), extends the path with
    ``motion_path``'s two complex operations per pair and returns ``(g0, corrections (k,4) float64)``: the rows W_g of
    ``motion_smooth`` for the frames g0 .. g0 + k - 1 that became FINAL -- frame g is final once frame g + radius has been seen.
    ``finish()`` returns the rest, their windows clamped at the end of the video; ``radius=None`` holds the camera still and makes
    every frame final at once.  All returns together equal ``motion_smooth(motion_path(all models), radius)`` in every bit.
    The stabiliser holds no frames: the caller keeps its surfaces until their corrections come back, as with ``TrackPainter``, and
    warps them then (``warp_frames``).  ``neighbors=(back, ahead)``: after a ``step`` / ``finish`` that returned ``(g0, k rows)``,
    ``candidates(g0, k)`` returns the ``(frames, transforms)`` rows of those frames for ``warp_frames_fill``, equal in every bit to
    ``fill_candidates`` on the whole video's path and corrections.  ``ahead`` may not pass ``radius`` (0 with ``radius=None``): a
    final frame's ``ahead`` neighbours have then been seen; at ``finish`` the slots past the last frame are -1."""

    def __init__(self, radius=15, engine="library", neighbors=None, **motion_params):
        self.radius = _smooth_radius(radius)
        self.neighbors = None if neighbors is None else _fill_neighbors(neighbors)
        if self.neighbors is not None and self.neighbors[1] > (0 if self.radius is None else self.radius):
            raise ValueError(f"neighbors ahead = {self.neighbors[1]} passes radius = {self.radius}: a final frame's neighbours must have been seen")
        self.corr = []                                               # the corrections handed out, for candidates()
        self.estimator = MotionEstimator(engine=engine, **motion_params)
        self.A, self.T = complex(1.0, 0.0), complex(0.0, 0.0)
        self.path, self.g, self.done = [], [], 0                     # (A, T) and parameters of every frame seen; frames handed out

    def _emit(self, upto):
        rows = []
        for f in _range(self.done, upto):
            A, T = self.path[f]
            rows.append([A.real, A.imag, T.real, T.imag] if self.radius is None else _smooth_row(self.g, A, T, f, self.radius))
        g0, self.done = self.done, max(upto, self.done)
        if self.neighbors is not None:
            self.corr += rows
        return g0, torch.tensor(rows, dtype=torch.float64).reshape(len(rows), 4)

    def candidates(self, g0, k):
        """the ``fill_candidates`` rows of the frames g0 .. g0 + k - 1, all of them handed out already -> (frames (k,K) int64,
        transforms (k,K,4) float64).  Called after the ``step`` / ``finish`` that returned them: a slot ahead that has not been
        seen is past the end of the video only then"""
        if self.neighbors is None:
            raise ValueError("candidates() needs Stabilizer(neighbors=(back, ahead))")
        g0, k = _whole(g0, "g0", 0), _whole(k, "k", 0)
        if g0 + k > self.done:
            raise ValueError(f"frames [{g0}, {g0 + k}) have not all been handed out ({self.done} have)")
        offsets = _fill_offsets(*self.neighbors)
        frames, tr = _fill_rows(lambda g: self.path[g], self.corr[g0:g0 + k], g0, offsets, len(self.path))
        return (torch.tensor(frames, dtype=torch.int64).reshape(k, len(offsets)),
                torch.tensor(tr, dtype=torch.float64).reshape(k, len(offsets), 4))

    def _see(self, A, T):
        if self.radius is not None:
            self.g.append(_smooth_params(self.path[-1][0] if self.path else None, self.g[-1][1] if self.g else 0.0, A, T))
        self.path.append((A, T))

    @torch.no_grad()
    def step(self, f0, trajs, vis=None, ids=None):
        first = self.estimator.row is None                           # no row kept: the first row of this push ends no pair
        models = self.estimator.step(f0, trajs, vis, ids)
        if first and trajs.shape[1] > 0:
            self._see(self.A, self.T)
        for a_re, a_im, tx, ty in models.to("cpu", torch.float64).tolist():
            a, t = complex(a_re, a_im), complex(tx, ty)
            if a == 0:
                raise ValueError("a model with a = 0 has no inverse")
            self.A, self.T = self.A / a, self.T - (self.A / a) * t
            self._see(self.A, self.T)
        n = len(self.path)
        return self._emit(n if self.radius is None else max(n - self.radius, 0))

    def finish(self):
        return self._emit(len(self.path))


def find_cuts(rgbs, cut_thr=0.5, scan="torch", slice_frames=64):
    """The scene cuts of a video rgbs (1,T,3,H,W), uint8 or float 0..255 -> the ascending host list of the frames a cut lies
    before: frame f >= 1 whose distance to frame f - 1 (``cut_table_torch``'s) is above ``cut_limit(cut_thr, H, W)``.  The video is
    looked at in slices of ``slice_frames`` frames, the last histogram carried from slice to slice, where it lies (``scan="torch"``)
    or on the GPU (``scan="library"``: a ``pips_cut_table`` call per slice).  A caller of ``track_queries_batch`` splits a video
    there: ``rgbs[:, a:b]`` for consecutive entries a, b of ``[0] + cuts + [T]``."""
    cover = Cover(scan=scan, cut_thr=cut_thr)
    if cover.cut_thr is None:
        raise ValueError("cut_thr must lie in (0, 1), not None")
    if rgbs.dim() != 5 or rgbs.shape[0] != 1 or rgbs.shape[2] != 3:
        raise ValueError(f"rgbs must be (1,T,3,H,W), not {tuple(rgbs.shape)}")
    step = _whole(slice_frames, "slice_frames", 1)
    limit = cut_limit(cover.cut_thr, rgbs.shape[3], rgbs.shape[4])
    cuts, prev = [], None
    for f0 in range(0, rgbs.shape[1], step):
        hist, dist = cover.cut_table(rgbs[0, f0:f0 + step], prev)
        prev = hist[-1]
        cuts += [f0 + f for f in torch.nonzero(dist > limit).squeeze(1).tolist()]
    return cuts


def cover_place_torch(seeds, table, H, W, cell, min_corner):
    """pips_cover_place as torch ops, on any device: seeds (k,3) = (t, x, y) of a cover step and the table (gh,gw,3) of their frame
    -> new seeds, each on the corner of its cell where that scores above ``min_corner`` and where it was otherwise"""
    gh, gw = (int(H) - 1) // int(cell) + 1, (int(W) - 1) // int(cell) + 1

    def cell_of(v, g):                                                                # cover_scan's quotient; no position: cell 0
        q = torch.div(v, float(cell)).floor()
        return torch.where(q >= 0, q, torch.zeros_like(q)).clamp(max=float(g - 1)).to(torch.int64)

    e = table[cell_of(seeds[:, 2], gh), cell_of(seeds[:, 1], gw)]
    use = (e[:, 2] > float(min_corner)).unsqueeze(1)
    return torch.cat([seeds[:, :1], torch.where(use, e[:, :2], seeds[:, 1:])], dim=1)


class _CoverBook:
    """What a covered stream keeps per query beside the tracker's own state: the identity of each column (``ids``), the frame of
    each identity (``born``), identity -> (frame, reason) of the retired ones (``retired``), their hop lists (``hops``, when recorded)
    and, on the device, the arrays a cover step reads -- ``tq`` / ``lost`` (n) int32, ``xy`` (n,2) and ``crowd``, (n) int32 under
    ``Cover(per_cell=)`` and None without.  ``start`` runs the first step (no rows: every query is pending and the seeds land on
    frame 0), ``step`` the one after a push; both act on the tracker through ``add(queries (1,k,3))`` and ``remove(columns)``.
    ``_StreamCore`` is the only caller of ``start`` / ``see`` / ``step`` / ``look`` / ``cut``; its docstring says when each runs.
    Under ``seed="corners"`` the book also keeps ``table`` (T - table0, gh, gw, 3), the best corners of the frames ``[table0, T)``
    that were pushed and not yet returned when the last push began -- ``see`` takes the frames of a push before they are encoded
    -- and ``held``: the ``(frame, seeds)`` of a step whose frame was not pushed yet.  Held seeds have no column and no identity;
    the ``see`` that brings their frame places and adds them before anything of that push is encoded."""

    def __init__(self, cover, tq_host, record_hops):
        self.cover, self.size = cover, None
        self.corners, self.table, self.table0, self.T, self.held = cover.seed == "corners", None, 0, 0, None
        self.ids, self.born, self.retired = list(range(tq_host.numel())), tq_host.tolist(), {}
        self.hops = {} if record_hops else None
        self.prev_hist, self.cuts = None, []           # Cover(cut_thr=): the last pushed frame's histogram; the cut frames so far

    def start(self, H, W, dev, tq_host, xy, add, remove):
        self.size = (int(H), int(W))
        self.tq, self.xy = tq_host.to(dev, torch.int32), xy.to(dev, torch.float32).contiguous()
        self.lost = torch.zeros_like(self.tq)
        self.crowd = None if self.cover.per_cell is None else torch.zeros_like(self.tq)      # (the thin step's second run)
        if self.corners:
            self.table = self.xy.new_empty((0,) + self.cover.grid(int(H), int(W)) + (3,))
        n = self.tq.numel()
        self.step(0, self.xy.new_empty(0, n, 2), self.xy.new_empty(0, n), add, remove, None)

    def step(self, f0, trajs, vis, add, remove, hops, at=None):
        """the cover step on the rows trajs (m,n,2) / vis (m,n) of frames [f0, f0 + m); ``hops``: the hop list of each column.
        ``at``: the step without rows after a cut -- the first step's form (f0 = 0, m = 0) whose seeds land on frame ``at``"""
        n, m = len(self.ids), vis.shape[0]
        f1, (H, W) = f0 + m, self.size
        keep, self.lost, self.crowd, seeds, gone, why, counts = self.cover.step(trajs, vis, f1, self.tq, self.xy, self.lost, self.crowd,
                                                                                H, W)
        if gone:                                                                  # somebody is retired
            for c, r in zip(gone, why):
                self.retired[self.ids[c]] = (f1 - 1, r)
                if self.hops is not None:
                    self.hops[self.ids[c]] = hops[c]
            remove(gone)
            went = set(gone)
            self.ids = [i for c, i in enumerate(self.ids) if c not in went]
            k = keep.to(torch.int64)
            self.tq, self.xy = self.tq[k], self.xy[k]
        if at is not None:
            assert f1 == 0 and counts[0] == n
            f1, seeds = at, torch.cat([torch.full_like(seeds[:, :1], float(at)), seeds[:, 1:]], dim=1)
        if counts[1] > 0:                                                         # and so do the seeds
            if not self.corners:
                self._seed(f1, seeds, add)
            elif f1 < self.T:
                self._seed(f1, self.cover.place(seeds, self.table[f1 - self.table0], H, W), add)
            else:                                                                     # their frame comes with a later push
                assert self.held is None and f1 == self.T
                self.held = (f1, seeds)

    def _seed(self, f1, seeds, add):
        """the seeds (k,3) on frame f1 become queries: the columns and identities behind the present ones"""
        k = seeds.shape[0]
        add(seeds.unsqueeze(0))
        self.ids += list(range(len(self.born), len(self.born) + k))
        self.born += [f1] * k
        self.tq = torch.cat([self.tq, torch.full((k,), f1, dtype=torch.int32, device=self.tq.device)])
        self.xy = torch.cat([self.xy, seeds[:, 1:]])
        self.lost = torch.cat([self.lost, torch.zeros(k, dtype=torch.int32, device=self.tq.device)])
        if self.crowd is not None:
            self.crowd = torch.cat([self.crowd, torch.zeros(k, dtype=torch.int32, device=self.tq.device)])

    def see(self, frames, emitted, add):
        """``seed="corners"``: the frames (k,3,H,W) that a push is about to encode, ``[0, emitted)`` having been returned.  One table
        call for the chunk; the tables of the returned frames go; seeds held for the first of these frames are placed and added"""
        k = frames.shape[0]
        if k == 0:
            return
        new = self.cover.table(frames, self.tq.device)
        self.table = torch.cat([self.table[emitted - self.table0:], new])
        first, self.table0, self.T = self.T, emitted, self.T + k
        if self.held is not None:
            (f1, seeds), self.held = self.held, None
            assert f1 == first
            self._seed(f1, self.cover.place(seeds, self.table[f1 - self.table0], *self.size), add)

    def look(self, frames):
        """``Cover(cut_thr=)``: the frames (k,3,H,W) that a push brings -> the ascending list of the chunk positions a cut lies
        before.  One table call for the chunk; the last frame's histogram is carried to the next push"""
        if frames.shape[0] == 0:
            return []
        hist, dist = self.cover.cut_table(frames, self.prev_hist, self.tq.device)
        self.prev_hist = hist[-1].clone()
        return torch.nonzero(dist > cut_limit(self.cover.cut_thr, *self.size)).squeeze(1).tolist()      # the one host read

    def cut(self, c, keep, hops, add):
        """a cut before frame ``c``: the tracker ended every started query and kept the columns ``keep`` (``_StreamCore._cut``).
        The ended identities are retired as "cut" on frame c - 1, their runs go; then the step without rows seeds frame ``c`` in
        every cell that holds no pending query (seeds held for frame ``c`` by an earlier step are among them again)"""
        kept = keep.tolist()
        for col in sorted(set(range(len(self.ids))) - set(kept)):
            self.retired[self.ids[col]] = (c - 1, "cut")
            if self.hops is not None:
                self.hops[self.ids[col]] = hops[col]
        self.ids = [self.ids[col] for col in kept]
        k = keep.to(self.tq.device)
        self.tq, self.xy, self.lost = self.tq[k], self.xy[k], self.lost[k]
        if self.crowd is not None:
            self.crowd = self.crowd[k]
        self.held = None
        self.cuts.append(c)
        n = len(self.ids)
        self.step(0, self.xy.new_empty(0, n, 2), self.xy.new_empty(0, n), add, None, None, at=c)

    def all_hops(self, live):
        """hop lists by identity: the saved ones of the retired queries and ``live``, those of the present columns"""
        out = dict(self.hops)
        out.update(zip(self.ids, live))
        return [out[i] for i in range(len(self.born))]


def _scatter(parts, col, K, first=0):
    """the ``(f0, trajs, vis, ids)`` parts of a covered stream, frames ``first`` and up -> trajs (1,T,K,2), vis (1,T,K) over the T
    frames the parts hold: identity i in column ``col[i]`` (host int64), NaN where no part has it"""
    T, dev = sum(p[1].shape[1] for p in parts), parts[0][1].device
    trajs = torch.full((1, T, K, 2), float("nan"), dtype=torch.float32, device=dev)
    vis = torch.full((1, T, K), float("nan"), dtype=torch.float32, device=dev)
    for f0, t, v, ids in parts:
        m = t.shape[1]
        if m > 0 and ids.numel() > 0:
            j = col[ids].to(dev)
            trajs[0][f0 - first:f0 - first + m][:, j] = t[0]
            vis[0][f0 - first:f0 - first + m][:, j] = v[0]
    return trajs, vis


def _by_identity(parts, book):
    """the ``(f0, trajs, vis, ids)`` parts of a covered stream -> trajs (1,T,K,2), vis (1,T,K) by identity, NaN outside each life,
    and born (K,), retired (K,) (-1: alive at the end) as host int64"""
    K = len(book.born)
    retired = torch.tensor([book.retired.get(i, (-1,))[0] for i in range(K)], dtype=torch.int64)
    return _scatter(parts, torch.arange(K), K) + (torch.tensor(book.born, dtype=torch.int64), retired)


class CoverTracker:
    """A stream that decides which queries it tracks: the one-stream form of a covered ``_StreamCore`` -- a ``StreamTracker`` (``st``)
    whose core has the policy ``cover`` (a ``Cover``) and the book of stream 0 (``book``); the core's docstring states the rules of a
    covered stream.  ``queries`` (1,N,3) or None are the caller's own; they are tracked, retired and counted like the seeds.
    ``push(frames)`` / ``finish()`` return ``(f0, trajs (1,m,n,2), vis (1,m,n), ids (n,))``: ``ids`` is the identity of each returned
    column (host int64) -- the caller's queries first, then the seeds in order of creation; an identity never changes and is never
    reused.  ``born[i]`` is the frame of identity i, ``retired[i] = (frame, "outside" | "lost" | "crowded" | "cut")`` the last frame
    returned for it and why, ``hops`` (``record_hops=True``) the hop list of each identity, ``cuts`` the cut frames so far.  Over its
    life an identity is what ``track_stream`` given that query alone returns -- an identity of a scene behind a cut, what a
    ``CoverTracker`` started on the cut frame gives it; frames of a retired query that were not returned before its retirement are
    discarded.  The queries are the cover's: ``st.add_queries`` / ``st.remove_queries`` / ``st.cut`` raise ValueError."""

    def __init__(self, model, cover, queries=None, iters=6, slots=24, record_hops=False, engine="torch", rounds="torch"):
        if not isinstance(cover, Cover):
            raise ValueError(f"cover must be a drivers.Cover, not {cover!r}")
        if queries is None:
            queries = torch.zeros(1, 0, 3)
        self.cover = cover
        self.st = StreamTracker(model, queries, iters=iters, slots=slots, record_hops=record_hops, engine=engine, rounds=rounds,
                                _cover=cover)
        self.book = self.st.core.books[0]

    ids = property(lambda self: torch.tensor(self.book.ids, dtype=torch.int64))
    born, retired = (property(lambda self, k=k: getattr(self.book, k)) for k in ("born", "retired"))
    hops = property(lambda self: None if self.book.hops is None else self.book.all_hops(self.st.hops))
    emitted, finished = (property(lambda self, k=k: getattr(self.st, k)) for k in ("emitted", "finished"))
    cuts = property(lambda self: list(self.book.cuts))

    def push(self, frames):
        return self.st.push(frames)

    def finish(self):
        return self.st.finish()


@torch.no_grad()
def track_cover(model, chunks, cover, queries=None, iters=6, slots=24, return_hops=False, engine="torch", rounds="torch"):
    """``CoverTracker`` over an iterable of ``(1,k,3,H,W)`` chunks -> trajs (1,T,K,2) px and vis (1,T,K) logits by identity, NaN
    outside each identity's life, born (K,) and retired (K,) frames (host int64; retired = -1 for those alive at the end).
    ``return_hops=True``: also the hop list of each identity."""
    ct = CoverTracker(model, cover, queries, iters=iters, slots=slots, record_hops=return_hops, engine=engine, rounds=rounds)
    return _joined([ct.push(c) for c in chunks] + [ct.finish()], ct.book, ct.hops, return_hops)


def corner_queries(rgbs, t=0, cell=32, min_corner=0, scan="torch"):
    """Queries for ``track_queries`` on the corners of frame ``t`` of rgbs (1,T,3,H,W): one per cell of the ``cell`` x ``cell`` grid
    whose best corner scores above ``min_corner`` (``Cover(seed="corners")``'s table and rule), in row-major order -> (1,K,3) =
    (t, x, y).  A flat cell gets none.  ``scan="torch"`` works where ``rgbs`` lies, ``scan="library"`` on the GPU."""
    cover = Cover(cell=cell, scan=scan, seed="corners", min_corner=min_corner)
    if rgbs.dim() != 5 or rgbs.shape[0] != 1 or rgbs.shape[2] != 3:
        raise ValueError(f"rgbs must be (1,T,3,H,W), not {tuple(rgbs.shape)}")
    t = _whole(t, "t", 0)
    if t >= rgbs.shape[1]:
        raise ValueError(f"frame {t} of a video of {rgbs.shape[1]} frames")
    e = cover.table(rgbs[0, t:t + 1])[0].reshape(-1, 3)
    e = e[e[:, 2] > float(cover.min_corner)]
    return torch.cat([torch.full_like(e[:, :1], float(t)), e[:, :2]], dim=1).unsqueeze(0)


# ---------------------------------------------------------------------------------------------- several streams at once
class MultiStreamTracker(_StreamCore):
    """``StreamTracker`` for V videos of one frame size at once -- ``_StreamCore`` (whose docstring states the rules) on one cache of V
    rings of ``slots`` slots (``Pips.ring_cache_videos``) and ONE state, V = 1 included: each stream has its own length, chunking,
    queries and end, and gets what a ``StreamTracker`` given that stream alone (same chunks, same ``slots``) returns -- bit for bit,
    hop lists included, while the mixer's GEMMs take the same route at both row counts (the contract of ``track_*_batch``).
      push(chunks)          a list with one ``(1,k_v,3,H,W)`` tensor or ``None`` per stream (the ``k_v`` may differ) -> per stream
                            ``(f0, trajs (1,m,N_v,2), vis (1,m,N_v))``, the frames of that stream that became final
      finish(v=None)        ends stream ``v`` (-> its tuple) or every stream still running (-> the list; None for one ended before)
      add_queries(v, q) / remove_queries(v, cols)   in positions among stream ``v``'s output columns
    ``rounds="torch"`` hops with ``_hop(..., clip=)``; ``rounds="library"`` makes one ``pips_stream_round_clips`` call per round.
    ``joint_encode=True`` sends the frames one wave appends across all streams through shared encoder passes
    (``Pips.encode_streams(joint=True)``): fuller passes, and maps that differ from the per-stream ones by the encoder's
    tile-order noise instead of matching bit for bit.
    ``cover`` (a ``Cover`` without ``cut_thr``; None: the tracker described so far): every stream is covered by the core's rules, the
    ones its own ``CoverTracker`` follows, so ``add_queries`` / ``remove_queries`` are the cover's alone (ValueError for a caller).
    ``push`` and ``finish`` return ``(f0, trajs, vis, ids)`` per stream, ``ids`` being the identity of each column as ``CoverTracker``
    numbers them; ``books[v]`` holds ``born`` / ``retired`` of stream v and ``cover_hops(v)`` its hop lists by identity.  Under
    ``Cover(seed="corners")`` a push makes one corner table per stream that got a chunk, and the first seeds of a stream whose first
    chunk is ``None`` wait for its first frames."""

    def __init__(self, model, queries_list, iters=6, slots=24, record_hops=False, rounds="torch", joint_encode=False, cover=None):
        if cover is not None and not isinstance(cover, Cover):
            raise ValueError(f"cover must be a drivers.Cover or None, not {cover!r}")
        if cover is not None and cover.cut_thr is not None:
            raise ValueError("MultiStreamTracker takes no Cover(cut_thr=): a cut of one stream on the shared rings is not supported")
        super().__init__(model, queries_list, iters, slots, record_hops, "torch", rounds, table=True, joint_encode=joint_encode,
                         cover=cover)


@torch.no_grad()
def track_streams(model, chunk_lists, queries_list, iters=6, slots=24, return_hops=False, rounds="torch", joint_encode=False,
                  cover=None):
    """``MultiStreamTracker`` over V lists of ``(1,k,3,H,W)`` chunks (the lists may differ in length: a stream whose list has run
    out is finished while the others go on) -> per stream what ``track_stream`` returns: ``(trajs_e (1,T_v,N_v,2), vis_e
    (1,T_v,N_v))``, with its hop lists behind them under ``return_hops=True``.  With a ``cover``: per stream what ``track_cover``
    returns."""
    chunk_lists = [list(c) for c in chunk_lists]
    mt = MultiStreamTracker(model, queries_list, iters=iters, slots=slots, record_hops=return_hops, rounds=rounds,
                            joint_encode=joint_encode, cover=cover)
    if len(chunk_lists) != mt.V:
        raise ValueError(f"{len(chunk_lists)} chunk lists for {mt.V} streams")
    parts = [[] for _ in range(mt.V)]
    for i in range(max(len(c) for c in chunk_lists) + 1):
        for v, c in enumerate(chunk_lists):
            if len(c) == i:                                                        # its last chunk went in with the wave before
                parts[v].append(mt.finish(v))
        wave = [c[i] if i < len(c) else None for c in chunk_lists]
        if any(w is not None for w in wave):
            for v, p in enumerate(mt.push(wave)):
                parts[v].append(p)
    hops = (mt.stream_hops if cover is None else mt.cover_hops) if return_hops else (lambda v: None)
    return [_joined(parts[v], None if cover is None else mt.books[v], hops(v), return_hops) for v in range(mt.V)]
