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

Host logic only (a few tiny torch ops on (8,N) tensors); all model arithmetic is in
libpips_hip.so through ``Pips.encode`` / ``Pips.track``.
"""
from __future__ import annotations

import torch


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


def _chain(model, cache, T, xy, f0, dirs=None, iters=6, with_vis=True):
    """The hop loop of chain_demo.py:40-83 for all particles at once.  xy (n,2) px at frames f0 (n,) int64; dirs (n,) +1 / -1
    per particle or None (all forward).  A backward particle runs the loop on the time-reversed video: its window rows
    read f, f-1, ... (``Pips.track``'s ``win_dir``) and it is finished when its start passes frame 0.
    -> trajs (T,n,2), vis (T,n) logits (None without ``with_vis``) -- each frame from the last window that wrote it -- and
    the hop log [(active, si)]."""
    dev = xy.device
    S = 8
    pad = S - 1
    n = xy.shape[0]
    # S - 1 frames of padding on both sides of the video: a window that runs past either end is written whole and cut off
    # on return (no per-row masks, no host round trips inside a hop)
    trajs = torch.zeros(1, T + 2 * pad, n, 2, dtype=torch.float32, device=dev)
    vis_p = torch.zeros(1, T + 2 * pad, n, dtype=torch.float32, device=dev) if with_vis else None
    active = torch.arange(n, device=dev)
    cur = f0 + pad                                                                 # window starts in padded frames
    trajs[0, cur, active] = xy.to(torch.float32)
    offs = torch.arange(S, device=dev).unsqueeze(1)                                # (S,1)
    feat = None
    log = []
    while active.numel() > 0:
        c = cur[active]
        start_xy = trajs[0, c, active].unsqueeze(0)                               # traj_e[:,cur_frame]
        fi = None if feat is None else feat[active].unsqueeze(0)
        kw, rows = {}, offs
        if dirs is not None:
            d = dirs[active]
            kw["win_dir"] = d.to(torch.int32).unsqueeze(0)
            rows = offs * d.unsqueeze(0)                                          # row s of a window is frame c + d * s
        preds, _, vis, ffeat, _ = model.track(cache, start_xy, iters=iters, feat_init=fi,
                                              win_start=(c - pad).to(torch.int32).unsqueeze(0), return_feat=True, **kw)
        if feat is None:
            feat = ffeat[0].clone()                                              # carried forever (:57)
        rows = c.unsqueeze(0) + rows                                              # (S,n)
        cols = active.unsqueeze(0).expand(S, -1)
        trajs[0, rows, cols] = preds[-1][0]                                       # traj_e[cur:cur+8] = xys[:S_local]
        if vis_p is not None:
            vis_p[0, rows, cols] = vis[0]
        si = skip_scan(torch.sigmoid(vis[0]))
        c = c + (si if dirs is None else si * d)
        cur[active] = c
        log.append((active, si))
        live = c < T + pad if dirs is None else (c < T + pad) & (c >= pad)
        active = active[live]                                                     # (one host sync per hop: the live count)
    return trajs[0, pad:pad + T], None if vis_p is None else vis_p[0, pad:pad + T], log


def _hops(log, n):
    hops = [[] for _ in range(n)]
    for act, si in log:
        for k, s in zip(act.tolist(), si.tolist()):
            hops[k].append(s)
    return hops


@torch.no_grad()
def track_chained(model, rgbs, xy0, iters=6, return_hops=False):
    """rgbs (1,T,3,H,W), xy0 (1,N,2) px at frame 0 -> trajs_e (1,T,N,2) (chain_demo.run_model).
    ``return_hops=True``: also the list, per particle, of the frame steps ``si`` its windows advanced by
    (chain_demo.py:63-79) -- what a parity test compares hop for hop."""
    assert rgbs.shape[0] == 1, "the reference chains one video at a time (chain_demo.py:24)"
    assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
    dev = rgbs.device
    T, N = rgbs.shape[1], xy0.shape[1]
    cache = model.encode(rgbs)
    trajs, _, log = _chain(model, cache, T, xy0[0].to(dev), torch.zeros(N, dtype=torch.int64, device=dev), iters=iters,
                           with_vis=False)
    out = trajs.unsqueeze(0).contiguous()
    if not return_hops:
        return out
    return out, _hops(log, N)


@torch.no_grad()
def track_queries(model, rgbs, queries, iters=6, return_hops=False):
    """Track query points from any frame over the whole video, forwards and backwards in time.

    rgbs (1,T,3,H,W), queries (1,N,3) = (t, x, y): ``t`` an integer frame index, ``x, y`` in pixels -- PIPs' xy order, not
    TAP-Vid's (t, y, x).  -> trajs_e (1,T,N,2) px and vis_e (1,T,N) logits (the units of ``forward``'s vis_e).

    Frames t >= t_q come from the reference's chaining loop (chain_demo.py:40-83) run on ``rgbs[:, t_q:]``, frames t < t_q
    from the same loop on the time-reversed ``rgbs[:, :t_q+1].flip(1)``, flipped back; within each chain the last window
    that wrote a frame gives its position and visibility.  The video is encoded once; every query is a forward particle,
    plus a backward one when t_q > 0, and all of them advance together, one ``model.track`` call per hop.
    ``return_hops=True``: also ``(forward, backward)``, per query the frame steps of each chain's windows (backward: [] when
    t_q = 0)."""
    assert rgbs.shape[0] == 1 and queries.shape[0] == 1, "one video at a time, as track_chained"
    assert model.S == 8, "chain_demo.py's visibility scan (frames 7..2 of an 8-frame window) is written for S = 8"
    dev = rgbs.device
    T, N = rgbs.shape[1], queries.shape[1]
    if queries.dim() != 3 or queries.shape[2] != 3:
        raise ValueError(f"queries must be (1,N,3) = (t, x, y), not {tuple(queries.shape)}")
    t = queries[0, :, 0].detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(t).all()) or not torch.equal(t, t.round()) or bool(((t < 0) | (t > T - 1)).any()):
        raise ValueError(f"query frames must be integers in [0, {T - 1}]")
    tq = t.to(torch.int64)
    back = torch.nonzero(tq > 0).squeeze(1)
    nb = back.numel()
    xy = queries[0, :, 1:3].to(dev, torch.float32)
    tq_d, back_d = tq.to(dev), back.to(dev)
    f0 = torch.cat([tq_d, tq_d[back_d]])
    dirs = torch.cat([torch.ones(N, dtype=torch.int64, device=dev), torch.full((nb,), -1, dtype=torch.int64, device=dev)])
    cache = model.encode(rgbs)
    tr, vi, log = _chain(model, cache, T, torch.cat([xy, xy[back_d]]), f0, dirs, iters=iters)
    trajs, vis = tr[:, :N].clone(), vi[:, :N].clone()
    before = torch.arange(T, device=dev).unsqueeze(1) < tq_d[back_d].unsqueeze(0)     # (T,nb): frames of the backward chain
    trajs[:, back_d] = torch.where(before.unsqueeze(-1), tr[:, N:], trajs[:, back_d])
    vis[:, back_d] = torch.where(before, vi[:, N:], vis[:, back_d])
    trajs, vis = trajs.unsqueeze(0), vis.unsqueeze(0)
    if not return_hops:
        return trajs, vis
    hops = _hops(log, N + nb)
    bwd = [[] for _ in range(N)]
    for j, q in enumerate(back.tolist()):
        bwd[q] = hops[N + j]
    return trajs, vis, (hops[:N], bwd)
