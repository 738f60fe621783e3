"""GPU: several videos in one call -- a per-particle video index on one flat cache (pips_mixer_input_build_clips, pips_track_clips /
Pips.track(win_clip=), Pips.encode_videos, pips_chain_*_clips / Pips.chain_hop(clip=), drivers.track_chained_batch /
track_queries_batch).  Every result is held, bit for bit, to what the single-video form gives on that video alone."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
NAN_FILL = 0x7FC12345          # a NaN with a payload: a stray write shows in the bit patterns
H, W, ST = 128, 160, 8
H8, W8 = H // ST, W // ST
E_ARG = -1


def _model(sd, mode="exact"):
    from pips_amd import Pips
    m = Pips(S=8, stride=ST)
    if sd is not None:
        m.load_state_dict(sd)
    if mode == "split":
        m.matmul = "split"
    if mode == "bf16":
        m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    return m.to(DEV).eval()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _nan_filled(*shape):
    return torch.full(shape, NAN_FILL, dtype=I32).view(torch.float32)


def _mirror_levels(pyr, F):
    """int16 views (F,H_l,W_l,128) of the bf16 mirror behind the fp32 levels"""
    from pips_amd import _lib
    lib = _lib.load()
    mir = pyr[lib.pips_pyramid_mirror_offset(F, H, W, ST):].view(torch.int16)
    out, h, w = [], H8, W8
    for l in range(4):
        off = lib.pips_pyramid_offset(F, H, W, ST, l)
        out.append(mir[off:off + F * h * w * 128].view(F, h, w, 128))
        h, w = h // 2, w // 2
    return out


def _table(lengths):
    frames = torch.tensor(lengths, dtype=I32)
    first = torch.cumsum(frames, 0, dtype=I32) - frames
    return first.to(DEV), frames.to(DEV)


def _random_caches(lengths, seed, mirror):
    """a flat pyramid of sum(lengths) random-filled frames and, per video, the pyramid of its own slice"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(seed)
    F = sum(lengths)
    flat = torch.zeros(lib.pips_pyramid_floats(F, H, W, ST), dtype=torch.float32, device=DEV)
    for lv in ops.pyramid_levels(flat, F, H, W, ST):
        lv.copy_(torch.randn(lv.shape, generator=g))
    own, f0 = [], 0
    for T in lengths:
        p = torch.zeros(lib.pips_pyramid_floats(T, H, W, ST), dtype=torch.float32, device=DEV)
        for d, s in zip(ops.pyramid_levels(p, T, H, W, ST), ops.pyramid_levels(flat, F, H, W, ST)):
            d.copy_(s[f0:f0 + T])
        own.append(p)
        f0 += T
    if mirror:
        ops.pyramid_mirror(flat, F, H, W, ST)
        for p, T in zip(own, lengths):
            ops.pyramid_mirror(p, T, H, W, ST)
    return flat, own


# (video, window start in frames of that video, direction); lengths 9, 5, 13
LENGTHS_A = (9, 5, 13)
WINDOWS = [
    (0, 8, 1),        # the last frame of video 0, forward: repeats it, never video 1's frame 0
    (1, 0, -1),       # frame 0 of video 1, backward: repeats it, never video 0's last frame
    (0, 12, 1),       # past the end of video 0 (flat frame 12 is video 1's frame 3)
    (1, -3, 1),       # negative
    (1, 2, 1),        # runs over the end of the 5-frame video
    (1, 4, -1), (2, 12, -1), (2, 0, 1), (2, 9, 1), (0, 3, -1), (0, 5, 1),
    (2, 40, -1),      # past the end, backward
    (2, -2, -1), (0, 0, 1), (1, 4, 1),
]


def _windows():
    clip = torch.tensor([w[0] for w in WINDOWS], dtype=I32)
    ws = torch.tensor([w[1] for w in WINDOWS], dtype=I32)
    wd = torch.tensor([w[2] for w in WINDOWS], dtype=I32)
    return clip, ws, wd


# ------------------------------------------------------------------ 1. gather and point sample
def _build_win(pyr, T, ff, co, ws, wd, bf16, S):
    """pips_mixer_input_build_win on one video's own pyramid"""
    from pips_amd import _lib, ops
    N = ws.numel()
    X = torch.empty(N * S, 544, dtype=torch.float32, device=DEV)
    tt = ops.times_table(DEV, S)
    _lib.check(_lib.load().pips_mixer_input_build_win(_lib.ptr(pyr), 1, T, H8, W8, _lib.ptr(ff), _lib.ptr(co), _lib.ptr(tt), N,
                                                      _lib.ptr(ws), _lib.ptr(wd), ops.FLAG_BF16_MAPS if bf16 else 0, S, _lib.ptr(X),
                                                      _stream()), "pips_mixer_input_build_win")
    return X


@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_clip_gather_equals_the_gather_on_each_videos_own_slice(S, bf16):
    """pips_mixer_input_build_clips on a flat cache of three random-filled videos (T = 9, 5, 13) against
    pips_mixer_input_build_win on each video's own slice: X rows bitwise equal, fp32 maps and the bf16 mirror, S = 8 and the
    generic S = 5 instantiation; windows at and over both ends of their video, starts past the end and negative ones.  A video
    index outside the table is clamped into it (-1 -> video 0, 7 -> video 2)."""
    from pips_amd import ops
    g = torch.Generator().manual_seed(41)
    flat, own = _random_caches(LENGTHS_A, 40, bf16)
    F = sum(LENGTHS_A)
    first, frames = _table(LENGTHS_A)
    clip, ws, wd = _windows()
    clip_in = torch.cat([clip, torch.tensor([-1, 7], dtype=I32)])            # corrupt indices: contained
    clip = torch.cat([clip, torch.tensor([0, 2], dtype=I32)])
    ws, wd = torch.cat([ws, torch.tensor([7, 10], dtype=I32)]), torch.cat([wd, torch.tensor([1, 1], dtype=I32)])
    N = clip.numel()
    ff = torch.randn(N * S, 128, generator=g).to(DEV)
    co = (torch.rand(N * S, 2, generator=g) * torch.tensor([W8 + 4.0, H8 + 4.0]) - 2.0).to(DEV)
    got = ops.mixer_input_build_clips(flat, F, H8, W8, ff, co, ws.to(DEV), wd.to(DEV), clip_in.to(DEV), first, frames, bf16, S)
    assert bool(torch.isfinite(got).all())
    rows = torch.arange(N * S).view(N, S)
    for v, T in enumerate(LENGTHS_A):
        sel = torch.nonzero(clip == v).squeeze(1)
        r = rows[sel].reshape(-1).to(DEV)
        ref = _build_win(own[v], T, ff[r].contiguous(), co[r].contiguous(), ws[sel].to(DEV), wd[sel].to(DEV), bf16, S)
        assert torch.equal(got[r], ref), f"video {v}"
    # the table matters: the same windows read as frames of the flat axis give other rows at the videos' ends
    plain = ops.mixer_input_build_clips(flat, F, H8, W8, ff, co, (ws + first.cpu()[clip.long()]).to(DEV), wd.to(DEV), None, None, None,
                                        bf16, S)
    for j in (0, 1):
        assert not torch.equal(plain[rows[j].to(DEV)], got[rows[j].to(DEV)])
    assert torch.equal(plain[rows[7].to(DEV)], got[rows[7].to(DEV)])         # a window inside its video: the same frames


def _cache(pyr, lengths=None, T=None):
    from pips_amd.pips import FeatureCache
    c = FeatureCache(pyr, 1, sum(lengths) if lengths else T, H, W, ST)
    if lengths:
        c.clip_lengths = list(lengths)
        c.clip_first, c.clip_frames = _table(lengths)
    return c


def test_clip_point_sample_equals_the_point_sample_on_each_videos_own_slice():
    """The point sample of the first window (feat_init = NULL; Pips.track with iters = 0 returns it) reads
    clip_first[v] + clamp(win_start, 0, T_v - 1): bitwise the sample on the video's own slice, border positions included."""
    g = torch.Generator().manual_seed(43)
    flat, own = _random_caches(LENGTHS_A, 42, False)
    clip, ws, wd = _windows()
    N = clip.numel()
    xy = torch.rand(1, N, 2, generator=g) * torch.tensor([W + 8.0, H + 8.0]) - 4.0
    xy[0, 0] = torch.tensor([0.0, 0.0])
    xy[0, 1] = torch.tensor([W - 1.0, H - 1.0])
    m = _model(None)
    got = m.track(_cache(flat, LENGTHS_A), xy.to(DEV), iters=0, win_start=ws.view(1, -1), win_dir=wd.view(1, -1),
                  win_clip=clip.view(1, -1), return_feat=True)[3]
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    for v, T in enumerate(LENGTHS_A):
        sel = torch.nonzero(clip == v).squeeze(1)
        ref = m.track(_cache(own[v], T=T), xy[:, sel].to(DEV), iters=0, win_start=ws[sel].view(1, -1), win_dir=wd[sel].view(1, -1),
                      return_feat=True)[3]
        assert torch.equal(got[:, sel.to(DEV)], ref), f"video {v}"


# ------------------------------------------------------------------ shared videos
def _video(T, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


@functools.lru_cache(maxsize=None)
def _videos(lengths):
    return tuple(_video(T, 50 + i).to(DEV) for i, T in enumerate(lengths))


def _assert_route_0(particle_counts, mode):
    """every GEMM of the mixer takes route 0 (rows computed independently of M) at M = 8 n for each n"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    for n in particle_counts:
        M = 8 * n
        if mode == "bf16":
            res = 2 | ops.EPI_RES_BF16
            shapes = [(M, 512, 544, 0, 0, 1), (M, 2048, 512, 1, 1, 1), (M, 512, 2048, res, 1, 1), (n, 1040, 512, 0, 0, 0)]
            assert all(lib.pips_gemm_bf16_route(*s) == 0 for s in shapes), n
        else:
            shapes = [(M, 512, 544, 0), (M, 2048, 512, 1), (M, 512, 2048, 2), (n, 1040, 512, 0)]
            assert all(lib.pips_gemm_f32_route(*s) == 0 for s in shapes), n


# ------------------------------------------------------------------ 2. tracker
@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
def test_track_with_win_clip_equals_track_on_each_video(weights_tamed, mode):
    """Pips.track(win_clip=) on the mixed particles of three videos against Pips.track on encode(video) for each: every
    iterate, the visibility and the initial features torch.equal (exact fp32, matmul='split', the bf16 mode), with the
    sampled features and with feat_init given.  All row counts on GEMM route 0, asserted first."""
    m = _model(weights_tamed, mode)
    videos = _videos(LENGTHS_A)
    clip, ws, wd = _windows()
    N = clip.numel()
    _assert_route_0([N] + [int((clip == v).sum()) for v in range(3)], mode)
    g = torch.Generator().manual_seed(44)
    xy = (torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    fi = torch.randn(1, N, 128, generator=g).to(DEV) * 0.1
    flat = m.encode_videos(videos)
    own = [m.encode(v) for v in videos]
    for feat in (None, fi):
        got = m.track(flat, xy, iters=3, win_start=ws.view(1, -1), win_dir=wd.view(1, -1), win_clip=clip.view(1, -1),
                      feat_init=feat, return_feat=True)
        for v in range(3):
            sel = torch.nonzero(clip == v).squeeze(1)
            sd = sel.to(DEV)
            ref = m.track(own[v], xy[:, sd], iters=3, win_start=ws[sel].view(1, -1), win_dir=wd[sel].view(1, -1),
                          feat_init=None if feat is None else feat[:, sd], return_feat=True)
            assert all(torch.equal(a[:, :, sd], b) for a, b in zip(got[0], ref[0])), f"video {v}"
            assert torch.equal(got[2][:, :, sd], ref[2]) and torch.equal(got[3][:, sd], ref[3]), f"video {v}"
    assert bool(torch.isfinite(got[0][-1]).all())


# ------------------------------------------------------------------ 3. encoder
LENGTHS_B = (13, 9, 21)


@pytest.mark.parametrize("frames_per_pass", [16, 8])
@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_encode_videos_is_encode_per_video(weights_tamed, mode, frames_per_pass):
    """encode_videos: each video's slice of the flat levels (and, in the bf16 mode, of the mirror) is encode(video) byte for
    byte, with one pass per video and with several (13 = 8 + 5 frames, 21 = 16 + 5 = 8 + 8 + 5); the clip table is the lengths."""
    from pips_amd import ops
    m = _model(weights_tamed, mode)
    videos = _videos(LENGTHS_B)
    flat = m.encode_videos(videos, frames_per_pass=frames_per_pass)
    F = sum(LENGTHS_B)
    assert (flat.B, flat.T, flat.slots, flat.clip_lengths) == (1, F, F, list(LENGTHS_B))
    assert flat.clip_frames.dtype == I32 and flat.clip_frames.tolist() == list(LENGTHS_B) and flat.clip_first.tolist() == [0, 13, 22]
    assert flat.bf16_maps == (mode == "bf16")
    lv, f0 = ops.pyramid_levels(flat.pyr, F, H, W, ST), 0
    for video, T in zip(videos, LENGTHS_B):
        one = m.encode(video, frames_per_pass=frames_per_pass)
        for a, b in zip(lv, ops.pyramid_levels(one.pyr, T, H, W, ST)):
            assert torch.equal(_bits(a[f0:f0 + T]), _bits(b))
        if mode == "bf16":
            for a, b in zip(_mirror_levels(flat.pyr, F), _mirror_levels(one.pyr, T)):
                assert torch.equal(a[f0:f0 + T], b)
        f0 += T


# ------------------------------------------------------------------ 4. drivers
def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, n, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0


XY0S = [_points(n, 60 + i) for i, n in enumerate((5, 16, 9))]
TQS = ([0, 12, 5, 5, 8], [8, 0, 3, 8, 1, 4, 7, 0, 0, 2, 6, 0, 5, 0, 3, 8], [20, 0, 13, 7, 19, 9, 9, 2, 16])
QUERIES = [torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), _points(len(tq), 70 + i)], dim=-1)
           for i, tq in enumerate(TQS)]


def test_track_chained_batch_equals_track_chained_on_both_engines(weights_tamed):
    """Three videos (T = 13, 9, 21; 5, 16 and 9 points): per video the bits and the hops of track_chained, torch engine and
    native engine alike."""
    from pips_amd import drivers
    m = _model(weights_tamed)
    videos = _videos(LENGTHS_B)
    xy0s = [x.to(DEV) for x in XY0S]
    _assert_route_0([sum(x.shape[1] for x in XY0S)], "exact")
    got = drivers.track_chained_batch(m, videos, xy0s, iters=6, return_hops=True)
    nat = drivers.track_chained_batch(m, videos, xy0s, iters=6, return_hops=True, engine="native")
    plain = drivers.track_chained_batch(m, videos, xy0s, iters=6, engine="native")
    for v, (video, xy0, T) in enumerate(zip(videos, xy0s, LENGTHS_B)):
        ref, ref_hops = drivers.track_chained(m, video, xy0, iters=6, return_hops=True)
        assert tuple(ref.shape) == (1, T, xy0.shape[1], 2) and any(len(h) > 1 for h in ref_hops)
        for tr, hops in (got[v], nat[v]):
            assert hops == ref_hops and torch.equal(tr, ref), f"video {v}"
        assert torch.equal(plain[v], ref)


def test_track_queries_batch_equals_track_queries_on_both_engines(weights_tamed):
    """The same videos with 5, 16 and 9 queries at frames 0 .. T_v - 1 (duplicates, first and last frames): per video the
    trajectories, visibilities and both hop lists of track_queries, torch engine and native engine alike."""
    from pips_amd import drivers
    m = _model(weights_tamed)
    videos = _videos(LENGTHS_B)
    qs = [q.to(DEV) for q in QUERIES]
    _assert_route_0([sum(len(tq) + sum(t > 0 for t in tq) for tq in TQS)], "exact")
    got = drivers.track_queries_batch(m, videos, qs, iters=6, return_hops=True)
    nat = drivers.track_queries_batch(m, videos, qs, iters=6, return_hops=True, engine="native")
    for v, (video, q, T) in enumerate(zip(videos, qs, LENGTHS_B)):
        ref, ref_vis, ref_hops = drivers.track_queries(m, video, q, iters=6, return_hops=True)
        assert tuple(ref.shape) == (1, T, q.shape[1], 2)
        for tr, vi, hops in (got[v], nat[v]):
            assert hops == ref_hops, f"video {v}"
            assert torch.equal(tr, ref) and torch.equal(vi, ref_vis), f"video {v}"
    assert any(len(h) > 1 for h in got[2][2][0]) and any(len(h) > 1 for h in got[2][2][1])


# ------------------------------------------------------------------ 5. chain stages
ACTIVE = [0, 1, 3, 4, 6, 9, 10, 12, 13, 15, 17, 18, 20, 21, 23, 24, 26, 28, 30, 31, 33, 35, 36]
N_ALL = 37
P_SET = (0.05, 0.5, 0.85, 0.87, 0.89, 0.91, 0.95)       # each >= 0.01 from every threshold 0.9 - 0.02 k
LENGTHS_C = (9, 21, 13)


def _synthetic(seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = 0.05, 0.95
    only2 = [lo, lo, hi, lo, lo, lo, lo, lo]               # si = 2
    f36 = [lo, lo, lo, hi, lo, lo, hi, lo]                 # si = 6
    # (video, cur, dir, confidences)
    named = [(0, 7, 1, only2),          # lands on 9 = past the end of ITS 9-frame video: finished, while ...
             (1, 7, 1, only2),          # ... the same step in the 21-frame video stays live
             (0, 6, 1, only2),          # lands on 8 = the last frame of video 0: live
             (2, 7, 1, f36),            # lands on 13 = T_2: finished (below the longest video's 21)
             (2, 6, 1, f36),            # lands on 12: live
             (1, 15, 1, f36),           # lands on 21 = T_1: finished
             (0, 1, -1, only2),         # backward, lands on -1: finished
             (2, 6, -1, f36),           # backward, lands on 0: live
             (-4, 7, 1, only2),         # video index below the table: video 0, finished
             (9, 11, 1, only2)]         # above it: the last video (13 frames), lands on 13: finished
    n_act = len(ACTIVE)
    clip = torch.randint(0, 3, (N_ALL,), generator=g).to(I32)
    cur = torch.randint(0, 9, (N_ALL,), generator=g).to(I32)
    dirs = torch.where(torch.rand(N_ALL, generator=g) < 0.5, -1, 1).to(I32)
    pick = torch.tensor(P_SET)[torch.randint(0, len(P_SET), (8, n_act), generator=g)]
    for j, (v, c, d, ps) in enumerate(named):
        clip[ACTIVE[j]], cur[ACTIVE[j]], dirs[ACTIVE[j]] = v, c, d
        pick[:, j] = torch.tensor(ps)
    win_vis = torch.log(pick.double() / (1.0 - pick.double())).float()
    L = max(LENGTHS_C) + 14
    return dict(L=L, base=7, n=N_ALL, n_act=n_act, active=torch.tensor(ACTIVE, dtype=I32), cur=cur, dirs=dirs, clip=clip,
                win_vis=win_vis, win_trajs=torch.randn(8, n_act, 2, generator=g) * 50,
                win_ffeat0=torch.randn(n_act, 128, generator=g), feat=torch.randn(N_ALL, 128, generator=g),
                trajs=_nan_filled(L, N_ALL, 2), vis=_nan_filled(L, N_ALL))


def _expected_step(s, with_vis, sample_feat):
    """The lines of drivers._hop after the track call and of drivers._TorchEngine.hop after it, on the CPU."""
    from pips_amd import drivers
    L, base = s["L"], s["base"]
    active = s["active"].long()
    trajs, vis, cur, feat = s["trajs"].clone(), s["vis"].clone(), s["cur"].clone().long(), s["feat"].clone()
    c = cur[active]
    d = torch.where(s["dirs"].long()[active] < 0, -1, 1)
    rows = (c.unsqueeze(0) + torch.arange(8).unsqueeze(1) * d.unsqueeze(0) + base) % L
    cols = active.unsqueeze(0).expand(8, -1)
    trajs[rows, cols] = s["win_trajs"]
    if with_vis:
        vis[rows, cols] = s["win_vis"]
    si = drivers.skip_scan(torch.sigmoid(s["win_vis"]))
    c = c + si * d
    cur[active] = c
    if sample_feat:
        feat[active] = s["win_ffeat0"]
    end = torch.tensor(LENGTHS_C)[s["clip"].long().clamp(0, len(LENGTHS_C) - 1)][active]
    live = (c < end) & (c >= 0)
    return dict(trajs=trajs, vis=vis, cur=cur.to(I32), feat=feat, steps=si.to(I32), next_active=active[live].to(I32))


@pytest.mark.parametrize("sample_feat", [False, True])
@pytest.mark.parametrize("with_vis", [True, False])
def test_chain_stages_with_clips_are_the_torch_lines_of_hop(with_vis, sample_feat):
    """pips_chain_gather_clips and pips_chain_step_clips on 23 of 37 particles of three videos (T = 9, 21, 13; L = 35, base 7)
    against skip_scan and _hop's indexed assignments with the live test of _TorchEngine.hop, c < T of the particle's own video:
    the staged video indices, steps, window starts, the compacted list and its count, the carried features, and trajs / vis as
    bit patterns over the whole NaN-payload buffers.  A particle of the 9-frame video finishes on frame 9 while the same step
    in the 21-frame video stays live."""
    from pips_amd import ops
    s = _synthetic(seed=45)
    exp = _expected_step(s, with_vis, sample_feat)
    act, nxt_exp = s["active"].tolist(), exp["next_active"].tolist()
    newc = exp["cur"].long()[s["active"].long()].tolist()
    assert exp["steps"].tolist()[:5] == [2, 2, 2, 6, 6]
    assert newc[0] == 9 and act[0] not in nxt_exp and newc[1] == 9 and act[1] in nxt_exp
    assert newc[2] == 8 and act[2] in nxt_exp and newc[3] == 13 and act[3] not in nxt_exp and act[4] in nxt_exp
    assert newc[5] == 21 and act[5] not in nxt_exp and newc[6] == -1 and act[6] not in nxt_exp and newc[7] == 0 and act[7] in nxt_exp
    assert act[8] not in nxt_exp and act[9] not in nxt_exp
    n_act = s["n_act"]
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    vis = d["vis"] if with_vis else None
    frames = torch.tensor(LENGTHS_C, dtype=I32, device=DEV)
    a = s["active"].long()
    xy, ws, wd, wc, fi = ops.chain_gather(d["trajs"], s["base"], d["cur"], d["dirs"], d["feat"], d["active"], n_act, sample_feat,
                                          clip=d["clip"])
    assert torch.equal(_bits(xy), _bits(s["trajs"][(s["cur"].long()[a] + s["base"]) % s["L"], a]))
    assert torch.equal(ws.cpu(), s["cur"][a]) and torch.equal(wd.cpu(), s["dirs"][a]) and torch.equal(wc.cpu(), s["clip"][a])
    if not sample_feat:
        assert torch.equal(fi.cpu(), s["feat"][a])
    nxt = torch.full((n_act,), -77, dtype=I32, device=DEV)
    count = torch.full((1,), -1, dtype=I32, device=DEV)
    steps = torch.full((n_act,), -1, dtype=I32, device=DEV)
    # T (the flat cache's frames) is not what ends a particle
    ops.chain_step(d["win_trajs"], d["win_vis"], d["win_ffeat0"], sum(LENGTHS_C), d["active"], n_act, d["trajs"], vis, s["base"],
                   d["cur"], d["dirs"], d["feat"], nxt, count, steps, sample_feat=sample_feat, clips=(d["clip"], frames))
    torch.cuda.synchronize()
    k = exp["next_active"].numel()
    assert int(count.item()) == k
    assert torch.equal(nxt.cpu()[:k], exp["next_active"]) and bool((nxt.cpu()[k:] == -77).all())
    assert torch.equal(steps.cpu(), exp["steps"]) and torch.equal(d["cur"].cpu(), exp["cur"])
    assert torch.equal(_bits(d["feat"]), _bits(exp["feat"]))
    assert torch.equal(_bits(d["trajs"]), _bits(exp["trajs"])) and torch.equal(_bits(d["vis"]), _bits(exp["vis"]))
    assert int((_bits(exp["trajs"]) != NAN_FILL).sum()) == 8 * n_act * 2


# ------------------------------------------------------------------ 6. argument errors
def test_clip_gather_and_track_reject_bad_arguments_and_write_nothing():
    """Every PIPS_E_ARG case of pips_mixer_input_build_clips and pips_track_clips -- V < 1, a NULL table, win_clip without
    win_start, B != 1, a ring (R != T), the score-map block -- returns its code ahead of any launch: X, the outputs and the
    workspace keep their bit patterns."""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(46)
    lengths = (3, 2)
    F, N, S, iters = 5, 4, 8, 1
    first, frames = _table(lengths)
    pyr = torch.zeros(lib.pips_pyramid_floats(2 * F, H, W, ST), dtype=torch.float32, device=DEV)    # (room for the B = 2 case)
    ff = torch.randn(N * S, 128, generator=g).to(DEV)
    co = (torch.rand(N * S, 2, generator=g) * 10 + 2).to(DEV)
    tt = ops.times_table(DEV, S)
    ws = torch.zeros(N, dtype=I32, device=DEV)
    wd = torch.ones(N, dtype=I32, device=DEV)
    wc = torch.tensor([0, 1, 1, 0], dtype=I32, device=DEV)
    X = _nan_filled(2 * N * S, 544).to(DEV)
    good = dict(B=1, T=F, R=F, ws=ws, wc=wc, first=first, frames=frames, V=2, ce=None)
    bad = [dict(V=0), dict(V=-3), dict(first=None), dict(frames=None), dict(ws=None), dict(B=2), dict(R=F - 1), dict(R=F + 1)]
    p = _lib.ptr

    def gather(**over):
        a = dict(good, **over)
        return lib.pips_mixer_input_build_clips(p(pyr), a["B"], a["T"], a["R"], H8, W8, p(ff), p(co), p(tt), N, p(a["ws"]), p(wd),
                                                p(a["wc"]), p(a["first"]), p(a["frames"]), a["V"], 0, S, p(X), _stream())
    for over in bad:
        assert gather(**over) == E_ARG, over
        assert lib.pips_last_error()
        torch.cuda.synchronize()
        assert bool((_bits(X) == NAN_FILL).all()), over
    assert gather() == 0 and gather(wc=None, first=None, frames=None, V=0) == 0       # without win_clip the table is not read
    torch.cuda.synchronize()
    assert bool(torch.isfinite(X[:N * S]).all())

    # the tracker
    arena = _model(None)._aux(torch.device(DEV))[0]
    nb = lib.pips_track_workspace_bytes_s(2, N, S)
    work = _nan_filled(nb // 4).to(DEV)
    xy = (torch.rand(2, N, 2, generator=g) * 100 + 10).to(DEV)
    outs = dict(trajs=_nan_filled(iters + 1, 2, S, N, 2).to(DEV), vis=_nan_filled(2, S, N).to(DEV), ffeat=_nan_filled(2, N, 128).to(DEV),
                terms=_nan_filled(iters, 2 * N * S, 2).to(DEV))
    ce_tgt = torch.zeros(N * S, 3, device=DEV)
    ce_ws = torch.zeros(max(lib.pips_score_map_workspace_bytes(1, F, H8, W8) // 4, 1), device=DEV)

    def track(**over):
        a = dict(good, **over)
        ce = a["ce"]
        return lib.pips_track_clips(p(arena), p(pyr), a["B"], a["T"], a["R"], H8, W8, p(xy), None, None, p(a["ws"]), p(wd), p(a["wc"]),
                                    p(a["first"]), p(a["frames"]), a["V"], p(tt), N, ST, iters, 0, S, p(work), nb, p(outs["trajs"]),
                                    p(outs["vis"]), p(outs["ffeat"]), p(ce), p(outs["terms"]) if ce is not None else None,
                                    p(ce_ws) if ce is not None else None, ce_ws.numel() * 4 if ce is not None else 0, _stream())
    for over in bad + [dict(ce=ce_tgt)]:
        assert track(**over) == E_ARG, over
        assert lib.pips_last_error()
        torch.cuda.synchronize()
        assert all(bool((_bits(t) == NAN_FILL).all()) for t in list(outs.values()) + [work]), over
    assert track() == 0
    torch.cuda.synchronize()
    # (the buffers have room for B = 2: the accepted B = 1 call fills the first (iters + 1, 1, S, N, 2) / (1, S, N) elements)
    assert bool(torch.isfinite(outs["trajs"].flatten()[:(iters + 1) * S * N * 2]).all())
    assert bool(torch.isfinite(outs["vis"].flatten()[:S * N]).all())
    assert bool((_bits(outs["trajs"]).flatten()[(iters + 1) * S * N * 2:] == NAN_FILL).all())


def test_chain_clip_forms_reject_bad_arguments_and_leave_the_state_alone():
    """pips_chain_hop_clips (V < 1, a NULL clip_first / clip_frames, R != T), pips_chain_step_clips (V < 1, a NULL clip_frames)
    and pips_chain_gather_clips (a NULL wc) return PIPS_E_ARG ahead of any launch; trajs, vis, cur, feat, next_active,
    next_count, steps and the staging arrays keep their bit patterns."""
    from pips_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(47)
    n, n_act, L, T, iters = 12, 5, 24, 10, 2
    state = dict(trajs=torch.randn(L, n, 2, generator=g), vis=torch.randn(L, n, generator=g),
                 cur=torch.randint(0, 4, (n,), generator=g).to(I32), feat=torch.randn(n, 128, generator=g),
                 next_active=torch.full((n,), -77, dtype=I32), next_count=torch.full((1,), 99, dtype=I32),
                 steps=torch.full((n,), -5, dtype=I32), xy=_nan_filled(n_act, 2), ws=torch.full((n_act,), -9, dtype=I32),
                 wd=torch.full((n_act,), -9, dtype=I32), fi=_nan_filled(n_act, 128))
    dev = {k: v.to(DEV) for k, v in state.items()}
    active = torch.tensor([1, 4, 5, 8, 11], dtype=I32, device=DEV)
    clip = torch.randint(0, 2, (n,), generator=g).to(I32).to(DEV)
    first, frames = _table((6, 4))
    nb = lib.pips_chain_workspace_bytes(n_act, iters)
    ws = torch.zeros(nb // 4, device=DEV)
    dummy = torch.zeros(64, device=DEV)                      # stands for the arena, the pyramid, the time table and the windows: never read
    good = dict(R=T, clip=clip, first=first, frames=frames, V=2, wc=dev["ws"])
    p = _lib.ptr

    def untouched():
        torch.cuda.synchronize()
        for k, v in state.items():
            assert torch.equal(_bits(dev[k]), _bits(v)), k

    def hop(**over):
        a = dict(good, **over)
        return lib.pips_chain_hop_clips(p(dummy), p(dummy), T, a["R"], 16, 20, p(dummy), 8, iters, 0, n, p(active), n_act, 1,
                                        p(dev["trajs"]), p(dev["vis"]), L, 7, p(dev["cur"]), None, p(a["clip"]), p(a["first"]),
                                        p(a["frames"]), a["V"], p(dev["feat"]), p(dev["next_active"]), p(dev["next_count"]),
                                        p(dev["steps"]), p(ws), nb, _stream())

    def step(**over):
        a = dict(good, **over)
        return lib.pips_chain_step_clips(p(dummy), p(dummy), p(dummy), T, n, p(active), n_act, 1, p(dev["trajs"]), p(dev["vis"]), L, 7,
                                         p(dev["cur"]), None, p(a["clip"]), p(a["frames"]), a["V"], p(dev["feat"]),
                                         p(dev["next_active"]), p(dev["next_count"]), p(dev["steps"]), _stream())

    def gather(**over):
        a = dict(good, **over)
        return lib.pips_chain_gather_clips(p(dev["trajs"]), L, 7, n, p(dev["cur"]), None, p(a["clip"]), p(dev["feat"]), p(active), n_act,
                                           0, p(dev["xy"]), p(dev["ws"]), p(dev["wd"]), p(a["wc"]), p(dev["fi"]), _stream())
    for over in (dict(V=0), dict(V=-1), dict(first=None), dict(frames=None), dict(R=T - 1), dict(R=T + 1)):
        assert hop(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    for over in (dict(V=0), dict(frames=None)):
        assert step(**over) == E_ARG, over
        untouched()
    assert gather(wc=None) == E_ARG
    untouched()
    assert math.isnan(float(dev["xy"][0, 0]))
