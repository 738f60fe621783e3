"""GPU: tracking from any frame, forwards and backwards in time -- the per-particle window direction ``win_dir`` of the direct
correlation gather (pips_mixer_input_build_win), of the tracker (pips_track_win / Pips.track) and the driver built on it
(drivers.track_queries).  A backward window from frame f is a forward window from T-1-f on the frame-flipped maps, bit for
bit; the driver is held to the reference's chaining loop (oracle/chain_oracle.py) run on sliced and flipped videos."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(sd, stride=8, S=8):
    from pips_amd import Pips
    m = Pips(S=S, stride=stride)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV).eval()


def _flip_frames(pyr, B, T, H, W, stride, bf16):
    """A packed pyramid with the frames of every clip in reverse order (fp32 levels moved, bf16 mirror rewritten from them)."""
    from pips_amd import ops
    out = torch.empty_like(pyr)
    for d, s in zip(ops.pyramid_levels(out, B * T, H, W, stride), ops.pyramid_levels(pyr, B * T, H, W, stride)):
        d.copy_(s.reshape(B, T, *s.shape[1:]).flip(1).reshape(s.shape))
    if bf16:
        ops.pyramid_mirror(out, B * T, H, W, stride)
    return out


def _build_win(pyr, B, T, H8, W8, ff, co, N, S, ws, wd, flags):
    from pips_amd import _lib, ops
    lib = _lib.load()
    X = torch.empty(B * N * S, 544, dtype=torch.float32, device=DEV)
    tt = ops.times_table(DEV, S)
    _lib.check(lib.pips_mixer_input_build_win(_lib.ptr(pyr), B, T, H8, W8, _lib.ptr(ff), _lib.ptr(co), _lib.ptr(tt), N,
                                              _lib.ptr(ws), _lib.ptr(wd), flags, S, _lib.ptr(X),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pips_mixer_input_build_win")
    return X


@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_backward_gather_is_forward_gather_on_flipped_maps(S, bf16):
    """pips_mixer_input_build_win: row s of a particle with win_dir < 0 and start f reads frame clamp(f - s, 0, T-1) -- the
    same bits as a forward window from T-1-f on the frame-flipped pyramid (fp32 levels and the bf16 mirror; S = 8 and the
    generic S = 5 instantiation; starts at both ends so the clamp is hit; both directions in one launch)."""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(21)
    B, T, H, W, st = 2, 11, 128, 160, 8
    H8, W8 = H // st, W // st
    pyr = torch.empty(lib.pips_pyramid_floats(B * T, H, W, st), dtype=torch.float32, device=DEV)
    pyr.zero_()
    for lv in ops.pyramid_levels(pyr, B * T, H, W, st):
        lv.copy_(torch.randn(lv.shape, generator=g))
    if bf16:
        ops.pyramid_mirror(pyr, B * T, H, W, st)
    fl = 32 if bf16 else 0                                                                 # PIPS_FLAG_BF16_MAPS
    starts = torch.tensor([0, 1, 2, 5, T - 3, T - 2, T - 1, 4, T - 1, 0], dtype=torch.int32)
    N = starts.numel()
    dirs = torch.tensor([-1, -1, -7, 1, -1, 1, -1, 3, 1, 1], dtype=torch.int32)         # any negative value is backward
    ws = starts.repeat(B).to(DEV)
    wd = dirs.repeat(B).to(DEV)
    ff = torch.randn(B * N * S, 128, generator=g).to(DEV)
    co = (torch.rand(B * N * S, 2, generator=g) * torch.tensor([W8 + 4.0, H8 + 4.0]) - 2.0).to(DEV)   # borders included
    X = _build_win(pyr, B, T, H8, W8, ff, co, N, S, ws, wd, fl).view(B, N, S, 544)
    back = (wd < 0).view(B, N)
    flip = _flip_frames(pyr, B, T, H, W, st, bf16)
    fwd_ref = _build_win(pyr, B, T, H8, W8, ff, co, N, S, ws, None, fl).view(B, N, S, 544)
    bwd_ref = _build_win(flip, B, T, H8, W8, ff, co, N, S, (T - 1 - ws).contiguous(), None, fl).view(B, N, S, 544)
    assert bool(back.any()) and bool((~back).any())
    assert torch.equal(X[back], bwd_ref[back]) and torch.equal(X[~back], fwd_ref[~back])
    # the windows really differ from the forward ones on the same maps (the direction is not ignored)
    assert not torch.equal(X[back][..., 128:324], fwd_ref[back][..., 128:324])
    if S == 8:                                                              # win_dir = NULL is pips_mixer_input_build_ex
        Xex = torch.empty_like(X.view(-1, 544))
        _lib.check(lib.pips_mixer_input_build_ex(_lib.ptr(pyr), B, T, H8, W8, _lib.ptr(ff), _lib.ptr(co),
                                                 _lib.ptr(ops.times_table(DEV)), N, _lib.ptr(ws), fl, _lib.ptr(Xex),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pips_mixer_input_build_ex")
        assert torch.equal(Xex.view(B, N, S, 544), fwd_ref)


def _video(T, H, W, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


@pytest.mark.parametrize("mode", ["exact", "split", "bf16", "s5"])
def test_backward_track_is_forward_track_on_flipped_cache(weights_tamed, mode):
    """Pips.track(cache, xys, win_start=f, win_dir=-1) equals Pips.track on the frame-flipped cache from T-1-f: trajectories,
    visibility and the initial features, bit for bit (exact fp32, matmul='split', the bf16 mode, and S = 5)."""
    from pips_amd.pips import FeatureCache
    m = _model(None if mode == "s5" else weights_tamed, S=5 if mode == "s5" else 8)
    if mode == "split":
        m.matmul = "split"
    if mode == "bf16":
        m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    T, H, W = 13, 128, 160
    video = _video(T, H, W, seed=22).to(DEV)
    cache = m.encode(video)
    assert cache.bf16_maps == (mode == "bf16")
    flip = FeatureCache(_flip_frames(cache.pyr, 1, T, H, W, 8, cache.bf16_maps), 1, T, H, W, 8, bf16_maps=cache.bf16_maps)
    g = torch.Generator().manual_seed(23)
    f = torch.tensor([[0, 2, 6, T - 2, T - 1, 4, 1]])
    N = f.shape[1]
    xys = (torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    got = m.track(cache, xys, iters=4, win_start=f, win_dir=torch.full((1, N), -1), return_feat=True)
    ref = m.track(flip, xys, iters=4, win_start=T - 1 - f, return_feat=True)
    for a, b in zip(got[0] + [got[2], got[3]], ref[0] + [ref[2], ref[3]]):
        assert torch.equal(a, b)
    fwd = m.track(cache, xys, iters=4, win_start=f, return_feat=True)
    assert not torch.equal(fwd[0][-1], got[0][-1])                               # the direction reaches the gather
    same = m.track(cache, xys, iters=4, win_start=f, win_dir=torch.ones(1, N, dtype=torch.int32), return_feat=True)
    for a, b in zip(fwd[0] + [fwd[2], fwd[3]], same[0] + [same[2], same[3]]):
        assert torch.equal(a, b)                                                  # win_dir = +1 is the forward track


def _oracle_queries(chain, tq, xy, video, **kw):
    """The reference's loop per query frame: forward on video[:, t:], backward on video[:, :t+1].flip(1) flipped back.
    -> trajs (1,T,N,2) on the CPU, forward and backward hop sequences per query."""
    T, N = video.shape[1], len(tq)
    out = torch.zeros(1, T, N, 2)
    fh, bh = [None] * N, [[] for _ in range(N)]
    for t in sorted(set(tq)):
        idx = [n for n in range(N) if tq[n] == t]
        x = xy[:, idx]
        ref, hops = chain(video[:, t:], x, **kw)
        out[:, t:, idx] = ref.cpu()
        for n, h in zip(idx, hops):
            fh[n] = h
        if t > 0:
            ref, hops = chain(video[:, :t + 1].flip(1), x, **kw)
            out[:, :t, idx] = ref.flip(1)[:, :t].cpu()
            for n, h in zip(idx, hops):
                bh[n] = h
        del ref
        torch.cuda.empty_cache()
    return out, fh, bh


def test_track_queries_against_reference_loop(weights_tamed):
    """drivers.track_queries at T = 21, 128x160, stride 8: queries at frames 0, 3, 10, 17, 20 (duplicates included) against
    oracle/chain_oracle.chain (CPU, frame maps cached) on the sliced and flipped videos -- identical hop sequences in both
    directions and 1e-3 px over all T x N positions."""
    from functools import partial
    from pips_amd import drivers
    from oracle import chain_oracle
    T, H, W = 21, 128, 160
    video = _video(T, H, W, seed=24)
    tq = [0, 3, 10, 17, 20, 20, 3, 10]
    g = torch.Generator().manual_seed(25)
    xy = torch.rand(1, len(tq), 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    q = torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), xy], dim=-1)
    ref, rfh, rbh = _oracle_queries(partial(chain_oracle.chain, weights_tamed, iters=6, stride=8, cache_frames=True), tq, xy, video)
    got, vis, (fh, bh) = drivers.track_queries(_model(weights_tamed), video.to(DEV), q.to(DEV), iters=6, return_hops=True)
    err = float((got.cpu() - ref).abs().max())
    print("track_queries vs reference loop: max |dtraj| %.2e px; forward hops %s; backward hops %s" % (err, fh, bh))
    assert tuple(got.shape) == (1, T, len(tq), 2) and tuple(vis.shape) == (1, T, len(tq))
    assert any(len(h) > 1 for h in bh)
    assert fh == rfh and bh == rbh
    assert err < 1e-3
    assert bool(torch.isfinite(vis).all())


def test_track_queries_at_frame_zero_against_reference_loop_text_golden(weights_tamed):
    """All queries at t = 0: drivers.track_queries is the reference's own loop text (tests/golden/chain_t13.npz) -- the same
    window starts and hop steps, trajectories within 1e-3 px."""
    import os
    from pips_amd import drivers
    case = G.CHAIN_CASE
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "chain_t13.npz"))
    video, xy0 = G.make_chain_inputs(case)
    q = torch.cat([torch.zeros(1, case["N"], 1), xy0], dim=-1)
    got, vis, (hops, bh) = drivers.track_queries(_model(weights_tamed, case["stride"]), video.to(DEV), q.to(DEV),
                                                 iters=case["iters"], return_hops=True)
    starts = []
    for seq in hops:
        cur = 0
        for si in seq:
            starts.append(cur)
            cur += si
    assert bh == [[]] * case["N"]
    assert starts == gold["window_starts"].tolist()
    assert [si for seq in hops for si in seq[:-1]] == gold["hop_steps"].tolist()
    assert [len(seq) - 1 for seq in hops] == gold["hops_per_particle"].tolist()
    err = float((got.cpu() - torch.from_numpy(gold["trajs_e"])).abs().max())
    print("track_queries (t = 0) vs reference loop text: max |dtraj| = %.2e px" % err)
    assert tuple(got.shape) == (1, case["T"], case["N"], 2) and err < 1e-3


def test_track_queries_config5_size_against_oracle_on_device(weights_tamed):
    """BASELINE configs[4] geometry: 100 frames of 360x640, stride 4, N = 256 queries split over frames 0, 33, 66 and 99,
    against oracle/chain_oracle.chain_lockstep on the same GPU per query frame and direction (sliced and flipped videos).
    Gate: identical hop sequences in both directions for every query and 1e-3 px over all 100 x 256 positions."""
    from functools import partial
    from pips_amd import drivers
    from oracle import chain_oracle
    T, H, W, N = 100, 360, 640, 256
    video = _video(T, H, W, seed=9, slope=0.005, step=1.2, noise=30).to(DEV)
    gy, gx = torch.meshgrid(torch.linspace(16, H - 17, 16), torch.linspace(16, W - 17, 16), indexing="ij")
    xy = torch.stack([gx.reshape(-1), gy.reshape(-1)], -1).unsqueeze(0).to(DEV)
    tq = [(0, 33, 66, 99)[n % 4] for n in range(N)]
    sd = {k: v.to(DEV) for k, v in weights_tamed.items()}
    ref, rfh, rbh = _oracle_queries(partial(chain_oracle.chain_lockstep, sd, iters=6, stride=4), tq, xy, video)
    del sd
    torch.cuda.empty_cache()
    q = torch.cat([torch.tensor(tq, dtype=torch.float32, device=DEV).view(1, N, 1), xy], dim=-1)
    got, vis, (fh, bh) = drivers.track_queries(_model(weights_tamed, stride=4), video, q, iters=6, return_hops=True)
    err = float((got.cpu() - ref).abs().max())
    diff = [n for n in range(N) if fh[n] != rfh[n] or bh[n] != rbh[n]]
    nh = sum(len(h) for h in fh) + sum(len(h) for h in bh)
    print(f"track_queries at config-5 size (T=100, N=256 over frames 0/33/66/99): max |dtraj| {err:.2e} px, {nh} windows, "
          f"queries with a different hop sequence: {len(diff)}")
    assert tuple(got.shape) == (1, T, N, 2)
    assert not diff
    assert err < 1e-3
