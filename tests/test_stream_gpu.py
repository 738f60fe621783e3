"""GPU: streamed video through a ring of encoded frames -- ring addressing of the direct gather and the tracker
(pips_mixer_input_build_ring, pips_track_ring / Pips.track on a ring cache), the append kernel (pips_pyramid_append /
Pips.encode(..., into=)) and the driver built on them (drivers.track_stream), held to the linear cache bit for bit, to
track_chained and to the reference's chaining loop (oracle/chain_oracle.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(sd, stride=8, S=8):
    from pips_amd import Pips
    m = Pips(S=S, stride=stride)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV).eval()


def _mirror_levels(pyr, F, H, W, stride):
    """int16 views (F,H_l,W_l,128) of the bf16 mirror behind the fp32 levels"""
    from pips_amd import _lib
    lib = _lib.load()
    mir = pyr[lib.pips_pyramid_mirror_offset(F, H, W, stride):].view(torch.int16)
    out, h, w = [], H // stride, W // stride
    for l in range(4):
        off = lib.pips_pyramid_offset(F, H, W, stride, l)
        out.append(mir[off:off + F * h * w * 128].view(F, h, w, 128))
        h, w = h // 2, w // 2
    return out


def _ring_from(pyr, T, R, frames, H, W, stride, mirror):
    """a ring pyramid of R slots holding the given logical frames of a linear T-frame pyramid (frame f in slot f % R)"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    ring = torch.zeros(lib.pips_pyramid_floats(R, H, W, stride), dtype=torch.float32, device=DEV)
    for d, s in zip(ops.pyramid_levels(ring, R, H, W, stride), ops.pyramid_levels(pyr, T, H, W, stride)):
        for f in frames:
            d[f % R].copy_(s[f])
    if mirror:
        ops.pyramid_mirror(ring, R, H, W, stride)
    return ring


def _build(pyr, T, R, H8, W8, ff, co, N, S, ws, wd, flags):
    from pips_amd import _lib, ops
    lib = _lib.load()
    X = torch.empty(N * S, 544, dtype=torch.float32, device=DEV)
    tt, st = ops.times_table(DEV, S), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if R is None:
        rc = lib.pips_mixer_input_build_win(_lib.ptr(pyr), 1, T, H8, W8, _lib.ptr(ff), _lib.ptr(co), _lib.ptr(tt), N,
                                            _lib.ptr(ws), _lib.ptr(wd), flags, S, _lib.ptr(X), st)
    else:
        rc = lib.pips_mixer_input_build_ring(_lib.ptr(pyr), 1, T, R, H8, W8, _lib.ptr(ff), _lib.ptr(co), _lib.ptr(tt), N,
                                             _lib.ptr(ws), _lib.ptr(wd), flags, S, _lib.ptr(X), st)
    _lib.check(rc, "pips_mixer_input_build")
    return X


@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_ring_gather_equals_linear_gather(S, bf16):
    """pips_mixer_input_build_ring with T = 20 logical frames in R = 12 slots holding frames 8..19 (wrapped) is the linear
    build of the same windows bit for bit: forward windows from 8..19 (clamped at frame 19), backward ones whose frames are
    all held, fp32 levels and the bf16 mirror, S = 8 and the generic S = 5 instantiation."""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(31)
    T, R, H, W, st = 20, 12, 128, 160, 8
    H8, W8 = H // st, W // st
    pyr = torch.zeros(lib.pips_pyramid_floats(T, H, W, st), dtype=torch.float32, device=DEV)
    for lv in ops.pyramid_levels(pyr, T, H, W, st):
        lv.copy_(torch.randn(lv.shape, generator=g))
    if bf16:
        ops.pyramid_mirror(pyr, T, H, W, st)
    ring = _ring_from(pyr, T, R, range(8, T), H, W, st, bf16)
    starts = torch.tensor([8, 9, 11, 12, 15, 18, 19, T - 1, 16, 19, 8 + S - 1, 17], dtype=torch.int32)
    dirs = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -3], dtype=torch.int32)
    N = starts.numel()
    ws, wd = starts.to(DEV), dirs.to(DEV)
    ff = torch.randn(N * S, 128, generator=g).to(DEV)
    co = (torch.rand(N * S, 2, generator=g) * torch.tensor([W8 + 4.0, H8 + 4.0]) - 2.0).to(DEV)
    fl = 32 if bf16 else 0                                                                   # PIPS_FLAG_BF16_MAPS
    got = _build(ring, T, R, H8, W8, ff, co, N, S, ws, wd, fl)
    ref = _build(pyr, T, None, H8, W8, ff, co, N, S, ws, wd, fl)
    assert torch.equal(got, ref)
    # the linear cache is the ring of R = T slots
    assert torch.equal(_build(pyr, T, T, H8, W8, ff, co, N, S, ws, wd, fl), ref)


def _video(T, H, W, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


def _mode(m, mode):
    if mode == "split":
        m.matmul = "split"
    if mode == "bf16":
        m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    return m


@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
def test_track_on_ring_equals_linear(weights_tamed, mode):
    """Pips.track on a ring cache (12 slots holding frames 8..19 of 20) equals Pips.track on the linear cache: trajectories,
    visibility and initial features bit for bit, with feat_init = None (the point sample reads the ring) and given, windows
    clamped at the last frame included (exact fp32, matmul='split', the bf16 mode)."""
    from pips_amd.pips import FeatureCache
    m = _mode(_model(weights_tamed), mode)
    T, R, H, W = 20, 12, 128, 160
    lin = m.encode(_video(T, H, W, seed=32).to(DEV))
    ring = FeatureCache(_ring_from(lin.pyr, T, R, range(8, T), H, W, 8, lin.bf16_maps), 1, T, H, W, 8,
                        bf16_maps=lin.bf16_maps, slots=R)
    g = torch.Generator().manual_seed(33)
    f = torch.tensor([[8, 9, 12, 13, 16, 18, 19, 11]])
    N = f.shape[1]
    xys = (torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    feat = torch.randn(1, N, 128, generator=g).to(DEV)
    for fi in (None, feat):
        got = m.track(ring, xys, iters=4, win_start=f, feat_init=fi, return_feat=True)
        ref = m.track(lin, xys, iters=4, win_start=f, feat_init=fi, return_feat=True)
        for a, b in zip(got[0] + [got[2], got[3]], ref[0] + [ref[2], ref[3]]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_append_wraps_into_ring(weights_tamed, mode):
    """Pips.encode(chunk, into=ring) in chunks of 5 into 12 slots (pips_pyramid_append, wrapping): after every chunk the
    slots of the last min(T, 12) frames hold exactly the fp32 levels and the bf16 mirror bytes of Pips.encode of the whole
    23-frame video (more frames than frames_per_pass, so both mirrors are written from the fp32 levels), in the fp32 and
    the bf16 encoder modes."""
    from pips_amd import ops
    m = _mode(_model(weights_tamed), mode)
    T, R, H, W, st = 23, 12, 128, 160, 8
    video = _video(T, H, W, seed=34)
    lin = m.encode(video.to(DEV), frames_per_pass=5)
    if mode == "exact":                                   # the fp32 encoder leaves the mirror unwritten: write it here
        ops.pyramid_mirror(lin.pyr, T, H, W, st)
    ring = m.ring_cache(H, W, R)
    lin_lv = ops.pyramid_levels(lin.pyr, T, H, W, st) + _mirror_levels(lin.pyr, T, H, W, st)
    for t0 in range(0, T, 5):
        m.encode(video[:, t0:t0 + 5].to(torch.uint8), into=ring)          # host frames, uint8: read as they are
        assert ring.T == min(T, t0 + 5) and ring.slots == R and ring.bf16_maps == (mode == "bf16")
        ring_lv = ops.pyramid_levels(ring.pyr, R, H, W, st) + _mirror_levels(ring.pyr, R, H, W, st)
        for f in range(max(0, ring.T - R), ring.T):
            for a, b in zip(ring_lv, lin_lv):
                assert torch.equal(a[f % R], b[f])


def test_stream_single_chunk_is_track_chained(weights_tamed):
    """One chunk, slots >= T + 8, all queries at t = 0: track_stream is track_chained -- torch.equal trajectories and identical
    hop sequences."""
    from pips_amd import drivers
    T, H, W, N = 21, 128, 160, 16
    video = _video(T, H, W, seed=35).to(DEV)
    g = torch.Generator().manual_seed(36)
    xy = (torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    m = _model(weights_tamed)
    q = torch.cat([torch.zeros(1, N, 1, device=DEV), xy], dim=-1)
    got, vis, hops = drivers.track_stream(m, [video], q, iters=6, slots=T + 8, return_hops=True)
    ref, ref_h = drivers.track_chained(m, video, xy, iters=6, return_hops=True)
    assert any(len(h) > 1 for h in hops)
    assert hops == ref_h and torch.equal(got, ref)
    assert bool(torch.isfinite(vis).all())


def test_track_stream_against_reference_loop(weights_tamed):
    """drivers.track_stream at T = 21, 128x160, stride 8, chunks of 5 and 16 slots, queries at frames 0, 3, 10, 17, 20
    (duplicates included) against oracle/chain_oracle.chain on video[:, t_q:] -- identical hop sequences and 1e-3 px over
    every frame from t_q on (the gate of test_queries_gpu.py); NaN before t_q."""
    from pips_amd import drivers
    from oracle import chain_oracle
    T, H, W = 21, 128, 160
    video = _video(T, H, W, seed=37)
    tq = [0, 3, 10, 17, 20, 20, 3, 10]
    N = len(tq)
    g = torch.Generator().manual_seed(38)
    xy = torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    q = torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), xy], dim=-1)
    chunks = [video[:, i:i + 5] for i in range(0, T, 5)]                                  # host chunks
    got, vis, hops = drivers.track_stream(_model(weights_tamed), chunks, q.to(DEV), iters=6, slots=16, return_hops=True)
    got = got.cpu()
    err = 0.0
    for t in sorted(set(tq)):
        idx = [n for n in range(N) if tq[n] == t]
        ref, rh = chain_oracle.chain(weights_tamed, video[:, t:], xy[:, idx], iters=6, stride=8, cache_frames=True)
        for j, n in enumerate(idx):
            assert hops[n] == rh[j]
            err = max(err, float((got[0, t:, n] - ref[0, :, j].cpu()).abs().max()))
            assert bool(got[0, :t, n].isnan().all()) and bool(vis[0, :t, n].isnan().all())
            assert bool(torch.isfinite(vis[0, t:, n]).all())
    print("track_stream vs reference loop: max |dtraj| %.2e px; hops %s" % (err, hops))
    assert err < 1e-3


def test_stream_memory_is_bounded(weights_tamed):
    """Stride 4: the peak allocation while streaming 144 frames exceeds that of 48 frames by less than one frame's pyramid
    (frames made chunk by chunk on the host; the returned trajectories are the only state that grows with T)."""
    from pips_amd import _lib, drivers
    H, W, st = 128, 192, 4
    m = _model(weights_tamed, stride=st)
    g = torch.Generator().manual_seed(39)
    N = 32
    xy = torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    q = torch.cat([torch.tensor([(0, 5, 20)[n % 3] for n in range(N)], dtype=torch.float32).view(1, N, 1), xy], dim=-1).to(DEV)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).to(torch.uint8)

    def chunks(T):
        for t0 in range(0, T, 16):
            k = min(16, T - t0)
            yield ((base.float() + 3.0 * torch.arange(t0, t0 + k).view(1, k, 1, 1, 1)) % 256).to(torch.uint8)

    def peak(T):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        out = drivers.track_stream(m, chunks(T), q, iters=6, slots=24)
        torch.cuda.synchronize()
        assert out[0].shape[1] == T and bool(torch.isfinite(out[0][0, 20:]).all())
        del out
        return torch.cuda.max_memory_allocated() - start

    peak(48)                                                        # warm-up: weights, workspaces
    p48, p144 = peak(48), peak(144)
    frame = _lib.load().pips_pyramid_floats(1, H, W, st) * 4
    print(f"stream peak: T=48 {p48 / 2**20:.1f} MiB, T=144 {p144 / 2**20:.1f} MiB, one frame's pyramid {frame / 2**20:.2f} MiB")
    assert p144 - p48 < frame
