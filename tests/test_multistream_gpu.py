"""GPU: several streamed videos at once -- V rings on one flat cache behind a clip table (pips_mixer_input_build_rings,
pips_track_rings / Pips.track(win_clip=) on Pips.ring_cache_videos, pips_pyramid_append_at / Pips.encode(into=, clip=)), one state
for the queries of all streams (pips_stream_select_clips / pips_stream_round_clips / pips_stream_emit_cols) and
drivers.MultiStreamTracker.  The stages are held, bit for bit, to the single-ring forms on each stream's own ring and to torch
restatements written here; the drivers to ``track_stream`` on each stream alone and to the reference's chaining loop."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
INT_MAX = 2 ** 31 - 1
NAN_FILL = 0x7FC12345          # a NaN with a payload: a stray write shows in the bit patterns
QUIET_NAN = 0x7FC00000
H, W, ST = 128, 160, 8
H8, W8 = H // ST, W // ST
E_ARG, E_WORKSPACE = -1, -2


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


def _levels(pyr, F):
    from pips_amd import ops
    return ops.pyramid_levels(pyr, F, H, W, ST)


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


def _video(T, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


def _queries(tq, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(1, len(tq), 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    return torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), xy], dim=-1)


def _assert_route_0(n_max, mode):
    """every GEMM of the mixer takes route 0 (rows computed independently of M) at M = 8 k for every row count k <= n_max a round
    can have: a query then computes the same bits whichever queries -- of whichever streams -- share its round"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    for k in range(1, n_max + 1):
        M = 8 * k
        if mode == "bf16":
            res = 2 | ops.EPI_RES_BF16
            shapes = [(M, 512, 544, 0, 0, 1), (M, 2048, 512, 1, 1, 1), (M, 512, 2048, res, 1, 1), (k, 1040, 512, 0, 0, 0)]
            assert all(lib.pips_gemm_bf16_route(*s) == 0 for s in shapes), k
        else:
            shapes = [(M, 512, 544, 0), (M, 2048, 512, 1), (M, 512, 2048, 2), (k, 1040, 512, 0)]
            assert all(lib.pips_gemm_f32_route(*s) == 0 for s in shapes), k


# ------------------------------------------------------------------ (a) gather and point sample on rings of clips
R_ = 9
FRAMES_A = (9, 14, 5)            # full and not wrapped / wrapped (frames 5..13 held) / short
# (stream, window start in frames of that stream, direction)
WINDOWS = [
    (0, 0, 1), (0, 8, 1), (0, 12, 1), (0, -3, 1), (0, 3, -1), (0, 5, 1), (0, 8, -1),
    (1, 6, 1),        # across the wrap: frames 6..13 live in slots 6, 7, 8, 0, 1, 2, 3, 4 of the ring
    (1, 13, -1),      # the same slots backwards
    (1, 13, 1),       # the last frame, repeated
    (1, 40, -1),      # past the end, backward
    (1, -2, 1), (1, 9, 1), (1, 8, -1), (1, 11, 1),
    (2, 0, 1), (2, 2, 1), (2, 4, -1), (2, -3, 1), (2, 7, 1), (2, 0, -1),
]


def _windows():
    return tuple(torch.tensor([w[i] for w in WINDOWS], dtype=I32) for i in range(3))


def _ring_table(frames, R=R_):
    return (torch.arange(len(frames), dtype=I32) * R).to(DEV), torch.tensor(frames, dtype=I32).to(DEV)


def _random_rings(V, seed, mirror):
    """a flat pyramid of V rings of R_ random-filled slots and, per stream, the ring pyramid of its own slots"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(seed)
    F = V * R_
    flat = torch.zeros(lib.pips_pyramid_floats(F, H, W, ST), dtype=torch.float32, device=DEV)
    for lv in _levels(flat, F):
        lv.copy_(torch.randn(lv.shape, generator=g))
    own = []
    for v in range(V):
        p = torch.zeros(lib.pips_pyramid_floats(R_, H, W, ST), dtype=torch.float32, device=DEV)
        for d, s in zip(_levels(p, R_), _levels(flat, F)):
            d.copy_(s[v * R_:(v + 1) * R_])
        own.append(p)
    if mirror:
        ops.pyramid_mirror(flat, F, H, W, ST)
        for p in own:
            ops.pyramid_mirror(p, R_, H, W, ST)
    return flat, own


def _build_ring(pyr, T, ff, co, ws, wd, bf16, S):
    """pips_mixer_input_build_ring on one stream's own ring of R_ slots holding T logical frames"""
    from pips_amd import _lib, ops
    N = ws.numel()
    X = torch.empty(N * S, 544, dtype=torch.float32, device=DEV)
    tt = ops.times_table(DEV, S)
    _lib.check(_lib.load().pips_mixer_input_build_ring(_lib.ptr(pyr), 1, T, R_, H8, W8, _lib.ptr(ff), _lib.ptr(co), _lib.ptr(tt), N,
                                                       _lib.ptr(ws), _lib.ptr(wd), ops.FLAG_BF16_MAPS if bf16 else 0, S,
                                                       _lib.ptr(X), _stream()), "pips_mixer_input_build_ring")
    return X


@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_ring_gather_equals_the_gather_on_each_streams_own_ring(S, bf16):
    """pips_mixer_input_build_rings on V = 3 rings of 9 random-filled slots holding 9 (full, not wrapped), 14 (wrapped) and 5
    (short) logical frames against pips_mixer_input_build_ring on each stream's own ring buffer: X rows bitwise equal, fp32 maps
    and the bf16 mirror, S = 8 and the generic S = 5 instantiation; windows at both ends, both directions, negative starts,
    starts past the end and across the wrap.  A stream index outside the table is clamped into it."""
    from pips_amd import ops
    g = torch.Generator().manual_seed(71)
    flat, own = _random_rings(3, 70, bf16)
    F = 3 * R_
    first, frames = _ring_table(FRAMES_A)
    clip, ws, wd = _windows()
    clip_in = torch.cat([clip, torch.tensor([-1, 7], dtype=I32)])            # corrupt indices: contained
    clip = torch.cat([clip, torch.tensor([0, 2], dtype=I32)])
    ws, wd = torch.cat([ws, torch.tensor([7, 3], dtype=I32)]), torch.cat([wd, torch.tensor([1, 1], dtype=I32)])
    N = clip.numel()
    ff = torch.randn(N * S, 128, generator=g).to(DEV)
    co = (torch.rand(N * S, 2, generator=g) * torch.tensor([W8 + 4.0, H8 + 4.0]) - 2.0).to(DEV)
    got = ops.mixer_input_build_rings(flat, F, R_, H8, W8, ff, co, ws.to(DEV), wd.to(DEV), clip_in.to(DEV), first, frames, bf16, S)
    assert bool(torch.isfinite(got).all())
    rows = torch.arange(N * S).view(N, S)
    for v, T in enumerate(FRAMES_A):
        sel = torch.nonzero(clip == v).squeeze(1)
        r = rows[sel].reshape(-1).to(DEV)
        ref = _build_ring(own[v], T, ff[r].contiguous(), co[r].contiguous(), ws[sel].to(DEV), wd[sel].to(DEV), bf16, S)
        assert torch.equal(got[r], ref), f"stream {v}"
    # the wrap matters: stream 1's window across the wrap read as a LINEAR clip of 9 frames at the same place gives other rows
    lin = ops.mixer_input_build_clips(flat, F, H8, W8, ff, co, ws.to(DEV), wd.to(DEV), clip_in.to(DEV), first,
                                      torch.full((3,), R_, dtype=I32, device=DEV), bf16, S)
    j = WINDOWS.index((1, 6, 1))
    assert not torch.equal(lin[rows[j].to(DEV)], got[rows[j].to(DEV)])
    assert torch.equal(lin[rows[0].to(DEV)], got[rows[0].to(DEV)])           # stream 0 never wraps: the linear form


STREAM_CHUNKS_A = ((9,), (9, 5), (5,))        # appends that leave 9 / 14 / 5 frames in rings of 9 slots


@functools.lru_cache(maxsize=None)
def _videos(lengths, seed=80):
    return tuple(_video(T, seed + i) for i, T in enumerate(lengths))


def _fill(m, videos, chunking, slots, only=None, fill=None):
    """(the cache of V rings, each stream's own ring cache) after the same appends; ``only``: append to these streams alone;
    ``fill``: an int32 bit pattern both kinds of buffer hold before the first append"""
    multi = m.ring_cache_videos(H, W, slots, len(videos))
    if fill is not None:
        multi.pyr.view(I32).fill_(fill)
    own = []
    for v, (video, sizes) in enumerate(zip(videos, chunking)):
        single = m.ring_cache(H, W, slots)
        if fill is not None:
            single.pyr.view(I32).fill_(fill)
        f = 0
        for k in sizes:
            if only is None or v in only:
                m.encode(video[:, f:f + k], into=multi, clip=v)
                m.encode(video[:, f:f + k], into=single)
            f += k
        own.append(single)
    return multi, own


@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
def test_track_on_rings_equals_track_on_each_streams_own_ring(weights_tamed, mode):
    """Pips.track(win_clip=) on a cache of three rings (9, 14 and 5 frames appended to 9 slots) against Pips.track on each
    stream's own ring cache: the point sample (iters = 0), every iterate, the visibility and the features torch.equal in exact
    fp32, matmul='split' and the bf16 mode (the gather on the bf16 mirror), with sampled and with given features.  All row
    counts on GEMM route 0, asserted first."""
    m = _model(weights_tamed, mode)
    clip, ws, wd = _windows()
    N = clip.numel()
    _assert_route_0(N, "bf16" if mode == "bf16" else "exact")
    multi, own = _fill(m, _videos(FRAMES_A), STREAM_CHUNKS_A, R_)
    assert multi.rings == 3 and multi.slots == R_ and multi.clip_lengths == list(FRAMES_A) and multi.clip_frames.tolist() == list(FRAMES_A)
    assert multi.clip_first.tolist() == [0, 9, 18] and multi.bf16_maps == (mode == "bf16") and [c.T for c in own] == list(FRAMES_A)
    g = torch.Generator().manual_seed(72)
    xy = (torch.rand(1, N, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    fi = torch.randn(1, N, 128, generator=g).to(DEV) * 0.1
    for feat, iters in ((None, 0), (None, 3), (fi, 3)):
        got = m.track(multi, xy, iters=iters, win_start=ws.view(1, -1), win_dir=wd.view(1, -1), win_clip=clip.view(1, -1),
                      feat_init=feat, return_feat=True)
        for v in range(3):
            sel = torch.nonzero(clip == v).squeeze(1)
            sd = sel.to(DEV)
            ref = m.track(own[v], xy[:, sd], iters=iters, win_start=ws[sel].view(1, -1), win_dir=wd[sel].view(1, -1),
                          feat_init=None if feat is None else feat[:, sd], return_feat=True)
            assert all(torch.equal(a[:, :, sd], b) for a, b in zip(got[1], ref[1])), f"stream {v}"
            assert torch.equal(got[2][:, :, sd], ref[2]) and torch.equal(got[3][:, sd], ref[3]), f"stream {v}"
    assert bool(torch.isfinite(got[0][-1]).all())
    with pytest.raises(ValueError):
        m.track(multi, xy, iters=1, win_start=ws.view(1, -1))                   # a cache of rings needs win_clip


# ------------------------------------------------------------------ (b) append_at
@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_append_to_one_ring_is_the_single_ring_and_spares_the_neighbours(weights_tamed, mode):
    """encode(into=, clip=1) of 9 + 5 frames (the second append wraps) on a NaN-payload-filled cache of three rings: ring 1 holds
    the fp32 levels and the mirror bytes of encode(into=) on a single ring; the slots of rings 0 and 2 keep the fill in the levels
    and in the mirror."""
    m = _model(weights_tamed, mode)
    multi, own = _fill(m, _videos(FRAMES_A), STREAM_CHUNKS_A, R_, only=(1,), fill=NAN_FILL)
    torch.cuda.synchronize()
    assert multi.clip_lengths == [0, 14, 0] and multi.clip_frames.tolist() == [0, 14, 0] and own[1].T == 14
    F = 3 * R_
    for got, ref in list(zip(_levels(multi.pyr, F), _levels(own[1].pyr, R_))) + list(zip(_mirror_levels(multi.pyr, F),
                                                                                      _mirror_levels(own[1].pyr, R_))):
        if got.dtype == torch.float32:
            got, ref = got.view(I32), ref.view(I32)
        fill = _nan_filled(1).view(got.dtype).to(DEV)             # one int32 or two int16
        assert torch.equal(got[R_:2 * R_], ref)
        for nb in (got[:R_], got[2 * R_:]):                       # the neighbours' slots: still the fill pattern
            assert bool((nb.reshape(-1, fill.numel()) == fill).all())
    assert bool(torch.isfinite(_levels(own[1].pyr, R_)[0]).all())


def test_append_at_between_two_positions():
    """pips_pyramid_append_at alone: frames [2, 5) of a random-filled pyramid of 6 frames into the ring at flat slot 9 of a buffer
    of 27, T0 = 7 -- slots 16, 17 and, wrapped, 9.  Those slots hold the frames' fp32 bytes and their bf16 rounding in the mirror;
    every other slot (the rest of the ring and both neighbours) keeps its NaN-payload fill."""
    from pips_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(73)
    src = torch.zeros(lib.pips_pyramid_floats(6, H, W, ST), dtype=torch.float32, device=DEV)
    for lv in _levels(src, 6):
        lv.copy_(torch.randn(lv.shape, generator=g))
    F = 27
    dst = torch.full((lib.pips_pyramid_floats(F, H, W, ST),), NAN_FILL, dtype=I32, device=DEV).view(torch.float32)
    ops.pyramid_append_at(src, 6, 2, 3, dst, F, 9, 9, 7, H, W, ST)
    torch.cuda.synchronize()
    slots = [16, 17, 9]
    rest = [s for s in range(F) if s not in slots]
    for s_lv, d_lv, d_mir in zip(_levels(src, 6), _levels(dst, F), _mirror_levels(dst, F)):
        assert torch.equal(d_lv[slots].view(I32), s_lv[2:5].view(I32))
        assert torch.equal(d_mir[slots], s_lv[2:5].bfloat16().view(torch.int16))
        assert bool((d_lv[rest].view(I32) == NAN_FILL).all())
        pat = _nan_filled(1).view(torch.int16).to(DEV)
        assert bool((d_mir[rest].reshape(-1, 2) == pat).all())


# ------------------------------------------------------------------ (c) select over several streams
SEL_L = 32
SEL_FRAMES = (40, 33, 37)


def _select_state(n, seed, final, all_done=False):
    """n queries of 3 streams with statuses 0 / 1 / 2 mixed and window starts spread around the frames T_v of their OWN stream;
    the named starts (cur + 8 == T_v, cur + 8 == T_v + 1, cur == T_v - 1, cur == T_v) come first, under status 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    clip = torch.randint(0, 3, (n,), generator=g).to(I32)
    T = torch.tensor(SEL_FRAMES, dtype=I32)[clip.long()]
    status = torch.randint(0, 3, (n,), generator=g).to(I32)
    cur = T + torch.randint(-12, 4, (n,), generator=g).to(I32)
    named = [-8, -7, -1, 0]
    for j in range(min(n, 8)):
        cur[j], status[j] = T[j] + named[j % 4], j // 4
    if all_done:
        status[:] = 2
    tq = torch.where(status == 0, cur, cur - torch.randint(0, 20, (n,), generator=g).to(I32))
    xy = torch.randn(n, 2, generator=g) * 50
    return dict(n=n, tq=tq, cur=cur, status=status, xy=xy, clip=clip, trajs=_nan_filled(SEL_L, n, 2),
                frames=torch.tensor(SEL_FRAMES, dtype=I32), final=torch.tensor(final, dtype=I32))


def _expected_select(s):
    """the lines of drivers._TorchRounds.run / lows (the clip-table form) that pips_stream_select_clips stands for, on the CPU"""
    L = SEL_L
    status, cur, tq, clip = s["status"].clone().long(), s["cur"].long(), s["tq"].long(), s["clip"].long()
    T, fin = s["frames"].long()[clip], s["final"][clip] != 0
    trajs = s["trajs"].clone()
    status[fin & (status == 1) & (cur >= T)] = 2
    live = status != 2
    ready = live & torch.where(fin, cur < T, cur + 8 <= T)
    active = torch.nonzero(ready).squeeze(1)
    new = torch.nonzero(ready & (status == 0)).squeeze(1)
    trajs[tq[new] % L, new] = s["xy"][new]
    status[new] = 1
    lows = [int(cur[live & (clip == v)].min()) if bool((live & (clip == v)).any()) else INT_MAX for v in range(3)]
    return dict(active=active.to(I32), new=new.to(I32), status=status.to(I32), trajs=trajs,
                counts=torch.tensor([active.numel(), new.numel(), min(lows), 0] + lows, dtype=I32))


@pytest.mark.parametrize("final", [(0, 0, 0), (0, 1, 0), (1, 1, 1)])
@pytest.mark.parametrize("n", [1, 256, 600])
def test_select_over_streams_is_the_torch_lines_of_rounds(n, final):
    """pips_stream_select_clips over n = 600 (three chunks of the block), 256 and 1 queries of V = 3 streams with 40 / 33 / 37
    frames, none / one / all of them ended: active, new_list, the 4 + V counts (the per-stream lows behind the four), status and
    the seeded rows of a NaN-payload trajs buffer equal the torch restatement as bit patterns; nothing is written past the
    counts; cur / tq / xy / clip and the tables stay."""
    from pips_amd import ops
    s = _select_state(n, 90 + n, final)
    exp = _expected_select(s)
    if n == 600:
        act, new = exp["active"].tolist(), exp["new"].tolist()
        for j in range(8):                                       # every named start does what it was built for, in ITS stream
            fin = bool(final[int(s["clip"][j])])
            want = {0: True, 1: fin, 2: fin, 3: False}[j % 4]
            assert (j in act) == want and (j in new) == (want and j < 4), j
        for lst in (act, new):
            assert any(q < 256 for q in lst) and any(256 <= q < 512 for q in lst) and any(q >= 512 for q in lst)
        assert exp["counts"][4:].tolist() == [T - 12 for T in SEL_FRAMES] and len(set(exp["counts"][4:].tolist())) == 3
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    active = torch.full((n,), -77, dtype=I32, device=DEV)
    new_list = torch.full((n,), -78, dtype=I32, device=DEV)
    counts = torch.full((4 + 3 + 2,), -1, dtype=I32, device=DEV)
    ops.stream_select_clips(d["tq"], d["xy"], d["cur"], d["status"], d["clip"], d["frames"], d["final"], d["trajs"], active, new_list,
                            counts)
    torch.cuda.synchronize()
    ka, kn = exp["active"].numel(), exp["new"].numel()
    assert torch.equal(counts.cpu()[:7], exp["counts"]) and counts.cpu()[7:].tolist() == [-1, -1]
    assert torch.equal(active.cpu()[:ka], exp["active"]) and bool((active.cpu()[ka:] == -77).all())
    assert torch.equal(new_list.cpu()[:kn], exp["new"]) and bool((new_list.cpu()[kn:] == -78).all())
    assert torch.equal(d["status"].cpu(), exp["status"])
    assert torch.equal(_bits(d["trajs"]), _bits(exp["trajs"]))
    assert int((_bits(exp["trajs"]) != NAN_FILL).sum()) == 2 * kn
    for k in ("cur", "tq", "clip", "frames", "final"):
        assert torch.equal(d[k].cpu(), s[k]), k
    assert torch.equal(_bits(d["xy"]), _bits(s["xy"]))


def test_select_over_streams_with_every_query_done_and_an_empty_stream():
    from pips_amd import ops
    n = 300
    s = _select_state(n, 91, (0, 1, 0), all_done=True)
    s["status"][5], s["clip"][5], s["cur"][5] = 1, 2, 11          # one live query, in stream 2: streams 0 and 1 have none
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    active, new_list = (torch.full((n,), -77, dtype=I32, device=DEV) for _ in range(2))
    counts = torch.full((7,), -1, dtype=I32, device=DEV)
    ops.stream_select_clips(d["tq"], d["xy"], d["cur"], d["status"], d["clip"], d["frames"], d["final"], d["trajs"], active, new_list,
                            counts)
    assert counts.tolist() == [1, 0, 11, 0, INT_MAX, INT_MAX, 11] and active.tolist()[:2] == [5, -77]
    assert torch.equal(_bits(d["trajs"]), _bits(s["trajs"]))


# ------------------------------------------------------------------ (d) emit of one stream's columns
@pytest.mark.parametrize("frames", ["wrap", "none", "all"])
@pytest.mark.parametrize("L,n,cols", [(17, 5, [0, 2, 4]), (32, 64, list(range(16, 24))), (32, 64, list(range(5, 12))),
                                      (32, 64, [3, 8, 9, 63, 64, 70])])
def test_emit_cols_moves_the_columns_of_one_stream(L, n, cols, frames):
    """pips_stream_emit_cols on buffers of arbitrary bit patterns: L = 17, n = 5 with columns 0, 2, 4; L = 32, n = 64 with a
    16-byte-aligned run of columns, an unaligned one, and a list with members outside [0, n) (skipped: their outputs are the
    NaN).  The frames wrap past row L - 1; f1 - f0 of 0 and of L.  The outputs are the elements' bits, exactly those elements
    are 0x7fc00000 afterwards, every other element is untouched."""
    from pips_amd import ops
    g = torch.Generator().manual_seed(92 + L)
    trajs = torch.randint(-2 ** 31, 2 ** 31, (L, n, 2), generator=g).to(I32)
    vis = torch.randint(-2 ** 31, 2 ** 31, (L, n), generator=g).to(I32)
    trajs[1, cols[0], 0], vis[L - 1, cols[0]] = NAN_FILL, NAN_FILL
    f0 = 3 * L + L - 3                                          # rows L-3, L-2, L-1, 0, 1, ...
    f1 = {"wrap": f0 + 7, "none": f0, "all": f0 + L}[frames]
    rows = (torch.arange(f0, f1) % L).view(-1, 1)
    d_t, d_v = trajs.to(DEV).view(torch.float32), vis.to(DEV).view(torch.float32)
    out_t, out_v = ops.stream_emit_cols(d_t, d_v, f0, f1, torch.tensor(cols, dtype=I32, device=DEV))
    torch.cuda.synchronize()
    m = len(cols)
    assert tuple(out_t.shape) == (f1 - f0, m, 2) and tuple(out_v.shape) == (f1 - f0, m)
    inside = [j for j, c in enumerate(cols) if 0 <= c < n]
    ci = torch.tensor([cols[j] for j in inside]).view(1, -1)
    want_ot = torch.full((f1 - f0, m, 2), QUIET_NAN, dtype=I32)
    want_ov = torch.full((f1 - f0, m), QUIET_NAN, dtype=I32)
    want_ot[:, inside], want_ov[:, inside] = trajs[rows, ci], vis[rows, ci]
    assert torch.equal(_bits(out_t), want_ot) and torch.equal(_bits(out_v), want_ov)
    want_t, want_v = trajs.clone(), vis.clone()
    want_t[rows, ci], want_v[rows, ci] = QUIET_NAN, QUIET_NAN
    assert torch.equal(_bits(d_t), want_t) and torch.equal(_bits(d_v), want_v)
    if frames != "none":
        assert int((want_t != trajs).sum()) >= 2 * (f1 - f0) * len(inside) - 2     # (a random word may be the NaN already)


# ------------------------------------------------------------------ (e) drivers: every stream is the stream alone
TS_E, CHUNKS_E = (21, 29, 13), (5, 7, 3)
TQS_E = ([0, 3, 11, 11], [0, 3, 11], [0, 3, 11, 0])


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_multi_stream_rounds_equal_each_stream_alone(weights_tamed, mode, slots):
    """Three streams (T = 21 / 29 / 13 in chunks of 5 / 7 / 3, queries at frames 0, 3 and 11) through MultiStreamTracker with
    library rounds and with torch rounds, against track_stream on each stream alone: identical hop lists and trajectories and
    visibilities equal as bit patterns (the NaN frames before each query included), fp32 and bf16, rings of 9 (the minimum)
    and 24 slots.  Route 0 for every row count up to the total number of queries is asserted first."""
    from pips_amd import drivers
    n_all = sum(len(t) for t in TQS_E)
    _assert_route_0(n_all, mode)
    m = _model(weights_tamed, mode)
    videos = _videos(TS_E, seed=93)
    lists = [[v[:, i:i + c] for i in range(0, v.shape[1], c)] for v, c in zip(videos, CHUNKS_E)]
    qs = [_queries(tq, 94 + v).to(DEV) for v, tq in enumerate(TQS_E)]
    lib = drivers.track_streams(m, lists, qs, iters=6, slots=slots, return_hops=True, rounds="library")
    tor = drivers.track_streams(m, lists, qs, iters=6, slots=slots, return_hops=True, rounds="torch")
    for v in range(3):
        ref_t, ref_v, ref_h = drivers.track_stream(m, lists[v], qs[v], iters=6, slots=slots, return_hops=True)
        assert tuple(ref_t.shape) == (1, TS_E[v], len(TQS_E[v]), 2)
        for name, got in (("library", lib[v]), ("torch", tor[v])):
            assert got[2] == ref_h, (name, v)
            assert torch.equal(_bits(got[0]), _bits(ref_t)) and torch.equal(_bits(got[1]), _bits(ref_v)), (name, v)
        assert bool(torch.isnan(ref_t[0, :11, 2]).all()) and bool(torch.isfinite(ref_t[0, 11:, 2]).all())
    assert any(len(h) > 1 for h in lib[1][2])
    if mode == "exact" and slots == 9:
        plain = drivers.track_streams(m, lists, qs, iters=6, slots=slots, rounds="library")          # without the hop log
        assert all(torch.equal(_bits(p[0]), _bits(g[0])) and torch.equal(_bits(p[1]), _bits(g[1])) for p, g in zip(plain, lib))


def test_add_queries_to_one_stream_under_library_rounds(weights_tamed):
    """add_queries(1, ...) at the oldest frame of stream 1 not yet returned and at a frame not pushed yet, under library rounds:
    stream 1 is track_stream given all its queries up front, the other streams are untouched, bit for bit with the hops."""
    from pips_amd import drivers
    _assert_route_0(sum(len(t) for t in TQS_E) + 2, "exact")
    m = _model(weights_tamed)
    videos = _videos(TS_E, seed=93)
    lists = [[v[:, i:i + c] for i in range(0, v.shape[1], c)] for v, c in zip(videos, CHUNKS_E)]
    qs = [_queries(tq, 94 + v).to(DEV) for v, tq in enumerate(TQS_E)]
    mt = drivers.MultiStreamTracker(m, qs, iters=6, slots=9, record_hops=True, rounds="library")
    parts = [[], [], []]
    for i in range(5):
        if i == 2:
            late = _queries([mt.emitted[1], 20], 97)
            assert mt.add_queries(1, late.to(DEV)).tolist() == [3, 4]
        for v, p in enumerate(mt.push([l[i] if i < len(l) else None for l in lists])):
            parts[v].append(p)
    for v, p in enumerate(mt.finish()):
        parts[v].append(p)
    full = [torch.full((1, TS_E[1], 5, 2), float("nan"), device=DEV), torch.full((1, TS_E[1], 5), float("nan"), device=DEV)]
    for f0, tr, vi in parts[1]:
        full[0][:, f0:f0 + tr.shape[1], :tr.shape[2]] = tr
        full[1][:, f0:f0 + vi.shape[1], :vi.shape[2]] = vi
    q1 = torch.cat([qs[1], late.to(DEV)], dim=1)
    ref_t, ref_v, ref_h = drivers.track_stream(m, lists[1], q1, iters=6, slots=9, return_hops=True, rounds="library")
    assert torch.equal(_bits(full[0]), _bits(ref_t)) and torch.equal(_bits(full[1]), _bits(ref_v)) and mt.stream_hops(1) == ref_h
    for v in (0, 2):
        ref_t, ref_v, ref_h = drivers.track_stream(m, lists[v], qs[v], iters=6, slots=9, return_hops=True)
        assert torch.equal(_bits(torch.cat([p[1] for p in parts[v]], dim=1)), _bits(ref_t)) and mt.stream_hops(v) == ref_h
        assert torch.equal(_bits(torch.cat([p[2] for p in parts[v]], dim=1)), _bits(ref_v))


def test_multi_stream_tracker_makes_the_clip_table_library_calls(weights_tamed, monkeypatch):
    """A MultiStreamTracker of V = 2 under rounds="library" -- 21 frames each in chunks of 5 through rings of 9 slots, one query of
    stream 0 removed on the way -- calls the clip-table entry points it always called, and none of the one-video forms (the set
    is read off the drivers before the two trackers shared a core); the outputs are those of rounds="torch", bit for bit with
    the hop lists."""
    from pips_amd import drivers, ops
    _assert_route_0(8, "exact")
    m = _model(weights_tamed)
    videos = _videos((21, 21), seed=101)
    qs = [_queries([0, 3, 11, 11], 103 + v).to(DEV) for v in range(2)]

    def run(rounds):
        mt = drivers.MultiStreamTracker(m, qs, iters=6, slots=9, record_hops=True, rounds=rounds)
        parts = []
        for i in range(0, 21, 5):
            parts.append(mt.push([v[:, i:i + 5] for v in videos]))
            if i == 10:
                assert mt.remove_queries(0, [1]).tolist() == [0, 2, 3]
        return parts + [mt.finish()], [mt.stream_hops(v) for v in range(2)]

    names, real = [], ops._call

    def recorded(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", recorded)
    parts, hops = run("library")
    seen = {n for n in names if n.startswith(("pips_stream_", "pips_pyramid_append"))}
    assert seen == {"pips_pyramid_append_at", "pips_stream_select_clips", "pips_stream_round_clips", "pips_stream_emit_cols",
                    "pips_stream_keep"}
    ref, ref_hops = run("torch")
    assert hops == ref_hops and any(len(h) > 1 for h in hops[0] + hops[1])
    for part, ref_part in zip(parts, ref):
        for (f0, tr, vi), (g0, ref_t, ref_v) in zip(part, ref_part):
            assert f0 == g0 and torch.equal(_bits(tr), _bits(ref_t)) and torch.equal(_bits(vi), _bits(ref_v))
    assert all(sum(p[v][1].shape[1] for p in parts) == 21 for v in range(2))


# ------------------------------------------------------------------ (f) against the reference's loop; the joint encoder option
@pytest.mark.parametrize("joint", [False, True])
def test_one_stream_against_reference_loop(weights_tamed, joint):
    """One stream of T = 21 from frame 0 through MultiStreamTracker(rounds="library") at 128x160, stride 8, against
    oracle/chain_oracle.chain: identical hop sequences and the gate of tests/test_stream_gpu.py, 1e-3 px over every frame
    (3.1e-5 px measured for the single stream); once more with joint_encode=True."""
    from pips_amd import drivers
    from oracle import chain_oracle
    T, N = 21, 8
    video = _video(T, seed=37)
    q = _queries([0] * N, seed=38)
    (got, vis, hops), = drivers.track_streams(_model(weights_tamed), [[video]], [q.to(DEV)], iters=6, slots=T + 8, return_hops=True,
                                              rounds="library", joint_encode=joint)
    ref, rh = chain_oracle.chain(weights_tamed, video, q[:, :, 1:], iters=6, stride=8, cache_frames=True)
    assert hops == rh and any(len(h) > 1 for h in hops)
    err = float((got.cpu() - ref.cpu()).abs().max())
    print("track_streams (library rounds, joint_encode=%s) vs reference loop: max |dtraj| %.2e px; hops %s" % (joint, err, hops))
    assert tuple(got.shape) == (1, T, N, 2) and bool(torch.isfinite(vis).all())
    assert err < 1e-3


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_joint_rings_against_per_stream_rings(weights_tamed, mode):
    """Pips.encode_streams(joint=True): 5 + 7 + 3 frames of three streams in ONE shared encoder pass of 15 frames, then 7 + 7 + 6
    more in two (16 + 4: stream 2's frames straddle the passes, stream 0 wraps its ring of 9 slots) against the per-stream
    passes.  The fp32 levels agree within the encoder's tile-order noise (the 1e-4 gate of
    tests/test_drivers_gpu.py::test_encode_in_passes_matches_single_pass; exact fp32 only -- the bf16 encoder's noise is its
    rounding), the clip table is the same, and the mirror IS bf16 of the fp32 levels, bit for bit, in every slot written."""
    m = _model(weights_tamed, mode)
    videos = _videos((12, 14, 9), seed=98)
    waves = [(5, 7, 3), (7, 7, 6)]
    joint, per = m.ring_cache_videos(H, W, R_, 3), m.ring_cache_videos(H, W, R_, 3)
    at = [0, 0, 0]
    for wave in waves:
        chunks = [(v, videos[v][:, at[v]:at[v] + k]) for v, k in enumerate(wave)]
        m.encode_streams(joint, chunks, joint=True)
        m.encode_streams(per, chunks)
        at = [a + k for a, k in zip(at, wave)]
    assert joint.clip_lengths == per.clip_lengths == [12, 14, 9] and joint.clip_frames.tolist() == [12, 14, 9]
    F = 3 * R_
    for lj, lp, mj in zip(_levels(joint.pyr, F), _levels(per.pyr, F), _mirror_levels(joint.pyr, F)):
        err = float((lj - lp).abs().max())
        print("joint against per-stream levels (%s): max |d| %.2e" % (mode, err))
        if mode == "exact":
            assert err < 1e-4
        assert torch.equal(mj, lj.bfloat16().view(torch.int16))
    assert bool(torch.isfinite(_levels(joint.pyr, F)[0]).all()) and float(_levels(joint.pyr, F)[0].abs().max()) > 0


# ------------------------------------------------------------------ (g) argument handling
def test_multi_stream_calls_reject_bad_arguments_and_leave_the_state_alone():
    """Every PIPS_E_ARG / PIPS_E_WORKSPACE case of the new entry points returns its code ahead of any launch and leaves the
    NaN-payload state (and the outputs) bit-identical; n_act == 0, f0 == f1 and m == 0 are PIPS_OK and touch nothing."""
    from pips_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(99)
    n, n_act, n_new, L, F, R, V, iters, N = 12, 5, 2, 24, 30, 10, 3, 2, 4
    state = dict(tq=torch.randint(0, 10, (n,), generator=g).to(I32), xy=torch.randn(n, 2, generator=g),
                 cur=torch.randint(0, 10, (n,), generator=g).to(I32), status=torch.randint(0, 3, (n,), generator=g).to(I32),
                 clip=torch.randint(0, V, (n,), generator=g).to(I32), feat=torch.randn(n, 128, generator=g),
                 trajs=_nan_filled(L, n, 2), vis=_nan_filled(L, n), active=torch.full((n,), -77, dtype=I32),
                 new_list=torch.full((n,), -78, dtype=I32), counts=torch.full((4 + V,), 99, dtype=I32),
                 steps=torch.full((n,), -5, dtype=I32), out_trajs=_nan_filled(L, n, 2), out_vis=_nan_filled(L, n),
                 clip_first=torch.arange(V, dtype=I32) * R, clip_frames=torch.tensor([10, 12, 4], dtype=I32),
                 clip_final=torch.tensor([0, 1, 0], dtype=I32), cols=torch.tensor([1, 4, 5], dtype=I32),
                 X=_nan_filled(N * 8, 544), win_start=torch.tensor([0, 3, 5, 1], dtype=I32), win_clip=torch.tensor([0, 1, 2, 1], dtype=I32),
                 dst=_nan_filled(4096))
    dev = {k: v.to(DEV) for k, v in state.items()}
    dev["active"][:n_act] = torch.tensor([1, 4, 5, 8, 11], dtype=I32)
    dev["new_list"][:n_new] = torch.tensor([4, 8], dtype=I32)
    state["active"], state["new_list"] = dev["active"].cpu(), dev["new_list"].cpu()
    nb = lib.pips_stream_workspace_bytes_clips(n, iters, V)
    assert nb > lib.pips_stream_workspace_bytes(n, iters) > 0
    ws = torch.zeros(nb // 4, device=DEV)
    dummy = torch.zeros(64, device=DEV)                      # stands for the arena, the pyramids, ffeats, ...: never read
    stream = _stream()
    good = dict(dev, arena=dummy, pyramid=dummy, F=F, R=R, V=V, H8=16, W8=20, times=dummy, stride=8, iters=iters, flags=0, n=n,
                n_act=n_act, n_new=n_new, L=L, workspace=ws, workspace_bytes=nb, f0=20, f1=27, m=3, B=1, N=N, S=8, ffeats=dummy,
                coords=dummy, win_dir=None, xys=dummy, src=dummy, F_src=6, src_first=2, k=3, ring_first=10, T0=7, ce_tgt=None)

    def args(over):
        a = dict(good, **over)
        return {k: (_lib.ptr(v) if torch.is_tensor(v) or v is None else v) for k, v in a.items()}

    def select(**over):
        p = args(over)
        return lib.pips_stream_select_clips(p["n"], p["tq"], p["xy"], p["cur"], p["status"], p["clip"], p["clip_frames"],
                                            p["clip_final"], p["V"], p["trajs"], p["L"], p["active"], p["new_list"], p["counts"], stream)

    def round_(**over):
        p = args(over)
        return lib.pips_stream_round_clips(p["arena"], p["pyramid"], p["F"], p["R"], p["H8"], p["W8"], p["times"], p["stride"],
                                           p["iters"], p["flags"], p["n"], p["n_act"], p["n_new"], p["tq"], p["xy"], p["cur"],
                                           p["status"], p["clip"], p["feat"], p["trajs"], p["vis"], p["L"], p["clip_first"],
                                           p["clip_frames"], p["clip_final"], p["V"], p["active"], p["new_list"], p["counts"],
                                           p["steps"], p["workspace"], p["workspace_bytes"], stream)

    def emit(**over):
        p = args(over)
        return lib.pips_stream_emit_cols(p["trajs"], p["vis"], p["L"], p["n"], p["f0"], p["f1"], p["cols"], p["m"], p["out_trajs"],
                                         p["out_vis"], stream)

    def gather(**over):
        p = args(over)
        return lib.pips_mixer_input_build_rings(p["pyramid"], p["B"], p["F"], p["R"], p["H8"], p["W8"], p["ffeats"], p["coords"],
                                                p["times"], p["N"], p["win_start"], p["win_dir"], p["win_clip"], p["clip_first"],
                                                p["clip_frames"], p["V"], p["flags"], p["S"], p["X"], stream)

    def track(**over):
        p = args(over)
        return lib.pips_track_rings(p["arena"], p["pyramid"], p["B"], p["F"], p["R"], p["H8"], p["W8"], p["xys"], None, None,
                                    p["win_start"], p["win_dir"], p["win_clip"], p["clip_first"], p["clip_frames"], p["V"], p["times"],
                                    p["N"], p["stride"], p["iters"], p["flags"], p["S"], p["workspace"], p["workspace_bytes"],
                                    p["out_trajs"], p["out_vis"], None, p["ce_tgt"], None, None, 0, stream)

    def append(**over):
        p = args(over)
        return lib.pips_pyramid_append_at(p["src"], p["F_src"], p["src_first"], p["k"], p["dst"], p["F"], p["ring_first"], p["R"],
                                          p["T0"], H, W, ST, stream)

    def untouched():
        torch.cuda.synchronize()
        for k, v in state.items():
            assert torch.equal(_bits(dev[k]), _bits(v)), k
        assert not bool(ws.any())

    nulls = ["tq", "xy", "cur", "status", "trajs", "active", "new_list", "counts", "clip", "clip_frames", "clip_final"]
    for over in [dict(n=0), dict(L=15), dict(V=0), dict(V=65)] + [{k: None} for k in nulls]:
        assert select(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    bad = [dict(n=0), dict(n_act=-1), dict(n_act=n + 1), dict(n_new=-1), dict(n_new=n + 1), dict(n_new=n_act + 1), dict(L=15),
           dict(R=8), dict(F=0), dict(F=V * R - 1), dict(V=0), dict(V=65)]
    for over in bad + [{k: None} for k in nulls + ["clip_first", "feat", "vis", "arena", "pyramid", "times", "workspace"]]:
        assert round_(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    assert round_(workspace_bytes=nb - 4) == E_WORKSPACE and b"workspace" in lib.pips_last_error()
    untouched()
    assert round_(workspace_bytes=lib.pips_stream_workspace_bytes(n, iters)) == E_WORKSPACE       # the one-stream size is too small
    untouched()
    assert round_(n_act=0, n_new=0) == 0
    untouched()
    for over in [dict(n=0), dict(m=-1), dict(L=15), dict(f1=19), dict(f1=20 + L + 1), dict(trajs=None), dict(vis=None), dict(cols=None),
                 dict(out_trajs=None), dict(out_vis=None)]:
        assert emit(**over) == E_ARG, over
        untouched()
    assert emit(f1=20) == 0 and emit(m=0) == 0
    untouched()
    ring_bad = [dict(V=0), dict(R=0), dict(win_clip=None), dict(clip_first=None), dict(clip_frames=None), dict(win_start=None),
                dict(B=2), dict(F=V * R - 1)]
    for over in ring_bad:
        assert gather(**over) == E_ARG, over
        assert track(**over) == E_ARG, over
        untouched()
    assert track(ce_tgt=dummy) == E_ARG                      # no score-map block on a clip table
    untouched()
    for over in [dict(src=None), dict(dst=None), dict(R=0), dict(T0=-1), dict(k=0), dict(k=R + 1), dict(src_first=-1), dict(src_first=4),
                 dict(F_src=4), dict(ring_first=-1), dict(ring_first=F - R + 1), dict(F=R + 9)]:
        assert append(**over) == E_ARG, over
        untouched()
    # the forms this work left alone still reject a clip table on a ring
    p = args({})
    assert lib.pips_mixer_input_build_clips(p["pyramid"], 1, F, R, 16, 20, p["ffeats"], p["coords"], p["times"], N, p["win_start"], None,
                                            p["win_clip"], p["clip_first"], p["clip_frames"], V, 0, 8, p["X"], stream) == E_ARG
    untouched()
    assert lib.pips_abi_version() == 3
