"""GPU: the visibility-aware chaining behind the C ABI (pips_chain_gather / pips_chain_step / pips_chain_hop) and the drivers'
``engine="native"``.  The step kernel is held, bit for bit, to the torch lines of ``drivers._hop`` (``skip_scan`` and its indexed
assignments) on synthetic windows; the native engine to the torch engine on the same model, video and queries (identical hops,
identical bits), and to the reference's own loop text (tests/golden/chain_t13.npz)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
NAN_FILL = 0x7FC12345          # a NaN with a payload: a stray write into trajs / vis shows in the bit patterns
P_SET = (0.05, 0.5, 0.85, 0.87, 0.89, 0.91, 0.95)       # each >= 0.01 from every threshold 0.9 - 0.02 k


def _model(sd, stride=8):
    from pips_amd import Pips
    m = Pips(S=8, stride=stride)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _logit(p):
    return math.log(p / (1.0 - p))


def _nan_filled(*shape):
    return torch.full(shape, NAN_FILL, dtype=I32).view(torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


# ------------------------------------------------------------------ synthetic windows
# 23 of 37 particles: not contiguous, not a multiple of the wave size
ACTIVE = [0, 1, 3, 4, 6, 9, 10, 12, 13, 15, 17, 18, 20, 21, 23, 24, 26, 28, 30, 31, 33, 35, 36]
N_ALL = 37


def _rows(layout):
    """(T, L, base, per active particle: (cur, dir, the 8 confidences or None = drawn from P_SET)).  The named rows of the issue
    come first; ``dir`` is None for the forward-only ring layout."""
    lo, hi, nan = 0.05, 0.95, float("nan")
    only2 = [lo, lo, hi, lo, lo, lo, lo, lo]               # si = 2
    f36 = [lo, lo, lo, hi, lo, lo, hi, lo]                 # si = 6
    half = [0.5] * 8                                       # the threshold falls 21 times, si = 7
    nans = [nan] * 8                                       # nothing admitted: si = 7
    if layout == "padded":
        T = 21
        named = [(5, 1, half), (4, 1, only2), (7, 1, f36), (3, 1, nans),
                 (T - 3, 1, only2),                        # lands on T - 1: live
                 (T - 2, 1, only2),                        # lands on T: not live
                 (1, -1, only2),                           # lands on -1: not live, rows below the video's start
                 (0, -7, f36),                             # backward from 0 (any negative dir): rows -1..-7, lands on -6
                 (6, -1, f36),                             # backward, lands on 0: live
                 (1, -1, half), (T - 1, 3, half)]          # forward past the end (any positive dir)
        return T, T + 14, 7, named
    T = 200
    named = [(30, None, half), (31, None, only2), (63, None, f36), (100, None, nans),
             (T - 3, None, only2), (T - 2, None, only2), (25, None, f36)]       # the modulo wraps inside the windows
    return T, 32, 0, named


def _synthetic(layout, seed):
    g = torch.Generator().manual_seed(seed)
    T, L, base, named = _rows(layout)
    n_act = len(ACTIVE)
    cur = torch.randint(0, T, (N_ALL,), generator=g).to(I32)
    dirs = None if layout == "ring" else torch.where(torch.rand(N_ALL, generator=g) < 0.5, -1, 1).to(I32)
    pick = torch.tensor(P_SET)[torch.randint(0, len(P_SET), (8, n_act), generator=g)]
    for j, (c, d, ps) in enumerate(named):
        cur[ACTIVE[j]] = c
        if d is not None:
            dirs[ACTIVE[j]] = d
        pick[:, j] = torch.tensor(ps)
    win_vis = torch.log(pick.double() / (1.0 - pick.double())).float()         # logit(p); NaN stays NaN
    assert bool(torch.isnan(win_vis[:, 3]).all()) and abs(float(win_vis[0, 0]) - _logit(0.5)) < 1e-6
    return dict(T=T, L=L, base=base, n=N_ALL, n_act=n_act, active=torch.tensor(ACTIVE, dtype=I32), cur=cur, dirs=dirs,
                win_vis=win_vis, win_trajs=torch.randn(8, n_act, 2, generator=g) * 50,
                win_ffeat0=torch.randn(n_act, 128, generator=g), feat=torch.randn(N_ALL, 128, generator=g),
                trajs=_nan_filled(L, N_ALL, 2), vis=_nan_filled(L, N_ALL))


def _expected_step(s, with_vis, sample_feat):
    """The lines of drivers._hop after the track call, and of drivers._TorchEngine.hop after it, on the CPU."""
    from pips_amd import drivers
    L, base, T = s["L"], s["base"], s["T"]
    active = s["active"].long()
    trajs, vis, cur, feat = s["trajs"].clone(), s["vis"].clone(), s["cur"].clone().long(), s["feat"].clone()
    c = cur[active]
    d = torch.ones_like(c) if s["dirs"] is None else torch.where(s["dirs"].long()[active] < 0, -1, 1)
    rows = torch.arange(8).unsqueeze(1) * d.unsqueeze(0)
    rows = (c.unsqueeze(0) + rows + base) % L
    cols = active.unsqueeze(0).expand(8, -1)
    trajs[rows, cols] = s["win_trajs"]
    if with_vis:
        vis[rows, cols] = s["win_vis"]
    si = drivers.skip_scan(torch.sigmoid(s["win_vis"]))
    c = c + si * d
    cur[active] = c
    if sample_feat:
        feat[active] = s["win_ffeat0"]
    live = (c < T) & (c >= 0)
    return dict(trajs=trajs, vis=vis, cur=cur.to(I32), feat=feat, steps=si.to(I32), next_active=active[live].to(I32))


@pytest.mark.parametrize("sample_feat", [False, True])
@pytest.mark.parametrize("with_vis", [True, False])
@pytest.mark.parametrize("layout", ["padded", "ring"])
def test_chain_step_is_the_torch_lines_of_hop(layout, with_vis, sample_feat):
    """pips_chain_gather and pips_chain_step on 23 of 37 particles against ``skip_scan`` and the indexed assignments of ``_hop``:
    steps, window starts, the compacted list and its count, the carried features, and trajs / vis as int32 bit patterns over
    the WHOLE buffers (pre-filled with a NaN payload).  Padded layout (L = T + 14, base 7, both directions, rows below frame
    0) and ring layout (L = 32, base 0, window starts 30, 31, 63, 100: the modulo wraps inside a window)."""
    from pips_amd import ops
    s = _synthetic(layout, seed=31)
    exp = _expected_step(s, with_vis, sample_feat)
    # the named rows do what they were built for (the expectation itself is not vacuous)
    st = exp["steps"].tolist()
    assert st[:4] == [7, 2, 6, 7] and st[4:6] == [2, 2]
    act = s["active"].tolist()
    newc = exp["cur"].long()[s["active"].long()].tolist()
    assert newc[4] == s["T"] - 1 and act[4] in exp["next_active"].tolist()
    assert newc[5] == s["T"] and act[5] not in exp["next_active"].tolist()
    if layout == "padded":
        assert newc[6] == -1 and act[6] not in exp["next_active"].tolist()
        assert newc[8] == 0 and act[8] in exp["next_active"].tolist()
    n_act = s["n_act"]
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    vis = d["vis"] if with_vis else None
    # gather: the staging arrays of pips_track_ring
    xy, ws, wd, fi = ops.chain_gather(d["trajs"], s["base"], d["cur"], d["dirs"], d["feat"], d["active"], n_act, sample_feat)
    a = s["active"].long()
    want_xy = s["trajs"][(s["cur"].long()[a] + s["base"]) % s["L"], a]
    assert torch.equal(_bits(xy), _bits(want_xy))
    assert torch.equal(ws.cpu(), s["cur"][a])
    assert torch.equal(wd.cpu(), torch.ones(n_act, dtype=I32) if s["dirs"] is None else s["dirs"][a])
    if not sample_feat:
        assert torch.equal(fi.cpu(), s["feat"][a])
    # step
    nxt = torch.full((n_act,), -77, dtype=I32, device=DEV)
    count = torch.full((1,), -1, dtype=I32, device=DEV)
    steps = torch.full((n_act,), -1, dtype=I32, device=DEV)
    ops.chain_step(d["win_trajs"], d["win_vis"], d["win_ffeat0"], s["T"], d["active"], n_act, d["trajs"], vis, s["base"], d["cur"],
                   d["dirs"], d["feat"], nxt, count, steps, sample_feat=sample_feat)
    torch.cuda.synchronize()
    k = exp["next_active"].numel()
    assert int(count.item()) == k
    assert torch.equal(nxt.cpu()[:k], exp["next_active"]) and bool((nxt.cpu()[k:] == -77).all())
    assert torch.equal(steps.cpu(), exp["steps"])
    assert torch.equal(d["cur"].cpu(), exp["cur"])
    assert torch.equal(_bits(d["feat"]), _bits(exp["feat"]))
    assert sample_feat == (not torch.equal(exp["feat"], s["feat"]))
    assert torch.equal(_bits(d["trajs"]), _bits(exp["trajs"]))
    assert torch.equal(_bits(d["vis"]), _bits(exp["vis"]))                 # vis = NULL: the buffer is untouched
    assert int((_bits(exp["trajs"]) != NAN_FILL).sum()) == 8 * n_act * 2


def test_chain_step_compaction_keeps_the_order_over_many_chunks():
    """n_act = 2500 of n = 4000, about half of them live after the step: next_active == active[live] element for element (the
    scan carries its offset over the kernel's chunks), the count is exact and nothing is written past it."""
    from pips_amd import drivers, ops
    g = torch.Generator().manual_seed(32)
    n, n_act, T, L = 4000, 2500, 20, 40
    active = torch.sort(torch.randperm(n, generator=g)[:n_act]).values.to(I32)
    cur = torch.randint(0, 30, (n,), generator=g).to(I32)
    pick = torch.tensor(P_SET)[torch.randint(0, len(P_SET), (8, n_act), generator=g)]
    win_vis = torch.log(pick.double() / (1.0 - pick.double())).float()
    si = drivers.skip_scan(torch.sigmoid(win_vis))
    newc = cur.long()[active.long()] + si
    live = newc < T
    assert 0.3 * n_act < int(live.sum()) < 0.7 * n_act
    trajs = torch.zeros(L, n, 2, device=DEV)
    feat = torch.zeros(n, 128, device=DEV)
    cur_d = cur.to(DEV)
    nxt = torch.full((n_act,), -77, dtype=I32, device=DEV)
    count = torch.full((1,), -1, dtype=I32, device=DEV)
    steps = torch.full((n_act,), -1, dtype=I32, device=DEV)
    ops.chain_step(torch.zeros(8, n_act, 2, device=DEV), win_vis.to(DEV), None, T, active.to(DEV), n_act, trajs, None, 0, cur_d, None,
                   feat, nxt, count, steps)
    torch.cuda.synchronize()
    k = int(live.sum())
    assert int(count.item()) == k
    assert torch.equal(nxt.cpu()[:k], active[live])
    assert bool((nxt.cpu()[k:] == -77).all())
    assert torch.equal(steps.cpu(), si.to(I32))
    want_cur = cur.clone()
    want_cur[active.long()] = newc.to(I32)
    assert torch.equal(cur_d.cpu(), want_cur)


# ------------------------------------------------------------------ native engine against the torch engine
def _video(T, H, W, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


TQ = [0, 3, 10, 17, 20, 20, 3, 10]


def _queries(T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(1, len(TQ), 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
    return torch.cat([torch.tensor(TQ, dtype=torch.float32).view(1, -1, 1), xy], dim=-1)


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_track_queries_native_engine_equals_torch_engine(weights_tamed, mode):
    """T = 21, 128x160, query frames 0, 3, 10, 17, 20 (duplicates included), both directions: identical hop sequences and
    torch.equal trajectories and visibilities, in exact fp32 and in the bf16 mode."""
    from pips_amd import drivers
    m = _model(weights_tamed)
    if mode == "bf16":
        m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    T, H, W = 21, 128, 160
    video = _video(T, H, W, seed=24).to(DEV)
    q = _queries(T, H, W, seed=25).to(DEV)
    ref, ref_vis, ref_hops = drivers.track_queries(m, video, q, iters=6, return_hops=True)
    got, vis, hops = drivers.track_queries(m, video, q, iters=6, return_hops=True, engine="native")
    assert any(len(h) > 1 for h in hops[0]) and any(len(h) > 1 for h in hops[1])
    assert hops == ref_hops
    assert torch.equal(got, ref) and torch.equal(vis, ref_vis)
    plain = drivers.track_queries(m, video, q, iters=6, engine="native")                  # without the hop log
    assert torch.equal(plain[0], ref) and torch.equal(plain[1], ref_vis)


def test_track_chained_native_engine_equals_torch_engine(weights_tamed):
    from pips_amd import drivers
    case = G.CHAIN_CASE
    video, xy0 = G.make_chain_inputs(case)
    m = _model(weights_tamed, case["stride"])
    ref, ref_hops = drivers.track_chained(m, video.to(DEV), xy0.to(DEV), iters=case["iters"], return_hops=True)
    got, hops = drivers.track_chained(m, video.to(DEV), xy0.to(DEV), iters=case["iters"], return_hops=True, engine="native")
    assert hops == ref_hops and any(len(h) > 1 for h in hops)
    assert torch.equal(got, ref)
    assert torch.equal(drivers.track_chained(m, video.to(DEV), xy0.to(DEV), iters=case["iters"], engine="native"), ref)


@pytest.mark.parametrize("slots", [9, 24])
def test_track_stream_native_engine_equals_torch_engine(weights_tamed, slots):
    """T = 21 in chunks of 5 through a ring of 9 (the minimum) and of 24 slots: identical hops, and trajectories and visibilities
    equal as bit patterns (the NaN frames before each query included)."""
    from pips_amd import drivers
    m = _model(weights_tamed)
    T, H, W = 21, 128, 160
    video = _video(T, H, W, seed=24)
    q = _queries(T, H, W, seed=25).to(DEV)
    chunks = [video[:, i:i + 5] for i in range(0, T, 5)]
    ref, ref_vis, ref_hops = drivers.track_stream(m, chunks, q, iters=6, slots=slots, return_hops=True)
    got, vis, hops = drivers.track_stream(m, chunks, q, iters=6, slots=slots, return_hops=True, engine="native")
    assert hops == ref_hops and any(len(h) > 1 for h in hops)
    assert bool(torch.isnan(ref[0, 0, 1]).all()) and tuple(got.shape) == (1, T, len(TQ), 2)
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(vis), _bits(ref_vis))


def test_track_queries_native_engine_against_reference_loop_text_golden(weights_tamed):
    """test_track_queries_at_frame_zero_against_reference_loop_text_golden with engine="native": the window starts, hop steps
    and hops per particle of the reference's own loop text (tests/golden/chain_t13.npz) and its trajectories within 1e-3 px."""
    from pips_amd import drivers
    case = G.CHAIN_CASE
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "chain_t13.npz"))
    video, xy0 = G.make_chain_inputs(case)
    q = torch.cat([torch.zeros(1, case["N"], 1), xy0], dim=-1)
    got, vis, (hops, bh) = drivers.track_queries(_model(weights_tamed, case["stride"]), video.to(DEV), q.to(DEV),
                                                 iters=case["iters"], return_hops=True, engine="native")
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
    print("track_queries (t = 0, native engine) vs reference loop text: max |dtraj| = %.2e px" % err)
    assert tuple(got.shape) == (1, case["T"], case["N"], 2) and err < 1e-3


# ------------------------------------------------------------------ argument handling
def test_chain_hop_rejects_bad_arguments_and_leaves_the_state_alone():
    """Every PIPS_E_ARG / PIPS_E_WORKSPACE case of pips_chain_hop returns its code ahead of any launch and leaves trajs, vis, cur,
    feat, next_active and next_count bit-identical; n_act == 0 is PIPS_OK, sets the count to 0 and touches nothing else."""
    from pips_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(33)
    n, n_act, L, T, iters = 12, 5, 24, 10, 2
    state = dict(trajs=torch.randn(L, n, 2, generator=g), vis=torch.randn(L, n, generator=g),
                 cur=torch.randint(0, T, (n,), generator=g).to(I32), feat=torch.randn(n, 128, generator=g),
                 next_active=torch.full((n,), -77, dtype=I32), next_count=torch.full((1,), 99, dtype=I32),
                 steps=torch.full((n,), -5, dtype=I32))
    dev = {k: v.to(DEV) for k, v in state.items()}
    active = torch.tensor([1, 4, 5, 8, 11], dtype=I32, device=DEV)
    nb = lib.pips_chain_workspace_bytes(n_act, iters)
    assert nb > lib.pips_track_workspace_bytes_s(1, n_act, 8) > 0
    assert lib.pips_chain_workspace_bytes(0, iters) == 0 and lib.pips_chain_workspace_bytes(n_act, -1) == 0
    ws = torch.zeros(nb // 4, device=DEV)
    dummy = torch.zeros(64, device=DEV)                      # stands for the arena, the pyramid and the time table: never read
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(arena=dummy, pyramid=dummy, T=T, R=T, H8=16, W8=20, times=dummy, stride=8, iters=iters, flags=0, n=n, active=active,
                n_act=n_act, sample_feat=1, trajs=dev["trajs"], vis=dev["vis"], L=L, base=7, cur=dev["cur"], dir=None,
                feat=dev["feat"], next_active=dev["next_active"], next_count=dev["next_count"], steps=dev["steps"], workspace=ws,
                workspace_bytes=nb)

    def call(**over):
        a = dict(good, **over)
        p = {k: (_lib.ptr(v) if torch.is_tensor(v) or v is None else v) for k, v in a.items()}
        return lib.pips_chain_hop(p["arena"], p["pyramid"], p["T"], p["R"], p["H8"], p["W8"], p["times"], p["stride"], p["iters"],
                                  p["flags"], p["n"], p["active"], p["n_act"], p["sample_feat"], p["trajs"], p["vis"], p["L"],
                                  p["base"], p["cur"], p["dir"], p["feat"], p["next_active"], p["next_count"], p["steps"],
                                  p["workspace"], p["workspace_bytes"], stream)

    def untouched(but_count=None):
        torch.cuda.synchronize()
        for k, v in state.items():
            want = v if but_count is None or k != "next_count" else torch.full((1,), but_count, dtype=I32)
            assert torch.equal(_bits(dev[k]), _bits(want)), k

    E_ARG, E_WORKSPACE = -1, -2
    bad = [dict(n_act=-1), dict(n_act=n + 1), dict(L=7), dict(R=0), dict(T=0), dict(active=None), dict(trajs=None), dict(cur=None),
           dict(feat=None), dict(next_active=None), dict(next_count=None), dict(next_active=active)]
    for over in bad:
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    assert call(workspace_bytes=nb - 4) == E_WORKSPACE and b"workspace" in lib.pips_last_error()
    untouched()
    assert call(workspace_bytes=0) == E_WORKSPACE
    untouched()
    assert call(n_act=0) == 0
    untouched(but_count=0)
    # the stage on its own takes the same checks
    def step(**over):
        a = dict(good, **over)
        p = {k: (_lib.ptr(v) if torch.is_tensor(v) or v is None else v) for k, v in a.items()}
        return lib.pips_chain_step(_lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy), p["T"], p["n"], p["active"], p["n_act"],
                                   p["sample_feat"], p["trajs"], p["vis"], p["L"], p["base"], p["cur"], p["dir"], p["feat"],
                                   p["next_active"], p["next_count"], p["steps"], stream)
    dev["next_count"].fill_(99)
    for over in [dict(n_act=n + 1), dict(L=7), dict(T=0), dict(cur=None), dict(next_count=None), dict(next_active=active)]:
        assert step(**over) == E_ARG, over
        untouched()
    assert step(n_act=0) == 0
    untouched(but_count=0)


# ------------------------------------------------------------------ the forwarding entry points
def test_forwarding_entry_points_equal_the_wrappers_clip_forms(weights_tamed):
    """pips_track_ring, pips_chain_gather, pips_chain_step and pips_chain_hop stay in the ABI as one-line forwards, and no Python
    wrapper reaches them any more (Pips.track and ops.chain_* call the _clips forms with a NULL table).  Each is called here through
    the binding table and its outputs and updated state are held, bit for bit, to the wrapper's: one video of 10 frames at 128x160,
    3 particles -- from frame 0, a window 5..12 that runs past the last frame, a backward one (win_dir = -1) from frame 6 that runs
    past frame 0 -- iters = 1, exact fp32."""
    from pips_amd import _lib, ops
    lib, P = _lib.load(), _lib.ptr
    m = _model(weights_tamed)
    T, H, W, n, iters, L, base = 10, 128, 160, 3, 1, 24, 7
    cache = m.encode(_video(T, H, W, seed=34).to(DEV))
    H8, W8 = cache.map_size
    arena, times = m._aux(cache.device)
    flags, stride = m._track_flags(cache), int(cache.stride)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(35)
    xy = (torch.rand(n, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
    feat0 = (torch.randn(n, 128, generator=g) * 0.1).to(DEV)
    cur = torch.tensor([0, 5, 6], dtype=I32, device=DEV)
    dirs = torch.tensor([1, 1, -1], dtype=I32, device=DEV)
    active = torch.arange(n, dtype=I32, device=DEV)

    def same(got, want, what):
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), (what, k)

    # tracker: Pips.track = pips_track_clips(win_clip = NULL)
    preds, preds2, vis, ffeat, _ = m.track(cache, xy[None], iters=iters, win_start=cur[None], win_dir=dirs[None], return_feat=True)
    nb = lib.pips_track_workspace_bytes_s(1, n, 8)
    ws = torch.empty(nb // 4, device=DEV)
    tr, vi, ff = torch.zeros(iters + 1, 1, 8, n, 2, device=DEV), torch.zeros(1, 8, n, device=DEV), torch.zeros(1, n, 128, device=DEV)
    assert lib.pips_track_ring(P(arena), P(cache.pyr), 1, T, T, H8, W8, P(xy), None, None, P(cur), P(dirs), P(times), n, stride, iters,
                               flags, 8, P(ws), nb, P(tr), P(vi), P(ff), stream) == 0
    same((tr[0], tr[1], vi, ff), (preds2[0], preds[-1], vis, ffeat), "track")
    assert bool(torch.isfinite(tr).all()) and not torch.equal(tr[1, 0, 0], tr[1, 0, 7])

    def state():
        s = dict(trajs=_nan_filled(L, n, 2).to(DEV), vis=_nan_filled(L, n).to(DEV), cur=cur.clone(), feat=feat0.clone(),
                 nxt=torch.full((n,), -77, dtype=I32, device=DEV), count=torch.full((1,), -1, dtype=I32, device=DEV),
                 steps=torch.full((n,), -1, dtype=I32, device=DEV))
        s["trajs"][(cur.long() + base) % L, torch.arange(n, device=DEV)] = xy
        return s

    # gather (the carried features are staged: sample_feat = 0)
    a = state()
    want = ops.chain_gather(a["trajs"], base, a["cur"], dirs, a["feat"], active, n)
    got = [torch.zeros_like(t) for t in want]
    assert len(want) == 4
    assert lib.pips_chain_gather(P(a["trajs"]), L, base, n, P(a["cur"]), P(dirs), P(a["feat"]), P(active), n, 0, *[P(t) for t in got],
                                 stream) == 0
    same(got, want, "gather")
    assert torch.equal(got[0], xy) and got[2].tolist() == [1, 1, -1]
    # step, on the windows the tracker gave (first window: the features are taken from it)
    win = (tr[1, 0].contiguous(), vi[0].contiguous(), ff[0].contiguous())
    a, b = state(), state()
    ops.chain_step(*win, T, active, n, a["trajs"], a["vis"], base, a["cur"], dirs, a["feat"], a["nxt"], a["count"], a["steps"],
                   sample_feat=True)
    assert lib.pips_chain_step(*[P(t) for t in win], T, n, P(active), n, 1, P(b["trajs"]), P(b["vis"]), L, base, P(b["cur"]), P(dirs),
                               P(b["feat"]), P(b["nxt"]), P(b["count"]), P(b["steps"]), stream) == 0
    same(b.values(), a.values(), "step")
    assert all(2 <= s <= 7 for s in b["steps"].tolist()) and torch.equal(b["feat"], ff[0])
    # hop
    a, b = state(), state()
    m.chain_hop(cache, active, n, a["trajs"], a["vis"], base, a["cur"], dirs, a["feat"], a["nxt"], a["count"], a["steps"], iters=iters,
                sample_feat=True)
    nb = lib.pips_chain_workspace_bytes(n, iters)
    ws = torch.empty(nb // 4, device=DEV)
    assert lib.pips_chain_hop(P(arena), P(cache.pyr), T, T, H8, W8, P(times), stride, iters, flags, n, P(active), n, 1, P(b["trajs"]),
                              P(b["vis"]), L, base, P(b["cur"]), P(dirs), P(b["feat"]), P(b["nxt"]), P(b["count"]), P(b["steps"]), P(ws),
                              nb, stream) == 0
    same(b.values(), a.values(), "hop")
    k = int(b["count"].item())
    assert all(2 <= s <= 7 for s in b["steps"].tolist()) and 0 <= k <= n and bool((b["nxt"][k:] == -77).all())
    assert int((_bits(b["trajs"]) != NAN_FILL).sum()) == 8 * n * 2 and not torch.equal(b["cur"], cur)
