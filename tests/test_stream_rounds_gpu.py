"""GPU: the rounds of a streamed video behind the C ABI (pips_stream_select / pips_stream_round / pips_stream_emit) and the
drivers' ``rounds="library"``.  The select and emit kernels are held, bit for bit, to torch restatements written here on
synthetic state; the library rounds to the torch rounds of ``drivers.StreamTracker`` on the same model, video and queries
(identical hops, identical bits), with queries added while the video runs, and to the reference's chaining loop
(oracle/chain_oracle.py)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
INT_MAX = 2 ** 31 - 1
NAN_FILL = 0x7FC12345          # a NaN with a payload: a stray write into trajs / vis shows in the bit patterns
QUIET_NAN = 0x7FC00000


def _model(sd, mode="exact"):
    from pips_amd import Pips
    m = Pips(S=8, stride=8)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    if mode == "bf16":
        m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    return m


def _nan_filled(*shape):
    return torch.full(shape, NAN_FILL, dtype=I32).view(torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


# ------------------------------------------------------------------ select alone
SEL_T, SEL_L = 40, 32


def _select_state(n, seed, all_done=False):
    """n queries with statuses 0 / 1 / 2 mixed and window starts spread around T; the named starts (cur + 8 == T, cur + 8 ==
    T + 1, cur == T - 1, cur == T) come first, each under status 0 and 1 when n allows.  A waiting query has cur == tq."""
    g = torch.Generator().manual_seed(seed)
    T = SEL_T
    status = torch.randint(0, 3, (n,), generator=g).to(I32)
    cur = torch.randint(T - 12, T + 4, (n,), generator=g).to(I32)
    named = [T - 8, T - 7, T - 1, T]
    for j in range(min(n, 8)):
        cur[j], status[j] = named[j % 4], j // 4
    if n > 8:
        cur[8], status[8] = T + 2, 2                                            # done, beyond the video
    if all_done:
        status[:] = 2
    tq = torch.where(status == 0, cur, cur - torch.randint(0, 20, (n,), generator=g).to(I32))
    xy = torch.randn(n, 2, generator=g) * 50
    return dict(n=n, tq=tq, cur=cur, status=status, xy=xy, trajs=_nan_filled(SEL_L, n, 2))


def _expected_select(s, final):
    """the lines of drivers._TorchRounds.run / lows (the form without a clip table) that pips_stream_select stands for, on the CPU"""
    T, L = SEL_T, SEL_L
    status, cur, tq = s["status"].clone().long(), s["cur"].long(), s["tq"].long()
    trajs = s["trajs"].clone()
    if final:
        status[(status == 1) & (cur >= T)] = 2
    live = status != 2
    ready = live & ((cur < T) if final else (cur + 8 <= T))
    active = torch.nonzero(ready).squeeze(1)
    new = torch.nonzero(ready & (status == 0)).squeeze(1)
    trajs[tq[new] % L, new] = s["xy"][new]
    status[new] = 1
    low = int(cur[live].min()) if bool(live.any()) else INT_MAX
    return dict(active=active.to(I32), new=new.to(I32), status=status.to(I32), trajs=trajs,
                counts=torch.tensor([active.numel(), new.numel(), low, 0], dtype=I32))


@pytest.mark.parametrize("final", [0, 1])
@pytest.mark.parametrize("n", [1, 256, 600])
def test_select_is_the_torch_lines_of_rounds(n, final):
    """pips_stream_select over n = 600 queries (three chunks of the 256-thread block: the offsets of both lists are carried
    twice), one full chunk and a single query: active, new_list, counts, status and the seeded rows of a NaN-payload trajs
    buffer equal the torch restatement as int32 bit patterns; nothing is written past the counts, cur / tq / xy stay."""
    from pips_amd import ops
    s = _select_state(n, seed=40 + n)
    exp = _expected_select(s, final)
    if n == 600:                         # the expectation is not vacuous: every named start does what it was built for
        act, new = exp["active"].tolist(), exp["new"].tolist()
        assert (0 in act) and (0 in new) and (4 in act) and (4 not in new)               # cur + 8 == T: ready
        assert (1 in act) == bool(final) and (5 in act) == bool(final)                   # cur + 8 == T + 1: ready at the end only
        assert (2 in act) == bool(final) and (3 not in act) and (7 not in act)           # cur == T - 1 / cur == T
        assert int(exp["status"][7]) == (2 if final else 1) and int(exp["status"][3]) == 0
        for lst in (act, new):           # each of the block's three chunks adds to both lists: the offsets are carried twice
            assert any(q < 256 for q in lst) and any(256 <= q < 512 for q in lst) and any(q >= 512 for q in lst)
        assert 100 < len(act) < n and 20 < len(new) < len(act)
        assert int(exp["counts"][2]) == SEL_T - 12
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    active = torch.full((n,), -77, dtype=I32, device=DEV)
    new_list = torch.full((n,), -78, dtype=I32, device=DEV)
    counts = torch.full((4,), -1, dtype=I32, device=DEV)
    ops.stream_select(SEL_T, final, d["tq"], d["xy"], d["cur"], d["status"], d["trajs"], active, new_list, counts)
    torch.cuda.synchronize()
    ka, kn = exp["active"].numel(), exp["new"].numel()
    assert torch.equal(counts.cpu(), exp["counts"])
    assert torch.equal(active.cpu()[:ka], exp["active"]) and bool((active.cpu()[ka:] == -77).all())
    assert torch.equal(new_list.cpu()[:kn], exp["new"]) and bool((new_list.cpu()[kn:] == -78).all())
    assert torch.equal(d["status"].cpu(), exp["status"])
    assert torch.equal(_bits(d["trajs"]), _bits(exp["trajs"]))
    assert int((_bits(exp["trajs"]) != NAN_FILL).sum()) == 2 * kn
    assert torch.equal(d["cur"].cpu(), s["cur"]) and torch.equal(d["tq"].cpu(), s["tq"]) and torch.equal(_bits(d["xy"]), _bits(s["xy"]))


@pytest.mark.parametrize("final", [0, 1])
def test_select_with_every_query_done(final):
    from pips_amd import ops
    n = 600
    s = _select_state(n, seed=41, all_done=True)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    active = torch.full((n,), -77, dtype=I32, device=DEV)
    new_list = torch.full((n,), -78, dtype=I32, device=DEV)
    counts = torch.full((4,), -1, dtype=I32, device=DEV)
    ops.stream_select(SEL_T, final, d["tq"], d["xy"], d["cur"], d["status"], d["trajs"], active, new_list, counts)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, INT_MAX, 0]
    assert bool((active == -77).all()) and bool((new_list == -78).all()) and bool((d["status"] == 2).all())
    assert torch.equal(_bits(d["trajs"]), _bits(s["trajs"]))


# ------------------------------------------------------------------ emit alone
@pytest.mark.parametrize("frames", ["wrap", "none", "all"])
@pytest.mark.parametrize("L,n", [(17, 5), (32, 64)])
def test_emit_moves_the_final_rows_out_of_the_ring(L, n, frames):
    """pips_stream_emit on buffers of arbitrary bit patterns (NaNs with payloads among them): L = 17, n = 5 -- rows of 40 and 20
    bytes, moved word by word -- and L = 32, n = 64 -- rows of 512 and 256 bytes, moved in 16-byte pieces.  The frames wrap
    past row L - 1; f1 - f0 of 0 and of L.  The outputs are the rows' bits, the emitted rows are 0x7fc00000, every other row
    is untouched."""
    from pips_amd import ops
    g = torch.Generator().manual_seed(42 + L)
    trajs = torch.randint(-2 ** 31, 2 ** 31, (L, n, 2), generator=g).to(I32)
    vis = torch.randint(-2 ** 31, 2 ** 31, (L, n), generator=g).to(I32)
    trajs[1, 0, 0], vis[L - 1, n - 1] = NAN_FILL, NAN_FILL
    f0 = 3 * L + L - 3                                          # rows L-3, L-2, L-1, 0, 1, ...
    f1 = {"wrap": f0 + 7, "none": f0, "all": f0 + L}[frames]
    rows = torch.arange(f0, f1) % L
    d_t, d_v = trajs.to(DEV).view(torch.float32), vis.to(DEV).view(torch.float32)
    out_t, out_v = ops.stream_emit(d_t, d_v, f0, f1)
    torch.cuda.synchronize()
    assert tuple(out_t.shape) == (f1 - f0, n, 2) and tuple(out_v.shape) == (f1 - f0, n)
    assert torch.equal(_bits(out_t), trajs[rows]) and torch.equal(_bits(out_v), vis[rows])
    want_t, want_v = trajs.clone(), vis.clone()
    want_t[rows], want_v[rows] = QUIET_NAN, QUIET_NAN
    assert torch.equal(_bits(d_t), want_t) and torch.equal(_bits(d_v), want_v)
    if frames == "wrap":
        assert rows.tolist() == [L - 3, L - 2, L - 1, 0, 1, 2, 3]
        assert torch.equal(_bits(torch.full((1,), float("nan"))), torch.tensor([QUIET_NAN], dtype=I32))   # torch's own NaN fill


# ------------------------------------------------------------------ library rounds against the torch rounds
def _video(T, H, W, seed, slope=0.03, step=7.0, noise=40):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 1, 3, H, W), generator=g).float()
    video = torch.cat([(base * (1 - slope * t) + step * t).clamp(0, 255).round() for t in range(T)], dim=1)
    return (video + torch.randint(0, noise, video.shape, generator=g).float()).clamp(0, 255)


H_, W_ = 128, 160


def _queries(tq, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(1, len(tq), 2, generator=g) * torch.tensor([W_ - 17.0, H_ - 17.0]) + 8.0
    return torch.cat([torch.tensor(tq, dtype=torch.float32).view(1, -1, 1), xy], dim=-1)


def _assert_route_0(n_max, mode):
    """every GEMM of the mixer takes route 0 (rows computed independently of M) at M = 8 k for every row count k <= n_max a round
    can have: a query then computes the same bits whichever queries share its round"""
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


TQ = [0, 3, 11, 11, 0, 3]


@pytest.mark.parametrize("T,chunk,slots,mode", [(21, 5, 9, "exact"), (21, 5, 24, "exact"), (21, 5, 9, "bf16"), (21, 5, 24, "bf16"),
                                                (40, 16, 24, "exact")])
def test_library_rounds_equal_torch_rounds(weights_tamed, T, chunk, slots, mode):
    """track_stream(rounds="library") against rounds="torch" under both engines: queries at frames 0, 3 and 11, T = 21 in chunks
    of 5 through rings of 9 (the minimum) and 24 slots in fp32 and bf16, T = 40 in chunks of 16 -- identical hop lists, and
    trajectories and visibilities equal as bit patterns (the NaN frames before each query included)."""
    from pips_amd import drivers
    _assert_route_0(len(TQ), mode)
    m = _model(weights_tamed, mode)
    video = _video(T, H_, W_, seed=43)
    q = _queries(TQ, seed=44).to(DEV)
    chunks = [video[:, i:i + chunk] for i in range(0, T, chunk)]
    got, vis, hops = drivers.track_stream(m, chunks, q, iters=6, slots=slots, return_hops=True, rounds="library")
    assert tuple(got.shape) == (1, T, len(TQ), 2) and any(len(h) > 1 for h in hops)
    assert bool(torch.isnan(got[0, :11, 2]).all()) and bool(torch.isfinite(got[0, 11:, 2]).all())
    for engine in ("torch", "native"):
        ref, ref_vis, ref_hops = drivers.track_stream(m, chunks, q, iters=6, slots=slots, return_hops=True, engine=engine)
        assert hops == ref_hops, engine
        assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(vis), _bits(ref_vis)), engine
    plain = drivers.track_stream(m, chunks, q, iters=6, slots=slots, rounds="library")          # without the hop log
    assert torch.equal(_bits(plain[0]), _bits(got)) and torch.equal(_bits(plain[1]), _bits(vis))


def _recorded_entries(monkeypatch):
    """-> the list that receives the name of every entry point called through ops._call from now on"""
    from pips_amd import ops
    names, real = [], ops._call

    def recorded(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", recorded)
    return names


def test_stream_tracker_makes_the_one_video_library_calls(weights_tamed, monkeypatch):
    """A StreamTracker under rounds="library" -- 21 frames in chunks of 5 through 9 slots, one query removed on the way -- calls the
    NULL-table entry points it always called, and no _clips / _cols / _at form (the set is read off the drivers before the two
    trackers shared a core); the outputs are those of rounds="torch", bit for bit with the hop lists."""
    from pips_amd import drivers
    _assert_route_0(4, "exact")
    m = _model(weights_tamed)
    video = _video(21, H_, W_, seed=43)
    q = _queries([0, 3, 11, 11], seed=44).to(DEV)

    def run(rounds):
        st = drivers.StreamTracker(m, q, iters=6, slots=9, record_hops=True, rounds=rounds)
        parts = []
        for i in range(0, 21, 5):
            parts.append(st.push(video[:, i:i + 5]))
            if i == 10:
                assert st.remove_queries([1]).tolist() == [0, 2, 3]
        return parts + [st.finish()], st.hops

    names = _recorded_entries(monkeypatch)
    parts, hops = run("library")
    seen = {n for n in names if n.startswith(("pips_stream_", "pips_pyramid_append"))}
    assert seen == {"pips_pyramid_append", "pips_stream_select", "pips_stream_round", "pips_stream_emit", "pips_stream_keep"}
    ref, ref_hops = run("torch")
    assert hops == ref_hops and any(len(h) > 1 for h in hops) and sum(p[1].shape[1] for p in parts) == 21
    for (f0, tr, vi), (g0, ref_t, ref_v) in zip(parts, ref):
        assert f0 == g0 and torch.equal(_bits(tr), _bits(ref_t)) and torch.equal(_bits(vi), _bits(ref_v))


# ------------------------------------------------------------------ queries added while the video runs
ADD_T = 29


@functools.lru_cache(maxsize=None)
def _add_video():
    return _video(ADD_T, H_, W_, seed=45)


def _add_stream(m, chunk, slots):
    """the schedule of tests/test_stream_rounds.py under rounds="library": queries at frames 0 and 5 at construction, 9 and 20
    added once 8 frames were pushed, 25 and the oldest frame not returned yet once 16 were -> (trajs, vis with NaN for the
    columns a part did not have yet, hops, all queries)"""
    from pips_amd import drivers
    video = _add_video()

    def chunks(a, b):
        return [video[:, i:min(i + chunk, b)] for i in range(a, b, chunk)]

    first, early = _queries([0, 5], 46), _queries([9, 20], 47)
    st = drivers.StreamTracker(m, first.to(DEV), iters=6, slots=slots, record_hops=True, rounds="library")
    parts = [st.push(c) for c in chunks(0, 8)]
    assert st.add_queries(early.to(DEV)).tolist() == [2, 3]
    parts += [st.push(c) for c in chunks(8, 16)]
    late = _queries([25, st.emitted], 48)
    assert st.add_queries(late.to(DEV)).tolist() == [4, 5]
    parts += [st.push(c) for c in chunks(16, ADD_T)] + [st.finish()]
    full_t = torch.full((1, ADD_T, 6, 2), float("nan"), device=DEV)
    full_v = torch.full((1, ADD_T, 6), float("nan"), device=DEV)
    nxt = 0
    for f0, tr, vi in parts:
        assert f0 == nxt
        full_t[:, f0:f0 + tr.shape[1], :tr.shape[2]] = tr
        full_v[:, f0:f0 + vi.shape[1], :vi.shape[2]] = vi
        nxt += tr.shape[1]
    assert nxt == ADD_T
    return full_t, full_v, st.hops, torch.cat([first, early, late], dim=1)


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_added_queries_under_library_rounds(weights_tamed, chunk, slots):
    """add_queries under rounds="library" at T = 29: the outputs are those of a stream given all six queries up front -- under
    library rounds and under torch rounds -- as bit patterns, hop lists included; every frame comes back once."""
    from pips_amd import drivers
    _assert_route_0(6, "exact")
    m = _model(weights_tamed)
    got_t, got_v, hops, q = _add_stream(m, chunk, slots)
    video = _add_video()
    up_front = [video[:, i:i + 7] for i in range(0, ADD_T, 7)]
    for rounds in ("library", "torch"):
        ref_t, ref_v, ref_h = drivers.track_stream(m, up_front, q.to(DEV), iters=6, slots=24, return_hops=True, rounds=rounds)
        assert hops == ref_h, rounds
        assert torch.equal(_bits(got_t), _bits(ref_t)) and torch.equal(_bits(got_v), _bits(ref_v)), rounds
    assert any(len(h) > 1 for h in hops)
    for n, t in enumerate(q[0, :, 0].long().tolist()):
        assert bool(got_t[0, :t, n].isnan().all()) and bool(torch.isfinite(got_t[0, t:, n]).all())


# ------------------------------------------------------------------ against the reference's loop
def test_library_rounds_against_reference_loop(weights_tamed):
    """One chunk from frame 0 through rounds="library" at T = 21, 128x160, stride 8, against oracle/chain_oracle.chain: identical
    hop sequences and the gate of tests/test_stream_gpu.py::test_track_stream_against_reference_loop, 1e-3 px over every
    frame (3.1e-5 px measured there)."""
    from pips_amd import drivers
    from oracle import chain_oracle
    T, N = 21, 8
    video = _video(T, H_, W_, seed=37)
    q = _queries([0] * N, seed=38)
    got, vis, hops = drivers.track_stream(_model(weights_tamed), [video], q.to(DEV), iters=6, slots=T + 8, return_hops=True,
                                          rounds="library")
    ref, rh = chain_oracle.chain(weights_tamed, video, q[:, :, 1:], iters=6, stride=8, cache_frames=True)
    assert hops == rh and any(len(h) > 1 for h in hops)
    err = float((got.cpu() - ref.cpu()).abs().max())
    print("track_stream (library rounds) vs reference loop: max |dtraj| %.2e px; hops %s" % (err, hops))
    assert tuple(got.shape) == (1, T, N, 2) and bool(torch.isfinite(vis).all())
    assert err < 1e-3


# ------------------------------------------------------------------ argument handling
def test_stream_calls_reject_bad_arguments_and_leave_the_state_alone():
    """Every PIPS_E_ARG / PIPS_E_WORKSPACE case of pips_stream_select / pips_stream_round / pips_stream_emit returns its code
    ahead of any launch and leaves the NaN-payload state bit-identical; n_act == 0 and f0 == f1 are PIPS_OK and touch nothing."""
    from pips_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(49)
    n, n_act, n_new, L, T, R, iters = 12, 5, 2, 24, 10, 16, 2
    state = dict(tq=torch.randint(0, T, (n,), generator=g).to(I32), xy=torch.randn(n, 2, generator=g),
                 cur=torch.randint(0, T, (n,), generator=g).to(I32), status=torch.randint(0, 3, (n,), generator=g).to(I32),
                 feat=torch.randn(n, 128, generator=g), trajs=_nan_filled(L, n, 2), vis=_nan_filled(L, n),
                 active=torch.full((n,), -77, dtype=I32), new_list=torch.full((n,), -78, dtype=I32),
                 counts=torch.full((4,), 99, dtype=I32), steps=torch.full((n,), -5, dtype=I32),
                 out_trajs=_nan_filled(L, n, 2), out_vis=_nan_filled(L, n))
    dev = {k: v.to(DEV) for k, v in state.items()}
    dev["active"][:n_act] = torch.tensor([1, 4, 5, 8, 11], dtype=I32)
    dev["new_list"][:n_new] = torch.tensor([4, 8], dtype=I32)
    state["active"], state["new_list"] = dev["active"].cpu(), dev["new_list"].cpu()
    nb = lib.pips_stream_workspace_bytes(n, iters)
    assert nb > lib.pips_chain_workspace_bytes(n, iters) > 0
    ws = torch.zeros(nb // 4, device=DEV)
    dummy = torch.zeros(64, device=DEV)                      # stands for the arena, the pyramid and the time table: never read
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(dev, arena=dummy, pyramid=dummy, T=T, R=R, H8=16, W8=20, times=dummy, stride=8, iters=iters, flags=0, final=0, n=n,
                n_act=n_act, n_new=n_new, L=L, workspace=ws, workspace_bytes=nb, f0=20, f1=27)

    def args(over):
        a = dict(good, **over)
        return {k: (_lib.ptr(v) if torch.is_tensor(v) or v is None else v) for k, v in a.items()}

    def select(**over):
        p = args(over)
        return lib.pips_stream_select(p["T"], p["final"], p["n"], p["tq"], p["xy"], p["cur"], p["status"], p["trajs"], p["L"],
                                      p["active"], p["new_list"], p["counts"], stream)

    def round_(**over):
        p = args(over)
        return lib.pips_stream_round(p["arena"], p["pyramid"], p["T"], p["R"], p["H8"], p["W8"], p["times"], p["stride"], p["iters"],
                                     p["flags"], p["final"], p["n"], p["n_act"], p["n_new"], p["tq"], p["xy"], p["cur"], p["status"],
                                     p["feat"], p["trajs"], p["vis"], p["L"], p["active"], p["new_list"], p["counts"], p["steps"],
                                     p["workspace"], p["workspace_bytes"], stream)

    def emit(**over):
        p = args(over)
        return lib.pips_stream_emit(p["trajs"], p["vis"], p["L"], p["n"], p["f0"], p["f1"], p["out_trajs"], p["out_vis"], stream)

    def untouched():
        torch.cuda.synchronize()
        for k, v in state.items():
            assert torch.equal(_bits(dev[k]), _bits(v)), k
        assert not bool(ws.any())

    E_ARG, E_WORKSPACE = -1, -2
    nulls = ["tq", "xy", "cur", "status", "trajs", "active", "new_list", "counts"]
    for over in [dict(n=0), dict(L=15), dict(T=0)] + [{k: None} for k in nulls]:
        assert select(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    bad = [dict(n=0), dict(n_act=-1), dict(n_act=n + 1), dict(n_new=-1), dict(n_new=n + 1), dict(n_new=n_act + 1), dict(L=15),
           dict(R=8), dict(T=0)]
    for over in bad + [{k: None} for k in nulls + ["feat", "vis", "arena", "pyramid", "times", "workspace"]]:
        assert round_(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    assert round_(workspace_bytes=nb - 4) == E_WORKSPACE and b"workspace" in lib.pips_last_error()
    untouched()
    assert round_(workspace_bytes=0) == E_WORKSPACE
    untouched()
    assert round_(n_act=0, n_new=0) == 0
    untouched()
    for over in [dict(n=0), dict(L=15), dict(f1=19), dict(f1=20 + L + 1), dict(trajs=None), dict(vis=None), dict(out_trajs=None),
                 dict(out_vis=None)]:
        assert emit(**over) == E_ARG, over
        untouched()
    assert emit(f1=20) == 0
    untouched()
