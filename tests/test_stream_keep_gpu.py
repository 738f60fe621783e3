"""GPU: queries leave a running stream.  pips_stream_keep (ops.stream_keep) is held, bit for bit, to a torch restatement --
``index_select`` on int32 views of a state filled with random bit patterns and NaN payloads -- with its containment columns, its
counts and its return codes; ``remove_queries`` of drivers.StreamTracker / MultiStreamTracker on the real model under
``rounds="library"`` and ``rounds="torch"`` (both engines) to each other and to the stream given the kept queries up front."""
import ctypes as C

import pytest
import torch

from test_stream_rounds_gpu import H_, W_, _assert_route_0, _model, _queries, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
INT_MAX = 2 ** 31 - 1
QUIET_NAN = 0x7FC00000
V_ = 3


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


# ------------------------------------------------------------------ the entry point against index_select
def _state(n, L, seed):
    """a state of n queries as int32 bit patterns (float arrays: any pattern, NaNs with distinct payloads among them).  The lowest
    window start of all sits on a finished query; clip takes streams 0 and 2 of V_ = 3 (and values that clamp onto them), so
    stream 1 owns no query."""
    g = torch.Generator().manual_seed(seed)

    def pattern(*shape):
        t = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g).to(I32)
        flat = t.view(-1)
        k = torch.arange(0, flat.numel(), 5)
        flat[k] = (0x7FC00001 + k).to(I32)                          # a NaN with its own payload in every fifth word
        return t

    s = dict(tq=torch.randint(0, 500, (n,), generator=g).to(I32), cur=torch.randint(100, 900, (n,), generator=g).to(I32),
             status=torch.randint(0, 3, (n,), generator=g).to(I32), xy=pattern(n, 2), feat=pattern(n, 128),
             trajs=pattern(L, n, 2), vis=pattern(L, n))
    clip = torch.randint(0, 2, (n,), generator=g).to(I32) * 2
    if n > 8:
        s["cur"][n - 1], s["status"][n - 1] = -1000, 2              # finished: below every other start, in no low
        s["status"][3], s["status"][n - 2] = 0, 1
        clip[2], clip[4] = -3, 7                                    # clamped to streams 0 and 2
    else:
        s["status"][:] = 1
    s["clip"] = clip
    return s


def _keep_list(n, kind):
    if kind == "all":
        return list(range(n))
    if kind == "none":
        return []
    if kind == "second":
        return list(range(0, n, 2))
    if kind == "last":
        return [n - 1]
    assert kind == "bad" and n > 8                                   # -1 and n among valid members; ascending, m <= n
    return [-1] + list(range(3, n, 3)) + [n]


def _expected_keep(s, keep, n, clips):
    k = torch.tensor(keep, dtype=torch.int64)
    ok = (k >= 0) & (k < n)
    safe = torch.where(ok, k, torch.zeros_like(k))
    out = {}
    for name, bad in (("tq", 0), ("cur", 0), ("status", 2), ("clip", 0), ("xy", 0), ("feat", 0)):
        v = s[name].index_select(0, safe).clone()
        v[~ok] = bad
        out[name] = v
    for name in ("trajs", "vis"):
        v = s[name].index_select(1, safe).clone()
        v[:, ~ok] = QUIET_NAN
        out[name] = v
    live = ok & (out["status"] != 2)
    cur = out["cur"].long()
    counts = [0, 0, int(cur[live].min()) if bool(live.any()) else INT_MAX, 0]
    if clips:
        v = out["clip"].long().clamp(0, V_ - 1)
        counts += [int(cur[live & (v == u)].min()) if bool((live & (v == u)).any()) else INT_MAX for u in range(V_)]
    return out, counts


def _run_keep(s, keep, clips, offset=False):
    from pips_amd import ops

    def dev(name):
        t = s[name]
        if t.dtype == I32 and name in ("xy", "feat", "trajs", "vis"):
            if offset:                                               # a base 4 bytes past a 16-byte boundary
                buf = torch.empty(t.numel() + 1, dtype=I32, device=DEV)
                buf[1:] = t.view(-1).to(DEV)
                return buf[1:].view(t.shape).view(torch.float32)
            return t.to(DEV).view(torch.float32)
        return t.to(DEV)

    d = {k: dev(k) for k in s}
    res = ops.stream_keep(torch.tensor(keep, dtype=I32, device=DEV), d["tq"], d["xy"], d["cur"], d["status"], d["feat"], d["trajs"],
                          d["vis"], clip=d["clip"] if clips else None, V=V_ if clips else 0)
    torch.cuda.synchronize()
    names = ["tq", "xy", "cur", "status", "feat", "trajs", "vis"] + (["clip"] if clips else [])
    assert len(res) == len(names) + 1
    return d, dict(zip(names, res[:-1])), res[-1]


def _check_keep(n, kind, clips, offset=False):
    keep = _keep_list(n, kind)
    m = len(keep)
    L = 32 if m % 4 == 0 else 17                                     # rows on the 16-byte grid / off it (odd m)
    s = _state(n, L, seed=100 + n)
    d, got, counts = _run_keep(s, keep, clips, offset)
    exp, exp_counts = _expected_keep(s, keep, n, clips)
    assert counts.dtype == I32 and counts.tolist() == exp_counts
    for name, g in got.items():
        want = exp[name]
        assert tuple(g.shape) == tuple(want.shape) and g.is_contiguous(), name
        assert torch.equal(_bits(g), want), name
    for name, t in s.items():                                        # every input array is bit-identical afterwards
        assert torch.equal(_bits(d[name]), t), name
    return m, L, exp_counts


CASES = [(n, kind) for n in (1, 37, 600) for kind in ("all", "none", "second", "last", "bad") if not (n == 1 and kind == "bad")]


@pytest.mark.parametrize("clips", [False, True])
@pytest.mark.parametrize("n,kind", CASES)
def test_keep_is_index_select_on_the_bit_patterns(n, kind, clips):
    """n = 1, 37 and 600 (three chunks of the 256-thread walk, the last one partial); keep = all, none, every second, the last one,
    and a list with -1 and n in it.  Odd m goes with L = 17 (vis rows off the 16-byte grid), m a multiple of 4 with L = 32.  Every
    output equals the restatement as int32 bit patterns (NaN payloads included), a member outside [0, n) gives the finished, empty
    column (status 2, zeros, rows 0x7fc00000) and enters no low, counts are the restated lows with the finished columns left
    out -- with clip and V = 3, stream 1 owns no query and reports INT_MAX -- and the inputs are untouched."""
    m, L, counts = _check_keep(n, kind, clips)
    if kind == "none":
        assert counts[2] == INT_MAX
    if n == 600 and kind == "all":
        assert (m, L) == (600, 32) and counts[2] >= 100              # the finished query's -1000 is not the low
    if n == 37 and kind == "all":
        assert (m, L) == (37, 17)
    if n > 8 and kind == "last":
        assert counts[2] == INT_MAX                                  # the one kept query is the finished one
    if clips and n > 8 and kind in ("all", "second", "bad"):
        assert counts[5] == INT_MAX and counts[4] < INT_MAX and counts[6] < INT_MAX and counts[2] == min(counts[4], counts[6])


@pytest.mark.parametrize("clips", [False, True])
def test_keep_with_bases_off_the_16_byte_grid(clips):
    """xy / feat / trajs / vis based 4 bytes past an aligned address: the word-by-word moves of both launches"""
    _check_keep(37, "second", clips, offset=True)
    _check_keep(600, "bad", clips, offset=True)


# ------------------------------------------------------------------ return codes
def test_keep_rejects_bad_arguments_and_writes_nothing():
    """every PIPS_E_ARG case of pips_stream_keep answers ahead of any launch and leaves poisoned outputs and counts untouched;
    m == 0 is PIPS_OK and writes counts alone"""
    from pips_amd import _lib
    lib = _lib.load()
    n, m, L = 12, 5, 24
    s = _state(n, L, seed=7)
    ins = {k: (v.to(DEV).view(torch.float32) if k in ("xy", "feat", "trajs", "vis") else v.to(DEV)) for k, v in s.items()}
    ins["keep"] = torch.tensor([1, 4, 5, 8, 11], dtype=I32, device=DEV)
    poison = dict(tq_out=(m,), cur_out=(m,), status_out=(m,), clip_out=(m,), xy_out=(m, 2), feat_out=(m, 128), trajs_out=(L, m, 2),
                  vis_out=(L, m), counts=(4 + V_,))
    outs = {k: torch.full(shape, -77, dtype=I32, device=DEV) for k, shape in poison.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(ins, **outs, n=n, m=m, L=L, V=V_)
    order = ["n", "keep", "m", "tq", "xy", "cur", "status", "clip", "feat", "trajs", "vis", "L", "tq_out", "xy_out", "cur_out",
             "status_out", "clip_out", "feat_out", "trajs_out", "vis_out", "V", "counts"]

    def keep(**over):
        a = dict(good, **over)
        return lib.pips_stream_keep(*[(_lib.ptr(a[k]) if torch.is_tensor(a[k]) or a[k] is None else a[k]) for k in order], stream)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t == -77).all()) for t in outs.values())
        for k, t in s.items():
            assert torch.equal(_bits(ins[k]), t), k

    E_ARG = -1
    arrays = [k for k in order if torch.is_tensor(good[k]) and k not in ("clip", "clip_out")]
    bad = [dict(n=0), dict(m=-1), dict(m=n + 1), dict(L=15), dict(V=0), dict(V=65), dict(clip=None), dict(clip_out=None)]
    for over in bad + [{k: None} for k in arrays]:
        assert keep(**over) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    assert keep(clip=None, clip_out=None, V=0) == 0                   # the one-stream form: V is not read
    torch.cuda.synchronize()
    assert outs["counts"].tolist()[:2] == [0, 0] and outs["counts"].tolist()[4:] == [-77] * V_
    assert bool((outs["clip_out"] == -77).all()) and not bool((outs["tq_out"] == -77).any())
    for t in outs.values():
        t.fill_(-77)
    assert keep(m=0, keep=None, tq_out=None, trajs_out=None) == 0     # no query kept: counts alone
    torch.cuda.synchronize()
    assert outs["counts"].tolist() == [0, 0, INT_MAX, 0] + [INT_MAX] * V_
    outs["counts"].fill_(-77)
    untouched()


# ------------------------------------------------------------------ end to end on the device
E2E_T = 21
E2E_TQ = [0, 0, 3, 3, 8, 11, 11, 14, 0, 16]
E2E_DROP = [1, 4, 7, 9]                                              # frames 14 and 16 are still waiting after 12 frames
E2E_KEPT = [c for c in range(len(E2E_TQ)) if c not in E2E_DROP]


def _collect(parts, T, n):
    """parts [(f0, trajs, vis, ids)] -> (1,T,n,2) / (1,T,n) by identity, NaN where nothing was returned"""
    tr, vi = torch.full((1, T, n, 2), float("nan"), device=DEV), torch.full((1, T, n), float("nan"), device=DEV)
    nxt = 0
    for f0, t, v, ids in parts:
        assert f0 == nxt and tuple(t.shape[2:]) == (len(ids), 2) and v.shape[2] == len(ids)
        tr[:, f0:f0 + t.shape[1], ids], vi[:, f0:f0 + v.shape[1], ids] = t, v
        nxt += t.shape[1]
    assert nxt == T
    return tr, vi


def _removal_stream(m, video, chunk, slots, late, **kw):
    """ten queries; columns E2E_DROP removed once 12 frames were pushed, then the queries ``late(st)`` added
    -> (trajs, vis by identity, hops, the late queries, the tracker)"""
    from pips_amd import drivers
    st = drivers.StreamTracker(m, _queries(E2E_TQ, 51).to(DEV), iters=6, slots=slots, record_hops=True, **kw)
    ids, parts = list(range(10)), []
    for i in range(0, 12, chunk):
        parts.append(st.push(video[:, i:i + chunk]) + (list(ids),))
    assert st.remove_queries(E2E_DROP).tolist() == E2E_KEPT
    ids = list(E2E_KEPT)
    state = st.state
    assert st.N == 6 and tuple(st.trajs.shape) == (slots + 8, 6, 2) and tuple(st.vis.shape) == (slots + 8, 6) and st.cur.shape[0] == 6
    assert state.tq.shape[0] == 6 and tuple(state.xy.shape) == (6, 2)
    if kw.get("rounds") == "library":
        assert tuple(state.feat.shape) == (6, 128) and state.status.shape[0] == state.active.shape[0] == state.new_list.shape[0] == 6
    else:
        assert state.joined.shape[0] == state.done.shape[0] == 6 and (state.eng.feat is None or tuple(state.eng.feat.shape) == (6, 128))
    q_late = late(st)
    assert st.add_queries(q_late.to(DEV)).tolist() == [6, 7]
    ids += [10, 11]
    for i in range(12, E2E_T, chunk):
        parts.append(st.push(video[:, i:i + chunk]) + (list(ids),))
    parts.append(st.finish() + (list(ids),))
    return _collect(parts, E2E_T, 12) + (st.hops, q_late, st)


@pytest.mark.parametrize("slots,chunk", [(9, 1), (24, 4)])
@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_removal_on_the_device_equals_the_stream_given_the_kept_set(weights_tamed, mode, slots, chunk):
    """T = 21 at 128x160: ten queries, four removed after 12 frames (two of them still waiting), two added after that; library
    rounds and torch rounds under both engines agree in bits and hops, and each equals the stream given the six kept and the
    two added queries up front.  At most ten rows per round: every GEMM on route 0.  One-frame pushes at slots = 9 and chunks of
    4 at slots = 24 are never split, so every frame goes through the same encoder pass in all the streams."""
    from pips_amd import drivers
    _assert_route_0(12, mode)
    m = _model(weights_tamed, mode)
    video = _video(E2E_T, H_, W_, seed=50)
    runs = {}
    for name, kw in (("library", dict(rounds="library")), ("torch", dict(engine="torch")), ("native", dict(engine="native"))):
        late = (lambda st: _queries([st.emitted, 17], 52)) if name == "library" else (lambda st: runs["library"][3])
        runs[name] = _removal_stream(m, video, chunk, slots, late, **kw)
    tr, vi, hops, q_late, st = runs["library"]
    ids = E2E_KEPT + [10, 11]
    for name in ("torch", "native"):
        assert runs[name][2] == hops, name
        assert torch.equal(_bits(runs[name][0]), _bits(tr)) and torch.equal(_bits(runs[name][1]), _bits(vi)), name
    q = torch.cat([_queries(E2E_TQ, 51)[:, E2E_KEPT], q_late], dim=1)
    pushes = [video[:, i:i + chunk] for i in range(0, 12, chunk)] + [video[:, i:i + chunk] for i in range(12, E2E_T, chunk)]
    ref_t, ref_v, ref_h = drivers.track_stream(m, pushes, q.to(DEV), iters=6, slots=slots, return_hops=True, rounds="library")
    assert hops == ref_h and any(len(h) > 1 for h in hops)
    assert torch.equal(_bits(tr[:, :, ids]), _bits(ref_t)) and torch.equal(_bits(vi[:, :, ids]), _bits(ref_v))
    for c, t in zip(ids, q[0, :, 0].long().tolist()):
        assert bool(tr[0, :t, c].isnan().all()) and bool(torch.isfinite(tr[0, t:, c]).all())


def test_removing_every_query_under_library_rounds(weights_tamed):
    """every query removed under rounds="library" (pips_stream_keep with m = 0: counts alone): the tracker runs on with no column,
    and a query added afterwards is the stream given that query alone"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(E2E_T, H_, W_, seed=50)
    st = drivers.StreamTracker(m, _queries([0, 3, 0], 57).to(DEV), iters=6, slots=24, record_hops=True, rounds="library")
    parts = [st.push(video[:, :8])]
    assert st.remove_queries([0, 1, 2]).numel() == 0 and st.N == 0 and tuple(st.trajs.shape) == (32, 0, 2) and st.state.lows() == [None]
    parts.append(st.push(video[:, 8:12]))
    assert st.emitted == 12 and tuple(parts[-1][1].shape) == (1, 12 - parts[-1][0], 0, 2)
    one = _queries([13], 58)
    assert st.add_queries(one.to(DEV)).tolist() == [0]
    parts += [st.push(video[:, 12:]), st.finish()]
    got_t, got_v = torch.cat([p[1] for p in parts[2:]], dim=1), torch.cat([p[2] for p in parts[2:]], dim=1)
    ref_t, ref_v, ref_h = drivers.track_stream(m, [video[:, :8], video[:, 8:12], video[:, 12:]], one.to(DEV), iters=6, slots=24,
                                               return_hops=True, rounds="library")
    assert parts[2][0] == 12 and torch.equal(_bits(got_t), _bits(ref_t[:, 12:])) and torch.equal(_bits(got_v), _bits(ref_v[:, 12:]))
    assert st.hops == ref_h and bool(torch.isfinite(got_t[0, 1:]).all())


def test_multi_stream_removal_on_the_device(weights_tamed):
    """two streams of 21 / 13 frames on two rings under library rounds, two queries of stream 0 removed after the second wave: each
    stream is handed, call by call, what its own StreamTracker (library rounds, same removals) hands out, hop lists included"""
    from pips_amd import drivers
    _assert_route_0(12, "exact")
    m = _model(weights_tamed)
    videos = [_video(21, H_, W_, seed=53), _video(13, H_, W_, seed=54)]
    qs = [_queries([0, 3, 3, 8, 0, 11], 55).to(DEV), _queries([0, 0, 5, 9], 56).to(DEV)]
    mt = drivers.MultiStreamTracker(m, qs, iters=6, slots=24, record_hops=True, rounds="library")
    singles = [drivers.StreamTracker(m, q, iters=6, slots=24, record_hops=True, rounds="library") for q in qs]

    def same(got, want):
        assert got[0] == want[0] and torch.equal(_bits(got[1]), _bits(want[1])) and torch.equal(_bits(got[2]), _bits(want[2]))

    for i in range(5):
        chunks = [v[:, 5 * i:5 * i + 5] for v in videos]
        chunks = [c if c.shape[1] > 0 else None for c in chunks]
        got = mt.push(chunks)
        for v, c in enumerate(chunks):
            if c is not None:
                same(got[v], singles[v].push(c))
        if i == 1:
            assert mt.remove_queries(0, [1, 5]).tolist() == singles[0].remove_queries([1, 5]).tolist() == [0, 2, 3, 4]
            st = mt.state
            assert mt.N == 8 and tuple(mt.trajs.shape) == (32, 8, 2) and st.clip.tolist() == [0] * 4 + [1] * 4
            assert tuple(st.feat.shape) == (8, 128) and st.active.shape[0] == 8 and mt.columns(1).tolist() == [4, 5, 6, 7]
    for v, g in enumerate(mt.finish()):
        same(g, singles[v].finish())
        assert mt.stream_hops(v) == singles[v].hops
    assert any(len(h) > 1 for h in mt.stream_hops(0))
