"""GPU: global motion from tracks in the library.  pips_motion_fit is held to drivers.motion_table_torch run on the CPU -- head, sums
and flags as integers, the model as bits -- over the sizes around a wave, a block and a tile, every count of hypothesis blocks, the
named columns and pairs of tests/test_motion.py, with poisoned outputs, guard bands and workspace tails, unchanged inputs and its
return codes.  drivers.motion_fit with shuffled ids equals the sorted call; MotionEstimator(engine="library") equals
engine="torch" push by push on synthetic pushes and on the parts of one real CoverTracker run at 128 x 192."""
import ctypes as C

import pytest
import torch

from test_cover_gpu import ECELL, EH, ET, EW, _user
from test_motion import INF, NAN, VIS_LOGIT, _f64_bits, _life_video, _mix, _scene
from test_stream_rounds_gpu import _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
GUARD = 256                                                              # bytes on either side of an output
E_ARG, E_WORKSPACE = -1, -2
ROW = {"head": 16, "sums": 64, "model": 32}                              # bytes a pair


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, skip=0):
    return C.c_void_p(t.data_ptr() + skip)


def _poisoned(nbytes):
    return torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)


def _fit_guarded(lib, trajs, vis, frame0, vis_logit, K, thr4, seed):
    """pips_motion_fit on the host rows into poisoned buffers with guard bands around every output and a poisoned tail behind the
    workspace -> (head, sums, model, flags) on the host; guards, tail and inputs are checked"""
    F, n = trajs.shape[:2]
    P = max(F - 1, 0)
    src, v = trajs.to(DEV), None if vis is None else vis.to(DEV)
    nbytes = lib.pips_motion_workspace_bytes(F, n, K)
    assert nbytes == (P * (8 * n + 4 * (1 + (K + 63) // 64)) if P and n else 0)
    out = {k: _poisoned(P * b) for k, b in ROW.items()}
    out["flags"] = _poisoned(P * n)
    ws = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    rc = lib.pips_motion_fit(_ptr(src) if n else None, None if v is None or not n else _ptr(v), F, n, frame0, vis_logit, K, thr4, seed,
                             _ptr(out["head"], GUARD), _ptr(out["sums"], GUARD), _ptr(out["model"], GUARD), _ptr(out["flags"], GUARD),
                             _ptr(ws) if nbytes else None, nbytes, _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    size = dict(ROW, flags=n)
    for k, t in out.items():
        assert bool((t[:GUARD] == POISON).all()) and bool((t[GUARD + P * size[k]:] == POISON).all()), k
    assert bool((ws[nbytes:] == POISON).all())
    assert torch.equal(src.cpu().view(torch.int32), trajs.view(torch.int32))                   # the inputs are left as they were
    assert v is None or torch.equal(v.cpu().view(torch.int32), vis.view(torch.int32))
    body = {k: t[GUARD:GUARD + P * size[k]].cpu() for k, t in out.items()}
    return (body["head"].view(torch.int32).view(P, 4), body["sums"].view(torch.int64).view(P, 8),
            body["model"].view(torch.float64).view(P, 4), body["flags"].view(P, n))


def _check(lib, trajs, vis, frame0, K, thr4, seed, vis_logit=VIS_LOGIT):
    from pips_amd import drivers, ops
    ref = drivers.motion_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed)             # on the CPU
    got = _fit_guarded(lib, trajs, vis, frame0, vis_logit, K, thr4, seed)
    what = (tuple(trajs.shape), K, thr4, frame0)
    assert torch.equal(got[0].long(), ref[0]), what
    assert torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3]), what
    assert _f64_bits(got[2]) == _f64_bits(ref[2]), what
    via = ops.motion_fit(trajs.to(DEV), None if vis is None else vis.to(DEV), frame0, vis_logit, K, thr4, seed)
    assert via[0].dtype == torch.int32 and via[1].dtype == torch.int64 and via[2].dtype == torch.float64 and via[3].dtype == torch.uint8
    assert all(torch.equal(a.cpu(), b) for a, b in zip(via[:2] + via[3:], got[:2] + got[3:])) and _f64_bits(via[2].cpu()) == _f64_bits(got[2])
    return ref


def _tile():
    from pips_amd import ops
    return ops.MOTION_TILE


# a wave, a block and a tile of points with one less and one more; K = 1, one block of hypotheses, five with a ragged last one, all 16
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 257, "tile+1"])
def test_motion_fit_is_the_torch_form(n):
    from pips_amd import _lib
    lib = _lib.load()
    n = _tile() + 1 if n == "tile+1" else n
    for F in (1, 2, 5):
        trajs = _scene(F, n, 10 * F + n % 97)
        g = torch.Generator().manual_seed(n)
        vis = torch.randn(F, n, generator=g) + 1.0
        for K, frame0, v in ((1, 0, None), (64, 0, vis), (257, 31, None), (1024, 2 ** 31 - 1 - F, vis)):
            head = _check(lib, trajs, v, frame0, K, 8, 1234)[0]
            if F > 1 and n >= 63 and K >= 64:
                assert int(head[:, 2].min()) >= 0 and (v is not None or int(head[:, 1].min()) >= n // 4)   # a consensus was found
            if F > 1 and n > _tile() and v is None:
                assert int(head[:, 0].min()) == n                                              # more valid points than a tile holds


def test_the_named_columns():
    """NaN, +-inf, |x| = 2047.75 (usable) and 2048.0 (not), halves that round to even; vis NULL, at, above and below the threshold"""
    from pips_amd import _lib
    lib = _lib.load()
    t = _scene(3, 70, 5, outliers=0.1)
    t[0, 0, 0], t[1, 1, 1], t[0, 2, 0], t[1, 3, 1], t[2, 14, 0] = NAN, NAN, INF, -INF, NAN
    t[0, 4], t[1, 4] = torch.tensor([2047.75, -2047.75]), torch.tensor([-2047.75, 2047.75])
    t[0, 5, 0], t[1, 6, 1], t[0, 7, 0] = 2048.0, -2048.0, 3.0e38
    t[0, 8], t[1, 8] = torch.tensor([10.125, 10.375]), torch.tensor([-10.125, -10.375])
    head, _, _, flags = _check(lib, t, None, 0, 64, 8, 7)
    assert flags[0, :8].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and head[:, 0].tolist() == [70 - 7, 70 - 4]
    vis = torch.full((3, 70), 3.0)
    vis[0, 9], vis[1, 10], vis[0, 11], vis[1, 12] = VIS_LOGIT, VIS_LOGIT, NAN, -1.0
    vis[0, 13] = torch.nextafter(torch.tensor(VIS_LOGIT), torch.tensor(1.0))
    head, _, _, flags = _check(lib, t, vis, 0, 64, 8, 0xDEADBEEF)                              # (a seed with its top bit set)
    assert flags[0, 9:13].tolist() == [0, 0, 0, 0] and int(flags[0, 13]) >= 1 and head[:, 0].tolist() == [70 - 11, 70 - 6]


def test_pairs_without_a_model_ties_and_the_widest_products():
    from pips_amd import _lib
    lib = _lib.load()
    nan = torch.full((3, 70, 2), NAN)
    head, sums, model, flags = _check(lib, nan, None, 0, 64, 8, 1)                             # every column invalid
    assert head.tolist() == [[0, 0, -1, 0]] * 2 and model.tolist() == [[1.0, 0.0, 0.0, 0.0]] * 2 and int(flags.sum()) == 0
    two = nan.clone()
    two[:, 2], two[:, 67] = torch.tensor([5.0, 6.0]), torch.tensor([50.0, 9.0])
    two[1:, 67] += torch.tensor([1.0, 2.0])
    head, _, _, flags = _check(lib, two, None, 3, 5, 4, 1)                                     # m == 2
    assert head[:, :2].tolist() == [[2, 2], [2, 2]] and torch.nonzero(flags[0] == 2).squeeze(1).tolist() == [2, 67]
    same = torch.full((2, 300, 2), 33.25)
    same[1] = 40.0
    head, sums, model, flags = _check(lib, same, None, 0, 1024, 8, 1)                          # every hypothesis has d = 0
    assert head.tolist() == [[300, 0, -1, 0]] and bool((flags == 1).all()) and int(sums.abs().sum()) == 0
    g = torch.Generator().manual_seed(3)
    p = torch.randint(-400, 400, (300, 2), generator=g).float() * 0.25
    t = torch.stack([p, p + torch.tensor([3.25, -1.5])])
    i, j = (_mix(9, 1, 0) * 300) >> 32, (_mix(9, 1, 1) * 299) >> 32
    assert not torch.equal(p[i], p[j + (j >= i)])                                              # hypothesis 0 has d != 0
    for K in (64, 257, 1024):                                                                  # most hypotheses tie: the lowest h wins
        head, _, model, _ = _check(lib, t, None, 0, K, 4, 9)
        assert head[0, :2].tolist() == [300, 300] and model.tolist() == [[1.0, 0.0, 3.25, -1.5]]
        assert int(head[0, 2]) == 0
    c = 2047.75
    corners = torch.tensor([[c, c], [-c, c], [-c, -c], [c, -c]])
    t = torch.stack([corners, corners[[2, 3, 0, 1]], -corners[[1, 2, 3, 0]]])                  # a half turn, then a quarter turn
    for thr4 in (1, 1024):
        head, sums, model, _ = _check(lib, t, None, 5, 64, thr4, 2)
        assert head[:, :2].tolist() == [[4, 4], [4, 4]] and model[0].tolist() == [-1.0, 0.0, 0.0, 0.0]
        assert int(sums[0, 5]) == 8 * 8191 * 8191
    far = torch.cat([corners, torch.tensor([[c, -c + 300.0], [0.25, 0.0]])])
    _check(lib, torch.stack([far, far[[2, 3, 0, 1, 5, 4]]]), None, 0, 64, 1024, 2)


def test_bad_arguments_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    F, n, K = 3, 40, 100
    src = _scene(F, n, 1).to(DEV)
    vis = torch.zeros(F, n, device=DEV)
    keep = src.clone()
    nbytes = lib.pips_motion_workspace_bytes(F, n, K)
    assert nbytes == 2 * (320 + 12)
    bufs = {k: torch.full((s,), POISON, dtype=torch.uint8, device=DEV) for k, s in (("head", 32), ("sums", 128), ("model", 64),
                                                                                   ("flags", 2 * n), ("ws", nbytes + 16))}

    def call(**over):
        a = dict(dict(trajs=_ptr(src), vis=_ptr(vis), F=F, n=n, frame0=0, logit=0.0, K=K, thr4=8, seed=0, head=_ptr(bufs["head"]),
                      sums=_ptr(bufs["sums"]), model=_ptr(bufs["model"]), flags=_ptr(bufs["flags"]), ws=_ptr(bufs["ws"]), bytes=nbytes),
                 **over)
        rc = lib.pips_motion_fit(a["trajs"], a["vis"], a["F"], a["n"], a["frame0"], a["logit"], a["K"], a["thr4"], a["seed"], a["head"],
                                 a["sums"], a["model"], a["flags"], a["ws"], a["bytes"], _stream())
        torch.cuda.synchronize()
        assert all(bool((b == POISON).all()) for b in bufs.values()) and torch.equal(src, keep)
        return rc

    for over in (dict(F=-1), dict(F=(1 << 24) + 1), dict(n=-1), dict(n=65537), dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025),
                 dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(logit=NAN), dict(trajs=None), dict(head=None), dict(sums=None),
                 dict(model=None), dict(flags=None), dict(ws=None), dict(ws=_ptr(bufs["ws"], 8))):
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error().decode().startswith("motion_fit:"), over
    for short in (0, 1, nbytes - 1):
        assert call(bytes=short) == E_WORKSPACE
        assert lib.pips_last_error().decode().startswith("motion_fit:")
    assert call(F=1) == 0 and call(F=0, trajs=None, vis=None, head=None, sums=None, model=None, flags=None, ws=None, bytes=0) == 0
    assert lib.pips_abi_version() == 3


def test_driver_with_shuffled_ids_equals_the_sorted_call():
    from pips_amd import drivers
    trajs, g = _scene(6, 90, 8), torch.Generator().manual_seed(8)
    vis = torch.randn(6, 90, generator=g) + 1.5
    kw = dict(frame0=11, thr=1.5, hypotheses=96, vis_thr=0.7, seed=99)
    ref = drivers.motion_fit_torch(trajs[None], vis[None], **kw)                               # on the CPU
    got = drivers.motion_fit(trajs[None].to(DEV), vis[None].to(DEV), **kw)
    assert got[0].is_cuda and got[0].dtype == torch.float64 and got[1].dtype == torch.bool and got[3].dtype == torch.int64
    assert _f64_bits(got[0].cpu()) == _f64_bits(ref[0]) and all(torch.equal(a.cpu(), b) for a, b in zip(got[1:], ref[1:]))
    assert int(ref[3][:, 1].min()) >= 2 and int(ref[3][:, 0].max()) < 90                       # a consensus in every pair; vis drops columns
    perm = torch.randperm(90, generator=g)
    mixed = drivers.motion_fit(trajs[None][:, :, perm].to(DEV), vis[None][:, :, perm].to(DEV), ids=perm, **kw)
    assert _f64_bits(mixed[0].cpu()) == _f64_bits(ref[0]) and torch.equal(mixed[1].cpu(), ref[1][:, perm])
    assert torch.equal(mixed[2].cpu(), ref[2][:, perm]) and torch.equal(mixed[3].cpu(), ref[3])


def _same_steps(pushes, **kw):
    """the ``(f0, trajs, vis, ids)`` pushes through MotionEstimator(engine="library") on the device and engine="torch" on the CPU"""
    from pips_amd import drivers
    lib_est, ref_est = drivers.MotionEstimator(engine="library", **kw), drivers.MotionEstimator(engine="torch", **kw)
    pairs, inliers = 0, 0
    for f0, t, v, ids in pushes:
        got = lib_est.step(f0, t.to(DEV), None if v is None else v.to(DEV), ids=ids)
        ref = ref_est.step(f0, t.cpu(), None if v is None else v.cpu(), ids=ids)
        assert _f64_bits(got.cpu()) == _f64_bits(ref) and lib_est.T == ref_est.T
        if t.shape[1] > 0:
            assert torch.equal(lib_est.inliers.cpu(), ref_est.inliers) and torch.equal(lib_est.valid.cpu(), ref_est.valid)
            assert torch.equal(lib_est.counts.cpu(), ref_est.counts)
            inliers += int(ref_est.inliers.sum())
        pairs += ref.shape[0]
    return pairs, inliers


@pytest.mark.parametrize("with_vis", [False, True])
def test_estimator_library_equals_torch_on_synthetic_pushes(with_vis):
    """T = 19, 40 identities born and retired on the way, pushes of 3 frames with the columns in an order of their own"""
    T, K = 19, 40
    trajs, vis, born, last = _life_video(T, K, 21)
    g = torch.Generator().manual_seed(22)
    pushes = []
    for f0 in range(0, T, 3):
        f1 = min(f0 + 3, T)
        alive = torch.nonzero((born < f1) & (last >= f0)).squeeze(1)
        ids = alive[torch.randperm(alive.numel(), generator=g)]
        pushes.append((f0, trajs[None][:, f0:f1][:, :, ids], vis[None][:, f0:f1][:, :, ids] if with_vis else None, ids))
    pairs, inliers = _same_steps(pushes, thr=1.5, hypotheses=48, vis_thr=0.6, seed=5)
    assert pairs == T - 1 and inliers >= 8 * (T - 1)


def test_estimator_library_equals_torch_on_a_real_cover_run(weights_tamed):
    """one CoverTracker run at 128 x 192 (T = 24 in chunks of 4, cells of 64 px, lost_after = 2), whose identities come and go: the
    parts it returns, with their ids, through both engines"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    ct = drivers.CoverTracker(m, drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan="library"), _user(71).to(DEV), iters=6,
                              slots=24, rounds="library")
    parts = [ct.push(video[:, i:i + 4]) for i in range(0, ET, 4)] + [ct.finish()]
    assert sum(p[1].shape[1] for p in parts) == ET and len({tuple(p[3].tolist()) for p in parts if p[1].shape[1]}) > 1
    assert len(ct.retired) > 0 and len(ct.born) > parts[-1][3].numel()                         # identities came and went
    pairs, _ = _same_steps(parts, thr=2.0, hypotheses=64, vis_thr=0.1, seed=1)
    assert pairs == ET - 1
    pairs, _ = _same_steps([(f0, t, None, ids) for f0, t, _, ids in parts], hypotheses=256)
    assert pairs == ET - 1
