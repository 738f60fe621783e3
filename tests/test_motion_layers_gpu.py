"""GPU: motion layers in the library.  pips_motion_layers is held to drivers.motion_layers_table_torch run on the CPU -- head, sums,
box, layer and overlap as integers, the model as bits -- over the sizes around a wave, a block and a tile, every count of layers and
hypothesis blocks, the named columns of tests/test_motion_gpu.py, with poisoned outputs, guard bands and workspace tails, unchanged
inputs and its return codes.  Layer 0 equals ops.motion_fit on the same device rows.  drivers.motion_layers with shuffled ids equals
the sorted call; MotionLayers(engine="library") equals engine="torch" push by push on the scene of tests/test_motion_layers.py and
on the parts of one real CoverTracker run at 128 x 192."""
import ctypes as C

import pytest
import torch

from test_cover_gpu import ECELL, EH, ET, EW, _user
from test_motion import INF, NAN, VIS_LOGIT, _f64_bits, _scene
from test_motion_layers import SCENE_SEEDS, _meaning_scene, _scene_conditions
from test_stream_rounds_gpu import _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
GUARD = 256                                                              # bytes on either side of an output
E_ARG, E_WORKSPACE = -1, -2
ROW = {"head": 16, "sums": 64, "model": 32, "box": 16}                   # bytes a (pair, layer)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, skip=0):
    return C.c_void_p(t.data_ptr() + skip)


def _poisoned(nbytes):
    return torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)


def _layers_guarded(lib, trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev):
    """pips_motion_layers on the host rows into poisoned buffers with guard bands around every output and a poisoned tail behind the
    workspace -> (head, sums, model, box, layer, overlap) on the host; guards, tail and inputs are checked"""
    F, n = trajs.shape[:2]
    P = max(F - 1, 0)
    src, v, pv = trajs.to(DEV), None if vis is None else vis.to(DEV), None if prev is None else prev.to(DEV)
    nbytes = lib.pips_motion_layers_workspace_bytes(F, n, K, L)
    assert nbytes == (P * (24 * n + 4 * (1 + (K + 63) // 64)) if P and n else 0)               # the header's formula
    size = {k: L * b for k, b in ROW.items()}
    size.update(layer=n, overlap=4 * L * L)
    out = {k: _poisoned(P * b) for k, b in size.items()}
    ws = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    rc = lib.pips_motion_layers(_ptr(src) if n else None, None if v is None or not n else _ptr(v),
                                None if pv is None or not n else _ptr(pv), F, n, frame0, vis_logit, K, thr4, seed, L, min_in,
                                _ptr(out["head"], GUARD), _ptr(out["sums"], GUARD), _ptr(out["model"], GUARD), _ptr(out["box"], GUARD),
                                _ptr(out["layer"], GUARD), _ptr(out["overlap"], GUARD), _ptr(ws) if nbytes else None, nbytes, _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t[:GUARD] == POISON).all()) and bool((t[GUARD + P * size[k]:] == POISON).all()), k
    assert bool((ws[nbytes:] == POISON).all())
    assert torch.equal(src.cpu().view(torch.int32), trajs.view(torch.int32))                   # the inputs are left as they were
    assert v is None or torch.equal(v.cpu().view(torch.int32), vis.view(torch.int32))
    assert pv is None or torch.equal(pv.cpu(), prev)
    body = {k: t[GUARD:GUARD + P * size[k]].cpu() for k, t in out.items()}
    return (body["head"].view(torch.int32).view(P, L, 4), body["sums"].view(torch.int64).view(P, L, 8),
            body["model"].view(torch.float64).view(P, L, 4), body["box"].view(torch.int32).view(P, L, 4), body["layer"].view(P, n),
            body["overlap"].view(torch.int32).view(P, L, L))


def _check(lib, trajs, vis, frame0, K, thr4, seed, L, min_in, prev=None, vis_logit=VIS_LOGIT):
    from pips_amd import drivers, ops
    ref = drivers.motion_layers_table_torch(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev)   # on the CPU
    signed = seed - (1 << 32) if seed >= 1 << 31 else seed
    got = _layers_guarded(lib, trajs, vis, frame0, vis_logit, K, thr4, signed, L, min_in, prev)
    what = (tuple(trajs.shape), K, thr4, frame0, L, min_in)
    for k in (0, 1, 3, 4, 5):
        assert torch.equal(got[k].long(), ref[k].long()), (k, what)
    assert _f64_bits(got[2]) == _f64_bits(ref[2]), what
    dev = trajs.to(DEV), None if vis is None else vis.to(DEV)
    via = ops.motion_layers(dev[0], dev[1], frame0, vis_logit, K, thr4, seed, L, min_in, None if prev is None else prev.to(DEV))
    assert [t.dtype for t in via] == [torch.int32, torch.int64, torch.float64, torch.int32, torch.uint8, torch.int32]
    assert all(torch.equal(a.cpu(), b) for a, b in zip(via[:2] + via[3:], got[:2] + got[3:])) and _f64_bits(via[2].cpu()) == _f64_bits(got[2])
    # layer 0 is pips_motion_fit on the same device rows, bit for bit
    fit = ops.motion_fit(dev[0], dev[1], frame0, vis_logit, K, thr4, seed)
    assert torch.equal(via[0][:, 0], fit[0]) and torch.equal(via[1][:, 0], fit[1]) and _f64_bits(via[2][:, 0].cpu()) == _f64_bits(fit[2].cpu())
    assert torch.equal(via[4] == 0, fit[3] == 2) and torch.equal(via[4] == 255, fit[3] == 0)
    return ref


def _tile():
    from pips_amd import ops
    return ops.MOTION_TILE


# a wave, a block and a tile of points with one less and one more; every (L, K): one layer and one hypothesis, two layers and one block
# of hypotheses, four and five blocks with a ragged last one, eight and all 16
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 257, "tile+1"])
def test_motion_layers_is_the_torch_form(n):
    from pips_amd import _lib
    lib = _lib.load()
    n = _tile() + 1 if n == "tile+1" else n
    found = 0
    for F in (1, 2, 5):
        trajs = _scene(F, n, 10 * F + n % 97, outliers=0.4)
        g = torch.Generator().manual_seed(n)
        vis = torch.randn(F, n, generator=g) + 1.0
        prev = torch.randint(0, 10, (n,), generator=g).to(torch.uint8)
        prev[prev == 8], prev[prev == 9] = 254, 255
        for L, K, frame0, v, pv, min_in in ((1, 1, 0, None, None, 2), (2, 64, 0, vis, prev, 3), (4, 257, 31, None, prev, 2),
                                            (8, 1024, 2 ** 31 - 1 - F, vis, None, 2)):
            head = _check(lib, trajs, v, frame0, K, 8, 1234, L, min_in, pv)[0]
            if F > 1 and n >= 63 and K >= 64:
                assert int(head[:, 0, 2].min()) >= 0 and (v is not None or int(head[:, 0, 1].min()) >= n // 4)   # a consensus
                found += int((head[:, 1:, 2] >= 0).sum())
            if F > 1 and n > _tile() and v is None:
                assert int(head[:, 0, 0].min()) == n                                           # more valid points than a tile holds
    assert n < 63 or found >= 10                                                               # layers above 0 were found


def test_the_named_columns():
    """NaN, +-inf, |x| = 2047.75 (usable) and 2048.0 (not), halves that round to even; vis NULL, at, above and below the threshold"""
    from pips_amd import _lib
    lib = _lib.load()
    t = _scene(3, 70, 5, outliers=0.3)
    t[0, 0, 0], t[1, 1, 1], t[0, 2, 0], t[1, 3, 1], t[2, 14, 0] = NAN, NAN, INF, -INF, NAN
    t[0, 4], t[1, 4] = torch.tensor([2047.75, -2047.75]), torch.tensor([-2047.75, 2047.75])
    t[0, 5, 0], t[1, 6, 1], t[0, 7, 0] = 2048.0, -2048.0, 3.0e38
    t[0, 8], t[1, 8] = torch.tensor([10.125, 10.375]), torch.tensor([-10.125, -10.375])
    head, _, _, _, layer, _ = _check(lib, t, None, 0, 64, 8, 7, 4, 2)
    assert [int(x) for x in layer[0, :8]] == [255, 255, 255, 255, int(layer[0, 4]), 255, 255, 255] and int(layer[0, 4]) != 255
    assert head[:, 0, 0].tolist() == [70 - 7, 70 - 4]
    vis = torch.full((3, 70), 3.0)
    vis[0, 9], vis[1, 10], vis[0, 11], vis[1, 12] = VIS_LOGIT, VIS_LOGIT, NAN, -1.0
    vis[0, 13] = torch.nextafter(torch.tensor(VIS_LOGIT), torch.tensor(1.0))
    head, _, _, _, layer, _ = _check(lib, t, vis, 0, 64, 8, 0xDEADBEEF, 4, 2)                  # (a seed with its top bit set)
    assert layer[0, 9:13].tolist() == [255] * 4 and int(layer[0, 13]) != 255 and head[:, 0, 0].tolist() == [70 - 11, 70 - 6]


def test_pairs_and_layers_without_a_model():
    from pips_amd import _lib
    lib = _lib.load()
    nan = torch.full((3, 70, 2), NAN)
    head, sums, model, box, layer, overlap = _check(lib, nan, None, 0, 64, 8, 1, 3, 2)         # every column invalid
    assert head.tolist() == [[[0, 0, -1, 0]] * 3] * 2 and model.tolist() == [[[1.0, 0.0, 0.0, 0.0]] * 3] * 2
    assert bool((layer == 255).all()) and int(overlap.abs().sum()) == 0 and int(box.abs().sum()) == 0
    two = nan.clone()
    two[:, 2], two[:, 67] = torch.tensor([5.0, 6.0]), torch.tensor([50.0, 9.0])
    two[1:, 67] += torch.tensor([1.0, 2.0])
    head, _, _, _, layer, overlap = _check(lib, two, None, 3, 5, 4, 1, 2, 8)                   # m == 2: need_0 = 2 whatever min_in
    assert head[:, 0, :2].tolist() == [[2, 2], [2, 2]] and torch.nonzero(layer[0] == 0).squeeze(1).tolist() == [2, 67]
    assert head[:, 1].tolist() == [[0, 0, -1, 0]] * 2 and overlap[1].tolist() == [[2, 0], [0, 0]]
    same = torch.full((2, 300, 2), 33.25)
    same[1] = 40.0
    head, sums, _, _, layer, _ = _check(lib, same, None, 0, 1024, 8, 1, 4, 2)                  # every hypothesis of every layer has d = 0
    assert head.tolist() == [[[300, 0, -1, 0]] * 4] and bool((layer == 254).all()) and int(sums.abs().sum()) == 0
    # min_in at the boundary: twelve columns shift one way, five another, three go ways of their own
    g = torch.Generator().manual_seed(1)
    p = torch.randperm(2000, generator=g)[:40].view(20, 2).float() * 0.25 + 3.0
    shift = torch.tensor([[2.0, 1.0]] * 12 + [[-30.0, 40.5]] * 5 + [[100.0, -60.0], [137.0, -113.0], [-174.0, 166.0]])
    t = torch.stack([p, p + shift])
    head = _check(lib, t, None, 6, 256, 4, 0xF0000000, 3, 5)[0]
    assert head[0, :, :2].tolist() == [[20, 12], [8, 5], [3, 0]]
    head = _check(lib, t, None, 6, 256, 4, 0xF0000000, 3, 6)[0]
    assert head[0, :, :2].tolist() == [[20, 12], [8, 0], [8, 0]]                               # nothing left layer 1's list


def test_bad_arguments_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    F, n, K, L = 3, 40, 100, 3
    src = _scene(F, n, 1).to(DEV)
    vis = torch.zeros(F, n, device=DEV)
    prev = torch.zeros(n, dtype=torch.uint8, device=DEV)
    keep = src.clone()
    nbytes = lib.pips_motion_layers_workspace_bytes(F, n, K, L)
    assert nbytes == 2 * (960 + 12)
    bufs = {k: torch.full((s,), POISON, dtype=torch.uint8, device=DEV)
            for k, s in (("head", 32 * L), ("sums", 128 * L), ("model", 64 * L), ("box", 32 * L), ("layer", 2 * n), ("overlap", 8 * L * L),
                         ("ws", nbytes + 16), ("lay2", 4 * n))}

    def call(**over):
        a = dict(dict(trajs=_ptr(src), vis=_ptr(vis), prev=_ptr(prev), F=F, n=n, frame0=0, logit=0.0, K=K, thr4=8, seed=0, L=L, min_in=8,
                      head=_ptr(bufs["head"]), sums=_ptr(bufs["sums"]), model=_ptr(bufs["model"]), box=_ptr(bufs["box"]),
                      layer=_ptr(bufs["layer"]), overlap=_ptr(bufs["overlap"]), ws=_ptr(bufs["ws"]), bytes=nbytes), **over)
        rc = lib.pips_motion_layers(a["trajs"], a["vis"], a["prev"], a["F"], a["n"], a["frame0"], a["logit"], a["K"], a["thr4"], a["seed"],
                                    a["L"], a["min_in"], a["head"], a["sums"], a["model"], a["box"], a["layer"], a["overlap"], a["ws"],
                                    a["bytes"], _stream())
        torch.cuda.synchronize()
        assert all(bool((b == POISON).all()) for b in bufs.values()) and torch.equal(src, keep)
        return rc

    for over in (dict(F=-1), dict(F=(1 << 24) + 1), dict(n=-1), dict(n=65537), dict(K=0), dict(K=1025), dict(thr4=0), dict(thr4=1025),
                 dict(frame0=-1), dict(frame0=2 ** 31 - 3), dict(logit=NAN), dict(L=0), dict(L=9), dict(min_in=1), dict(min_in=65537),
                 dict(trajs=None), dict(head=None), dict(sums=None), dict(model=None), dict(box=None), dict(layer=None),
                 dict(overlap=None), dict(ws=None), dict(ws=_ptr(bufs["ws"], 8)),
                 # prev_layer inside this call's layer output: its first row, its last row, a row that straddles its end or its start
                 dict(prev=_ptr(bufs["layer"])), dict(prev=_ptr(bufs["layer"], n)), dict(prev=_ptr(bufs["layer"], 2 * n - 1)),
                 dict(layer=_ptr(bufs["lay2"], n - 1), prev=_ptr(bufs["lay2"]))):
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error().decode().startswith("motion_layers:"), over
    for short in (0, 1, nbytes - 1):
        assert call(bytes=short) == E_WORKSPACE
        assert lib.pips_last_error().decode().startswith("motion_layers:")
    assert call(F=1) == 0
    assert call(F=0, trajs=None, vis=None, prev=None, head=None, sums=None, model=None, box=None, layer=None, overlap=None, ws=None,
                bytes=0) == 0
    assert lib.pips_abi_version() == 3
    # a prev_layer that ends where layer begins, or begins where it ends, is a buffer of its own: accepted
    for skip in (0, 3 * n):
        rc = lib.pips_motion_layers(_ptr(src), _ptr(vis), _ptr(bufs["lay2"], skip), F, n, 0, 0.0, K, 8, 0, L, 8, _ptr(bufs["head"]),
                                    _ptr(bufs["sums"]), _ptr(bufs["model"]), _ptr(bufs["box"]), _ptr(bufs["lay2"], n),
                                    _ptr(bufs["overlap"]), _ptr(bufs["ws"]), nbytes, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.pips_last_error()
        assert bool((bufs["lay2"][:n] == POISON).all()) and bool((bufs["lay2"][3 * n:] == POISON).all())


def test_driver_with_shuffled_ids_equals_the_sorted_call():
    from pips_amd import drivers
    trajs, g = _scene(6, 90, 8, outliers=0.4), torch.Generator().manual_seed(8)
    vis = torch.randn(6, 90, generator=g) + 1.5
    kw = dict(frame0=11, thr=1.5, hypotheses=96, vis_thr=0.7, seed=99, layers=4, min_inliers=2)
    ref = drivers.motion_layers_torch(trajs[None], vis[None], **kw)                            # on the CPU
    got = drivers.motion_layers(trajs[None].to(DEV), vis[None].to(DEV), **kw)
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.float64 and got[5].dtype == torch.float64
    assert all(t.dtype == torch.int64 for t in got[1:5])
    assert _f64_bits(got[0].cpu()) == _f64_bits(ref[0]) and all(torch.equal(a.cpu(), b) for a, b in zip(got[1:], ref[1:]))
    assert int(ref[3].max()) >= 4 and int(ref[1][:, 0, 0].max()) < 90                          # objects are found; vis drops columns
    perm = torch.randperm(90, generator=g)
    mixed = drivers.motion_layers(trajs[None][:, :, perm].to(DEV), vis[None][:, :, perm].to(DEV), ids=perm, **kw)
    assert _f64_bits(mixed[0].cpu()) == _f64_bits(ref[0]) and torch.equal(mixed[1].cpu(), ref[1])
    assert torch.equal(mixed[2].cpu(), ref[2][:, perm]) and torch.equal(mixed[3].cpu(), ref[3])
    assert torch.equal(mixed[4].cpu(), ref[4][:, perm]) and torch.equal(mixed[5].cpu(), ref[5])


def _same_steps(pushes, **kw):
    """the ``(f0, trajs, vis, ids)`` pushes through MotionLayers(engine="library") on the device and engine="torch" on the CPU ->
    (pairs, the torch engine's labels (P,n) and object ids (P,L) of every push)"""
    from pips_amd import drivers
    lib_ml, ref_ml = drivers.MotionLayers(engine="library", **kw), drivers.MotionLayers(engine="torch", **kw)
    pairs, labels, object_ids = 0, [], []
    for f0, t, v, ids in pushes:
        got = lib_ml.step(f0, t.to(DEV), None if v is None else v.to(DEV), ids=ids)
        ref = ref_ml.step(f0, t.cpu(), None if v is None else v.cpu(), ids=ids)
        assert _f64_bits(got[0].cpu()) == _f64_bits(ref[0]) and lib_ml.T == ref_ml.T and lib_ml.next_id == ref_ml.next_id
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got[1:], ref[1:]))
        pairs += ref[0].shape[0]
        labels.append(ref[2]), object_ids.append(ref[3])
    return pairs, labels, object_ids


@pytest.mark.parametrize("n", [64, 200])
def test_layers_library_equals_torch_on_the_scene_with_meaning(n):
    """the camera, two blobs and wild columns of tests/test_motion_layers.py in pushes of 2 frames: both engines agree push by
    push, and what they agree on meets the scene's conditions"""
    trajs, group = _meaning_scene(n, SCENE_SEEDS[n])
    pushes = [(f0, trajs[None][:, f0:f0 + 2], None, None) for f0 in range(0, 6, 2)]
    pairs, labels, object_ids = _same_steps(pushes, thr=2.0, hypotheses=256, seed=0, layers=4, min_inliers=8)
    assert pairs == 5 and _scene_conditions(torch.cat(labels).tolist(), torch.cat(object_ids).tolist(), group.tolist())


def test_layers_library_equals_torch_on_a_real_cover_run(weights_tamed):
    """one CoverTracker run at 128 x 192 (T = 24 in chunks of 4, cells of 64 px, lost_after = 2), whose identities come and go: the
    parts it returns, with their ids, through both engines"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    ct = drivers.CoverTracker(m, drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan="library"), _user(71).to(DEV), iters=6,
                              slots=24, rounds="library")
    parts = [ct.push(video[:, i:i + 4]) for i in range(0, ET, 4)] + [ct.finish()]
    assert sum(p[1].shape[1] for p in parts) == ET and len({tuple(p[3].tolist()) for p in parts if p[1].shape[1]}) > 1
    pairs, _, _ = _same_steps(parts, thr=2.0, hypotheses=64, vis_thr=0.1, seed=1, layers=3, min_inliers=2)
    assert pairs == ET - 1
    pairs, _, _ = _same_steps([(f0, t, None, ids) for f0, t, _, ids in parts], hypotheses=256, layers=4, min_inliers=3)
    assert pairs == ET - 1
