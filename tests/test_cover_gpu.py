"""GPU: the cover step in the library.  pips_cover_step is held, bit for bit, to the torch scan (drivers.cover_scan) on synthetic rows
-- the lists, the counts, the runs, the inputs left as they were and the output tails behind the counts left untouched -- at the
sizes where its two block scans can break, with its return codes; ``scan="library"`` of drivers.CoverTracker / MultiStreamTracker
on the real model equals ``scan="torch"`` in ids and bits under both ``rounds`` values and both engines."""
import ctypes as C

import pytest
import torch

from test_stream_rounds_gpu import _bits, _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
INT_MAX = 2 ** 31 - 1
POISON = -77
E_ARG, E_WORKSPACE = -1, -2
ORDER = ["n", "m", "f1", "trajs", "vis", "tq", "xy", "lost", "H", "W", "cell", "vis_logit", "lost_after", "max_queries", "keep",
         "lost_out", "seeds", "counts", "ws", "ws_bytes"]
VIS_LOGIT = float(torch.logit(torch.tensor(0.6, dtype=torch.float32)))


def _rows(n, m, H, W, cell, seed):
    """n queries and the m rows of frames [f1 - m, f1): t_q on both sides of every returned frame (pending ones, ones that start
    inside the chunk, old ones), runs carried in, visibilities around the threshold with NaNs among them, positions inside and
    around the frame -- and, in the leading columns of the last row and of xy, points exactly on cell borders, on W-1 / H-1, on
    W / H, just below a border, negative, -0.0, NaN and +-inf"""
    g = torch.Generator().manual_seed(seed)
    f1 = 37 if m > 0 else 0
    tq = torch.randint(f1 - m - 3, f1 + 3, (n,), generator=g).clamp(min=0).to(I32)
    lost = torch.randint(0, 3, (n,), generator=g).to(I32)
    span = torch.tensor([W + 16.0, H + 16.0])
    xy = torch.rand(n, 2, generator=g) * span - 8.0
    trajs = torch.rand(m, n, 2, generator=g) * span - 8.0
    vis = torch.randn(m, n, generator=g) + VIS_LOGIT
    vis[torch.rand(m, n, generator=g) < 0.05] = float("nan")
    below = float(torch.nextafter(torch.tensor(float(cell)), torch.tensor(0.0)))
    nan, inf = float("nan"), float("inf")
    special = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [float(W), H - 1.0], [W - 1.0, float(H)], [float(W), float(H)], [-0.0, 5.0],
                            [-1e-3, 5.0], [float(cell), float(cell)], [2.0 * cell, below], [below, 2.0 * cell], [nan, 5.0], [5.0, nan],
                            [inf, 5.0], [5.0, -inf], [W - 1.0, 0.0], [W - 0.5, 3.0], [3.0, H - 0.5], [3.0 * cell, 1.0]])
    k = min(n, special.shape[0])
    xy[:k] = special[:k]
    if m > 0:
        trajs[m - 1, n - k:] = special[:k]                       # (the trailing columns: xy's specials stand in the leading ones)
        if n > 40:
            tq[n - k:] = 0                                       # started, so that the special positions are judged
            tq[:k] = f1 + 1                                      # pending on the special query positions
    return dict(n=n, m=m, f1=f1, trajs=trajs, vis=vis, tq=tq, xy=xy, lost=lost, H=H, W=W, cell=cell)


def _call(lib, a):
    from pips_amd import _lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.pips_cover_step(*[(_lib.ptr(a[k]) if torch.is_tensor(a[k]) or a[k] is None else a[k]) for k in ORDER], stream)


def _buffers(n, cells):
    return dict(keep=torch.full((max(n, 1),), POISON, dtype=I32, device=DEV), lost_out=torch.full((max(n, 1),), POISON, dtype=I32, device=DEV),
                seeds=torch.full((cells, 3), POISON, dtype=I32, device=DEV).view(torch.float32),
                counts=torch.full((4,), POISON, dtype=I32, device=DEV))


def _check_one(lib, host, lost_after, max_queries):
    """one pips_cover_step call on poisoned outputs against drivers.cover_scan on the same device tensors -> the counts"""
    from pips_amd import drivers
    n, m, H, W, cell = (host[k] for k in ("n", "m", "H", "W", "cell"))
    gh, gw = -(-H // cell), -(-W // cell)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
    ref = drivers.cover_scan(dev["trajs"], dev["vis"], dev["f1"], dev["tq"], dev["xy"], dev["lost"], H, W, cell, VIS_LOGIT, lost_after,
                             max_queries)
    out = _buffers(n, gh * gw)
    nbytes = lib.pips_cover_workspace_bytes(n, gh, gw)
    assert nbytes == 4 * (2 * n + gh * gw)
    ws = torch.full((nbytes // 4,), POISON, dtype=I32, device=DEV)
    rc = _call(lib, dict(dev, **out, vis_logit=VIS_LOGIT, lost_after=lost_after, max_queries=max_queries, ws=ws, ws_bytes=nbytes))
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    keep, run, seeds, counts = ref
    what = (n, m, H, W, cell, lost_after, max_queries)
    assert out["counts"].tolist() == counts, what
    n_keep, n_seed = counts[:2]
    assert torch.equal(out["keep"][:n_keep], keep) and bool((out["keep"][n_keep:] == POISON).all()), what
    assert torch.equal(out["lost_out"][:n_keep], run) and bool((out["lost_out"][n_keep:] == POISON).all()), what
    got = out["seeds"].view(I32)
    assert torch.equal(got[:n_seed], seeds.contiguous().view(I32)) and bool((got[n_seed:] == POISON).all()), what
    for k in ("trajs", "vis", "tq", "xy", "lost"):                                # every input as it was, `lost` included
        assert torch.equal(_bits(dev[k]), _bits(host[k])), (k, what)
    # the lists ascend and the kept, the outside and the lost are all the queries
    assert bool((keep[1:] > keep[:-1]).all()) and counts[0] + counts[2] + counts[3] == n
    return counts


@pytest.mark.parametrize("H,W,cell", [(40, 60, 8), (264, 328, 8), (45, 70, 16)])
def test_cover_step_is_the_torch_scan(H, W, cell):
    """grids of 40 cells, of 1 353 cells (five full chunks of the 256-thread block and a ragged sixth) and one whose frame is no
    multiple of the cell, each at n = 0 .. 1000 around the chunk and wave sizes and at m = 0 (the first step), 1 and 5; the cap
    absent, cutting the seed list in its middle, at zero seeds, below the kept queries and at 0"""
    from pips_amd import _lib
    lib = _lib.load()
    seen = dict(outside=0, lost=0, seeds=0, cut=0)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        for m in (0, 1, 5):
            host = _rows(n, m, H, W, cell, seed=1000 * m + n)
            n_keep, n_empty, n_out, n_lost = _check_one(lib, host, 2, INT_MAX)
            seen["outside"] += n_out
            seen["lost"] += n_lost
            seen["seeds"] += n_empty
            for cap in (n_keep + n_empty // 2, n_keep, n_keep // 2, 0):
                c = _check_one(lib, host, 2, cap)
                assert c[0] == n_keep and c[1] == min(n_empty, max(cap - n_keep, 0))
                seen["cut"] += 0 < c[1] < n_empty
            if n == 257:
                c = _check_one(lib, host, INT_MAX, INT_MAX)                       # never lost
                assert c[3] == 0 and c[2] == n_out
                c = _check_one(lib, host, 1, INT_MAX)
                assert c[3] >= n_lost
    assert seen["outside"] > 0 and seen["lost"] > 0 and seen["seeds"] > 0 and seen["cut"] > 0, seen


def test_the_named_positions_are_judged_as_the_rule_says():
    """the special columns of _rows at n = 64, m = 1 on the 45 x 70 frame with cells of 16 (gh = 3, gw = 5), read off the flags the
    kept list implies: W-1 / H-1 and -0.0 are inside, W / H, negatives, NaN and +-inf are outside; a position just below a
    border belongs to the cell before it"""
    from pips_amd import drivers, ops
    host = _rows(64, 1, 45, 70, 16, seed=5)
    host["lost"].zero_()
    host["vis"].fill_(5.0)                                                       # nobody is lost
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
    keep, lost_out, seeds, counts = ops.cover_step(d["trajs"], d["vis"], d["f1"], d["tq"], d["xy"], d["lost"], 45, 70, 16, 0.0, 2, INT_MAX)
    n_keep, n_seed, n_out, n_lost = counts.tolist()
    kept = set(keep[:n_keep].tolist())
    base = 64 - 18                                                                # where the special positions stand in the last row
    outside = {2, 3, 4, 6, 10, 11, 12, 13, 15, 16}                                # W, H, negative, NaN, inf, W-0.5, H-0.5
    for s in range(18):
        assert ((base + s) in kept) == (s not in outside), s
    assert n_lost == 0 and bool((lost_out[:n_keep] == 0).all())
    # cells: the seeds are the centres of the empty cells, clamped to the frame (x of the last column: min(72, 69) = 69)
    got = seeds[:n_seed].cpu()
    ref = drivers.cover_scan(d["trajs"], d["vis"], d["f1"], d["tq"], d["xy"], d["lost"], 45, 70, 16, 0.0, 2, INT_MAX)[2].cpu()
    assert torch.equal(got, ref) and bool((got[:, 0] == 37.0).all()) and bool((got[:, 1] <= 69.0).all()) and bool((got[:, 2] <= 44.0).all())
    assert set(got[:, 1].tolist()) <= {8.0, 24.0, 40.0, 56.0, 69.0} and set(got[:, 2].tolist()) <= {8.0, 24.0, 40.0}


def test_cover_step_rejects_bad_arguments_and_writes_nothing():
    """every PIPS_E_ARG case and PIPS_E_WORKSPACE answer ahead of any launch: poisoned outputs and workspace stay untouched"""
    from pips_amd import _lib
    lib = _lib.load()
    n, m, H, W, cell = 12, 3, 40, 60, 8
    host = _rows(n, m, H, W, cell, seed=3)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
    out = _buffers(n, 40)
    nbytes = lib.pips_cover_workspace_bytes(n, 5, 8)
    ws = torch.full((nbytes // 4,), POISON, dtype=I32, device=DEV)
    good = dict(dev, **out, vis_logit=VIS_LOGIT, lost_after=2, max_queries=INT_MAX, ws=ws, ws_bytes=nbytes)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t.view(I32) == POISON).all()) for t in list(out.values()) + [ws])
        for k in ("trajs", "vis", "tq", "xy", "lost"):
            assert torch.equal(_bits(dev[k]), _bits(host[k])), k

    bad = [dict(n=-1), dict(m=-1), dict(cell=7), dict(cell=0), dict(H=0), dict(W=0), dict(lost_after=0), dict(max_queries=-1),
           dict(m=0), dict(m=0, f1=5), dict(f1=2), dict(H=1 << 20, W=1 << 20)]
    bad += [{k: None} for k in ("trajs", "vis", "tq", "xy", "lost", "keep", "lost_out", "seeds", "counts", "ws")]
    for over in bad:
        assert _call(lib, dict(good, **over)) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    for short in (nbytes - 1, 0):
        assert _call(lib, dict(good, ws_bytes=short)) == E_WORKSPACE
        untouched()
    # arrays that are not read may be NULL: the rows of a first step, everything per query at n = 0
    assert _call(lib, dict(good, m=0, f1=0, trajs=None, vis=None)) == 0
    torch.cuda.synchronize()
    assert out["counts"].tolist()[0] == n and out["keep"].tolist() == list(range(n))      # every query pending
    for t in out.values():
        t.view(I32).fill_(POISON)
    assert _call(lib, dict(good, n=0, tq=None, xy=None, lost=None, keep=None, lost_out=None, trajs=None, vis=None)) == 0
    torch.cuda.synchronize()
    assert out["counts"].tolist() == [0, 40, 0, 0] and bool((out["keep"] == POISON).all())


# ------------------------------------------------------------------ end to end on the device
EH, EW, ET = 128, 192, 24              # a 16 x 24 map: the hop takes no map below 16 x 16 (tests/test_small_maps.py), tracks are live
ECELL = 64                             # 2 x 3 cells


def _user(seed):
    """three queries of the caller: one on frame 0, one on frame 9, one that starts outside the frame (retired when it starts)"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(3, 2, generator=g) * torch.tensor([EW - 17.0, EH - 17.0]) + 8.0
    xy[2, 0] = EW + 20.0
    return torch.cat([torch.tensor([0.0, 9.0, 2.0]).view(3, 1), xy], dim=1).unsqueeze(0)


def _cover(scan):
    from pips_amd import drivers
    return drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan=scan)


def _same_parts(a, b):
    assert len(a) == len(b)
    for (f0, t, v, ids), (g0, gt, gv, gids) in zip(a, b):
        assert f0 == g0 and torch.equal(ids, gids) and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(v), _bits(gv))


def _assert_live(parts, book, user, what):
    """the run is on live tracks: at least one of the caller's in-frame queries ``user`` (identities) has finite positions and
    visibilities on every frame from its query frame to its end -- its retirement or the last frame of the video -- and that is more
    than the query frame alone.  The retirement reasons seen are printed."""
    from pips_amd import drivers
    trajs, vis, born, retired = drivers._by_identity(parts, book)
    live = []
    for q in user:
        first, last = int(born[q]), int(retired[q]) if int(retired[q]) >= 0 else trajs.shape[1] - 1
        if last > first and bool(torch.isfinite(trajs[0, first:last + 1, q]).all()) and bool(torch.isfinite(vis[0, first:last + 1, q]).all()):
            live.append((q, first, last))
    reasons = [r for _, r in book.retired.values()]
    print(f"{what}: live caller queries (id, first frame, last frame) {live}; {len(book.born)} identities, retired "
          f"{ {r: reasons.count(r) for r in sorted(set(reasons))} }")
    assert live, what


@pytest.mark.parametrize("kw", [dict(rounds="torch", engine="torch"), dict(rounds="torch", engine="native"), dict(rounds="library")],
                         ids=["torch", "native", "library"])
def test_library_scan_equals_torch_scan_end_to_end(weights_tamed, kw):
    """128 x 192 frames, T = 24 in chunks of 4, cells of 64 px (2 x 3), lost_after = 2: a CoverTracker under scan="library" hands
    out, push by push, the ids and the bits of the one under scan="torch", with the same births, retirements and hop lists, on
    tracks with finite positions and visibilities"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    runs = {}
    for scan in drivers.COVER_SCANS:
        ct = drivers.CoverTracker(m, _cover(scan), _user(71).to(DEV), iters=6, slots=24, record_hops=True, **kw)
        parts = [ct.push(video[:, i:i + 4]) for i in range(0, ET, 4)] + [ct.finish()]
        runs[scan] = (parts, ct)
    (pa, a), (pb, b) = runs["torch"], runs["library"]
    _same_parts(pa, pb)
    assert a.born == b.born and a.retired == b.retired and a.hops == b.hops
    print(f"cover e2e {kw}: {len(a.born)} identities, retired {sorted(r for _, r in a.retired.values())}")
    assert a.born[3:].count(0) in (4, 5) and a.retired[2][1] == "outside"      # the first step's seeds; the query outside the frame
    assert sum(p[1].shape[1] for p in pa) == ET and pa[-1][3].numel() >= 6      # the frame is still covered at the end
    _assert_live(pa, a.book, [0, 1], f"cover e2e {kw}")


def test_multi_stream_library_scan_equals_torch_scan(weights_tamed):
    """two streams of 24 / 13 frames under MultiStreamTracker(cover=), both ``rounds`` values: scan="library" equals scan="torch" part
    by part, ids included"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    videos = [_video(ET, EH, EW, seed=72), _video(13, EH, EW, seed=73)]
    for rounds in drivers.ROUNDS:
        runs = {}
        for scan in drivers.COVER_SCANS:
            mt = drivers.MultiStreamTracker(m, [_user(74).to(DEV), _user(75)[:, :1].to(DEV)], iters=6, slots=24, record_hops=True,
                                            rounds=rounds, cover=_cover(scan))
            parts = [[], []]
            for i in range(0, ET, 4):
                if i == 16:
                    parts[1].append(mt.finish(1))
                for v, p in enumerate(mt.push([videos[0][:, i:i + 4], videos[1][:, i:i + 4] if i < 13 else None])):
                    parts[v].append(p)
            parts[0].append(mt.finish(0))
            runs[scan] = (parts, mt)
        (pa, a), (pb, b) = runs["torch"], runs["library"]
        for v in range(2):
            _same_parts(pa[v], pb[v])
            assert a.books[v].born == b.books[v].born and a.books[v].retired == b.books[v].retired
            assert a.cover_hops(v) == b.cover_hops(v)
        assert a.books[0].retired[2][1] == "outside" and len(a.books[1].born) >= 6
        for v, user in enumerate(([0, 1], [0])):
            _assert_live(pa[v], a.books[v], user, f"cover streams {rounds}, stream {v}")
