"""GPU: the thin cover step in the library.  pips_cover_step_thin is held, bit for bit, to the torch form (drivers.cover_scan_thin) on
synthetic rows whose positions come from a few values, so that many queries share cells -- the lists, both runs, the seeds, the
five counts, gone / reason, the inputs left as they were, the output tails and the ints behind the workspace left untouched -- at the
sizes where its tiles and block scans can break, with its return codes; with per_cell = INT_MAX it is pips_cover_step; and
``scan="library"`` of a thinned CoverTracker / MultiStreamTracker on the real model equals ``scan="torch"`` in ids, reasons and bits
under both ``rounds`` values and both engines (128 x 192, a 16 x 24 map: live tracks that the model's visibilities retire) and on a
128 x 160 video on which no track is ever lost and the crowded ones are retired."""
import ctypes as C

import pytest
import torch

from test_cover_gpu import _assert_live
from test_stream_rounds_gpu import _bits, _model, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
INT_MAX = 2 ** 31 - 1
POISON = -77
GUARD = 64                                                                       # poisoned ints behind the workspace
E_ARG, E_WORKSPACE = -1, -2
ORDER = ["n", "m", "f1", "trajs", "vis", "tq", "xy", "lost", "crowd", "H", "W", "cell", "vis_logit", "lost_after", "max_queries",
         "per_cell", "crowd_after", "keep", "lost_out", "crowd_out", "seeds", "gone", "reason", "counts", "ws", "ws_bytes"]
INPUTS = ("trajs", "vis", "tq", "xy", "lost", "crowd")
VIS_LOGIT = float(torch.logit(torch.tensor(0.6, dtype=torch.float32)))


def _axis(size, cell):
    """the values one coordinate is drawn from: integers and halves, cell borders and the float just below one, size-1 and size,
    negatives, -0.0, NaN and +-inf -- the values inside the frame several times, so that most positions are"""
    below = float(torch.nextafter(torch.tensor(float(cell)), torch.tensor(0.0)))
    good = [0.0, -0.0, 0.5, 3.0, cell - 0.5, below, float(cell), cell + 0.5, 2.0 * cell, 2.0 * cell + 1.0, size - 1.0, size - 1.5,
            float((size // cell) * cell if size % cell else size - cell), size / 2.0, size / 2.0 + 0.5, 3.0 * cell + 2.0]
    bad = [float(size), size - 0.5, -1.0, -1e-3, float("nan"), float("inf"), -float("inf")]
    return torch.tensor([min(v, size - 1.0) for v in good] * 4 + bad)


def _rows(n, m, H, W, cell, seed):
    """n queries and the m rows of frames [f1 - m, f1): t_q on both sides of every returned frame, both runs carried in,
    visibilities around the threshold with NaNs among them, positions from _axis"""
    g = torch.Generator().manual_seed(seed)
    f1 = 37 if m > 0 else 0
    xs, ys = _axis(W, cell), _axis(H, cell)

    def draw(*shape):
        return torch.stack([xs[torch.randint(0, xs.numel(), shape, generator=g)], ys[torch.randint(0, ys.numel(), shape, generator=g)]], dim=-1)

    tq = torch.randint(f1 - m - 3, f1 + 2, (n,), generator=g).clamp(min=0).to(I32)
    vis = torch.randn(m, n, generator=g) * 0.5 + VIS_LOGIT + 0.5
    vis[torch.rand(m, n, generator=g) < 0.05] = float("nan")
    return dict(n=n, m=m, f1=f1, trajs=draw(m, n), vis=vis, tq=tq, xy=draw(n), lost=torch.randint(0, 3, (n,), generator=g).to(I32),
                crowd=torch.randint(0, 3, (n,), generator=g).to(I32), H=H, W=W, cell=cell)


def _call(lib, a):
    from pips_amd import _lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.pips_cover_step_thin(*[(_lib.ptr(a[k]) if torch.is_tensor(a[k]) or a[k] is None else a[k]) for k in ORDER], stream)


def _buffers(n, cells):
    ints = lambda k: torch.full((max(k, 1),), POISON, dtype=I32, device=DEV)
    return dict(keep=ints(n), lost_out=ints(n), crowd_out=ints(n), gone=ints(n), reason=ints(n), counts=ints(5),
                seeds=torch.full((cells, 3), POISON, dtype=I32, device=DEV).view(torch.float32))


def _check_one(lib, host, dev, policy):
    """one pips_cover_step_thin call on poisoned outputs against drivers.cover_scan_thin on the same device tensors -> the counts"""
    from pips_amd import drivers
    n, m, H, W, cell = (host[k] for k in ("n", "m", "H", "W", "cell"))
    lost_after, max_queries, per_cell, crowd_after = policy
    gh, gw = -(-H // cell), -(-W // cell)
    ref = drivers.cover_scan_thin(dev["trajs"], dev["vis"], dev["f1"], dev["tq"], dev["xy"], dev["lost"], dev["crowd"], H, W, cell,
                                  VIS_LOGIT, lost_after, max_queries, per_cell, crowd_after)
    out = _buffers(n, gh * gw)
    nbytes = lib.pips_cover_thin_workspace_bytes(n, m, gh, gw)
    assert nbytes == 4 * (3 * n + gh * gw + m * n)
    ws = torch.full((nbytes // 4 + GUARD,), POISON, dtype=I32, device=DEV)
    rc = _call(lib, dict(dev, **out, vis_logit=VIS_LOGIT, lost_after=lost_after, max_queries=max_queries, per_cell=per_cell,
                         crowd_after=crowd_after, ws=ws, ws_bytes=nbytes))
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    keep, run, crun, seeds, gone, reason, counts = ref
    what = (n, m, H, W, cell) + tuple(policy)
    assert out["counts"].tolist() == counts, what
    n_keep, n_seed = counts[:2]
    for name, want in (("keep", keep), ("lost_out", run), ("crowd_out", crun), ("gone", gone), ("reason", reason)):
        k = want.numel()
        assert k == (n_keep if name in ("keep", "lost_out", "crowd_out") else n - n_keep), (name, what)
        assert torch.equal(out[name][:k], want) and bool((out[name][k:] == POISON).all()), (name, what)
    got = out["seeds"].view(I32)
    assert torch.equal(got[:n_seed], seeds.contiguous().view(I32)) and bool((got[n_seed:] == POISON).all()), what
    assert bool((ws[nbytes // 4:] == POISON).all()), what                        # nothing behind the workspace
    for k in INPUTS:                                                              # every input as it was, both runs included
        assert torch.equal(_bits(dev[k]), _bits(host[k])), (k, what)
    assert bool((keep[1:] > keep[:-1]).all()) and bool((gone[1:] > gone[:-1]).all()) and sum(counts) - counts[1] == n
    return counts


@pytest.mark.parametrize("H,W,cell", [(45, 70, 16), (40, 60, 8), (264, 328, 8)])
def test_cover_step_thin_is_the_torch_scan(H, W, cell):
    """grids of 3 x 5, of 40 and of 1 353 cells, each at n = 0 .. 1000 around the tile and wave sizes (at 257, 600 and 1000 elders
    stand in earlier tiles than their youngsters) and at m = 0 (the first step), 1 and 5; one and two tracks to a cell and no cap
    per cell, retirement after one and after three surplus frames; a cap that cuts the seed list"""
    from pips_amd import _lib
    lib = _lib.load()
    seen = dict(outside=0, lost=0, crowded=0, seeds=0, cut=0, run=0)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 600, 1000):
        for m in (0, 1, 5):
            host = _rows(n, m, H, W, cell, seed=1000 * m + n)
            dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
            for per_cell in (1, 2, INT_MAX):
                for crowd_after in (1, 3):
                    c = _check_one(lib, host, dev, (2, INT_MAX, per_cell, crowd_after))
                    assert per_cell < INT_MAX or c[4] == 0
                    for k, v in zip(("outside", "lost", "crowded", "seeds"), (c[2], c[3], c[4], c[1])):
                        seen[k] += v
                    seen["run"] += c[4] > 0 and crowd_after == 3
            c2 = _check_one(lib, host, dev, (2, c[0] + c[1] // 2, INT_MAX, 3))
            assert c2[0] == c[0] and c2[1] == c[1] // 2
            seen["cut"] += 0 < c2[1] < c[1]
            c3 = _check_one(lib, host, dev, (2, max(c[0] - 3, 0), 1, 1))          # the cap counts the kept of THIS step
            assert c3[1] == min(max(c[0] - 3 - c3[0], 0), c3[1]) and (c3[4] >= 3 or c3[1] == 0)
    assert all(v > 0 for v in seen.values()), seen


def test_elders_in_earlier_tiles_count():
    """n = 600 on a 3 x 5 grid with everybody started, visible and inside: per cell the first per_cell columns are kept whichever
    tile they stand in, and everybody behind them is retired as crowded after one frame"""
    from pips_amd import ops
    n, H, W, cell = 600, 45, 70, 16
    g = torch.Generator().manual_seed(9)
    pos = torch.stack([torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)], dim=1).float()
    pos[:300] = torch.tensor([5.0, 5.0])                                          # cell (0, 0) alone holds the first 300 columns
    d = dict(trajs=pos.view(1, n, 2), vis=torch.full((1, n), 5.0), tq=torch.zeros(n, dtype=I32), xy=pos.clone(),
             lost=torch.zeros(n, dtype=I32), crowd=torch.zeros(n, dtype=I32))
    d = {k: v.to(DEV) for k, v in d.items()}
    for per_cell in (1, 2, 299, 300):
        keep, lost_out, crowd_out, seeds, gone, reason, counts = ops.cover_step_thin(d["trajs"], d["vis"], 7, d["tq"], d["xy"], d["lost"],
                                                                                     d["crowd"], H, W, cell, 0.0, 2, INT_MAX, per_cell, 1)
        n_keep, n_seed, n_out, n_lost, n_crowded = counts.tolist()
        cid = (pos[:, 1] // cell).long() * 5 + (pos[:, 0] // cell).long()
        rank = torch.tensor([int((cid[:j] == cid[j]).sum()) for j in range(n)])
        assert keep[:n_keep].tolist() == torch.nonzero(rank < per_cell).squeeze(1).tolist()
        assert gone[:n - n_keep].tolist() == torch.nonzero(rank >= per_cell).squeeze(1).tolist()
        assert n_crowded == n - n_keep and bool((reason[:n_crowded] == 3).all()) and n_out == n_lost == 0
        assert bool((crowd_out[:n_keep] == 0).all())


def test_without_a_cap_per_cell_it_is_pips_cover_step():
    """per_cell = INT_MAX against ops.cover_step on the same inputs: the first four counts, keep, lost_out and the seeds as bits"""
    from pips_amd import ops
    for (H, W, cell) in ((45, 70, 16), (264, 328, 8)):
        for n in (0, 1, 257, 1000):
            for m in (0, 1, 5):
                host = _rows(n, m, H, W, cell, seed=7 * n + m)
                d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
                for cap in (INT_MAX, n // 2 + 5):
                    old = ops.cover_step(d["trajs"], d["vis"], d["f1"], d["tq"], d["xy"], d["lost"], H, W, cell, VIS_LOGIT, 2, cap)
                    new = ops.cover_step_thin(d["trajs"], d["vis"], d["f1"], d["tq"], d["xy"], d["lost"], d["crowd"], H, W, cell, VIS_LOGIT,
                                              2, cap, INT_MAX, 1)
                    c_old, c_new = old[3].tolist(), new[6].tolist()
                    assert c_new == c_old + [0], (H, W, cell, n, m, cap)
                    assert torch.equal(new[0][:c_old[0]], old[0][:c_old[0]]) and torch.equal(new[1][:c_old[0]], old[1][:c_old[0]])
                    assert torch.equal(_bits(new[3][:c_old[1]]), _bits(old[2][:c_old[1]]))
                    assert bool((new[2][:c_old[0]] == 0).all()) and 3 not in new[5][:n - c_old[0]].tolist()


def test_cover_step_thin_rejects_bad_arguments_and_writes_nothing():
    """every PIPS_E_ARG case and PIPS_E_WORKSPACE answer ahead of any launch: poisoned outputs and workspace stay untouched"""
    from pips_amd import _lib
    lib = _lib.load()
    n, m, H, W, cell = 12, 3, 40, 60, 8
    host = _rows(n, m, H, W, cell, seed=3)
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
    out = _buffers(n, 40)
    nbytes = lib.pips_cover_thin_workspace_bytes(n, m, 5, 8)
    ws = torch.full((nbytes // 4,), POISON, dtype=I32, device=DEV)
    good = dict(dev, **out, vis_logit=VIS_LOGIT, lost_after=2, max_queries=INT_MAX, per_cell=1, crowd_after=2, ws=ws, ws_bytes=nbytes)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((t.view(I32) == POISON).all()) for t in list(out.values()) + [ws])
        for k in INPUTS:
            assert torch.equal(_bits(dev[k]), _bits(host[k])), k

    bad = [dict(n=-1), dict(m=-1), dict(cell=7), dict(cell=0), dict(H=0), dict(W=0), dict(lost_after=0), dict(max_queries=-1),
           dict(m=0), dict(m=0, f1=5), dict(f1=2), dict(H=1 << 20, W=1 << 20), dict(per_cell=0), dict(per_cell=-1),
           dict(crowd_after=0), dict(crowd_after=-5)]
    bad += [{k: None} for k in INPUTS + ("keep", "lost_out", "crowd_out", "seeds", "gone", "reason", "counts", "ws")]
    for over in bad:
        assert _call(lib, dict(good, **over)) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    old = lib.pips_cover_workspace_bytes(n, 5, 8)                                 # (the old step's size is too short for this one)
    for short in (nbytes - 1, old, 0):
        assert _call(lib, dict(good, ws_bytes=short)) == E_WORKSPACE
        untouched()
    # arrays that are not read may be NULL: the rows of a first step, everything per query at n = 0
    assert _call(lib, dict(good, m=0, f1=0, trajs=None, vis=None)) == 0
    torch.cuda.synchronize()
    assert out["counts"].tolist() == [n, out["counts"][1].item(), 0, 0, 0] and out["keep"].tolist() == list(range(n))
    assert out["crowd_out"].tolist() == [0] * n and bool((out["gone"] == POISON).all())      # every query pending, every run 0
    for t in out.values():
        t.view(I32).fill_(POISON)
    none = {k: None for k in INPUTS + ("keep", "lost_out", "crowd_out", "gone", "reason")}
    assert _call(lib, dict(good, n=0, **none)) == 0
    torch.cuda.synchronize()
    assert out["counts"].tolist() == [0, 40, 0, 0, 0] and bool((out["keep"] == POISON).all())


# ------------------------------------------------------------------ end to end on the device
EH, EW, ET = 128, 192, 24              # a 16 x 24 map: the hop takes no map below 16 x 16 (tests/test_small_maps.py), tracks are live
ECELL = 64                             # 2 x 3 cells


def _user(seed):
    """five queries of the caller: one on frame 0, one on frame 9, one that starts outside the frame, and two on frame 0 a pixel
    apart in the middle of cell (0, 1), the younger of which is surplus from its first frame on"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(5, 2, generator=g) * torch.tensor([EW - 17.0, EH - 17.0]) + 8.0
    xy[2, 0] = EW + 20.0
    xy[3], xy[4] = torch.tensor([95.0, 31.0]), torch.tensor([96.0, 32.0])
    return torch.cat([torch.tensor([0.0, 9.0, 2.0, 0.0, 0.0]).view(5, 1), xy], dim=1).unsqueeze(0)


def _cover(scan, crowd_after):
    from pips_amd import drivers
    return drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan=scan, per_cell=1, crowd_after=crowd_after)


def _same_parts(a, b):
    assert len(a) == len(b)
    for (f0, t, v, ids), (g0, gt, gv, gids) in zip(a, b):
        assert f0 == g0 and torch.equal(ids, gids) and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(v), _bits(gv))


@pytest.mark.parametrize("kw", [dict(rounds="torch", engine="torch"), dict(rounds="torch", engine="native"), dict(rounds="library")],
                         ids=["torch", "native", "library"])
def test_library_scan_equals_torch_scan_end_to_end(weights_tamed, kw):
    """128 x 192 frames, T = 24 in chunks of 4, cells of 64 px (2 x 3), one track to a cell after 1 and after 2 surplus frames: a
    thinned CoverTracker under scan="library" hands out, push by push, the ids and the bits of the one under scan="torch", with
    the same births, retirements (frame and reason) and hop lists, on tracks with finite positions and visibilities: the reasons
    of the thin step come from what the model returns, and the counts seen are printed.  (Crowding on tracks that are never lost:
    test_crowded_tracks_end_to_end.)"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    for crowd_after in (1, 2):
        runs = {}
        for scan in drivers.COVER_SCANS:
            ct = drivers.CoverTracker(m, _cover(scan, crowd_after), _user(71).to(DEV), iters=6, slots=24, record_hops=True, **kw)
            parts = [ct.push(video[:, i:i + 4]) for i in range(0, ET, 4)] + [ct.finish()]
            runs[scan] = (parts, ct)
        (pa, a), (pb, b) = runs["torch"], runs["library"]
        _same_parts(pa, pb)
        assert a.born == b.born and a.retired == b.retired and a.hops == b.hops
        reasons = [r for _, r in a.retired.values()]
        print(f"thin cover e2e {kw} crowd_after {crowd_after}: {len(a.born)} identities, retired "
              f"{ {r: reasons.count(r) for r in ('outside', 'lost', 'crowded')} }")
        assert a.retired[2][1] == "outside"
        assert sum(p[1].shape[1] for p in pa) == ET and pa[-1][3].numel() >= 6      # the frame is still covered at the end
        _assert_live(pa, a.book, [0, 1, 3, 4], f"thin cover e2e {kw} crowd_after {crowd_after}")


def test_crowded_tracks_end_to_end(weights_tamed):
    """128 x 160 frames (a 16 x 20 map, on which the tamed model moves a track by less than a pixel per frame), T = 16 in chunks of
    4, cells of 32 px, one track to a cell after 2 frames; the caller's queries 1 and 3 start a pixel beside 0 and 2, in the middle
    of their cells: both are surplus from frame 0 on and retired as crowded on the second frame that is returned, their elders
    stay, under both scans with the same ids, bits and hop lists"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(16, 128, 160, seed=76)
    user = torch.tensor([[[0.0, 47.0, 15.0], [0.0, 48.0, 16.0], [0.0, 111.0, 79.0], [0.0, 112.0, 80.0], [0.0, 16.0, 112.0]]])
    runs = {}
    for scan in drivers.COVER_SCANS:
        cover = drivers.Cover(cell=32, vis_thr=0.01, lost_after=None, scan=scan, per_cell=1, crowd_after=2)
        ct = drivers.CoverTracker(m, cover, user.to(DEV), iters=6, slots=24, record_hops=True, rounds="library")
        parts = [ct.push(video[:, i:i + 4]) for i in range(0, 16, 4)] + [ct.finish()]
        runs[scan] = (parts, ct)
    (pa, a), (pb, b) = runs["torch"], runs["library"]
    _same_parts(pa, pb)
    assert a.born == b.born and a.retired == b.retired and a.hops == b.hops
    print(f"thin cover crowded e2e: {len(a.born)} identities, retired {a.retired}")
    first = next(p for p in pa if p[1].shape[1] > 0)
    assert first[0] == 0 and first[1].shape[1] >= 2
    assert a.retired[1] == (first[1].shape[1] - 1, "crowded") and a.retired[3] == a.retired[1] and 0 not in a.retired and 2 not in a.retired
    assert pa[-1][3].tolist()[:3] == [0, 2, 4] and pa[-1][3].numel() >= 20      # the elders stay; every cell is held at the end


def test_multi_stream_library_scan_equals_torch_scan(weights_tamed):
    """two thinned streams of 24 / 13 frames under MultiStreamTracker(cover=), both ``rounds`` values: scan="library" equals
    scan="torch" part by part, ids and reasons included"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    videos = [_video(ET, EH, EW, seed=72), _video(13, EH, EW, seed=73)]
    for rounds in drivers.ROUNDS:
        runs = {}
        for scan in drivers.COVER_SCANS:
            mt = drivers.MultiStreamTracker(m, [_user(74).to(DEV), _user(75)[:, 3:].to(DEV)], iters=6, slots=24, record_hops=True,
                                            rounds=rounds, cover=_cover(scan, 1))
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
        print(f"thin cover streams {rounds}: retired {[sorted(r for _, r in a.books[v].retired.values()) for v in range(2)]}")
        for v, user in enumerate(([0, 1, 3, 4], [0, 1])):
            _assert_live(pa[v], a.books[v], user, f"thin cover streams {rounds}, stream {v}")
