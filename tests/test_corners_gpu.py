"""GPU: seeding on corners in the library.  pips_corner_table is held, bit for bit, to drivers.corner_table_torch run on the CPU --
uint8 and float32 frames, noise, a checkerboard full of ties and one planted corner, at frame and cell sizes with ragged last
cells, a single candidate, no candidate and cells larger than a tile -- with guard words around the table; pips_cover_place to
drivers.cover_place_torch; both with their return codes.  ``scan="library"`` of a CoverTracker / MultiStreamTracker that seeds on
corners equals ``scan="torch"`` on the real model."""
import ctypes as C

import pytest
import torch

from test_stream_rounds_gpu import _bits, _model, _video
from test_cover_gpu import ECELL, EH, ET, EW, _assert_live, _same_parts, _user

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
POISON = -77
GUARD = 64
E_ARG = -1
SIZES = [(44, 70, 8), (44, 70, 16), (44, 70, 40), (9, 9, 8), (8, 30, 8), (264, 328, 32)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frames(h, w, seed):
    """two sets of F = 3 uint8 frames: noise; and a checkerboard of 4 px squares, a bright quadrant on a dark field (one corner,
    wherever the frame has room for it) and noise laid over the checkerboard"""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randint(0, 256, (3, 3, h, w), generator=g, dtype=torch.uint8)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    board = (((y // 4 + x // 4) % 2) * 255).to(torch.uint8).expand(3, h, w)
    corner = torch.full((3, h, w), 20, dtype=torch.uint8)
    corner[:, (h * 5) // 9:, (w * 4) // 7:] = 220
    mixed = (board // 2 + torch.randint(0, 128, (3, h, w), generator=g, dtype=torch.uint8))
    return noise, torch.stack([board, corner, mixed])


def _as_float(u8, seed):
    """the same frames as float32 with fractions, some entries below 0 and above 255"""
    g = torch.Generator().manual_seed(seed)
    f = u8.float() + torch.rand(u8.shape, generator=g) * 0.98 - 0.49
    f[..., ::5, ::3] = -37.5
    f[..., 1::7, 2::4] = 300.25
    return f


def _table_guarded(lib, frames, cell):
    """pips_corner_table into a poisoned buffer with guard words on both sides -> the table; the guards are checked"""
    F, _, h, w = frames.shape
    gh, gw = (h - 1) // cell + 1, (w - 1) // cell + 1
    n = F * gh * gw * 3
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=I32, device=DEV)
    src = frames.to(DEV).contiguous()
    rc = lib.pips_corner_table(C.c_void_p(src.data_ptr()), int(src.dtype == torch.uint8), F, h, w, cell,
                               C.c_void_p(buf.data_ptr() + 4 * GUARD), _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all())
    assert torch.equal(src.cpu(), frames)                                            # the frames are left as they were
    return buf[GUARD:GUARD + n].view(torch.float32).view(F, gh, gw, 3).cpu()


@pytest.mark.parametrize("h,w,cell", SIZES)
def test_corner_table_is_the_torch_form(h, w, cell):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    seen = dict(flat=0, none=0)
    for k, u8 in enumerate(_frames(h, w, seed=h * w + cell)):
        for frames in (u8, _as_float(u8, seed=k)):
            ref = drivers.corner_table_torch(frames, cell)                          # on the CPU
            got = _table_guarded(lib, frames, cell)
            assert torch.equal(_bits(got), _bits(ref)), (h, w, cell, k, frames.dtype)
            assert torch.equal(_bits(ops.corner_table(frames.to(DEV), cell)), _bits(ref))
            seen["flat"] += int((ref[..., 2] == 0).sum())
            seen["none"] += int((ref[..., 2] < 0).sum())
    # what the sizes are there for: cells without a candidate, and cells that are flat (score 0: the centre stays)
    assert (seen["none"] > 0) == ((h, w, cell) != (44, 70, 16) and (h, w, cell) != (264, 328, 32))
    if (h, w) == (8, 30):
        assert seen["none"] == 4 * 4 * 3                                            # every entry of every call
    if h >= 44 and cell < 40:                                                       # (a 40 px cell of 44 x 70 always sees the corner)
        assert seen["flat"] > 0


def test_an_empty_call_writes_nothing():
    from pips_amd import _lib, ops
    lib = _lib.load()
    buf = torch.full((256,), POISON, dtype=I32, device=DEV)
    src = torch.zeros(1, 3, 44, 70, dtype=torch.uint8, device=DEV)
    assert lib.pips_corner_table(C.c_void_p(src.data_ptr()), 1, 0, 44, 70, 8, C.c_void_p(buf.data_ptr()), _stream()) == 0
    assert lib.pips_cover_place(C.c_void_p(buf.data_ptr()), 0, C.c_void_p(buf.data_ptr() + 512), 44, 70, 8, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())
    assert tuple(ops.corner_table(src[:0], 8).shape) == (0, 6, 9, 3)
    assert tuple(ops.cover_place(torch.empty(0, 3, device=DEV), torch.zeros(6, 9, 3, device=DEV), 44, 70, 8, 0).shape) == (0, 3)


@pytest.mark.parametrize("cell", [8, 16, 40])
def test_cover_place_is_the_torch_form(cell):
    """the seeds of a first cover step on 44 x 70 (every cell, the clamped centres of the last row and column among them) placed
    on a noise table, with min_corner below every score, between the scores and above all of them"""
    from pips_amd import drivers, ops
    h, w = 44, 70
    table = drivers.corner_table_torch(_frames(h, w, seed=cell)[0][:1], cell)[0]
    none = torch.zeros(0, dtype=I32)
    seeds = drivers.cover_scan(torch.zeros(0, 0, 2), torch.zeros(0, 0), 0, none, torch.zeros(0, 2), none, h, w, cell, 0.0, 2, 2 ** 31 - 1)[2]
    gh, gw = table.shape[:2]
    assert seeds.shape[0] == gh * gw and float(seeds[:, 1].max()) <= w - 1 and float(seeds[:, 2].max()) <= h - 1
    assert (float(seeds[-1, 1]), float(seeds[-1, 2])) != ((gw - 0.5) * cell, (gh - 0.5) * cell)         # a clamped centre
    scores = table[..., 2].reshape(-1)
    for min_corner in (0, int(scores[scores > 0].median()), int(scores.max()), int(scores.max()) + 1):
        ref = drivers.cover_place_torch(seeds, table, h, w, cell, min_corner)
        buf = torch.full((seeds.numel() + 2 * GUARD,), POISON, dtype=I32, device=DEV)
        mine = buf[GUARD:GUARD + seeds.numel()].view(torch.float32).view(-1, 3)
        mine.copy_(seeds)
        out = ops.cover_place(mine, table.to(DEV), h, w, cell, min_corner)
        torch.cuda.synchronize()
        assert out.data_ptr() == mine.data_ptr() and torch.equal(_bits(out), _bits(ref)), (cell, min_corner)
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + seeds.numel():] == POISON).all())
        # the seeds are every cell in row-major order, as the table is: who moves is read off the table (a best pixel may be
        # the centre itself)
        moves = (scores > min_corner) & (table[..., :2].reshape(-1, 2) != seeds[:, 1:]).any(dim=1)
        assert torch.equal((ref[:, 1:] != seeds[:, 1:]).any(dim=1), moves) and (int(moves.sum()) > 0) == (min_corner < int(scores.max()))
    assert torch.equal(ref, seeds)                                                   # above every score: nobody moves


def test_bad_arguments_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    src = torch.randint(0, 256, (2, 3, 44, 70), dtype=torch.uint8, device=DEV)
    keep = src.clone()
    table = torch.full((2 * 6 * 9 * 3,), POISON, dtype=I32, device=DEV)
    seeds = torch.full((12, 3), POISON, dtype=I32, device=DEV)
    tab1 = torch.full((6 * 9 * 3,), POISON, dtype=I32, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        assert bool((table == POISON).all()) and bool((seeds == POISON).all()) and bool((tab1 == POISON).all()) and torch.equal(src, keep)

    good = dict(frames=C.c_void_p(src.data_ptr()), u8=1, F=2, h=44, w=70, cell=8, table=C.c_void_p(table.data_ptr()))
    bad = [dict(F=-1), dict(h=0), dict(w=0), dict(h=-3), dict(cell=7), dict(cell=0), dict(frames=None), dict(table=None),
           dict(h=1 << 16, w=1 << 16), dict(F=1 << 20)]                        # 2^20 frames of 54 cells: more blocks than a launch takes
    for over in bad:
        a = dict(good, **over)
        assert lib.pips_corner_table(a["frames"], a["u8"], a["F"], a["h"], a["w"], a["cell"], a["table"], _stream()) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    good = dict(seeds=C.c_void_p(seeds.data_ptr()), k=12, table=C.c_void_p(tab1.data_ptr()), h=44, w=70, cell=8, min_corner=0)
    bad = [dict(k=-1), dict(h=0), dict(w=0), dict(cell=7), dict(min_corner=-1), dict(seeds=None), dict(table=None)]
    for over in bad:
        a = dict(good, **over)
        assert lib.pips_cover_place(a["seeds"], a["k"], a["table"], a["h"], a["w"], a["cell"], a["min_corner"], _stream()) == E_ARG, over
        assert lib.pips_last_error()
        untouched()
    assert lib.pips_abi_version() == 3


# ------------------------------------------------------------------ end to end on the device
def _cover(scan):
    from pips_amd import drivers
    return drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan=scan, seed="corners", min_corner=1000)


def _off_centre(xy):
    """how many of the positions (n,2) are no cell centre of the 2 x 3 grid"""
    centres = {(ECELL / 2.0 + ECELL * j, ECELL / 2.0 + ECELL * i) for i in range(2) for j in range(3)}
    return sum(tuple(p) not in centres for p in xy.tolist())


@pytest.mark.parametrize("rounds", ["torch", "library"])
def test_library_scan_equals_torch_scan_end_to_end(weights_tamed, rounds):
    """tests/test_cover_gpu.py's end-to-end run (128 x 192, T = 24 in chunks of 4, cells of 64 px) on its textured video with seeds
    on corners: scan="library" hands out, push by push, the ids and the bits of scan="torch", with the same births, retirements,
    hop lists and query positions -- which are corners, not centres"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _video(ET, EH, EW, seed=70)
    runs = {}
    for scan in drivers.COVER_SCANS:
        ct = drivers.CoverTracker(m, _cover(scan), _user(71).to(DEV), iters=6, slots=24, record_hops=True, rounds=rounds)
        parts, xy = [], []
        for i in range(0, ET, 4):
            parts.append(ct.push(video[:, i:i + 4]))
            xy.append(ct.st.xy_in.cpu())
        parts.append(ct.finish())
        runs[scan] = (parts, ct, xy)
    (pa, a, xa), (pb, b, xb) = runs["torch"], runs["library"]
    _same_parts(pa, pb)
    assert a.born == b.born and a.retired == b.retired and a.hops == b.hops
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(xa, xb))
    tables = drivers.corner_table_torch(video[0], ECELL)
    assert _off_centre(xa[0][3:]) >= 3 and all(tuple(p) in {tuple(e) for e in tables[0, :, :, :2].reshape(-1, 2).tolist()}
                                               for p in xa[0][3:].tolist())
    assert a.born[3:].count(0) in (4, 5) and a.retired[2][1] == "outside"
    assert sum(p[1].shape[1] for p in pa) == ET and pa[-1][3].numel() >= 6
    assert a.book.table.is_cuda and b.book.table.is_cuda and torch.equal(_bits(a.book.table), _bits(b.book.table))
    _assert_live(pa, a.book, [0, 1], f"corner cover e2e {rounds}")


def test_multi_stream_library_scan_equals_torch_scan(weights_tamed):
    """two streams of 24 / 13 frames under MultiStreamTracker(cover=), the second idle in the first push (its first seeds are held):
    scan="library" equals scan="torch" part by part, ids included"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    videos = [_video(ET, EH, EW, seed=72), _video(13, EH, EW, seed=73)]
    runs = {}
    for scan in drivers.COVER_SCANS:
        mt = drivers.MultiStreamTracker(m, [_user(74).to(DEV), _user(75)[:, :1].to(DEV)], iters=6, slots=24, record_hops=True,
                                        rounds="library", cover=_cover(scan))
        parts = [[], []]
        for i in range(0, ET, 4):
            if i == 20:
                parts[1].append(mt.finish(1))
            second = videos[1][:, i - 4:i] if 4 <= i <= 16 else None              # (the last of them is the 13th frame alone)
            for v, p in enumerate(mt.push([videos[0][:, i:i + 4], second])):
                parts[v].append(p)
            if i == 0:
                assert mt.books[1].held is not None and mt.stream_ids(1).tolist() == [0]
        parts[0].append(mt.finish(0))
        runs[scan] = (parts, mt)
    (pa, a), (pb, b) = runs["torch"], runs["library"]
    for v in range(2):
        _same_parts(pa[v], pb[v])
        assert a.books[v].born == b.books[v].born and a.books[v].retired == b.books[v].retired
        assert a.cover_hops(v) == b.cover_hops(v)
    assert a.books[0].retired[2][1] == "outside" and len(a.books[1].born) >= 6
    assert a.books[1].held is None and sum(p[1].shape[1] for p in pa[1]) == 13
    for v, user in enumerate(([0, 1], [0])):
        _assert_live(pa[v], a.books[v], user, f"corner cover streams, stream {v}")
