"""CPU: seeding on corners -- drivers.corner_table_torch / cover_place_torch, Cover(seed="corners") on CoverTracker, track_cover and
MultiStreamTracker(cover=), and drivers.corner_queries -- with ``scan="torch"`` on the fake model of tests/test_multistream.py.  The
rule of pips_corner_table (include/pips_hip.h) is restated here as a plain loop over pixels with math.isqrt for the root; the
cover rule is tests/test_cover.py's ``_Sim`` with the seeds' positions swapped in.  (``scan="library"``: tests/test_corners_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers

from test_multistream import _FakeModel, _bits, _chunks
from test_cover import CELL, H, LOST_AFTER, T, USER, VIDEO, W, _Sim, _cover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule, restated
def _luma(frame):
    """(3,h,w) uint8 or float32 -> (h,w) Python-int luma"""
    if frame.dtype != np.uint8:
        frame = np.floor(np.clip(frame.astype(np.float32), np.float32(0), np.float32(255)) + np.float32(0.5))
    u = frame.astype(np.int64)
    return (77 * u[0] + 150 * u[1] + 29 * u[2] + 128) >> 8


def _scores(frame):
    """{(y, x): S} of every candidate of one frame: a loop over pixels, exact integers"""
    Y = _luma(frame)
    h, w = Y.shape
    out = {}
    for y in range(4, h - 4):
        for x in range(4, w - 4):
            a = b = c = 0
            for v in range(y - 3, y + 4):
                for u in range(x - 3, x + 4):
                    gx, gy = int(Y[v, u + 1]) - int(Y[v, u - 1]), int(Y[v + 1, u]) - int(Y[v - 1, u])
                    a, b, c = a + gx * gx, b + gx * gy, c + gy * gy
            d = (a - c) ** 2 + 4 * b * b
            r = math.isqrt(d)
            out[(y, x)] = a + c - (r + (r * r < d))
    return out


def _table(frames, cell):
    """frames (F,3,h,w) numpy -> (F,gh,gw,3) float32 by the restated rule"""
    F, _, h, w = frames.shape
    gh, gw = (h - 1) // cell + 1, (w - 1) // cell + 1
    out = np.zeros((F, gh, gw, 3), dtype=np.float32)
    for f in range(F):
        S = _scores(frames[f])
        for i in range(gh):
            for j in range(gw):
                best = None
                for y in range(i * cell, min((i + 1) * cell, h)):
                    for x in range(j * cell, min((j + 1) * cell, w)):
                        if (y, x) in S and (best is None or S[(y, x)] > best[2]):       # strict: the first in (y, x) order stays
                            best = (x, y, S[(y, x)])
                if best is None:
                    best = (min(np.float32(j + 0.5) * np.float32(cell), np.float32(w - 1)),
                            min(np.float32(i + 0.5) * np.float32(cell), np.float32(h - 1)), -1)
                out[f, i, j] = best
    return out


def _same(got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


def _noise(F=2, h=44, w=70, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (F, 3, h, w), dtype=np.uint8)


def _checkerboard(h=44, w=70):
    """squares of 4 px, a period of 8: every crossing looks the same"""
    y, x = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((y // 4 + x // 4) % 2) * 255).astype(np.uint8), (1, 3, h, w)).copy()


def _planted(h=44, w=70, cy=24, cx=40):
    """a bright quadrant (y >= cy, x >= cx) on a dark field: one L-corner, two straight edges running out of the frame"""
    f = np.full((1, 3, h, w), 20, dtype=np.uint8)
    f[:, :, cy:, cx:] = 220
    return f


NOISE_REF = {}


def _noise_ref(cell):
    if cell not in NOISE_REF:
        NOISE_REF[cell] = _table(_noise(), cell)
    return NOISE_REF[cell]


@pytest.mark.parametrize("cell", [8, 16, 40])
def test_noise_uint8_and_ragged_last_cells(cell):
    """44 x 70 noise: the torch form is the loop bit for bit; 44 and 70 are no multiple of any of the cells"""
    got = drivers.corner_table_torch(torch.from_numpy(_noise()), cell)
    _same(got, _noise_ref(cell))
    assert tuple(got.shape[1:3]) == drivers.Cover(cell=cell).grid(44, 70)
    assert bool((got[..., 2] > 0).all()) == (cell == 16)     # cells of 8 and of 40 px: the last row is rows 40..43, no candidate
    x, y = got[..., 0], got[..., 1]
    i = torch.arange(got.shape[1]).view(1, -1, 1)
    j = torch.arange(got.shape[2]).view(1, 1, -1)
    assert bool(((y >= i * cell) & (y < (i + 1) * cell) & (x >= j * cell) & (x < (j + 1) * cell)).all())


def test_float_frames_are_quantised_first():
    """the same values with fractions (below one half: the same luma), and entries below 0 and above 255 that clamp"""
    g = np.random.default_rng(5)
    base = _noise()
    f = base.astype(np.float32) + g.uniform(-0.49, 0.49, base.shape).astype(np.float32)
    _same(drivers.corner_table_torch(torch.from_numpy(f), 16), _noise_ref(16))
    f[:, :, ::5, ::3] = -37.5
    f[:, :, 1::7, 2::4] = 300.25
    f[:, :, 2::9, ::2] += 0.5                                   # and values that round the other way
    _same(drivers.corner_table_torch(torch.from_numpy(f), 16), _table(f, 16))
    assert not np.array_equal(_table(f, 16), _noise_ref(16))


def test_checkerboard_ties_go_to_the_lowest_y_then_x():
    f = _checkerboard()
    want = _table(f, 16)
    got = drivers.corner_table_torch(torch.from_numpy(f), 16)
    _same(got, want)
    S = _scores(f[0])
    top = max(S.values())
    assert sum(1 for (y, x), s in S.items() if 16 <= y < 32 and 16 <= x < 32 and s == top) >= 16      # a cell full of ties
    first = min((y, x) for (y, x), s in S.items() if 16 <= y < 32 and 16 <= x < 32 and s == top)
    assert got[0, 1, 1].tolist() == [float(first[1]), float(first[0]), float(top)]


def test_planted_corner_is_found_two_pixels_inside_and_nothing_else_scores():
    """the corner of the quadrant is at (y, x) = (24, 40); the unweighted 7x7 window scores highest where it holds as much of
    both edges as it can, which is 2 px inside the corner along the diagonal; straight edges score exactly 0"""
    f = _planted()
    got = drivers.corner_table_torch(torch.from_numpy(f), 16)
    _same(got, _table(f, 16))
    x, y, s = got[0, 1, 2].tolist()
    assert (x, y) == (42.0, 26.0) and s > 5e5
    rest = got[0, :, :, 2].clone()
    rest[1, 2] = 0
    assert bool((rest <= 0).all())


def test_candidate_edge_cases():
    g = np.random.default_rng(9)
    f = g.integers(0, 256, (2, 3, 9, 9), dtype=np.uint8)
    got = drivers.corner_table_torch(torch.from_numpy(f), 8)
    _same(got, _table(f, 8))
    assert got[:, 0, 0, :2].tolist() == [[4.0, 4.0]] * 2 and bool((got[:, 0, 0, 2] > 0).all())       # the single candidate
    assert got[0, 1, 1].tolist() == [8.0, 8.0, -1.0] and got[0, 0, 1].tolist() == [8.0, 4.0, -1.0]     # clamped centres
    f = g.integers(0, 256, (2, 3, 8, 30), dtype=np.uint8)
    got = drivers.corner_table_torch(torch.from_numpy(f), 8)
    _same(got, _table(f, 8))
    assert got[0, 0].tolist() == [[4.0, 4.0, -1.0], [12.0, 4.0, -1.0], [20.0, 4.0, -1.0], [28.0, 4.0, -1.0]]
    assert tuple(drivers.corner_table_torch(torch.zeros(0, 3, 20, 20), 8).shape) == (0, 3, 3, 3)


def test_integer_frames_that_are_not_uint8_are_clamped_like_floats():
    """ops.corner_table sends every dtype but uint8 through float32, where the kernel clamps: the torch form does the same"""
    f = _noise().astype(np.int32)
    f[:, :, ::5, ::3] = -37
    f[:, :, 1::7, 2::4] = 300
    got = drivers.corner_table_torch(torch.from_numpy(f), 16)
    _same(got, _table(f.astype(np.float32), 16))
    _same(got, _table(np.clip(f, 0, 255).astype(np.uint8), 16))


def test_cover_place_torch():
    table = torch.tensor([[[1.0, 2.0, 50.0], [13.0, 3.0, 0.0]], [[5.0, 11.0, 7.0], [17.0, 15.0, 8.0]]])       # 16 x 20, cell 10
    seeds = torch.tensor([[3.0, 5.0, 5.0], [3.0, 15.0, 5.0], [3.0, 5.0, 15.0], [3.0, 19.0, 15.0]])
    keep = seeds.clone()
    got = drivers.cover_place_torch(seeds, table, 16, 20, 10, 0)
    assert torch.equal(seeds, keep)
    assert got.tolist() == [[3.0, 1.0, 2.0], [3.0, 15.0, 5.0], [3.0, 5.0, 11.0], [3.0, 17.0, 15.0]]           # S = 0 is not above 0
    got = drivers.cover_place_torch(seeds, table, 16, 20, 10, 7)
    assert got.tolist() == [[3.0, 1.0, 2.0], [3.0, 15.0, 5.0], [3.0, 5.0, 15.0], [3.0, 17.0, 15.0]]
    assert tuple(drivers.cover_place_torch(seeds[:0], table, 16, 20, 10, 0).shape) == (0, 3)


# ------------------------------------------------------------------------------------------------ the policy
@pytest.mark.parametrize("kw", [dict(seed="harris"), dict(seed=None), dict(min_corner=-1), dict(min_corner=1.5), dict(min_corner=True)])
def test_cover_rejects_bad_seed_arguments(kw):
    with pytest.raises(ValueError):
        drivers.Cover(**kw)


def test_cover_seed_defaults_and_values():
    c = drivers.Cover()
    assert (c.seed, c.min_corner) == ("centre", 0)
    c = drivers.Cover(seed="corners", min_corner=2000.0)
    assert (c.seed, c.min_corner) == ("corners", 2000) and isinstance(c.min_corner, int)


def _flat_video(T_=T, seed=11):
    """a colour per frame: no pixel of any frame has a gradient"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, T_, 3, 1, 1, generator=g) * 255).expand(1, T_, 3, H, W).contiguous()


@pytest.mark.parametrize("queries", [USER, None])
@pytest.mark.parametrize("chunk,slots", [(1, 9), (3, 9), (7, 9), (7, 24), (45, 24)])
def test_a_flat_video_is_seeded_at_the_centres(queries, chunk, slots):
    """every cell is flat: seed="corners" returns what seed="centre" returns, bit for bit, with born, retired and the hop lists"""
    chunks = _chunks(_flat_video(), chunk)
    ref = drivers.track_cover(_FakeModel(), chunks, _cover(), queries, iters=3, slots=slots, return_hops=True)
    got = drivers.track_cover(_FakeModel(), chunks, _cover(seed="corners"), queries, iters=3, slots=slots, return_hops=True)
    for a, b in zip(got[:4], ref[:4]):
        assert a.shape == b.shape and torch.equal(_bits(a.float()), _bits(b.float()))
    assert got[4] == ref[4] and len(ref[2]) > 24 and int((ref[3] >= 0).sum()) >= 1
    # a threshold no pixel reaches does the same on a textured video
    chunks = _chunks(VIDEO, chunk)
    ref = drivers.track_cover(_FakeModel(), chunks, _cover(), queries, iters=3, slots=slots)
    got = drivers.track_cover(_FakeModel(), chunks, _cover(seed="corners", min_corner=7000000), queries, iters=3, slots=slots)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and torch.equal(_bits(a.float()), _bits(b.float()))


TABLES = drivers.corner_table_torch(VIDEO[0], CELL)               # computed once, read by every test below


class _SimCorners(_Sim):
    """tests/test_cover.py's rule, each seed moved to the table entry of its own frame and cell; seeds whose frame was not pushed
    yet are held back without an identity until ``see`` is told that it has come"""

    def __init__(self, queries, tables, min_corner=0, **kw):
        super().__init__(queries, **kw)
        self.tables, self.min_corner, self.held, self.placed = tables, min_corner, None, []

    def step(self, f1, trajs, vis, pushed):
        n = len(self.live)
        super().step(f1, trajs, vis)
        k = len(self.steps[-1]["seeds"])
        assert len(self.live) == self.steps[-1]["n_keep"] + k and n == self.steps[-1]["n_before"]
        if k and f1 >= pushed:
            assert self.held is None
            self.held = self.live[-k:]
            del self.live[-k:], self.born[-k:]
            for q in self.held:
                del self.xy[q["id"]]
        elif k:
            self._place(self.live[-k:])

    def _place(self, seeds):
        for q in seeds:
            i, j = self.cell(*q["xy"])
            x, y, s = self.tables[q["tq"], i, j].tolist()
            if s > self.min_corner:
                q["xy"] = (x, y)
            self.xy[q["id"]] = q["xy"]
            self.placed.append((q["tq"], i, j, q["xy"], s > self.min_corner))

    def see(self, first):
        """a push whose first frame is ``first`` begins"""
        if self.held is not None:
            assert all(q["tq"] == first for q in self.held)
            for q in self.held:
                assert q["id"] == len(self.born)
                self.born.append(q["tq"])
                self.live.append(q)
            self._place(self.held)
            self.held = None


def _run_corners(chunks, slots, cover, queries, tables, model=None):
    ct = drivers.CoverTracker(_FakeModel() if model is None else model, cover, queries, iters=3, slots=slots)
    sim = _SimCorners(torch.zeros(1, 0, 3) if queries is None else queries, tables, cover.min_corner, max_queries=cover.max_queries)
    pushed, parts = 0, []
    sim.step(0, None, torch.zeros(0, len(sim.live)), pushed)
    for c in chunks:
        if c.shape[1] > 0:
            sim.see(pushed)
        pushed += c.shape[1]
        f0, trajs, vis, ids = ct.push(c)
        assert ids.tolist() == [q["id"] for q in sim.live]
        if trajs.shape[1] > 0:
            sim.step(f0 + trajs.shape[1], trajs[0], vis[0], pushed)
        # the tracker's queries are the rule's, positions included, after every push
        assert ct.ids.tolist() == [q["id"] for q in sim.live] and ct.st.tq_host.tolist() == [q["tq"] for q in sim.live]
        assert [tuple(p) for p in ct.st.xy_in.tolist()] == [q["xy"] for q in sim.live]
        # and it keeps the tables of the frames it has not returned, no others
        assert (ct.book.table0, ct.book.T) == (f0, pushed) and ct.book.table.shape[0] == pushed - f0
        assert torch.equal(ct.book.table, tables[f0:pushed])
        parts.append((f0, trajs, vis, ids))
    return ct, sim, parts


@pytest.mark.parametrize("chunk,slots", [(1, 9), (3, 9), (7, 24)])
@pytest.mark.parametrize("min_corner", [0, 400000])
def test_textured_video_seeds_stand_on_their_own_frame_s_corners(chunk, slots, min_corner):
    ct, sim, parts = _run_corners(_chunks(VIDEO, chunk), slots, _cover(seed="corners", min_corner=min_corner), USER, TABLES)
    f0, trajs, vis, ids = ct.finish()
    assert ids.tolist() == [q["id"] for q in sim.live if sim.held is None or q not in sim.held]
    assert ct.born == sim.born and ct.retired == sim.retired
    assert sum(p[1].shape[1] for p in parts) + trajs.shape[1] == T
    reasons = [r for _, r in sim.retired.values()]
    assert reasons.count("outside") >= 1 and reasons.count("lost") >= 1
    moved = [p for p in sim.placed if p[4]]
    assert len(moved) >= 24 and any(t > 0 for t, *_ in moved)
    assert (len(moved) < len(sim.placed)) == (min_corner > 0)                   # some cells are below the higher threshold
    other = 0
    for t, i, j, xy, _ in moved:
        assert xy == tuple(TABLES[t, i, j, :2].tolist())
        other += all(xy != tuple(TABLES[u, i, j, :2].tolist()) for u in (t - 1, t + 1) if 0 <= u < T)
    # noise: the neighbouring frames have another best pixel in nearly every cell (a cell has at most 100 pixels, so a few
    # coincide), so a seed placed from the frame before or behind its own would show
    assert other >= 0.75 * len(moved)


class _Invisible(_FakeModel):
    """every visibility logit is negative"""

    def track(self, *a, **kw):
        out = super().track(*a, **kw)
        return out[:2] + (-out[2].abs() - 1.0,) + out[3:]


def test_a_stream_that_loses_every_query_at_once():
    """lost_after=1 on all-invisible logits, no queries of the caller: every step retires every query; the frame the step seeds
    was pushed already (a window ends before the last pushed frame), so the new seeds are placed from its table at once"""
    cover = drivers.Cover(cell=CELL, lost_after=1, seed="corners")
    ct, sim, parts = _run_corners(_chunks(VIDEO, 5), 9, cover, None, TABLES, model=_Invisible())
    ct.finish()
    assert ct.born == sim.born and ct.retired == sim.retired
    emptied = [s for s in sim.steps[1:] if s["n_keep"] == 0 and s["n_before"] == 24]
    assert len(emptied) >= 3 and all(len(s["seeds"]) == 24 for s in emptied)
    assert sorted(set(ct.born)) == [0] + [s["f1"] for s in emptied]


def test_held_seeds_wait_for_their_frame():
    """the seeds of a step whose frame was not pushed yet: no identity and no column until the push that brings the frame, then
    the identities and columns of centre seeds, on the corners of that push's first frame"""
    cover = _cover(seed="corners")
    ct = drivers.CoverTracker(_FakeModel(), cover, USER, iters=3, slots=9)
    f0, trajs, vis, ids = ct.push(VIDEO[:, :0])                                  # the first step runs: frame 0 is not there
    n = USER.shape[1]
    assert ids.tolist() == list(range(n)) and ct.ids.tolist() == list(range(n)) and ct.born == USER[0, :, 0].int().tolist()
    assert ct.book.held is not None and ct.book.held[0] == 0 and ct.st.N == n
    centre = drivers.CoverTracker(_FakeModel(), _cover(), USER, iters=3, slots=9)
    centre.push(VIDEO[:, :0])
    k = centre.st.N - n
    assert k >= 20 and tuple(ct.book.held[1].shape) == (k, 3) and torch.equal(ct.book.held[1], centre.st.xy_in.new_tensor(
        [[0.0, *p] for p in centre.st.xy_in[n:].tolist()]))
    f0, trajs, vis, ids = ct.push(VIDEO[:, :3])                                  # frame 0 comes: placed before anything is encoded
    assert ids.tolist() == list(range(n + k)) == centre.ids.tolist() and ct.book.held is None and ct.born == centre.born
    sim = _SimCorners(USER, TABLES)
    for (x, y), (cx, cy) in zip(ct.st.xy_in[n:].tolist(), centre.st.xy_in[n:].tolist()):
        i, j = sim.cell(cx, cy)
        assert [x, y] == TABLES[0, i, j, :2].tolist() and (x, y) != (cx, cy)
    # a tracker whose only step so far is held: finish() drops the seeds, returns no frame and creates no identity
    ct = drivers.CoverTracker(_FakeModel(), cover, None, iters=3, slots=9)
    ct.push(VIDEO[:, :0])
    assert ct.book.held is not None and ct.born == []
    f0, trajs, vis, ids = ct.finish()
    assert (f0, tuple(trajs.shape), ids.tolist(), ct.born, ct.retired, ct.book.held) == (0, (1, 0, 0, 2), [], [], {}, None)


def test_seeds_of_a_stream_without_queries_are_held_mid_video():
    """the branch a push cannot reach while a stream has a query (a window ends before the last pushed frame): a step on a part
    that ends with the last pushed frame -- the part a stream without queries returns.  Driven on the book itself: the first seeds
    are held, join with frames 0..2, every one of them is then outside on frame 2, and the seeds of that step lie on frame 3,
    which is not there: held, and placed from frame 3's table when it comes"""
    from pips_amd.drivers import _CoverBook
    cover = _cover(seed="corners")
    book = _CoverBook(cover, torch.zeros(0, dtype=torch.int64), False)
    added, removed = [], []
    add, remove = (lambda q: added.append(q.clone())), (lambda cols: removed.append(list(cols)))
    none = torch.zeros(0, 2)
    book.start(H, W, torch.device("cpu"), torch.zeros(0, dtype=torch.int64), none, add, remove)
    assert book.held is not None and not added and book.ids == []
    book.see(VIDEO[0, :3], 0, add)
    assert book.held is None and len(added) == 1 and book.ids == list(range(24)) and book.born == [0] * 24
    assert torch.equal(added[0][0, :, 1:], TABLES[0, :, :, :2].reshape(-1, 2))
    rows = torch.full((3, 24, 2), -5.0)                                           # everybody left the frame
    book.step(0, rows, torch.zeros(3, 24), add, remove, None)
    assert removed == [list(range(24))] and book.ids == [] and len(book.retired) == 24 and len(added) == 1
    assert book.held is not None and book.held[0] == 3 and tuple(book.held[1].shape) == (24, 3) and book.born == [0] * 24
    book.see(VIDEO[0, 3:8], 3, add)
    assert book.held is None and len(added) == 2 and book.ids == list(range(24, 48)) and book.born == [0] * 24 + [3] * 24
    assert bool((added[1][0, :, 0] == 3).all()) and torch.equal(added[1][0, :, 1:], TABLES[3, :, :, :2].reshape(-1, 2))
    assert (book.table0, book.T) == (3, 8) and torch.equal(book.table, TABLES[3:8])


def test_a_chunk_of_another_size_leaves_the_book_as_it_was():
    ct = drivers.CoverTracker(_FakeModel(), _cover(seed="corners"), USER, iters=3, slots=9)
    ct.push(VIDEO[:, :4])
    before = (ct.book.T, ct.book.table0, ct.book.table.clone(), ct.ids.tolist(), ct.st.cache.T)
    for bad in (torch.zeros(1, 2, 3, H + 8, W), torch.zeros(1, 2, 3, H, W - 3), torch.zeros(1, 2, 3, H - 1, W - 1)):   # (the last: the same grid)
        with pytest.raises(ValueError):
            ct.push(bad)
        assert before[:2] == (ct.book.T, ct.book.table0) and torch.equal(before[2], ct.book.table)
        assert before[3:] == (ct.ids.tolist(), ct.st.cache.T)
    ct.push(VIDEO[:, 4:9])
    assert ct.book.T == 9


def test_multi_stream_with_an_idle_first_push():
    """MultiStreamTracker(cover=Cover(seed="corners")): stream 1 gets None in the first push, so its first seeds are held until
    its first frames come; each stream is its own CoverTracker"""
    cover = _cover(seed="corners")
    videos = [VIDEO[:, :31], VIDEO[:, 5:27], VIDEO[:, 20:20]]
    qs = [USER, USER[:, :2], torch.zeros(1, 0, 3)]
    waves = [(videos[0][:, :4], None, None), (videos[0][:, 4:11], videos[1][:, :9], None),
             (videos[0][:, 11:31], videos[1][:, 9:22], None)]
    mt = drivers.MultiStreamTracker(_FakeModel(), qs, iters=3, slots=9, record_hops=True, cover=cover)
    parts = [[], [], []]
    for n, wave in enumerate(waves):
        res = mt.push(list(wave))
        for v in range(3):
            if wave[v] is not None:
                parts[v].append(res[v])
        if n == 0:
            assert mt.books[1].held is not None and mt.books[0].held is None and mt.stream_ids(1).tolist() == [0, 1]
    assert mt.books[1].held is None and mt.books[2].held is not None
    fin = mt.finish()
    assert mt.books[2].held is None and mt.books[2].born == [] and fin[2][1].shape[1] == 0
    for v in range(2):
        parts[v].append(fin[v])
        ct = drivers.CoverTracker(_FakeModel(), cover, qs[v], iters=3, slots=9, record_hops=True)
        own = [ct.push(w[v]) for w in waves if w[v] is not None] + [ct.finish()]
        assert len(own) == len(parts[v])
        for (f0, t, vi, ids), (g0, gt, gv, gids) in zip(parts[v], own):
            assert f0 == g0 and torch.equal(ids, gids) and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(vi), _bits(gv))
        assert mt.books[v].born == ct.born and mt.books[v].retired == ct.retired and mt.cover_hops(v) == ct.hops
        assert len(ct.born) > qs[v].shape[1] + 20
    # and the seeds of stream 1 stand on the corners of ITS frame 0, which is frame 5 of the video
    ct = drivers.CoverTracker(_FakeModel(), cover, qs[1], iters=3, slots=9)
    ct.push(waves[1][1])
    x, y = ct.st.xy_in[2].tolist()
    assert [x, y] in TABLES[5, :, :, :2].reshape(-1, 2).tolist() and [x, y] not in TABLES[0, :, :, :2].reshape(-1, 2).tolist()


def test_corner_queries():
    f = torch.from_numpy(_planted())                                   # one corner, in cell (1, 2) of the 16 px grid
    video = torch.stack([torch.zeros_like(f[0]), f[0], torch.from_numpy(_noise(1)[0])]).unsqueeze(0)
    assert drivers.corner_queries(video, t=1, cell=16).tolist() == [[[1.0, 42.0, 26.0]]]
    assert tuple(drivers.corner_queries(video, t=0, cell=16).shape) == (1, 0, 3)
    q = drivers.corner_queries(video, t=2, cell=16)
    ref = _noise_table_of(video[0, 2].numpy())
    assert q.dtype == torch.float32 and q[0, :, 0].tolist() == [2.0] * 15 and q[0, :, 1:].tolist() == ref[..., :2].reshape(-1, 2).tolist()
    thr = int(np.sort(ref[..., 2].reshape(-1))[7])
    q = drivers.corner_queries(video, t=2, cell=16, min_corner=thr)
    want = [e[:2].tolist() for e in ref.reshape(-1, 3) if e[2] > thr]
    assert len(want) == 7 and q[0, :, 1:].tolist() == want                 # row-major order, the cells at or below it skipped
    for bad in (dict(t=3), dict(t=-1), dict(t=0.5), dict(cell=4), dict(min_corner=-1), dict(scan="hip")):
        with pytest.raises(ValueError):
            drivers.corner_queries(video, **bad)
    with pytest.raises(ValueError):
        drivers.corner_queries(video[0])


def _noise_table_of(frame):
    return _table(frame[None], 16)[0]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_corner_entry_points_are_declared_bound_and_exported():
    from pips_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    history = re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)
    assert "pips_corner_table" in history and "pips_cover_place" in history
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_corner_table\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 8
    proto = re.search(r"\bint\s+pips_cover_place\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 8
    for name in ("pips_corner_table", "pips_cover_place"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and len(_lib.SIGNATURES[name][1]) == 8
    assert _lib.SIGNATURES["pips_corner_table"][1][1:6] == [ctypes.c_int] * 5
    assert _lib.SIGNATURES["pips_cover_place"][1][3:7] == [ctypes.c_int] * 4
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_corner_table") and hasattr(raw, "pips_cover_place")
    assert callable(ops.corner_table) and callable(ops.cover_place)
    assert _lib.load().pips_abi_version() == 3
