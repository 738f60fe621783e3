"""CPU: the thin cover step -- ``drivers.Cover(per_cell=k, crowd_after=a)``, ``drivers.cover_scan_thin`` and the declaration of
pips_cover_step_thin -- a cover that also retires the youngest of more than k tracks that share a cell.  The rule is restated
here as plain Python over queries and frames (``_rule``), held against ``cover_scan_thin`` on synthetic rows, and run beside a
``CoverTracker`` on the fake model of tests/test_multistream.py (``_SimThin``, tests/test_cover.py's ``_Sim`` with the second run).
(``scan="library"`` needs the library's kernels: tests/test_cover_thin_gpu.py.)

One case of the rule's description cannot occur: "a crowded query that is alone in its cell on the last frame".  A query is
retired as crowded only with a run >= crowd_after >= 1, so it is surplus on the last returned frame f: at least per_cell >= 1
counting queries of lower column stand in its cell on f.  The lowest per_cell of the counting queries of that cell are not surplus
on f, so their runs are 0 and they are kept -- on the very position that was counted.  A crowded query therefore never frees its
cell; ``test_a_crowded_query_never_leaves_its_cell_empty`` asserts that instead."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers

from test_cover import CELL, GH, GW, H, LOST_AFTER, T, USER, VIDEO, W, _Sim, _video
from test_multistream import _FakeModel, _bits, _chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
I32 = torch.int32
NAN = float("nan")
REASONS = {1: "outside", 2: "lost", 3: "crowded"}


def _rule(trajs, vis, f1, tq, xy, lost, crowd, Hs, Ws, cell, vis_logit, lost_after, max_queries, per_cell, crowd_after):
    """the thin step restated: plain Python over queries and frames (fp32 only where the rule says fp32: the quotient) ->
    dict(keep, lost_out, crowd_out, seeds, gone, reason, counts)"""
    n, m, f = len(tq), len(vis), f1 - 1
    gh, gw = -(-Hs // cell), -(-Ws // cell)

    def inside(p):
        return p[0] >= 0 and p[0] <= Ws - 1 and p[1] >= 0 and p[1] <= Hs - 1

    def cell_of(p):
        q = lambda a: int(np.floor(np.float32(a) / np.float32(cell)))
        return min(q(p[1]), gh - 1), min(q(p[0]), gw - 1)

    pending = [m == 0 or tq[c] > f for c in range(n)]
    run, flag = list(lost), [0] * n
    for c in range(n):                                                           # 1. pending, outside, lost: the step's
        if pending[c]:
            run[c] = 0
            continue
        for g in range(m):
            if f1 - m + g >= tq[c]:
                run[c] = run[c] + 1 if vis[g][c] < vis_logit else 0
        flag[c] = 1 if not inside(trajs[m - 1][c]) else 2 if run[c] >= lost_after else 0
    crun = [0 if pending[c] else crowd[c] for c in range(n)]
    for g in range(m):
        frame = f1 - m + g
        counts = [not pending[c] and tq[c] <= frame and flag[c] == 0 and inside(trajs[g][c]) for c in range(n)]      # 2.
        where = [cell_of(trajs[g][c]) if counts[c] else None for c in range(n)]
        for j in range(n):
            if pending[j] or tq[j] > frame:
                continue
            older = sum(1 for i in range(j) if counts[i] and where[i] == where[j])
            crun[j] = crun[j] + 1 if counts[j] and older >= per_cell else 0      # 3. and 4.
    for c in range(n):
        if not pending[c] and flag[c] == 0 and crun[c] >= crowd_after:           # 5.
            flag[c] = 3
    keep = [c for c in range(n) if flag[c] == 0]
    occupied = set()
    for c in keep:                                                               # 6.
        p = xy[c] if pending[c] else trajs[m - 1][c]
        if inside(p):
            occupied.add(cell_of(p))
    empty = [(i, j) for i in range(gh) for j in range(gw) if (i, j) not in occupied][:max(max_queries - len(keep), 0)]
    seeds = [(float(f1), min((j + 0.5) * cell, Ws - 1.0), min((i + 0.5) * cell, Hs - 1.0)) for i, j in empty]
    gone = [c for c in range(n) if flag[c] != 0]
    return dict(keep=keep, lost_out=[run[c] for c in keep], crowd_out=[crun[c] for c in keep], seeds=seeds, gone=gone,
                reason=[flag[c] for c in gone], counts=[len(keep), len(seeds)] + [flag.count(r) for r in (1, 2, 3)])


def _scan(a, **policy):
    p = {**dict(lost_after=LOST_AFTER, max_queries=INT_MAX, per_cell=1, crowd_after=3), **policy}
    return drivers.cover_scan_thin(a["trajs"], a["vis"], a["f1"], a["tq"], a["xy"], a["lost"], a["crowd"], H, W, CELL, 0.0,
                                   p["lost_after"], p["max_queries"], p["per_cell"], p["crowd_after"])


def _restated(a, **policy):
    p = {**dict(lost_after=LOST_AFTER, max_queries=INT_MAX, per_cell=1, crowd_after=3), **policy}
    return _rule(a["trajs"].tolist(), a["vis"].tolist(), a["f1"], a["tq"].tolist(), a["xy"].tolist(), a["lost"].tolist(),
                 a["crowd"].tolist(), H, W, CELL, 0.0, p["lost_after"], p["max_queries"], p["per_cell"], p["crowd_after"])


def _assert_same(got, ref, what):
    keep, lost_out, crowd_out, seeds, gone, reason, counts = got
    assert counts == ref["counts"], what
    assert all(t.dtype == I32 for t in (keep, lost_out, crowd_out, gone, reason)) and seeds.dtype == torch.float32
    assert keep.tolist() == ref["keep"] and lost_out.tolist() == ref["lost_out"] and crowd_out.tolist() == ref["crowd_out"], what
    assert gone.tolist() == ref["gone"] and reason.tolist() == ref["reason"], what
    assert tuple(seeds.shape) == (len(ref["seeds"]), 3) and seeds.tolist() == [list(s) for s in ref["seeds"]], what


def _named_rows(m):
    """n = 12 queries on the 40 x 60 frame with cells of 10 (a 4 x 6 grid) and the last m of five rows, frames [15, 20):
      0     stands on (12, 12), cell (1, 1);
      1, 2  walk into that cell from the right / from below and are in it from row 2 on: three columns converging;
      3     stands on (45, 25), cell (2, 4);   4 flickers across the border x = 40 beside it: in (2, 4) on rows 0, 2, 4 only;
      5     stands on (55, 5) and is invisible on every row: retired as lost, so it does not count for 6 on (56, 6);
      7     starts on frame 17 (row 2) on (46, 26), cell (2, 4); NaN before;       8 is pending (t_q = 25) on (5, 35);
      9     stands exactly on the corner (30, 30) of cell (3, 3);  10 stands on (36, 36) with a NaN on row 3;
      11    stands on (W-1, H-1)."""
    n = 12
    trajs = torch.empty(5, n, 2)
    for c, p in {0: (12, 12), 3: (45, 25), 5: (55, 5), 6: (56, 6), 7: (46, 26), 9: (30, 30), 10: (36, 36), 11: (W - 1, H - 1)}.items():
        trajs[:, c] = torch.tensor([float(p[0]), float(p[1])])
    trajs[:, 1] = torch.tensor([[25.0, 12.0], [21.0, 12.0], [19.0, 12.0], [15.0, 12.0], [13.0, 12.0]])
    trajs[:, 2] = torch.tensor([[12.0, 25.0], [12.0, 22.0], [12.0, 19.0], [12.0, 18.0], [12.0, 15.0]])
    trajs[:, 4] = torch.tensor([[41.0, 25.0], [39.0, 25.0], [41.0, 25.0], [39.0, 25.0], [41.0, 25.0]])
    trajs[:2, 7] = NAN
    trajs[:, 8] = NAN
    trajs[3, 10] = NAN
    vis = torch.full((5, n), 2.0)
    vis[:, 5] = -2.0
    tq = torch.zeros(n, dtype=I32)
    tq[7], tq[8] = 17, 25
    xy = trajs[4].clone()
    xy[8] = torch.tensor([5.0, 35.0])
    lost = torch.tensor([0, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 0], dtype=I32)
    crowd = torch.tensor([0, 0, 0, 0, 2, 0, 1, 0, 5, 0, 0, 0], dtype=I32)
    if m == 0:
        return dict(trajs=trajs[:0], vis=vis[:0], f1=0, tq=tq, xy=xy, lost=lost, crowd=crowd)
    return dict(trajs=trajs[5 - m:].contiguous(), vis=vis[5 - m:].contiguous(), f1=20, tq=tq, xy=xy, lost=lost, crowd=crowd)


@pytest.mark.parametrize("crowd_after", [1, 3])
@pytest.mark.parametrize("per_cell", [1, 2])
@pytest.mark.parametrize("m", [0, 1, 5])
def test_the_scan_is_the_rule_restated(m, per_cell, crowd_after):
    """cover_scan_thin against the plain-Python rule on the named rows, without a cap and with caps that cut the seed list"""
    a = _named_rows(m)
    before = {k: v.clone() for k, v in a.items() if torch.is_tensor(v)}
    ref = _restated(a, per_cell=per_cell, crowd_after=crowd_after)
    _assert_same(_scan(a, per_cell=per_cell, crowd_after=crowd_after), ref, (m, per_cell, crowd_after))
    n_keep, n_seed = ref["counts"][:2]
    assert n_seed >= 8
    for cap in (n_keep + n_seed // 2, n_keep + 1, n_keep, 0):
        cut = _restated(a, per_cell=per_cell, crowd_after=crowd_after, max_queries=cap)
        assert cut["counts"][1] == min(n_seed, max(cap - n_keep, 0)) < n_seed and cut["seeds"] == ref["seeds"][:cut["counts"][1]]
        _assert_same(_scan(a, per_cell=per_cell, crowd_after=crowd_after, max_queries=cap), cut, (m, per_cell, crowd_after, cap))
    for k, v in before.items():                                                   # the inputs are left as they were
        assert torch.equal(_bits(a[k]), _bits(v)), k


def test_the_named_rows_hold_the_named_cases():
    """what the five rows are there for, read off the restated rule (and so, by the test above, off the scan)"""
    a = _named_rows(5)
    r = _restated(a, per_cell=1, crowd_after=3)
    why = dict(zip(r["gone"], r["reason"]))
    run = dict(zip(r["keep"], r["crowd_out"]))
    # 1 and 2 converge on 0: both were surplus on rows 2..4.  2's elders are 0 and 1 -- 1 counts although it is itself retired
    assert why == {1: 3, 2: 3, 5: 2, 7: 3} and r["counts"] == [8, 24 - 6, 0, 1, 3]
    assert run[4] == 1                       # the flicker: surplus on rows 0, 2, 4; every row between resets the run of 2 it came with
    assert run[6] == 0                       # its elder 5 is lost in this step and does not count: the run of 1 it came with is reset
    assert run[8] == 0 and 8 in r["keep"]    # pending: kept, run 0 whatever it came with
    assert run[10] == 1                      # the NaN on row 3 does not count; (30, 30) is 9's corner of the cell they share
    assert run[0] == run[3] == run[9] == run[11] == 0
    # 7 starts on row 2: three surplus rows from t_q on.  With two to a cell it is surplus only where 4 is in the cell too
    r2 = _restated(a, per_cell=2, crowd_after=3)
    assert dict(zip(r2["gone"], r2["reason"])) == {2: 3, 5: 2} and dict(zip(r2["keep"], r2["crowd_out"]))[7] == 1
    assert dict(zip(r2["keep"], r2["crowd_out"]))[1] == 0
    # crowd_after = 1: whoever is surplus on the last row goes
    r1 = _restated(a, per_cell=1, crowd_after=1)
    assert dict(zip(r1["gone"], r1["reason"])) == {1: 3, 2: 3, 4: 3, 5: 2, 7: 3, 10: 3}
    # one row: the runs that come in count (4 came with 2)
    one = _restated(_named_rows(1), per_cell=1, crowd_after=3)
    assert dict(zip(one["gone"], one["reason"])) == {4: 3} and dict(zip(one["keep"], one["crowd_out"]))[1] == 1
    # no row: everybody is pending, nobody is retired, every run is 0
    none = _restated(_named_rows(0), per_cell=1, crowd_after=1)
    assert none["keep"] == list(range(12)) and none["crowd_out"] == [0] * 12 and none["lost_out"] == [0] * 12 and none["gone"] == []


VALUES = [0.0, -0.0, 0.5, 9.5, 10.0, 19.5, 20.0, 29.0, 30.0, 35.5, 39.0, 39.5, 40.0, 50.0, 59.0, 60.0, -1.0, NAN, float("inf"),
          -float("inf")]


def _random_rows(n, m, seed):
    """positions drawn from a few values, so that many queries share cells: integers, halves, cell borders, W-1 / H-1, W / H,
    negatives, -0.0, NaN and +-inf; t_q around the rows; both runs random"""
    g = torch.Generator().manual_seed(seed)
    f1 = 20 if m > 0 else 0
    v = torch.tensor(VALUES)
    trajs = v[torch.randint(0, len(VALUES) - 4 * (seed % 2), (m, n, 2), generator=g)]
    xy = v[torch.randint(0, len(VALUES), (n, 2), generator=g)]
    vis = torch.randn(m, n, generator=g)
    tq = torch.randint(f1 - m - 2, f1 + 2, (n,), generator=g).clamp(min=0).to(I32)
    return dict(trajs=trajs, vis=vis, f1=f1, tq=tq, xy=xy, lost=torch.randint(0, 3, (n,), generator=g).to(I32),
                crowd=torch.randint(0, 3, (n,), generator=g).to(I32))


def test_the_scan_is_the_rule_on_drawn_rows():
    seen = [0, 0, 0]
    for seed in range(12):
        for m in (0, 1, 5):
            a = _random_rows(12, m, seed)
            for per_cell, crowd_after in ((1, 1), (1, 3), (2, 1), (2, 3)):
                ref = _restated(a, per_cell=per_cell, crowd_after=crowd_after)
                _assert_same(_scan(a, per_cell=per_cell, crowd_after=crowd_after), ref, (seed, m, per_cell, crowd_after))
                seen = [s + c for s, c in zip(seen, ref["counts"][2:])]
    assert min(seen) > 10, seen


def test_without_a_cap_per_cell_it_is_the_old_step():
    """per_cell = INT_MAX: nobody is surplus -- keep, lost_out, the seeds and the first four counts are cover_scan's, the fifth is 0"""
    for a in [_named_rows(m) for m in (0, 1, 5)] + [_random_rows(12, m, s) for m in (0, 1, 5) for s in range(4)]:
        for cap in (INT_MAX, 14):
            old = drivers.cover_scan(a["trajs"], a["vis"], a["f1"], a["tq"], a["xy"], a["lost"], H, W, CELL, 0.0, LOST_AFTER, cap)
            keep, lost_out, crowd_out, seeds, gone, reason, counts = _scan(a, per_cell=INT_MAX, crowd_after=1, max_queries=cap)
            assert counts == old[3] + [0] and torch.equal(keep, old[0]) and torch.equal(lost_out, old[1])
            assert torch.equal(_bits(seeds), _bits(old[2])) and bool((crowd_out == 0).all()) and 3 not in reason.tolist()
            assert sorted(keep.tolist() + gone.tolist()) == list(range(12))


def test_a_crowded_query_never_leaves_its_cell_empty():
    """(the module's docstring) every crowded query stands, on the last frame, in a cell that at least per_cell kept queries hold:
    none of the step's seeds lands there"""
    crowded = 0
    for seed in range(24):
        a = _random_rows(12, 5, seed)
        for per_cell in (1, 2):
            r = _restated(a, per_cell=per_cell, crowd_after=1)
            last = a["trajs"][-1].tolist()
            cell = lambda p: (min(int(p[1] // CELL), GH - 1), min(int(p[0] // CELL), GW - 1))
            held = [cell(last[c]) for c in r["keep"] if a["tq"][c] <= 19 and 0 <= last[c][0] <= W - 1 and 0 <= last[c][1] <= H - 1]
            for c, why in zip(r["gone"], r["reason"]):
                if why == 3:
                    crowded += 1
                    assert held.count(cell(last[c])) >= per_cell
                    assert all(cell(s[1:]) != cell(last[c]) for s in r["seeds"])
    assert crowded >= 8                       # (the case occurs)


# ------------------------------------------------------------------ end to end on the fake model
PER_CELL, CROWD_AFTER = 1, 3


def _cover(**kw):
    return drivers.Cover(**{**dict(cell=CELL, vis_thr=0.5, lost_after=LOST_AFTER, per_cell=PER_CELL, crowd_after=CROWD_AFTER), **kw})


class _SimThin(_Sim):
    """tests/test_cover.py's restated cover with the second run: ``_rule`` on the live queries of every step.  ``cells[id]`` is the
    cell of each returned frame of a started query (None outside the frame), for the invariant of the thinned cover"""

    def __init__(self, queries, cover, Hs=H, Ws=W):
        super().__init__(queries, cover.max_queries, Hs, Ws)
        self.cover, self.cells, self.carried = cover, {}, 0
        for q in self.live:
            q["crowd"] = 0

    def step(self, f1, trajs, vis):
        m, n, c = vis.shape[0], len(self.live), self.cover
        rows = trajs.tolist() if m > 0 else []
        r = _rule(rows, vis.tolist(), f1, [q["tq"] for q in self.live], [q["xy"] for q in self.live], [q["lost"] for q in self.live],
                  [q["crowd"] for q in self.live], self.H, self.W, CELL, 0.0, INT_MAX if c.lost_after is None else c.lost_after,
                  INT_MAX if self.max is None else self.max, c.per_cell, c.crowd_after)
        for g in range(m):
            for k, q in enumerate(self.live):
                if q["tq"] <= f1 - m + g:
                    self.cells.setdefault(q["id"], []).append(self.cell(*rows[g][k]) if self.inside(*rows[g][k]) else None)
        args = (rows, vis.tolist(), f1, [q["tq"] for q in self.live], [q["xy"] for q in self.live], [q["lost"] for q in self.live])
        fresh = _rule(*args, [0] * n, self.H, self.W, CELL, 0.0, INT_MAX if c.lost_after is None else c.lost_after,
                      INT_MAX if self.max is None else self.max, c.per_cell, c.crowd_after)
        for k, why in zip(r["gone"], r["reason"]):
            self.retired[self.live[k]["id"]] = (f1 - 1, REASONS[why])
            self.carried += why == 3 and k not in fresh["gone"]      # surplus frames of an earlier push were needed
        keep = []
        for k, lost, crowd in zip(r["keep"], r["lost_out"], r["crowd_out"]):
            q = self.live[k]
            q["lost"], q["crowd"] = lost, crowd
            keep.append(q)
        self.steps.append(dict(f1=f1, n_keep=len(keep), seeds=r["seeds"], counts=r["counts"], m=m))
        self.live = keep
        for t, x, y in r["seeds"]:
            i = len(self.born)
            self.live.append(dict(id=i, tq=int(t), xy=(x, y), lost=0, crowd=0))
            self.born.append(int(t))
            self.xy[i] = (x, y)
        if m > 0:                              # the invariant: nobody beyond per_cell has sat in one cell for crowd_after frames
            a, sat = c.crowd_after, {}
            for q in keep:
                h = self.cells.get(q["id"], [])
                if len(h) >= a and h[-1] is not None and all(x == h[-1] for x in h[-a:]):
                    sat[h[-1]] = sat.get(h[-1], 0) + 1
            assert all(k <= c.per_cell for k in sat.values()), (f1, sat)


def _run(chunk, slots, cover, queries=USER, video=VIDEO):
    ct = drivers.CoverTracker(_FakeModel(), cover, queries, iters=3, slots=slots)
    sim = _SimThin(queries, cover, *video.shape[3:])
    sim.step(0, None, torch.zeros(0, len(sim.live)))
    for c in _chunks(video, chunk):
        f0, trajs, vis, ids = ct.push(c)
        assert ids.tolist() == [q["id"] for q in sim.live]
        if trajs.shape[1] > 0:
            sim.step(f0 + trajs.shape[1], trajs[0], vis[0])
            assert ct.book.crowd.tolist() == [q["crowd"] for q in sim.live] and ct.book.lost.tolist() == [q["lost"] for q in sim.live]
    ct.finish()
    return ct, sim


@pytest.mark.parametrize("slots", [9, 24])
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_the_thinned_cover_is_the_rule_restated(chunk, slots):
    """40 x 60 frames, cells of 10, at most one track to a cell after 3 frames: ids at every push, both runs after every step,
    births and retirements with their reasons are those of the restated rule; the invariant holds after every step (asserted in
    _SimThin.step); queries are retired for every reason; in chunks of one every crowded retirement needs the run that was carried
    over from the pushes before (``carried``: the crowded whom the same step given runs of 0 keeps)"""
    ct, sim = _run(chunk, slots, _cover())
    assert ct.born == sim.born and ct.retired == sim.retired
    reasons = [r for _, r in sim.retired.values()]
    print(f"thin cover chunk {chunk} slots {slots}: {len(sim.born)} identities, "
          f"{ {r: reasons.count(r) for r in ('outside', 'lost', 'crowded')} }, carried {sim.carried}")
    assert reasons.count("crowded") >= 1 and reasons.count("outside") >= 1 and reasons.count("lost") >= 1
    if chunk == 1:                                 # a surplus that begins in one push completes two pushes later, on the frame the
        assert sim.carried == reasons.count("crowded")      # rule names (ct.retired == sim.retired): without the run nobody would go


def test_the_second_run_is_carried_from_step_to_step():
    """the five named rows as two steps, rows 0..2 and rows 3..4 with what the first step returned: the queries that were surplus
    on rows 2..4 are retired by the second step -- on frame 19, as the one step over all five rows retires them; the second step
    given runs of 0 retires nobody as crowded"""
    whole = _named_rows(5)
    whole["trajs"][1, 10] = NAN                                                   # (10 now counts on rows 0, 2 and 4 only)
    one = _scan(whole)
    first = dict(whole, trajs=whole["trajs"][:3].contiguous(), vis=whole["vis"][:3].contiguous(), f1=18)
    keep, lost_out, crowd_out, seeds, gone, reason, counts = _scan(first)
    _assert_same((keep, lost_out, crowd_out, seeds, gone, reason, counts), _restated(first), "rows 0..2")
    assert dict(zip(gone.tolist(), reason.tolist())) == {5: 2}                   # nobody is crowded yet: 1, 2 and 7 have one surplus row
    assert dict(zip(keep.tolist(), crowd_out.tolist())) == {0: 0, 1: 1, 2: 1, 3: 0, 4: 1, 6: 0, 7: 1, 8: 0, 9: 0, 10: 1, 11: 0}
    k = keep.long()
    second = dict(trajs=whole["trajs"][3:, k].contiguous(), vis=whole["vis"][3:, k].contiguous(), f1=20, tq=whole["tq"][k],
                  xy=whole["xy"][k], lost=lost_out, crowd=crowd_out)
    got = _scan(second)
    _assert_same(got, _restated(second), "rows 3..4")
    assert {int(k[c]): r for c, r in zip(got[4].tolist(), got[5].tolist())} == {1: 3, 2: 3, 7: 3}
    assert k[got[0].long()].tolist() == one[0].tolist() and got[1].tolist() == one[1].tolist() and got[2].tolist() == one[2].tolist()
    assert torch.equal(_bits(got[3]), _bits(one[3]))                             # the same seeds on frame 20
    fresh = _scan(dict(second, crowd=torch.zeros_like(crowd_out)))
    assert fresh[6][4] == 0 and fresh[2].tolist() == [0, 2, 2, 0, 1, 0, 2, 0, 0, 1, 0]


def test_each_identity_is_the_stream_given_it_alone():
    """over its life every identity of a thinned cover is track_stream given only that query, bit for bit with the hop lists"""
    chunks = _chunks(VIDEO, 3)
    trajs, vis, born, retired, hops = drivers.track_cover(_FakeModel(), chunks, _cover(), USER, iters=3, slots=9, return_hops=True)
    ct, sim = _run(3, 9, _cover())
    K = len(sim.born)
    assert tuple(trajs.shape) == (1, T, K, 2) and born.tolist() == sim.born
    assert retired.tolist() == [sim.retired.get(i, (-1,))[0] for i in range(K)]
    for i in range(K):
        q = torch.tensor([[[float(sim.born[i]), *sim.xy[i]]]])
        ref_t, ref_v, ref_h = drivers.track_stream(_FakeModel(), chunks, q, iters=3, slots=9, return_hops=True)
        end = T if int(retired[i]) < 0 else int(retired[i]) + 1
        assert torch.equal(_bits(trajs[0, :end, i]), _bits(ref_t[0, :end, 0])), i
        assert torch.equal(_bits(vis[0, :end, i]), _bits(ref_v[0, :end, 0])), i
        assert bool(torch.isnan(trajs[0, end:, i]).all()) and bool(torch.isnan(vis[0, end:, i]).all())
        assert hops[i] == (ref_h[0] if int(retired[i]) < 0 else ref_h[0][:len(hops[i])]), i
    assert any(r == "crowded" for _, r in sim.retired.values())


def test_three_thinned_streams_are_their_own_cover_trackers():
    """three streams of 37 / 21 / 9 frames under MultiStreamTracker(cover=Cover(per_cell=1)): every pushed part is the part of the
    stream's own CoverTracker -- f0, bits, ids -- with born, retired and the hop lists"""
    TS, queries = (37, 21, 9), [USER, USER[:, :2], torch.zeros(1, 0, 3)]
    lists = [_chunks(_video(t, 60 + v), 3) for v, t in enumerate(TS)]
    cover = _cover()
    mt = drivers.MultiStreamTracker(_FakeModel(), queries, iters=3, slots=9, record_hops=True, cover=cover)
    parts = [[] for _ in TS]
    for i in range(max(len(c) for c in lists) + 1):
        for v, c in enumerate(lists):
            if len(c) == i:
                parts[v].append(mt.finish(v))
        wave = [c[i] if i < len(c) else None for c in lists]
        if any(w is not None for w in wave):
            for v, p in enumerate(mt.push(wave)):
                if wave[v] is not None:
                    parts[v].append(p)
    crowded = 0
    for v in range(3):
        ct = drivers.CoverTracker(_FakeModel(), cover, queries[v], iters=3, slots=9, record_hops=True)
        own = [ct.push(c) for c in lists[v]] + [ct.finish()]
        assert len(own) == len(parts[v])
        for (f0, t, vi, ids), (g0, gt, gv, gids) in zip(parts[v], own):
            assert f0 == g0 and torch.equal(ids, gids) and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(vi), _bits(gv))
        assert mt.books[v].born == ct.born and mt.books[v].retired == ct.retired and mt.cover_hops(v) == ct.hops
        crowded += sum(r == "crowded" for _, r in ct.retired.values())
    assert crowded >= 1
    got = drivers.track_streams(_FakeModel(), lists, queries, iters=3, slots=9, cover=cover)
    for v in range(3):
        ref = drivers.track_cover(_FakeModel(), lists[v], cover, queries[v], iters=3, slots=9)
        for x, y in zip(got[v], ref):
            assert x.shape == y.shape and torch.equal(_bits(x.float()), _bits(y.float()))


# ------------------------------------------------------------------ arguments, defaults, the boundary
@pytest.mark.parametrize("kw", [dict(per_cell=0), dict(per_cell=-1), dict(per_cell=True), dict(per_cell=1.5), dict(per_cell="1"),
                                dict(per_cell=2 ** 31), dict(crowd_after=0), dict(crowd_after=-3), dict(crowd_after=False),
                                dict(crowd_after=2.5), dict(crowd_after=None), dict(crowd_after=float("nan"))])
def test_cover_rejects_bad_arguments(kw):
    with pytest.raises(ValueError):
        drivers.Cover(**kw)


def test_the_defaults_never_take_the_thin_step(monkeypatch):
    c = drivers.Cover()
    assert c.per_cell is None and c.crowd_after == 4
    c = drivers.Cover(per_cell=2.0, crowd_after=1)
    assert (c.per_cell, c.crowd_after) == (2, 1) and isinstance(c.per_cell, int)

    def never(*a, **k):
        raise AssertionError("the thin step was called without per_cell")

    from pips_amd import ops
    monkeypatch.setattr(drivers, "cover_scan_thin", never)
    monkeypatch.setattr(ops, "cover_step_thin", never)
    cover = drivers.Cover(cell=CELL, lost_after=LOST_AFTER)
    ct = drivers.CoverTracker(_FakeModel(), cover, USER, iters=3, slots=9)
    for c in _chunks(VIDEO, 7):
        ct.push(c)
    ct.finish()
    assert len(ct.retired) >= 4 and all(r in ("outside", "lost") for _, r in ct.retired.values())
    with pytest.raises(AssertionError):                                           # (and with per_cell it is the step that is called)
        drivers.CoverTracker(_FakeModel(), _cover(), USER, iters=3, slots=9).push(VIDEO[:, :9])


def test_cover_step_thin_is_declared_bound_and_exported():
    from pips_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    history = re.search(r"Still 3 after additions.*?\*/", hdr, flags=re.S).group(0)
    assert "pips_cover_step_thin" in history and "pips_cover_thin_workspace_bytes" in history
    rule = re.search(r"/\* The thin cover step.*?\*/", hdr, flags=re.S).group(0)
    assert "NOT greedy" in rule and "cell border" in rule
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"\bint\s+pips_cover_step_thin\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 27
    proto = re.search(r"\bsize_t\s+pips_cover_thin_workspace_bytes\s*\(([^)]*)\)\s*;", hdr)
    assert proto is not None and len(proto.group(1).split(",")) == 4
    sig = _lib.SIGNATURES["pips_cover_step_thin"]
    assert len(sig[1]) == 27 and sig[0] is ctypes.c_int and sig[1][12] is ctypes.c_float and sig[1][25] is ctypes.c_size_t
    assert _lib.SIGNATURES["pips_cover_thin_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "pips_cover_step_thin") and hasattr(raw, "pips_cover_thin_workspace_bytes") and callable(ops.cover_step_thin)
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    # the sizing query is a host function: the old step's workspace, a second run per query, a surplus bit per (row, query)
    assert lib.pips_cover_thin_workspace_bytes(1000, 16, 33, 41) == 4 * (2 * 1000 + 33 * 41 + 1000 + 16 * 1000)
    assert lib.pips_cover_thin_workspace_bytes(1000, 16, 33, 41) == lib.pips_cover_workspace_bytes(1000, 33, 41) + 4 * 17 * 1000
    assert lib.pips_cover_thin_workspace_bytes(0, 0, 1, 1) == 4
    assert lib.pips_cover_thin_workspace_bytes(-1, 1, 4, 6) == 0 and lib.pips_cover_thin_workspace_bytes(5, -1, 4, 6) == 0
    assert lib.pips_cover_thin_workspace_bytes(5, 1, 0, 6) == 0 and lib.pips_cover_thin_workspace_bytes(5, 1, 1 << 13, 1 << 12) == 0
    assert lib.pips_cover_workspace_bytes(1000, 33, 41) == 4 * (2 * 1000 + 33 * 41)      # the old query is as it was
