"""CPU: object masks that follow image edges -- drivers.object_masks_guided_torch and drivers.guide_plane_torch, the torch twins of
pips_object_masks_guided and pips_guide_plane (include/pips_hip.h).  The twin's keys are held to a plain heap Dijkstra on Python
integers -- cost first, then the lower column -- on every case of tests/test_masks_guided_gpu.py, which are made here and shown to
earn their place: the multi-tile cases span more than one tile with a ragged last one, the serpentine cases need more Jacobi steps
than two launches are good for, no case is mostly PIPS_MASK_NONE, the saturation case has a candidate past 32767.  What the edge
term means on a planted scene; the guide's twin against a per-pixel loop; every PIPS_E_ARG case of both entries through the loaded
library (nothing is launched).  (The kernels: tests/test_masks_guided_gpu.py.)"""
import heapq
import os
import re

import pytest
import torch

from pips_amd import drivers, ops
from test_draw import buffers, views
from test_masks import _quantise, mask_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 255
KEY_NONE = (1 << 32) - 1


def constant(name):
    """the value of the one ``constexpr int NAME = <number>;`` of csrc/masks_guided.hip"""
    text = open(os.path.join(ROOT, "pips_amd", "csrc", "masks_guided.hip")).read()
    found = re.findall(r"^\s*constexpr int %s = (\d+);" % name, text, flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


GUIDED_TILE, GUIDED_HALO = constant("GUIDED_TILE"), constant("GUIDED_HALO")


# ------------------------------------------------------------------------------------------------------------------ the cases
def guided_cases():
    """(name, h, w, n, edge, reach, F, src, guide kind, clustered)"""
    return [("two-tiles-across", 33, 70, 40, 4, 240, 3, None, "blocky", False),
            ("one-tile-high", 64, 48, 255, 8, 160, 1, None, "blocky", False),
            ("tiles-2x3", 65, 129, 12, 2, 400, 1, None, "blocky", False),
            ("strip", 5, 200, 3, 1, 1000, 1, None, "blocky", False),
            ("serpentine", 33, 70, 3, 64, 2000, 1, None, "serpentine", False),
            ("serpentine-transposed", 70, 33, 3, 64, 2000, 1, None, "serpentine", False),
            ("saturation", 8, 8, 1, 64, 32767, 1, None, "checker", False),
            ("saturation-bands", 8, 8, 1, 64, 32767, 1, None, "bands", False),
            ("no-column", 16, 16, 0, 4, 240, 3, None, "blocky", False),
            ("one-pixel", 1, 1, 1, 4, 0, 1, None, "blocky", False),
            ("seeds-only", 17, 15, 20, 4, 4, 1, None, "blocky", False),
            ("n257", 33, 70, 257, 4, 240, 1, None, "blocky", False),
            ("n600-clustered", 64, 48, 600, 1, 1000, 1, None, "blocky", True),
            ("resized", 33, 70, 40, 4, 240, 1, (66, 140), "blocky", False)]


def guided_id(c):
    return c[0]


MULTI_TILE = {"two-tiles-across": (1, 2), "tiles-2x3": (2, 3), "serpentine": (1, 2), "serpentine-transposed": (2, 1)}      # tiles down, across
DEGENERATE = ("no-column", "one-pixel", "seeds-only")                # cases whose point is that (nearly) nothing is labelled


def serpentine(h, w):
    """guide 20 with one-pixel walls of 235 at x = 6, 14, 22, ... that leave a gap of three pixels alternately at the bottom and at
    the top -> (guide (h,w) uint8, the two seed pixels (x, y): one in the first corridor, one in the last)"""
    g = torch.full((h, w), 20, dtype=torch.uint8)
    for k, x in enumerate(range(6, w, 8)):
        g[:, x] = 235
        if k % 2 == 0:
            g[:3, x] = 20
        else:
            g[h - 3:, x] = 20
    return g, ((2, h - 2), (w - 2, 1))


def guided_case_inputs(c):
    """-> (rows (G,n,2) float32, labels (G,n) int64, guide (F,h,w) uint8, first): G = F + 2 rows and first = 1, as
    test_masks.mask_case_inputs"""
    name, h, w, n, edge, reach, F, src, kind, cluster = c
    seed = 5000 + 31 * h + 7 * w + n + edge + reach
    g = torch.Generator().manual_seed(seed)
    G, first = F + 2, 1
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind == "blocky":
        guide = (60 + ((xx // 23 + yy // 19) % 3) * 50)[None] + torch.randint(-2, 3, (F, h, w), generator=g)
        guide = guide.to(torch.uint8)
    elif kind == "checker":
        guide = (((xx + yy) % 2) * 255).to(torch.uint8)[None].repeat(F, 1, 1)
    elif kind == "bands":                                            # columns 0..2 at 0, 3..4 at 255, 5..7 at 0: two full crossings
        guide = (((xx >= 3) & (xx <= 4)) * 255).to(torch.uint8)[None].repeat(F, 1, 1)
    else:
        tall = name.endswith("transposed")
        plane, seeds = serpentine(*((w, h) if tall else (h, w)))
        guide = (plane.t() if tall else plane).contiguous()[None].repeat(F, 1, 1)
        pts = [seeds[0], seeds[0], seeds[1]]                         # the first pixel twice: the lower column must win
        rows = torch.tensor([[(y, x) if tall else (x, y) for x, y in pts]], dtype=torch.float32).repeat(G, 1, 1)
        return rows, torch.tensor([[1, 2, 3]]).repeat(G, 1), guide, first
    if n >= 40:
        rows, lab = mask_tracks(G, n, h, w, seed + 1, src, cluster)  # NaN, infinite and far-outside points and labels 255 among them
    else:
        H, W = (h, w) if src is None else src
        rows = (torch.rand(G, n, 2, generator=g) * torch.tensor([(w + 2.0) * W / w, (h + 2.0) * H / h]) - 1.0).float()
        lab = torch.randint(0, 4, (G, n), generator=g)
    if name == "saturation":
        rows[:] = torch.tensor([3.0, 3.0])
    if name == "saturation-bands":
        rows[:] = torch.tensor([0.0, 3.0])
    if name == "one-pixel":
        rows[:] = torch.tensor([0.25, -0.25])
    return rows, lab, guide, first


def twin(c, with_keys=False):
    name, h, w, n, edge, reach, F, src, kind, cluster = c
    rows, lab, guide, first = guided_case_inputs(c)
    out = drivers._guided_keys(rows[None, :first + F], lab[:first + F], guide, src or (h, w), (h, w), reach / 5.0, edge, first)
    return out if with_keys else out[0]


# ------------------------------------------------------------------------------------------------- the rule as a heap Dijkstra
def rule_keys(row, labels, guide, size, src, edge, reach):
    """one frame by loops on Python integers: row n x 2 floats, labels n ints, guide h lists of w ints -> h lists of w keys"""
    (h, w), (src_h, src_w) = size, src
    key = [[KEY_NONE] * w for _ in range(h)]
    for i, (x, y) in enumerate(row):
        qx, qy = _quantise(x, src_w, w), _quantise(y, src_h, h)
        if qx is None or qy is None or labels[i] == NONE:
            continue
        X, Y = (qx + 4) >> 3, (qy + 4) >> 3
        if 0 <= X < w and 0 <= Y < h:
            key[Y][X] = min(key[Y][X], i)
    heap = [(key[Y][X], Y, X) for Y in range(h) for X in range(w) if key[Y][X] != KEY_NONE]
    heapq.heapify(heap)
    while heap:
        k, Y, X = heapq.heappop(heap)
        if k != key[Y][X]:
            continue
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y, x = Y + dy, X + dx
                if (dx == 0 and dy == 0) or not (0 <= x < w and 0 <= y < h):
                    continue
                cost = (k >> 16) + (7 if dx and dy else 5) + edge * abs(guide[Y][X] - guide[y][x])
                cand = cost << 16 | (k & 0xFFFF)
                if cost <= reach and cand < key[y][x]:
                    key[y][x] = cand
                    heapq.heappush(heap, (cand, y, x))
    return key


_checked = {}


def checked(c):
    """the twin's (masks, keys, steps) of a case, its keys held to the Dijkstra and its masks to the labels of the keys' columns"""
    if c[0] not in _checked:
        name, h, w, n, edge, reach, F, src, kind, cluster = c
        rows, lab, guide, first = guided_case_inputs(c)
        masks, keys, steps = twin(c, with_keys=True)
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (F, h, w) and len(steps) == F
        for k in range(F):
            labels = lab[first + k].tolist()
            want = rule_keys(rows[first + k].tolist(), labels, guide[k].tolist(), (h, w), src or (h, w), edge, reach)
            assert keys[k].tolist() == want, (name, k)
            assert masks[k].tolist() == [[NONE if v == KEY_NONE else labels[v & 0xFFFF] for v in line] for line in want], (name, k)
        _checked[c[0]] = (masks, keys, steps)
    return _checked[c[0]]


@pytest.mark.parametrize("case", guided_cases(), ids=guided_id)
def test_twin_is_dijkstra_on_the_keys(case):
    checked(case)


def test_the_constants_and_their_mirrors():
    assert (ops.GUIDED_TILE, ops.GUIDED_HALO) == (GUIDED_TILE, GUIDED_HALO)
    assert [ops.guided_launches(r) for r in (0, 4, 5, 5 * GUIDED_HALO + 4, 5 * GUIDED_HALO + 5, 32767)] == \
        [1, 1, 1, 1, 2, -(-(32767 // 5) // GUIDED_HALO)]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pips_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+PIPS_MASK_EDGE_MAX\s+%d\b" % ops.MASK_EDGE_MAX, hdr)
    assert re.search(r"#define\s+PIPS_MASK_REACH_MAX\s+%d\b" % ops.MASK_REACH_MAX, hdr)
    assert (ops.MASK_EDGE_MAX, ops.MASK_REACH_MAX) == (64, 32767)
    # with these a key never wraps and never collides with none
    assert 7 + ops.MASK_EDGE_MAX * 255 == 16327 and ops.MASK_REACH_MAX + 16327 == 49094 < 65535


def test_the_cases_earn_their_place():
    """multi-tile cases span more than one tile in the stated direction, the last one ragged; the serpentines' Jacobi takes more
    than 2 GUIDED_HALO steps, so their keys cross at least two hand-offs between launches; at most half of a non-degenerate case
    is PIPS_MASK_NONE; the saturation case has a candidate cost + c beyond 32767; the lower of two columns on one seed pixel wins"""
    seen = set()
    for c in guided_cases():
        name, h, w, n, edge, reach, F, src, kind, cluster = c
        masks, keys, steps = checked(c)
        tiles = (-(-h // GUIDED_TILE), -(-w // GUIDED_TILE))
        share = float((masks == NONE).float().mean())
        print(f"{name}: {tiles[0]} x {tiles[1]} tiles of {GUIDED_TILE}, Jacobi steps {steps}, {ops.guided_launches(reach)} launches, "
              f"{100 * share:.1f} % PIPS_MASK_NONE")
        if name in MULTI_TILE:
            down, across = MULTI_TILE[name]
            assert tiles == (down, across)
            assert (across == 1 or w % GUIDED_TILE != 0) and (down == 1 or h % GUIDED_TILE != 0)
        if kind == "serpentine":
            assert min(steps) > 2 * GUIDED_HALO and ops.guided_launches(reach) > 3
            assert set(masks.flatten().tolist()) == {1, 3, NONE}     # column 0 wins its pixel over column 1
        if name not in DEGENERATE:
            assert share <= 0.5, name
        seen.add((h, w))
    assert {(33, 70), (64, 48), (65, 129), (5, 200), (70, 33), (8, 8), (16, 16), (1, 1)} <= seen
    assert 64 % GUIDED_TILE == 0 and -(-64 // GUIDED_TILE) == 1       # exactly one tile high
    assert 5 < GUIDED_HALO                                            # a strip thinner than the halo
    assert 65 - GUIDED_TILE == 1 and 129 - 2 * GUIDED_TILE == 1       # one pixel past two seams

    by = {c[0]: c for c in guided_cases()}
    # saturation: the largest candidate cost(q) + c(p,q) that the relaxation forms from the final keys.  On the one-pixel checkerboard
    # every pixel of the seed's colour is a few diagonal steps of 7 away and every other pixel one crossing of 5 + 64 * 255 = 16325
    # more, so no candidate passes 2 * 16325 + 7 * 7 = 32699: that case holds the largest single step, the bands hold two crossings
    # in a row and with them candidates beyond 32767, which a key with 15 bits of cost would wrap
    worst = {}
    for which in ("saturation", "saturation-bands"):
        name, h, w, n, edge, reach, F, src, kind, cluster = by[which]
        _, keys, _ = checked(by[which])
        guide = guided_case_inputs(by[which])[2][0].tolist()
        cost = [[v >> 16 for v in line] for line in keys[0].tolist()]
        assert all(v != KEY_NONE for line in keys[0].tolist() for v in line)
        worst[which] = max(cost[y][x] + (7 if dx and dy else 5) + edge * abs(guide[y][x] - guide[y + dy][x + dx])
                           for y in range(h) for x in range(w) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                           if (dx or dy) and 0 <= y + dy < h and 0 <= x + dx < w)
        print(f"{which}: the largest candidate is {worst[which]}, the largest cost {max(max(line) for line in cost)}")
        assert max(max(line) for line in cost) >= 16325
    assert worst["saturation-bands"] > 32767 and 16383 < worst["saturation"] <= 32699
    # degenerate cases
    assert bool((checked(by["no-column"])[0] == NONE).all())
    assert checked(by["one-pixel"])[0].tolist() == [[[int(guided_case_inputs(by["one-pixel"])[1][1, 0])]]] != [[[NONE]]]
    m, k, _ = checked(by["seeds-only"])
    assert 0 < int((m != NONE).sum()) <= 20 and bool(((k[0] >> 16)[k[0] != KEY_NONE] == 0).all())
    # the clustered columns share pixels; labels 255 and absent points are among the 257
    rows, lab, _, first = guided_case_inputs(by["n600-clustered"])
    assert len({(int(x + 0.5), int(y + 0.5)) for x, y in rows[first].tolist() if x == x and abs(x) < 1e4 and abs(y) < 1e4}) < 300
    rows, lab, _, first = guided_case_inputs(by["n257"])
    assert bool((lab[first] == NONE).any()) and bool(torch.isnan(rows[first]).any()) and bool(torch.isinf(rows[first]).any())


def test_edge_zero_is_the_chamfer_voronoi_diagram():
    h, w = 24, 31
    rows = torch.tensor([[(4.0, 5.0), (20.3, 15.8), (27.0, 2.0)]])
    lab = torch.tensor([[7, 8, 9]])
    guide = torch.randint(0, 256, (1, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    got = drivers.object_masks_guided_torch(rows[None], lab, guide, (h, w), radius=9.0, edge=0)
    seeds = [(4, 5, 7), (20, 16, 8), (27, 2, 9)]
    for y in range(h):
        for x in range(w):
            best = (10 ** 9, NONE)
            for i, (sx, sy, l) in enumerate(seeds):
                dx, dy = abs(x - sx), abs(y - sy)
                d = 7 * min(dx, dy) + 5 * (max(dx, dy) - min(dx, dy))
                if d <= 45 and (d, i) < best[:2]:
                    best = (d, i, l)
            assert int(got[0, y, x]) == best[-1], (x, y)


# ---------------------------------------------------------------------------------------------------------------- meaning
def planted_scene(seed=11):
    """a 96 x 128 image of luma 90 with the box x 41..90, y 27..69 at 150, uniform noise of +-3; tracks on the 16 px lattice from 8,
    a little off their nodes, labelled 1 inside the box and 0 outside -> (trajs (1,1,n,2), labels (1,n), guide (1,h,w), box (h,w) bool)"""
    h, w = 96, 128
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    box = (xx >= 41) & (xx <= 90) & (yy >= 27) & (yy <= 69)
    guide = (torch.where(box, 150, 90) + torch.randint(-3, 4, (h, w), generator=g)).to(torch.uint8)
    ny, nx = torch.meshgrid(torch.arange(8, h, 16), torch.arange(8, w, 16), indexing="ij")
    X, Y = nx.flatten(), ny.flatten()
    trajs = torch.stack([X + 0.375, Y - 0.25], dim=1).float()
    labels = box[Y, X].to(torch.int64)
    return trajs[None, None], labels[None], guide[None], box


def test_the_boundary_follows_the_edge_of_a_planted_box():
    """the box's outline lies up to 8 px from the halfway lines between the lattice's tracks: with edge = 0 the mask is their chamfer
    Voronoi diagram and misses the box by hundreds of pixels; with edge = 4 crossing the 60-level edge costs 240, more than any
    path inside a region needs, and the mask is the box but for what the noise moves"""
    trajs, labels, guide, box = planted_scene()
    wrong = {}
    for edge in (0, 4):
        m = drivers.object_masks_guided_torch(trajs, labels, guide, (96, 128), radius=48.0, edge=edge)
        assert not bool((m == NONE).any())
        wrong[edge] = int(((m[0] == 1) != box).sum())
    print(f"pixels that differ from the box: edge=0 {wrong[0]}, edge=4 {wrong[4]}")
    assert wrong[0] > 500 and wrong[4] <= 0.05 * wrong[0]


# ------------------------------------------------------------------------------------------------- 65535 frames a launch
PERIOD = 7                                                           # a prime that does not divide 65535 = 3 * 5 * 17 * 257
FRAME_COUNTS = (65535, 65537)
SEAM_SIZE, SEAM_EDGE, SEAM_REACH = (2, 2), 1, 100           # (reach 100: two launches, so the key planes are crossed too)


def periodic(t, F):
    """``t`` (PERIOD, ...) repeated to F entries: entry f is t[f % PERIOD]"""
    return t[torch.arange(F) % PERIOD]


def seam_inputs():
    """one period: rows (PERIOD,1,2) float32 inside the 2 x 2 frame, labels (PERIOD,1), different ones in 0..254 and one 255, guides (PERIOD,2,2) and
    RGB frames (PERIOD,3,2,2) for pips_guide_plane"""
    g = torch.Generator().manual_seed(91)
    rows = torch.rand(PERIOD, 1, 2, generator=g)
    lab = torch.randperm(255, generator=g)[:PERIOD].view(PERIOD, 1)
    lab[4, 0] = NONE
    guide = torch.randint(0, 256, (PERIOD, 2, 2), generator=g, dtype=torch.uint8)
    rgb = torch.randint(0, 256, (PERIOD, 3, 2, 2), generator=g, dtype=torch.uint8)
    return rows.float(), lab, guide, rgb


def seam_reference():
    rows, lab, guide, _ = seam_inputs()
    return drivers.object_masks_guided_torch(rows[None], lab, guide, SEAM_SIZE, radius=SEAM_REACH / 5.0, edge=SEAM_EDGE)


def test_the_frame_counts_lie_at_and_beyond_the_frames_of_a_launch():
    """masks_guided.hip cuts a call at FRAMES_A_LAUNCH frames and its guide kernel strides over the frames past GUIDE_FRAMES_Y rows of
    blocks; the periodic expectation of the GPU test is the twin over every frame at a small count, its frames differ pairwise, and
    each holds a labelled pixel or -- the one with label 255 -- none"""
    for name in ("FRAMES_A_LAUNCH", "GUIDE_FRAMES_Y"):
        value = constant(name)
        assert value == 65535 and [F > value for F in FRAME_COUNTS] == [False, True] and FRAME_COUNTS[0] == value
        assert value % PERIOD != 0 and max(FRAME_COUNTS) - value >= 2
    assert ops.guided_launches(SEAM_REACH) == 2
    rows, lab, guide, rgb = seam_inputs()
    want = seam_reference()
    F = 2 * PERIOD + 3
    whole = drivers.object_masks_guided_torch(periodic(rows, F)[None], periodic(lab, F), periodic(guide, F), SEAM_SIZE,
                                              radius=SEAM_REACH / 5.0, edge=SEAM_EDGE)
    assert torch.equal(whole, periodic(want, F))
    assert all(not torch.equal(want[a], want[b]) for a in range(PERIOD) for b in range(a))
    assert bool((want[4] == NONE).all()) and all(bool((want[f] != NONE).any()) for f in range(PERIOD) if f != 4)
    assert bool((want == NONE).any(dim=(1, 2)).sum() > 1)            # the reach cuts paths off as well
    lum = drivers.guide_plane_torch([rgb], "planar8")
    assert all(not torch.equal(lum[a], lum[b]) for a in range(PERIOD) for b in range(a))


# ------------------------------------------------------------------------------------------------------------------- guide
GUIDE_SIZE = (9, 14)


@pytest.mark.parametrize("fmt", ops.GUIDE_FORMATS)
def test_guide_twin_is_the_luma_by_a_loop_over_pixels(fmt):
    h, w = GUIDE_SIZE
    planes = views(buffers(fmt, 2, h, w, 300 + len(fmt), pad=(7, 3)), fmt, h, w)
    got = drivers.guide_plane_torch(planes, fmt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h, w)
    p = planes[0]
    for f in range(2):
        for y in range(h):
            for x in range(w):
                if fmt == "planar8":
                    r, g, b = (int(p[f, c, y, x]) for c in (0, 1, 2))
                else:
                    px = p[f, y, x].tolist()
                    r, g, b = (px[2], px[1], px[0]) if fmt.startswith("bgr") else (px[0], px[1], px[2])
                assert int(got[f, y, x]) == (77 * r + 150 * g + 29 * b + 128) >> 8
    assert not planes[0].is_contiguous()


def test_the_y_plane_is_the_guide_without_a_copy():
    for fmt in ("nv12", "i420"):
        planes = views(buffers(fmt, 2, 9, 14, 7), fmt, 9, 14)
        for fn in (drivers.guide_plane_torch, drivers.guide_plane):
            g = fn(planes, fmt)
            assert g.data_ptr() == planes[0].data_ptr() and g.stride() == planes[0].stride() and tuple(g.shape) == (2, 9, 14)
    for fmt in ("p010", "i010", "yuv"):
        with pytest.raises(ValueError):
            drivers.guide_plane_torch([torch.zeros(1, 4, 4, dtype=torch.int16), torch.zeros(1, 2, 2, 2, dtype=torch.int16)], fmt)


# ------------------------------------------------------------------------------------------------- the library on the CPU
def test_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pips_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pips_object_masks_guided_workspace_bytes", "pips_object_masks_guided", "pips_guide_plane"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "masks_guided.hip" in _build.SOURCES


E_ARG = -1
GUIDED_GOOD = dict(trajs=0x3000, labels=0x4000, G=5, n=3, first=1, F=2, src_h=10, src_w=12, h=10, w=12, edge=4, reach=240, guide=0x6000,
                   guide_pitch=12, guide_step=120, mask=0x1000, pitch=12, step=120, workspace=0x5000, workspace_bytes=1 << 20, stream=None)


def test_object_masks_guided_rejects_bad_arguments_ahead_of_any_launch():
    """every PIPS_E_ARG case of the header through the loaded library: the pointers are never followed (nothing is launched), so this
    runs without a device; F = 0 launches nothing and returns PIPS_OK"""
    from pips_amd import _lib
    lib = _lib.load()
    rc = lambda **change: lib.pips_object_masks_guided(*[dict(GUIDED_GOOD, **change)[k] for k in GUIDED_GOOD])
    size = lib.pips_object_masks_guided_workspace_bytes
    need = size(2, 3, 10, 12)
    assert need == 48 + 2 * 4 * 2 * 10 * 12 and size(1, 3, 10, 12) == 32 + 2 * 4 * 10 * 12             # (24 bytes of records round up to 32)
    assert size(0, 3, 10, 12) == 0 and size(2, 0, 10, 12) == 0 and size(-1, 3, 10, 12) == 0 and size(2, -1, 10, 12) == 0
    assert size(2, 65537, 10, 12) == 0 and size(2, 3, 0, 12) == 0 and size(2, 3, 10, 8193) == 0
    assert size(1, 65536, 8192, 8192) == 8 * 65536 + 2 * 4 * 8192 * 8192
    assert rc(F=0) == 0 and rc(F=0, first=5) == 0
    assert rc(F=0, mask=None, trajs=None, labels=None, guide=None, workspace=None, workspace_bytes=0) == 0
    assert rc(F=0, edge=64, reach=32767, h=8192, w=8192, pitch=8192) == 0 and rc(F=0, edge=0, reach=0) == 0
    bad = [dict(F=-1), dict(n=-1), dict(G=-1), dict(n=65537), dict(h=0), dict(w=0), dict(src_h=0), dict(src_w=0),
           dict(h=8193, step=8193 * 12, guide_step=8193 * 12), dict(w=8193, pitch=8193, step=81930, guide_pitch=8193, guide_step=81930),
           dict(edge=-1), dict(edge=65), dict(reach=-1), dict(reach=32768), dict(first=-1), dict(first=4), dict(G=2), dict(pitch=11),
           dict(step=119), dict(mask=None), dict(trajs=None), dict(labels=None), dict(guide=None), dict(guide_pitch=11), dict(guide_step=119),
           dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=0x5008), dict(workspace=0x5004)]
    for change in bad:
        assert rc(**change) == E_ARG, change
        assert lib.pips_last_error().decode().startswith("object_masks_guided:"), change
    assert rc(n=0, mask=None) == E_ARG                               # n = 0 still writes the images


PLANE_GOOD = dict(format=8, F=2, h=10, w=12, p0=0x1000, pitch0=12, step0=120, p1=0x2000, pitch1=12, step1=120, p2=0x3000, pitch2=12,
                  step2=120, guide=0x4000, guide_pitch=12, guide_step=120, stream=None)


def test_guide_plane_rejects_bad_arguments_ahead_of_any_launch():
    from pips_amd import _lib
    lib = _lib.load()
    rc = lambda **change: lib.pips_guide_plane(*[dict(PLANE_GOOD, **change)[k] for k in PLANE_GOOD])
    assert rc(F=0) == 0 and rc(F=0, p0=None, p1=None, p2=None, guide=None) == 0
    assert rc(F=0, format=0, pitch0=36, step0=360) == 0 and rc(F=0, format=3, pitch0=48, step0=480) == 0
    bad = [dict(format=4), dict(format=5), dict(format=6), dict(format=7), dict(format=9), dict(format=-1), dict(F=-1), dict(h=0), dict(w=0),
           dict(h=8193, step0=8193 * 12, step1=8193 * 12, step2=8193 * 12, guide_step=8193 * 12),
           dict(w=8193, pitch0=8193, pitch1=8193, pitch2=8193, guide_pitch=8193, step0=81930, step1=81930, step2=81930, guide_step=81930),
           dict(pitch0=11), dict(pitch1=11), dict(pitch2=11), dict(step0=119), dict(step2=119), dict(guide_pitch=11), dict(guide_step=119),
           dict(p0=None), dict(p1=None), dict(p2=None), dict(guide=None), dict(format=0, pitch0=35), dict(format=2, pitch0=47),
           dict(format=1, pitch0=36, step0=359)]
    for change in bad:
        assert rc(**change) == E_ARG, change
        assert lib.pips_last_error().decode().startswith("guide_plane:"), change
    assert rc(format=0, F=0, p1=None, p2=None, pitch0=36, step0=360, pitch1=0, step1=0, pitch2=0, step2=0) == 0        # one plane alone


def test_python_layers_reject_bad_shapes_and_values():
    t, lab, guide = torch.zeros(1, 3, 4, 2), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 8, 8, dtype=torch.uint8)
    assert tuple(drivers.object_masks_guided_torch(t, lab, guide, (8, 8)).shape) == (3, 8, 8)
    assert tuple(drivers.object_masks_guided_torch(t, lab, guide[1:], (8, 8), first=1).shape) == (2, 8, 8)
    for args, kw in (((t[0], lab, guide, (8, 8)), {}), ((t, lab[:2], guide, (8, 8)), {}), ((t, lab, guide[:2], (8, 8)), {}),
                     ((t, lab, guide.float(), (8, 8)), {}), ((t, lab, guide[:, :7], (8, 8)), {}), ((t, lab, None, (8, 8)), {}),
                     ((t, lab, guide, (8, 8)), dict(out_size=(8, 9))), ((t, lab, guide, (8, 8)), dict(radius=-1.0)),
                     ((t, lab, guide, (8, 8)), dict(radius=6553.5)), ((t, lab, guide, (8, 8)), dict(edge=65)),
                     ((t, lab, guide, (8, 8)), dict(edge=-1)), ((t, lab, guide, (8, 8)), dict(edge=1.5)),
                     ((t, lab, guide, (8, 8)), dict(first=4)), ((t, lab, guide, (8, 8)), dict(first=1))):
        with pytest.raises(ValueError):
            drivers.object_masks_guided_torch(*args, **kw)
    with pytest.raises(ValueError):
        ops.object_masks_guided(t[0], lab, guide, (8, 8))            # labels of the library are uint8
    for bad in ("nv12", "p010", "yuv"):
        with pytest.raises(ValueError):
            ops.guide_check([torch.zeros(1, 4, 4, 3, dtype=torch.uint8)], bad)
    with pytest.raises(ValueError):
        ops.guide_check([torch.zeros(1, 4, 4, 4, dtype=torch.uint8)], "rgb24")
