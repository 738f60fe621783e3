"""CPU: object masks -- drivers.object_masks_torch and drivers.tint_masks_torch, the torch twins of pips_object_masks and
pips_masks_tint (include/pips_hip.h), against the two rules restated here as plain loops over pixels and columns on Python
integers; the cases the header names; what a mask means on a planted scene; object_colors; every PIPS_E_ARG case of both entries
through the loaded library (nothing is launched).  The cases of tests/test_masks_gpu.py are made here, and the twin's output on
them is checked not to be vacuous.  (The kernels: tests/test_masks_gpu.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pips_amd import drivers, ops
from test_draw import FORMATS, MATRICES, RANGES, SENTINEL, buffers, outside_untouched, views
from test_motion_layers import SCENE_SEEDS, _meaning_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NONE = 255
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the rules as plain loops
def _quantise(v, n_src, n_dst):
    """one coordinate -> eighths of a pixel of the n_dst wide axis, None when the point is absent; every operation rounded to fp32"""
    v = f32(v)
    if n_src != n_dst:
        s = f32(n_dst) / f32(n_src)
        v = f32(f32(f32(v + f32(0.5)) * s) - f32(0.5))
    if not abs(v) <= 32768.0:
        return None
    return int(math.floor(f32(f32(v * f32(8.0)) + f32(0.5))))


def rule_masks(rows, labels, size, src, radius8, vote, first):
    """pips_object_masks by loops: rows (G,n,2) float32, labels (G,n) lists of ints 0..255 -> F lists of h lists of w labels"""
    (h, w), (src_h, src_w) = size, src
    rows = rows.tolist()
    out = []
    for r in range(first, len(rows)):
        part = []
        for i, (x, y) in enumerate(rows[r]):
            qx, qy = _quantise(x, src_w, w), _quantise(y, src_h, h)
            if qx is not None and qy is not None and labels[r][i] != NONE:
                part.append((qx, qy, i, labels[r][i]))
        frame = []
        for Y in range(h):
            line = []
            for X in range(w):
                cand = []
                for qx, qy, i, lab in part:
                    dx, dy = 8 * X - qx, 8 * Y - qy
                    if abs(dx) <= radius8 and abs(dy) <= radius8 and dx * dx + dy * dy <= radius8 * radius8:
                        cand.append((dx * dx + dy * dy, i, lab))
                voters = sorted(cand)[:vote]
                best, most = NONE, 0
                for _, _, lab in voters:                           # in key order: a strict comparison keeps the smallest key
                    c = sum(1 for v in voters if v[2] == lab)
                    if c > most:
                        best, most = lab, c
                line.append(best)
            frame.append(line)
        out.append(frame)
    return out


def _twin(rows, labels, size, src=None, radius8=384, vote=1, first=0):
    """object_masks_torch on (G,n,2) rows with the radius in eighths"""
    return drivers.object_masks_torch(rows[None], torch.as_tensor(labels), src or size, out_size=size, radius=radius8 / 8.0, vote=vote,
                                      first=first)


def mask_tracks(G, n, h, w, seed, src=None, cluster=False):
    """Seeded positions (G,n,2) float32 for an h x w mask (coordinates of a ``src`` image when given) and labels (G,n) in 0..3 with
    some 255: uniform over the image and 3 px around it, or with ``cluster`` all inside the first 12 x 12 pixels.  From three
    columns on, column 1 is a NaN, 2 lies beyond 32768; from five on, 3 is at -inf and 4 carries the label 255."""
    g = torch.Generator().manual_seed(seed)
    H, W = (h, w) if src is None else src
    if cluster:
        t = torch.rand(G, n, 2, generator=g) * torch.tensor([12.0 * W / w, 12.0 * H / h])
    else:
        t = torch.rand(G, n, 2, generator=g) * torch.tensor([(w + 6.0) * W / w, (h + 6.0) * H / h]) - 3.0
    lab = torch.randint(0, 4, (G, n), generator=g)
    lab[torch.rand(G, n, generator=g) < 0.05] = NONE
    if n >= 3:
        t[:, 1, 0], t[:, 2, 1] = NAN, 40000.0
    if n >= 5:
        t[:, 3, 0], lab[:, 4] = -INF, NONE
    return t.float(), lab


# ---------------------------------------------------------------------------------------------------------- twin == loops
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (17, 33), (32, 48)])
@pytest.mark.parametrize("n", [0, 1, 3, 40])
def test_twin_is_the_rule_by_plain_loops(size, n):
    h, w = size
    for vote in (1, 3, 5):
        for src in (None, (2 * h + 1, 3 * w)):
            rows, lab = mask_tracks(3, n, h, w, 100 * h + n + vote, src)
            radius8 = 8 * 5 + 3
            want = rule_masks(rows, lab.tolist(), size, src or size, radius8, vote, 1)
            got = _twin(rows, lab, size, src, radius8, vote, first=1)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h, w)
            assert got.tolist() == want, (size, n, vote, src)


# ------------------------------------------------------------------------------------------------------------ named cases
def _one(points, labels, size=(9, 9), radius8=24, vote=1):
    rows = torch.tensor(points, dtype=torch.float32).view(1, -1, 2)
    return _twin(rows, torch.tensor([labels]), size, None, radius8, vote)[0]


def test_equal_distance_goes_to_the_lower_column():
    assert int(_one([(3, 4), (5, 4)], [7, 9])[4, 4]) == 7 and int(_one([(5, 4), (3, 4)], [9, 7])[4, 4]) == 9


def test_a_vote_tie_goes_to_the_nearest():
    m = _one([(4, 4), (6, 4)], [1, 2], vote=2)                    # one vote each everywhere within reach of both
    assert int(m[4, 4]) == 1 and int(m[4, 6]) == 2 and int(m[4, 5]) == 1          # (4, 5): equal distance, the lower column
    m3 = _one([(4, 4), (5, 4), (6, 4)], [1, 2, 2], vote=3)
    assert int(m3[4, 4]) == 2                                     # two votes against the nearest one


def test_the_radius_is_inclusive():
    m = _one([(4.0, 4.0)], [3], radius8=16)
    assert int(m[4, 6]) == 3 and int(m[4, 2]) == 3 and int(m[6, 4]) == 3 and int(m[4, 7]) == NONE
    assert int(m[5, 6]) == NONE                                   # inside the box of the radius, outside the circle
    m = _one([(4.125, 4.0)], [3], radius8=16)                     # one eighth further: (4, 2) is 17 eighths away
    assert int(m[4, 2]) == NONE and int(m[4, 6]) == 3


def test_radius_zero_labels_the_centres_tracks_sit_on():
    m = _one([(2.0, 3.0), (5.125, 5.0), (6.04, 6.0)], [1, 2, 3], radius8=0)
    assert int(m[3, 2]) == 1 and int(m[6, 6]) == 3 and int((m != NONE).sum()) == 2   # (5.125 is an eighth off; 6.04 rounds onto 6)


def test_absent_points_and_the_label_255_take_no_part():
    pts = [(4, 4), (NAN, 4), (4, INF), (-INF, 4), (40000.0, 4), (4, -32768.5), (4, 4)]
    m = _one(pts, [NONE, 1, 2, 3, 4, 5, 6])
    assert set(m.flatten().tolist()) == {6, NONE}
    assert bool((_one(pts[:6], [NONE, 1, 2, 3, 4, 5]) == NONE).all())       # a frame with no participant
    assert bool((_twin(torch.zeros(1, 0, 2), torch.zeros(1, 0, dtype=torch.int64), (4, 6)) == NONE).all())
    # values outside 0..254 of a wider dtype take no part either: motion_layers' -1 and -2
    rows = torch.tensor([[(4.0, 4.0), (4.0, 4.0), (4.0, 4.0), (5.0, 4.0)]])
    m = drivers.object_masks_torch(rows[None], torch.tensor([[-1, -2, 300, 8]]), (9, 9), radius=2.0)
    assert set(m.flatten().tolist()) == {8, NONE}


def test_a_vote_larger_than_the_candidates_uses_what_there_is():
    assert int(_one([(4, 4), (20, 20)], [5, 6], size=(24, 24), vote=5)[4, 4]) == 5
    m = _one([(4, 4), (5, 4), (30, 30)], [5, 6, 6], size=(32, 32), vote=5)
    assert int(m[4, 4]) == 5 and int(m[4, 5]) == 6               # one vote each: the nearest


# ------------------------------------------------------------------------------------------------------------------- tint
def rule_tint(planes, fmt, masks, colors, alpha, matrix, range_):
    """pips_masks_tint by loops, in place on ``planes`` (uint8 tensors of draw's shapes); alpha: ints 0..256"""
    F, h, w = masks.shape
    C = colors.shape[1]
    yuv = fmt in ("nv12", "i420")
    y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB_RULES[(matrix, range_)]
    clamp = lambda v: min(max(v, 0), 255)
    for f in range(F):
        comp = []
        for R, G, B in colors[f].tolist():
            comp.append((y0 + ((yr * R + yg * G + yb * B + 32768) >> 16), clamp(128 + ((ur * R + ug * G + ub * B + 32768) >> 16)),
                         clamp(128 + ((vr * R + vg * G + vb * B + 32768) >> 16))) if yuv else (R, G, B))
        lab = masks[f].tolist()
        A = [[alpha[f][l] if l < C else 0 for l in row] for row in lab]
        for y in range(h):
            for x in range(w):
                a = A[y][x]
                if a == 0:
                    continue
                c = comp[lab[y][x]]
                for k in range(1 if yuv else 3):
                    if fmt == "planar8":
                        at = planes[0][f, k, y]
                        i = x
                    elif yuv:
                        at, i = planes[0][f, y], x
                    else:
                        at, i = planes[0][f, y, x], (2 - k if fmt in ("bgr24", "bgra32") else k)
                    at[i] = (int(at[i]) * (256 - a) + c[k] * a + 128) >> 8
        if yuv:
            for cy in range((h + 1) // 2):
                for cx in range((w + 1) // 2):
                    px = [(y, x) for y in (2 * cy, 2 * cy + 1) for x in (2 * cx, 2 * cx + 1) if y < h and x < w]
                    SA = sum(A[y][x] for y, x in px)
                    if SA == 0:
                        continue
                    for k in (1, 2):
                        S = sum(comp[lab[y][x]][k] * A[y][x] for y, x in px if A[y][x])
                        at, i = (planes[1][f, cy, cx], k - 1) if fmt == "nv12" else (planes[k][f, cy], cx)
                        at[i] = (int(at[i]) * (1024 - SA) + S + 512) >> 10


def tint_inputs(case):
    """-> (surface buffers, the mask's buffer, colors (F,C,3), alpha ints (F,C)) of a tint case (fmt, matrix, range, h, w, C): F = 2
    pitched and stepped surfaces (test_draw.buffers), a pitched mask with labels 0 .. C + 1 and 255 drawn per pixel, a quarter of
    the opacities 0 and one 256"""
    fmt, matrix, range_, h, w, C = case
    seed = 7000 + 100 * h + w + C + FORMATS.index(fmt)
    g = torch.Generator().manual_seed(seed)
    F = 2
    mbuf = torch.full((F, h + 3, w + 5), SENTINEL, dtype=torch.uint8)
    lab = torch.randint(0, min(C + 2, 256), (F, h, w), generator=g)
    lab[torch.rand(F, h, w, generator=g) < 0.1] = NONE
    mbuf[:, :h, :w] = lab.to(torch.uint8)
    colors = torch.randint(0, 256, (F, C, 3), generator=g, dtype=torch.uint8)
    alpha = torch.randint(1, 256, (F, C), generator=g)
    alpha[torch.rand(F, C, generator=g) < 0.25] = 0
    alpha[0, 0], alpha[1, C - 1] = 256, 77
    if C > 1:
        colors[0, 1] = torch.tensor([90, 90, 90], dtype=torch.uint8)          # a grey
    return buffers(fmt, F, h, w, seed + 1), mbuf, colors, alpha


def tint_cases():
    """every format at 16x16, 17x15 and 33x70 with C cycling through 1, 4, 255; NV12 and I420 under every matrix and range"""
    out, k = [], 0
    for fmt in FORMATS:
        for h, w in ((16, 16), (17, 15), (33, 70)):
            out.append((fmt, "bt709", "limited", h, w, (1, 4, 255)[k % 3]))
            k += 1
    for fmt in ("nv12", "i420"):
        for i, (m, r) in enumerate((m, r) for m in MATRICES for r in RANGES):
            if (m, r) != ("bt709", "limited"):
                out.append((fmt, m, r, (17, 33, 16)[i % 3], (15, 70, 16)[i % 3], 4))
    return out


def tint_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("fmt", FORMATS)
def test_tint_twin_is_the_rule_by_plain_loops(fmt):
    for (h, w), C, matrix, range_ in (((5, 7), 4, "bt601", "full"), ((9, 13), 255, "bt709", "limited"), ((4, 6), 1, "bt709", "full")):
        bufs, mbuf, colors, alpha = tint_inputs((fmt, matrix, range_, h, w, C))
        before = [b.clone() for b in bufs]
        masks = mbuf[:, :h, :w]
        want = [p.clone() for p in views(bufs, fmt, h, w)]
        rule_tint(want, fmt, masks, colors, alpha.tolist(), matrix, range_)
        got = drivers.tint_masks_torch(views(bufs, fmt, h, w), fmt, masks, colors, alpha / 256.0, matrix, range_, inplace=True)
        got = [got] if torch.is_tensor(got) else got
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (fmt, h, w, C)
        assert any(not torch.equal(a, b) for a, b in zip(bufs, before))
        assert outside_untouched(bufs, before, fmt, h, w)           # padding, gaps and the alpha byte
        assert bool((mbuf[:, h:] == SENTINEL).all() and (mbuf[:, :, w:] == SENTINEL).all())


@pytest.mark.parametrize("fmt", FORMATS)
def test_tint_leaves_what_has_no_weight(fmt):
    h, w, C = 7, 9, 3
    bufs, mbuf, colors, alpha = tint_inputs((fmt, "bt709", "limited", h, w, C))
    planes = views(bufs, fmt, h, w)
    masks = mbuf[:, :h, :w].clone()
    out = drivers.tint_masks_torch(planes, fmt, masks, colors, torch.zeros(2, C))
    assert all(torch.equal(a, b) for a, b in zip([out] if torch.is_tensor(out) else out, planes))         # alpha 0
    masks[...] = torch.where(masks < C, masks + C, masks)           # every label >= C, 255 among them
    assert int(masks.min()) >= C and bool((masks == NONE).any())
    out = drivers.tint_masks_torch(planes, fmt, masks, colors, torch.ones(2, C))
    assert all(torch.equal(a, b) for a, b in zip([out] if torch.is_tensor(out) else out, planes))


def test_grey_on_nv12_gives_chroma_128():
    h, w = 6, 8
    planes = views(buffers("nv12", 1, h, w, 3), "nv12", h, w)
    out = drivers.tint_masks_torch(planes, "nv12", torch.zeros(1, h, w, dtype=torch.uint8), torch.full((1, 1, 3), 200, dtype=torch.uint8),
                                   torch.ones(1, 1), "bt601", "limited")
    assert bool((out[1] == 128).all()) and bool((out[0] == 16 + ((56284 * 200 + 32768) >> 16)).all())


# ---------------------------------------------------------------------------------------------------------------- meaning
GRID, JITTER = 16, 0.45
MEANING_SCENES = (((14.0, -9.0), 1), ((-11.0, 12.0), 2), ((0.0, 15.0), 3))       # the object's shift of a pair, the seed


def meaning_scene(shift, seed, H=240, W=320):
    """One pair of frames.  In the second frame a track sits on every node (16 i + 8, 16 j + 8) of a grid over H x W, each off its node
    by less than JITTER px an axis.  The tracks of the nodes i in 6..10, j in 4..8 came there by ``shift``, all others stood still
    (0.05 px of noise on the first frame) -> (trajs (2,n,2) float32, object (n,) bool, the rectangle (x0, y0, x1, y1) of the
    object's nodes).  The mask is made from the second frame alone, so the first may put the object on top of other tracks."""
    g = torch.Generator().manual_seed(seed)
    jj, ii = torch.meshgrid(torch.arange(H // GRID), torch.arange(W // GRID), indexing="ij")
    node = torch.stack([ii.flatten() * GRID + 8.0, jj.flatten() * GRID + 8.0], dim=1).double()
    obj = ((ii >= 6) & (ii <= 10) & (jj >= 4) & (jj <= 8)).flatten()
    q = node + (torch.rand(node.shape, generator=g, dtype=torch.float64) - 0.5) * 2 * JITTER
    p = q + (torch.rand(node.shape, generator=g, dtype=torch.float64) - 0.5) * 0.1
    p[obj] -= torch.tensor(shift, dtype=torch.float64)
    return torch.stack([p, q]).float(), obj, (6 * GRID + 8, 4 * GRID + 8, 10 * GRID + 8, 8 * GRID + 8)


@pytest.mark.parametrize("shift,seed", MEANING_SCENES)
def test_the_mask_of_a_moving_rectangle(shift, seed):
    """Labels from motion_layers_torch, vote = 1: the mask is the Voronoi diagram of the tracks.  A pixel at most 7 px outside the
    rectangle R of the object's nodes has an object node at nominal offsets (a, t), a <= 7, |t| <= 8, and every other track at
    least (16 - a, t) away; with every track less than j = JITTER off its node the object's track is nearer as long as
    (16 - a - j)^2 - (a + j)^2 > (|t| + j)^2 - (|t| - j)^2, i.e. 32 - 32 j > 32 j at a = 7, |t| = 8: j < 0.5 (at a corner, offsets
    (7, 7): 60 j < 32).  By the same count from the other side a pixel 10 px or more outside R is nearer to a track that is not the
    object's.  So the object's mask contains R grown by 8 - 1 px and lies inside R grown by 8 + 1 px."""
    assert JITTER < 0.5
    trajs, obj, (x0, y0, x1, y1) = meaning_scene(shift, seed)
    H, W = 240, 320
    labels = drivers.motion_layers_torch(trajs[None], thr=2.0, hypotheses=256, layers=3, min_inliers=8)[2]        # (1,n)
    mine = set(labels[0][obj].tolist())
    assert len(mine) == 1 and min(mine) >= 1 and bool((labels[0][~obj] == 0).all())
    mask = drivers.object_masks_torch(trajs[None, 1:], labels, (H, W), vote=1) == mine.pop()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grown = lambda d: (xx >= x0 - d) & (xx <= x1 + d) & (yy >= y0 - d) & (yy <= y1 + d)
    assert bool((mask[0] <= grown(9)).all()) and bool((mask[0] >= grown(7)).all())
    assert int(mask.sum()) > 0 and not bool(mask.all())


def test_object_colors_follow_the_object():
    """on test_motion_layers' scene an object's colour is the same on every pair, whatever layer carries it; the camera and a layer
    without a model are transparent"""
    trajs, group = _meaning_scene(64, SCENE_SEEDS[64])
    _, _, labels, object_ids, objects, _ = drivers.motion_layers_torch(trajs[None], thr=2.0, hypotheses=256, seed=0, layers=4, min_inliers=8)
    colors, alpha = drivers.object_colors(object_ids, alpha=0.5, camera_alpha=0.0)
    P, L = object_ids.shape
    assert tuple(colors.shape) == (P, L, 3) and colors.dtype == torch.uint8 and tuple(alpha.shape) == (P, L)
    for b in (1, 2):
        layer = [int(labels[f][group == b][0]) for f in range(P)]
        seen = {tuple(colors[f, layer[f]].tolist()) for f in range(P)}
        assert len(seen) == 1 and all(float(alpha[f, layer[f]]) == 0.5 for f in range(P))
        assert seen.pop() == tuple(drivers.track_colors(objects[0][group == b][:1])[0].tolist())
    assert bool((alpha[object_ids == 0] == 0).all()) and bool((alpha[object_ids < 0] == 0).all()) and bool((object_ids < 0).any())
    assert float(drivers.object_colors(object_ids, camera_alpha=0.25)[1][0, 0]) == 0.25
    for bad in (dict(alpha=1.5), dict(camera_alpha=-0.1)):
        with pytest.raises(ValueError):
            drivers.object_colors(object_ids, **bad)
    with pytest.raises(ValueError):
        drivers.object_colors(object_ids.float())


# ------------------------------------------------------------------------------------------------- the cases of the GPU file
def mask_cases():
    """(h, w, n, radius8, vote, F, src, cluster): every size, column count, radius, vote and F of the GPU grid at least once -- the
    counts around a wave (63, 64, 65) and around a chunk of 256 (255, 256, 257), 600 columns clustered into one tile so that its
    list passes two chunks, a one-pixel image, sizes that are no multiple of the tile or of four"""
    return [(1, 1, 1, 24, 1, 1, None, False), (1, 1, 63, 2048, 5, 3, None, False), (16, 16, 0, 24, 1, 3, None, False),
            (16, 16, 64, 24, 2, 1, None, False), (16, 16, 255, 1, 3, 1, None, False), (17, 15, 65, 24, 3, 3, None, False),
            (17, 15, 1, 2048, 1, 1, None, False), (17, 15, 256, 0, 1, 1, None, False), (33, 70, 257, 24, 4, 1, (24, 32), False),
            (33, 70, 63, 2048, 3, 3, None, False), (33, 70, 64, 1, 5, 1, None, False), (33, 70, 600, 24, 1, 1, None, False),
            (64, 48, 600, 24, 5, 1, None, True), (64, 48, 600, 2048, 3, 1, None, True), (64, 48, 255, 24, 2, 3, (96, 64), False),
            (64, 48, 257, 0, 4, 1, None, False), (64, 48, 65, 24, 1, 3, None, False)]


def mask_case_id(c):
    h, w, n, radius8, vote, F, src, cluster = c
    return f"{h}x{w}-n{n}-r{radius8}-v{vote}-F{F}" + ("" if src is None else f"-from{src[0]}x{src[1]}") + ("-clustered" if cluster else "")


def mask_case_inputs(c):
    """-> (rows (G,n,2), labels (G,n) int64, first): G = F + 2 rows, first = 1, so that a row lies before and one behind the call's"""
    h, w, n, radius8, vote, F, src, cluster = c
    rows, lab = mask_tracks(F + 2, n, h, w, 31 * h + 7 * w + n + radius8 + vote, src, cluster)
    return rows, lab, 1


def tile_candidates(rows, lab, r, size, src, radius8):
    """the participating columns of row ``r`` within reach of each MASK_TILE tile: what a raster block of masks.hip compacts"""
    (h, w), (src_h, src_w) = size, src
    qx, okx = drivers._draw_quantise(rows[r, :, 0], src_w, w)
    qy, oky = drivers._draw_quantise(rows[r, :, 1], src_h, h)
    part = okx & oky & (lab[r] != NONE)
    T = ops.MASK_TILE
    out = []
    for Y0 in range(0, h, T):
        for X0 in range(0, w, T):
            out.append(int((part & (qx >= 8 * X0 - radius8) & (qx <= 8 * min(X0 + T - 1, w - 1) + radius8) & (qy >= 8 * Y0 - radius8) &
                            (qy <= 8 * min(Y0 + T - 1, h - 1) + radius8)).sum()))
    return out


def test_the_gpu_cases_are_not_vacuous():
    """of the masks of the GPU grid: pixels of at least three labels and of 255, a pixel where vote 3 differs from vote 1, a tile
    with more than 512 candidate columns and a tile with none, every value of the grid; of the tint cases: a chroma sample whose
    four pixels carry different labels"""
    labels_seen, most, fewest, votes_differ = set(), 0, None, False
    seen = {k: set() for k in ("size", "n", "radius8", "vote", "F")}
    for c in mask_cases():
        h, w, n, radius8, vote, F, src, cluster = c
        for k, v in zip(("size", "n", "radius8", "vote", "F"), ((h, w), n, radius8, vote, F)):
            seen[k].add(v)
        rows, lab, first = mask_case_inputs(c)
        assert first > 0 and rows.shape[0] > first + F
        m = _twin(rows[:first + F], lab[:first + F], (h, w), src, radius8, vote, first)
        labels_seen |= set(m.flatten().tolist())
        if vote == 3:
            votes_differ |= bool((m != _twin(rows[:first + F], lab[:first + F], (h, w), src, radius8, 1, first)).any())
        for k in range(F):
            t = tile_candidates(rows, lab, first + k, (h, w), src or (h, w), radius8)
            most, fewest = max(most, max(t)), min(t) if fewest is None or n > 0 and min(t) < fewest else fewest
            if n == 600 and cluster and radius8 == 24:
                assert max(t) > 512 and min(t) == 0
    assert len(labels_seen - {NONE}) >= 3 and NONE in labels_seen and votes_differ and most > 512 and fewest == 0
    assert seen["size"] == {(1, 1), (16, 16), (17, 15), (33, 70), (64, 48)} and seen["n"] == {0, 1, 63, 64, 65, 255, 256, 257, 600}
    assert seen["radius8"] == {0, 1, 24, 2048} and seen["vote"] == {1, 2, 3, 4, 5} and seen["F"] == {1, 3}
    cases = tint_cases()
    assert {c[0] for c in cases} == set(FORMATS) and {c[5] for c in cases} == {1, 4, 255}
    assert {(c[3], c[4]) for c in cases} == {(16, 16), (17, 15), (33, 70)}
    assert {(c[1], c[2]) for c in cases if c[0] in ("nv12", "i420")} == {(m, r) for m in MATRICES for r in RANGES}
    four = False
    for c in cases:
        if c[0] in ("nv12", "i420"):
            _, mbuf, _, _ = tint_inputs(c)
            q = mbuf[:, :c[3] // 2 * 2, :c[4] // 2 * 2].view(2, c[3] // 2, 2, c[4] // 2, 2).permute(0, 1, 3, 2, 4).reshape(-1, 4)
            four |= bool(((q[:, 0] != q[:, 1]) & (q[:, 0] != q[:, 2]) & (q[:, 0] != q[:, 3]) & (q[:, 1] != q[:, 2]) & (q[:, 1] != q[:, 3]) &
                          (q[:, 2] != q[:, 3])).any())
    assert four


# ------------------------------------------------------------------------------------------------- the library on the CPU
def test_declared_bound_and_exported():
    from pips_amd import _build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pips_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pips_object_masks_workspace_bytes", "pips_object_masks", "pips_masks_tint"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "masks.hip" in _build.SOURCES
    for name, value in (("PIPS_MASK_NONE", ops.MASK_NONE), ("PIPS_MASK_RADIUS8_MAX", ops.MASK_RADIUS8_MAX), ("PIPS_MASK_VOTE_MAX", ops.MASK_VOTE_MAX),
                        ("PIPS_MASK_N_MAX", ops.MASK_N_MAX), ("PIPS_MASK_LABELS_MAX", ops.MASK_LABELS_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert (ops.MASK_NONE, ops.MASK_RADIUS8_MAX, ops.MASK_VOTE_MAX, ops.MASK_N_MAX) == (255, 2048, 5, 65536)


E_ARG = -1
MASKS_GOOD = dict(trajs=0x3000, labels=0x4000, G=5, n=3, first=1, F=2, src_h=10, src_w=12, h=10, w=12, radius8=384, vote=1, mask=0x1000,
                  pitch=12, step=120, workspace=0x5000, workspace_bytes=1 << 20, stream=None)


def test_object_masks_rejects_bad_arguments_ahead_of_any_launch():
    """every PIPS_E_ARG case of the header through the loaded library: the pointers are never followed (nothing is launched), so this
    runs without a device; F = 0 launches nothing and returns PIPS_OK"""
    from pips_amd import _lib
    lib = _lib.load()
    rc = lambda **change: lib.pips_object_masks(*[dict(MASKS_GOOD, **change)[k] for k in MASKS_GOOD])
    need = lib.pips_object_masks_workspace_bytes(2, 3)
    assert need == 8 * 2 * 3 and lib.pips_object_masks_workspace_bytes(0, 3) == 0 and lib.pips_object_masks_workspace_bytes(2, 0) == 0
    assert lib.pips_object_masks_workspace_bytes(-1, 3) == 0 and lib.pips_object_masks_workspace_bytes(2, -1) == 0
    assert lib.pips_object_masks_workspace_bytes(2, 65537) == 0 and lib.pips_object_masks_workspace_bytes(1, 65536) == 8 * 65536
    assert rc(F=0) == 0 and rc(F=0, first=5) == 0 and rc(F=0, mask=None, trajs=None, labels=None, workspace=None, workspace_bytes=0) == 0
    assert rc(F=0, radius8=2048, vote=5, h=8192, w=8192, pitch=8192) == 0 and rc(F=0, radius8=0) == 0
    bad = [dict(F=-1), dict(n=-1), dict(G=-1), dict(n=65537), dict(h=0), dict(w=0), dict(src_h=0), dict(src_w=0),
           dict(h=8193, step=8193 * 12), dict(w=8193, pitch=8193, step=81930), dict(radius8=-1), dict(radius8=2049), dict(vote=0),
           dict(vote=6), dict(first=-1), dict(first=4), dict(G=2), dict(pitch=11), dict(step=119), dict(mask=None), dict(trajs=None),
           dict(labels=None), dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=0x5008), dict(workspace=0x5004)]
    for change in bad:
        assert rc(**change) == E_ARG, change
        assert lib.pips_last_error().decode().startswith("object_masks:"), change
    assert rc(n=0, mask=None) == E_ARG                               # n = 0 still writes the images


TINT_GOOD = dict(format=4, matrix=1, range=0, F=2, h=10, w=12, p0=0x1000, pitch0=12, step0=120, p1=0x2000, pitch1=12, step1=60, p2=None,
                 pitch2=0, step2=0, mask=0x3000, mask_pitch=12, mask_step=120, colors=0x4000, alpha=None, C=3, stream=None)


def test_masks_tint_rejects_bad_arguments_ahead_of_any_launch():
    from pips_amd import _lib
    lib = _lib.load()
    table = lambda *v: (ctypes.c_int * len(v))(*v)
    ok = table(0, 256, 128, 1, 2, 3)

    def rc(**change):
        a = dict(TINT_GOOD, alpha=ok)
        a.update(change)
        return lib.pips_masks_tint(*[a[k] for k in TINT_GOOD])
    assert rc(F=0) == 0 and rc(F=0, p0=None, p1=None, mask=None, colors=None, alpha=None) == 0
    assert rc(F=0, format=0, matrix=7, range=7, pitch0=36, step0=360) == 0          # matrix and range: the YCbCr formats alone
    assert rc(F=0, C=255) == 0 and rc(F=0, h=8192, w=8192, pitch0=8192, pitch1=8192, mask_pitch=8192) == 0
    bad = [dict(format=6), dict(format=7), dict(format=9), dict(format=-1), dict(matrix=2), dict(matrix=-1), dict(range=2), dict(range=-1),
           dict(F=-1), dict(h=0), dict(w=0), dict(h=8193, step0=8193 * 12, step1=4097 * 12, mask_step=8193 * 12),
           dict(w=8193, pitch0=8193, pitch1=8194, mask_pitch=8193, step0=81930, step1=8194 * 5, mask_step=81930), dict(C=0), dict(C=256),
           dict(C=-1), dict(pitch0=11), dict(pitch1=11), dict(step0=119), dict(step1=59), dict(mask_pitch=11), dict(mask_step=119),
           dict(p0=None), dict(p1=None), dict(mask=None), dict(colors=None), dict(alpha=None), dict(alpha=table(0, 256, 128, 1, 2, 257)),
           dict(alpha=table(-1, 256, 128, 1, 2, 3)), dict(format=5), dict(format=5, p2=0x6000, pitch2=5, step2=30),
           dict(format=5, p2=0x6000, pitch2=6, step2=29), dict(format=8), dict(format=8, p2=0x6000, pitch2=12, step2=119),
           dict(format=2, pitch0=47), dict(format=0, pitch0=35)]
    for change in bad:
        assert rc(**change) == E_ARG, change
        assert lib.pips_last_error().decode().startswith("masks_tint:"), change


def test_python_layers_reject_bad_shapes_and_dtypes():
    t, lab = torch.zeros(1, 3, 4, 2), torch.zeros(3, 4, dtype=torch.int64)
    for args, kw in (((t[0], lab, (8, 8)), {}), ((t, lab[:2], (8, 8)), {}), ((t, lab.float(), (8, 8)), {}), ((t, lab, (0, 8)), {}),
                     ((t, lab, (8, 8)), dict(out_size=(8, 8193))), ((t, lab, (8, 8)), dict(radius=-1.0)), ((t, lab, (8, 8)), dict(radius=256.5)),
                     ((t, lab, (8, 8)), dict(vote=0)), ((t, lab, (8, 8)), dict(vote=6)), ((t, lab, (8, 8)), dict(vote=1.5)),
                     ((t, lab, (8, 8)), dict(first=4)), ((t, lab, (8, 8)), dict(first=-1))):
        with pytest.raises(ValueError):
            drivers.object_masks_torch(*args, **kw)
    with pytest.raises(ValueError):
        ops.object_masks(t[0], lab, (8, 8))                          # labels of the library are uint8
    with pytest.raises(ValueError):
        ops.object_masks(t[0].double(), lab.to(torch.uint8), (8, 8))
    planes = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    masks, colors, alpha = torch.zeros(2, 6, 8, dtype=torch.uint8), torch.zeros(2, 3, 3, dtype=torch.uint8), torch.full((2, 3), 0.5)
    good = dict(planes=planes, fmt="rgb24", masks=masks, colors=colors, alpha=alpha)
    assert torch.is_tensor(drivers.tint_masks_torch(**good))
    for bad in (dict(fmt="p010"), dict(fmt="yuv"), dict(masks=masks[:1]), dict(masks=masks.int()), dict(masks=masks[:, :5]),
                dict(colors=colors.float()), dict(colors=colors[:1]), dict(colors=colors[:, :, :2]), dict(colors=torch.zeros(2, 0, 3, dtype=torch.uint8)),
                dict(colors=torch.zeros(2, 256, 3, dtype=torch.uint8), alpha=torch.zeros(2, 256)), dict(alpha=alpha[:, :2]),
                dict(alpha=alpha + 0.6), dict(alpha=-alpha), dict(alpha=alpha * NAN), dict(matrix="bt2020"), dict(range="tv")):
        with pytest.raises(ValueError):
            drivers.tint_masks_torch(**dict(good, **bad))
    for bad in (torch.full((2, 3), 257), torch.full((2, 3), -1), torch.full((2, 3), 0.5)):
        with pytest.raises(ValueError):
            ops.tint_check([planes], "rgb24", masks, colors, bad, "bt709", "limited")
