"""CPU: tracks out -- drivers.draw_tracks_torch, the torch twin of pips_tracks_draw (include/pips_hip.h), against the rule restated
here as plain loops over pixels, subsamples, tracks and primitives on Python integers; the RGB -> YCbCr table against the float64
formula; track_colors; the properties the header names; TrackPainter against one whole-video call; every PIPS_E_ARG case through
the loaded library (nothing is launched).  The surfaces, tracks and cases of tests/test_draw_gpu.py are made here, and the twin's
output on them is checked not to be vacuous.  (The kernels: tests/test_draw_gpu.py.)"""
import math

import numpy as np
import pytest
import torch

from pips_amd import drivers, ops

PACKED = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgba32": (4, (0, 1, 2)), "bgra32": (4, (2, 1, 0))}
YUV = ("nv12", "i420")
FORMATS = list(PACKED) + list(YUV) + ["planar8"]
MATRICES, RANGES = ["bt601", "bt709"], ["limited", "full"]
KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SENTINEL = 0xA5
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ surfaces, tracks and cases
def buffers(fmt, F, h, w, seed, pad=(5, 2)):
    """the allocations behind F surfaces of ``fmt``: ``pad[0]`` more elements a row and ``pad[1]`` more rows a frame than the image,
    random bytes inside the image and SENTINEL everywhere else"""
    g = torch.Generator().manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt in PACKED:
        shapes = [(h, w, PACKED[fmt][0])]
    elif fmt == "nv12":
        shapes = [(h, w), (ch, cw, 2)]
    elif fmt == "i420":
        shapes = [(h, w), (ch, cw), (ch, cw)]
    else:
        shapes = [(3, h, w)]
    out = []
    for s in shapes:
        if fmt == "planar8":
            full = torch.full((F, 3, h + pad[1], w + pad[0]), SENTINEL, dtype=torch.uint8)
            full[:, :, :h, :w] = torch.randint(0, 256, (F, 3, h, w), generator=g, dtype=torch.uint8)
        else:
            full = torch.full((F, s[0] + pad[1], s[1] + pad[0]) + s[2:], SENTINEL, dtype=torch.uint8)
            full[:, :s[0], :s[1]] = torch.randint(0, 256, (F,) + s, generator=g, dtype=torch.uint8)
        out.append(full)
    return out


def views(bufs, fmt, h, w):
    """the surfaces inside ``buffers``' allocations, as the planes ``draw_tracks`` takes"""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "planar8":
        return [bufs[0][:, :, :h, :w]]
    sizes = [(h, w)] + [(ch, cw)] * (len(bufs) - 1)
    return [b[:, :r, :c] for b, (r, c) in zip(bufs, sizes)]


def outside_untouched(bufs, before, fmt, h, w):
    """every byte outside the w x h image of each plane -- pitch padding, the rows behind a frame -- is what it was"""
    masks = [torch.ones_like(b, dtype=torch.bool) for b in bufs]
    for v in views(masks, fmt, h, w):
        v[...] = False                                              # (a view of its mask: the image)
    for b, b0, mask in zip(bufs, before, masks):
        if not torch.equal(b[mask], b0[mask]) or not bool((b[mask] == SENTINEL).all()):
            return False
    if fmt in ("rgba32", "bgra32"):                                 # the alpha byte
        return torch.equal(bufs[0][..., 3], before[0][..., 3])
    return True


def tracks(G, n, h, w, seed, src=None):
    """Seeded tracks for a video of G rows drawn on h x w surfaces (coordinates of a ``src`` = (H, W) image when given): random
    walks, most of them in a quarter of the frame so that they overlap.  With n >= 5 the first five columns are the named cases:
    0 ends on a tile corner (the point between pixels 15 and 16, both ways) after crossing it; 1 runs from left of the frame to right
    of it and 2 from above to below, through the tile borders; 3 has a NaN row, a point beyond 32768 and one at -inf in its past; 4
    holds a segment longer than PIPS_DRAW_JUMP8_MAX.  Beyond column 5 eleven of twelve columns are absent or far away, so that 300 tracks
    do not paint the whole frame.  vis: logits on both sides of 0 with NaNs; -> trajs (1,G,n,2), vis (1,G,n)"""
    g = torch.Generator().manual_seed(seed)
    H, W = (h, w) if src is None else src
    start = torch.rand(1, n, 2, generator=g) * torch.tensor([W * 0.5, H * 0.5]) + torch.tensor([W * 0.2, H * 0.2])
    steps = torch.randn(G, n, 2, generator=g) * (1.4 if n >= 5 else 0.5)   # (a lone track stays in the frame)
    t = start + torch.cumsum(steps, dim=0)
    sx, sy = W / w, H / h                                           # surface pixels -> the model's
    if n >= 5:
        ramp = (torch.arange(G) / float(max(G - 2, 1))).clamp(max=1.0)            # 1 on row G - 2, the last one the cases draw
        t[:, 0, 0] = (15.5 - 6.0 * (1 - ramp) + 0.5) * sx - 0.5
        t[:, 0, 1] = (15.5 - 4.0 * (1 - ramp) + 0.5) * sy - 0.5
        t[:, 1, 0], t[:, 1, 1] = -4.0 + (W + 8.0) * ramp, H * 0.45 + 2.0 * ramp
        t[:, 2, 0], t[:, 2, 1] = W * 0.55 - 3.0 * ramp, -5.0 + (H + 9.0) * ramp
        if G >= 4:
            t[G - 4, 3] = NAN
            t[max(G - 6, 0), 3, 0] = 40000.0
            t[max(G - 7, 0), 3, 1] = -math.inf
            t[G - 3, 4, 0] = 300.0 * sx
        t[G - 2, 3, 0], t[G - 2, 3, 1] = (16.5 + 0.5) * sx - 0.5, (15.0 + 0.5) * sy - 0.5         # its last head overlaps column 0's
    for i in range(5, n):
        if i % 12 == 11:
            t[:, i, 0] += 5000.0
        elif i % 12 != 0:
            t[:, i] = NAN
    vis = torch.randn(G, n, generator=g) * 2.0
    vis[torch.rand(G, n, generator=g) < 0.1] = NAN
    return t.unsqueeze(0).float(), vis.unsqueeze(0).float()


# the cases of the GPU grid: (fmt, matrix, range, h, w, F, n, trail, src, style).  Thin lines and small dots: the frames are small.
STYLE = dict(width=1.5, dot=2.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5)
THIN = dict(width=1.0, dot=1.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5)
FAT = dict(width=5.0, dot=5.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5)       # one track alone has to change 2 % of the frame
SHAPES = [(16, 16), (17, 33), (37, 51)]


def format_cases():
    out = []
    for fmt in FORMATS:
        for matrix, range_ in ([(m, r) for m in MATRICES for r in RANGES] if fmt in YUV else [("bt709", "limited")]):
            for h, w in SHAPES:
                out.append((fmt, matrix, range_, h, w, 3, 5, 4, None, STYLE))
    return out


def grid_cases():
    out = []
    for fmt in ("nv12", "bgra32"):
        for n in (0, 1, 5, 300):
            for trail in (0, 1, 4, 32):
                for src in (None, (24, 32)):
                    out.append((fmt, "bt601", "full", 37, 51, 3, n, trail, src, THIN if n == 300 else FAT if n == 1 else STYLE))
    return out


def case_id(c):
    fmt, matrix, range_, h, w, F, n, trail, src, _ = c
    return f"{fmt}-{matrix}-{range_}-{h}x{w}-n{n}-t{trail}" + ("" if src is None else f"-from{src[0]}x{src[1]}")


def case_inputs(c, with_vis=True):
    """-> (buffers, trajs, vis, kwargs of draw_tracks / draw_tracks_torch) of a case; G = trail + F + 2 rows, first = 2 short of it"""
    fmt, matrix, range_, h, w, F, n, trail, src, style = c
    G = max(trail, 6) + F + 2
    seed = 1000 * h + 10 * w + n + trail
    trajs, vis = tracks(G, n, h, w, seed, src)
    kw = dict(size=src, first=G - F - 1, trail=trail, matrix=matrix, range=range_, **style)
    return buffers(fmt, F, h, w, seed + 1), trajs, (vis if with_vis else None), kw


def not_vacuous(c, before, after, trajs, kw):
    """the four conditions of a case with at least five tracks, on the twin's output ``after`` (planes) and its coverage: a pixel
    with partial coverage, a pixel under two tracks, a chroma sample with 0 < K < 16, and 2 % .. 60 % of the pixels changed.  With
    fewer tracks: what can hold (nothing drawn at n = 0; no overlap asked of one track)"""
    fmt, _, _, h, w, F, n, trail, src, style = c
    line8, dot8 = int(math.floor(4 * style["width"] + 0.5)), int(math.floor(8 * style["dot"] + 0.5))
    partial = overlap = chroma = False
    for f in range(F):
        k = drivers.draw_coverage_torch(trajs[0], kw["first"] + f, h, w, src or (h, w), trail, line8, dot8)
        partial |= bool(((k > 0) & (k < 4)).any())
        overlap |= bool(((k > 0).sum(dim=0) >= 2).any())
        K = torch.nn.functional.pad(k, (0, w % 2, 0, h % 2)).view(n, (h + 1) // 2, 2, (w + 1) // 2, 2).sum(dim=(2, 4))
        chroma |= bool(((K > 0) & (K < 16)).any())
    if fmt in PACKED:
        changed = (before[0][..., :3] != after[0][..., :3]).any(dim=-1)
    elif fmt == "planar8":
        changed = (before[0] != after[0]).any(dim=1)
    else:
        changed = before[0] != after[0]                             # luma: every covered pixel blends its Y
    frac = float(changed.float().mean())
    if n == 0:
        return frac == 0.0, dict(frac=frac)
    ok = partial and chroma and 0.02 <= frac <= 0.60 and (overlap or n < 5)
    return ok, dict(partial=partial, overlap=overlap, chroma=chroma, frac=round(frac, 4))


# ---------------------------------------------------------------------------------------------------- the rule, restated
def restate_points(trajs, r, trail, n_src, n_dst, axis):
    """rows max(r - trail, 0) .. r of one coordinate -> lists of Q (Python int) or None per row and track, numpy float32 arithmetic"""
    f32 = np.float32
    out = []
    for g in range(max(r - trail, 0), r + 1):
        row = []
        for v in trajs[g, :, axis]:
            u = f32(v)
            if n_src != n_dst:
                u = f32(f32(f32(u + f32(0.5)) * (f32(n_dst) / f32(n_src))) - f32(0.5))
            if not (np.isfinite(u) and abs(u) <= 32768.0):
                row.append(None)
            else:
                row.append(int(np.floor(f32(f32(u * f32(8.0)) + f32(0.5)))))
        out.append(row)
    return out


def inside(c, P0, P1, R):
    ax, ay, bx, by = P1[0] - P0[0], P1[1] - P0[1], c[0] - P0[0], c[1] - P0[1]
    L, t = ax * ax + ay * ay, ax * bx + ay * by
    if L == 0 or t <= 0:
        return bx * bx + by * by <= R * R
    if t >= L:
        return (c[0] - P1[0]) ** 2 + (c[1] - P1[1]) ** 2 <= R * R
    return (ax * by - ay * bx) ** 2 <= R * R * L


def restate_coverage(trajs, r, h, w, src, trail, line8, dot8):
    """k[i][y][x] by plain loops: the primitives of each track, then every subsample of every pixel against each"""
    trajs = trajs.numpy()
    n = trajs.shape[1]
    qx, qy = restate_points(trajs, r, trail, src[1], w, 0), restate_points(trajs, r, trail, src[0], h, 1)
    k = [[[0] * w for _ in range(h)] for _ in range(n)]
    for i in range(n):
        pts = [None if qx[g][i] is None or qy[g][i] is None else (qx[g][i], qy[g][i]) for g in range(len(qx))]
        if pts[-1] is None:
            continue
        prims = [(pts[-1], pts[-1], dot8)] if dot8 >= 0 else []
        for g in range(1, len(pts)):
            a, b = pts[g - 1], pts[g]
            if line8 >= 0 and a is not None and b is not None and abs(b[0] - a[0]) <= 2047 and abs(b[1] - a[1]) <= 2047:
                prims.append((a, b, line8))
        for y in range(h):
            for x in range(w):
                for dx, dy in ((-2, -2), (2, -2), (-2, 2), (2, 2)):
                    c = (8 * x + dx, 8 * y + dy)
                    k[i][y][x] += any(inside(c, P0, P1, R) for P0, P1, R in prims)
    return k


def restate_color(rgb, fmt, matrix, range_):
    R, G, B = (int(v) for v in rgb)
    if fmt not in YUV:
        return R, G, B
    y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB_RULES[(matrix, range_)]
    clamp = lambda v: min(max(v, 0), 255)
    return (y0 + ((yr * R + yg * G + yb * B + 32768) >> 16), clamp(128 + ((ur * R + ug * G + ub * B + 32768) >> 16)),
            clamp(128 + ((vr * R + vg * G + vb * B + 32768) >> 16)))


def restate_draw(planes, fmt, cover, A, colors, matrix, range_):
    """the blend by plain loops on clones of ``planes``: cover[f][i][y][x], A[f][i]"""
    planes = [p.clone() for p in planes]
    P = [p.tolist() for p in planes]
    F = len(cover)
    h, w = len(cover[0][0]), len(cover[0][0][0])
    for f in range(F):
        for i in range(len(cover[f])):
            col = restate_color(colors[i], fmt, matrix, range_)
            k = cover[f][i]
            for y in range(h):
                for x in range(w):
                    wg = k[y][x] * A[f][i]
                    if wg == 0:
                        continue
                    mix = lambda p, c: (p * (1024 - wg) + c * wg + 512) >> 10
                    if fmt in PACKED:
                        for q, b in enumerate(PACKED[fmt][1]):
                            P[0][f][y][x][b] = mix(P[0][f][y][x][b], col[q])
                    elif fmt == "planar8":
                        for q in range(3):
                            P[0][f][q][y][x] = mix(P[0][f][q][y][x], col[q])
                    else:
                        P[0][f][y][x] = mix(P[0][f][y][x], col[0])
            if fmt in YUV:
                for cy in range((h + 1) // 2):
                    for cx in range((w + 1) // 2):
                        K = sum(k[y][x] for y in (2 * cy, 2 * cy + 1) for x in (2 * cx, 2 * cx + 1) if y < h and x < w) * A[f][i]
                        if K == 0:
                            continue
                        mix = lambda p, c: (p * (4096 - K) + c * K + 2048) >> 12
                        if fmt == "nv12":
                            P[1][f][cy][cx] = [mix(P[1][f][cy][cx][0], col[1]), mix(P[1][f][cy][cx][1], col[2])]
                        else:
                            P[1][f][cy][cx], P[2][f][cy][cx] = mix(P[1][f][cy][cx], col[1]), mix(P[2][f][cy][cx], col[2])
    return [torch.tensor(p, dtype=torch.uint8).view(q.shape) for p, q in zip(P, planes)]


@pytest.mark.parametrize("h,w,n,src", [(10, 12, 4, None), (7, 9, 3, None), (7, 9, 4, (5, 6))])
def test_twin_is_the_rule_by_plain_loops(h, w, n, src):
    F, trail, first = 2, 3, 3
    G = first + F
    style = dict(width=1.5, dot=1.75, alpha=0.9, alpha_occ=0.4, vis_thr=0.6)
    line8, dot8, a_vis, a_occ = 6, 14, 230, 102
    assert (a_vis, a_occ) == (math.floor(256 * 0.9 + 0.5), math.floor(256 * 0.4 + 0.5))
    logit = float(torch.logit(torch.tensor(0.6, dtype=torch.float32)))
    g = torch.Generator().manual_seed(h * w + n)
    H, W = src or (h, w)
    trajs = (torch.rand(1, 1, n, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0]) + torch.randn(1, G, n, 2, generator=g).cumsum(1) * 1.2)
    trajs[0, 1, 0] = NAN                                            # a gap in the first track's past
    vis = torch.randn(1, G, n, generator=g)
    vis[0, first, 1] = NAN                                          # a NaN logit: occluded
    vis[0, first, 0], vis[0, first + 1, 2] = 3.0, -3.0              # one seen, one not
    colors = torch.randint(0, 256, (n, 3), generator=g, dtype=torch.uint8)
    cover = [restate_coverage(trajs[0], first + f, h, w, (H, W), trail, line8, dot8) for f in range(F)]
    for f in range(F):                                              # the twin's coverage is the loops'
        got = drivers.draw_coverage_torch(trajs[0], first + f, h, w, (H, W), trail, line8, dot8)
        assert got.tolist() == cover[f]
    assert any(0 < v < 4 for f in cover for t in f for row in t for v in row)
    A = [[a_vis if float(vis[0, first + f, i]) > logit else a_occ for i in range(n)] for f in range(F)]
    assert A[0][1] == a_occ and {a for row in A for a in row} == {a_vis, a_occ}
    for fmt in FORMATS:
        for matrix, range_ in ([(m, r) for m in MATRICES for r in RANGES] if fmt in YUV else [("bt709", "limited")]):
            bufs = buffers(fmt, F, h, w, 7 * h + w)
            before = [b.clone() for b in bufs]
            planes = views(bufs, fmt, h, w)
            want = restate_draw(planes, fmt, cover, A, colors.tolist(), matrix, range_)
            got = drivers.draw_tracks_torch(planes, fmt, trajs, vis, colors, size=src, first=first, trail=trail, matrix=matrix,
                                            range=range_, **style)
            got = [got] if torch.is_tensor(got) else got
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (fmt, matrix, range_)
            assert any(not torch.equal(a, b) for a, b in zip(got, planes))
            assert all(torch.equal(a, b) for a, b in zip(bufs, before))              # inplace=False drew on clones
            out = drivers.draw_tracks_torch(planes, fmt, trajs, vis, colors, size=src, first=first, trail=trail, matrix=matrix,
                                            range=range_, inplace=True, **style)
            out = [out] if torch.is_tensor(out) else out
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, planes))
            assert all(torch.equal(a, b) for a, b in zip(planes, want)) and outside_untouched(bufs, before, fmt, h, w)


# ------------------------------------------------------------------------------------------------------- the colour table
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("range_", RANGES)
def test_colour_table(matrix, range_):
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = (219.0 / 255.0, 224.0 / 255.0, 16) if range_ == "limited" else (1.0, 1.0, 0)
    grey = torch.arange(256).view(-1, 1).expand(-1, 3)
    out = drivers.rgb_to_yuv_torch(grey, matrix, range_)
    assert bool((out[:, 1:] == 128).all())                          # greys give (Y, 128, 128)
    assert out[0].tolist() == [y0, 128, 128] and out[255].tolist() == [235 if range_ == "limited" else 255, 128, 128]
    assert bool((out[1:, 0] >= out[:-1, 0]).all())
    v = torch.linspace(0, 255, 17).round().to(torch.int64)
    rgb = torch.cartesian_prod(v, v, v)
    got = drivers.rgb_to_yuv_torch(rgb, matrix, range_)
    R, G, B = rgb.double().unbind(1)
    Y = kr * R + kg * G + kb * B
    exact = torch.stack([y0 + ys * Y, 128 + cs * (B - Y) / (2 * (1 - kb)), 128 + cs * (R - Y) / (2 * (1 - kr))], dim=1)
    assert bool(((got - torch.floor(exact + 0.5).clamp(0, 255)).abs() <= 1).all())
    if range_ == "limited":
        assert 16 <= int(got[:, 0].min()) and int(got[:, 0].max()) <= 235 and 16 <= int(got[:, 1:].min()) and int(got[:, 1:].max()) <= 240
    else:                                                           # pure blue / red reach 256 ahead of the clamp
        y0_, yr, yg, yb, ur, ug, ub, vr, vg, vb = drivers.RGB_RULES[(matrix, range_)]
        assert 128 + ((ub * 255 + 32768) >> 16) == 256 and 128 + ((vr * 255 + 32768) >> 16) == 256
        assert drivers.rgb_to_yuv_torch(torch.tensor([[0, 0, 255], [255, 0, 0]]), matrix, range_)[:, 1:].tolist()[0][0] == 255
        assert int(got.max()) == 255 and int(got.min()) >= 0


def test_colour_table_is_stated_once_per_layer():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "pips_amd", "csrc", "yuv.h")).read()
    body = src[src.index("RGB_RULES[2][2]"):]
    rows = re.findall(r"\{(-?\d+(?:, -?\d+){9})\}", body[:body.index("};")])
    want = [drivers.RGB_RULES[(m, r)] for m in MATRICES for r in RANGES]
    assert [tuple(int(v) for v in row.split(",")) for row in rows] == want


def test_track_colors():
    ids = torch.arange(4096)
    c = drivers.track_colors(ids)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (4096, 3)
    assert torch.equal(c, drivers.track_colors(ids.tolist())) and torch.equal(c[[5, 77]], drivers.track_colors(torch.tensor([5, 77])))
    hue = [((i * 2654435769) % 2 ** 32) >> 24 for i in range(4096)]
    wheel = lambda s, up: [(255, up, 0), (255 - up, 255, 0), (0, 255, up), (0, 255 - up, 255), (up, 0, 255), (255, 0, 255 - up)][s]
    for i, h in enumerate(hue):
        assert tuple(c[i].tolist()) == wheel((6 * h) >> 8, (6 * h) & 255)
    # the six corners of the wheel: the first hue of each segment, where `up` is smallest
    for s in range(6):
        h = next(h for h in range(256) if (6 * h) >> 8 == s)
        i = hue.index(h)
        assert (6 * h) & 255 < 6 and tuple(c[i].tolist()) == wheel(s, (6 * h) & 255)
    assert tuple(c[hue.index(0)].tolist()) == (255, 0, 0) and tuple(c[hue.index(128)].tolist()) == (0, 255, 255)
    assert len({tuple(v) for v in c[:64].tolist()}) > 48            # neighbouring identities get different colours


# -------------------------------------------------------------------------------------------------------------- properties
def _canvas(h=24, w=24, F=1, fmt="planar8"):
    bufs = buffers(fmt, F, h, w, 3)
    return bufs, views(bufs, fmt, h, w)


def _line(points):
    """one track whose rows are ``points``"""
    return torch.tensor(points, dtype=torch.float32).view(1, len(points), 1, 2)


RED = torch.tensor([[255, 0, 0]], dtype=torch.uint8)


def _draw(planes, fmt, trajs, **kw):
    kw.setdefault("first", trajs.shape[1] - planes[0].shape[0])
    vis, colors = kw.pop("vis", None), kw.pop("colors", RED.expand(trajs.shape[2], 3).contiguous())
    out = drivers.draw_tracks_torch(planes, fmt, trajs, vis, colors, **kw)
    return [out] if torch.is_tensor(out) else out


def test_alpha_zero_leaves_every_byte():
    for fmt in ("planar8", "nv12"):
        _, planes = _canvas(fmt=fmt)
        t = _line([(3, 3), (20, 18)])
        assert any(not torch.equal(a, b) for a, b in zip(_draw(planes, fmt, t, alpha=0.5), planes))
        assert all(torch.equal(a, b) for a, b in zip(_draw(planes, fmt, t, alpha=0.0), planes))
        vis = torch.tensor([[[-5.0]], [[-5.0]]]).view(1, 2, 1)
        assert all(torch.equal(a, b) for a, b in zip(_draw(planes, fmt, t, vis=vis, alpha=1.0, alpha_occ=0.0), planes))


def test_an_absent_head_hides_the_whole_trail():
    _, planes = _canvas()
    for bad in (NAN, math.inf, 32768.5, -40000.0):
        assert torch.equal(_draw(planes, "planar8", _line([(3, 3), (12, 12), (bad, 12)]))[0], planes[0])
        assert torch.equal(_draw(planes, "planar8", _line([(3, 3), (12, 12), (12, bad)]))[0], planes[0])
    # an absent point in the past only breaks the trail there
    whole = _draw(planes, "planar8", _line([(3, 3), (12, 12), (20, 12)]), trail=2)[0]
    gap = _draw(planes, "planar8", _line([(NAN, 3), (12, 12), (20, 12)]), trail=2)[0]
    head = _draw(planes, "planar8", _line([(3, 3), (12, 12), (20, 12)]), trail=1)[0]
    assert torch.equal(gap, head) and not torch.equal(gap, whole)


def test_the_longest_drawn_segment():
    bufs = buffers("planar8", 1, 8, 300, 5)
    planes = views(bufs, "planar8", 8, 300)
    at = lambda dq: _draw(planes, "planar8", _line([(2.0, 4.0), (2.0 + dq / 8.0, 4.0)]), trail=1, dot=-1.0)[0]
    assert not torch.equal(at(2047), planes[0]) and torch.equal(at(2048), planes[0])
    assert bool((at(2047)[0, 0, 4, 3:250] != planes[0][0, 0, 4, 3:250]).any())
    down = lambda dq: _draw(planes, "planar8", _line([(2.0, -100.0), (2.0, -100.0 + dq / 8.0)]), trail=1, dot=-1.0)[0]
    assert not torch.equal(down(2047), planes[0]) and torch.equal(down(2048), planes[0])


def test_the_trail_is_clipped_at_row_zero():
    bufs = buffers("planar8", 3, 24, 24, 6)
    planes = views(bufs, "planar8", 24, 24)
    t = _line([(3, 3), (12, 5), (20, 12)])
    got = _draw(planes, "planar8", t, trail=16, first=0)[0]
    assert torch.equal(got[0], _draw([planes[0][:1]], "planar8", t[:, :1], trail=0, first=0)[0][0])      # frame 0: the head alone
    assert torch.equal(got[1], _draw([planes[0][1:2]], "planar8", t[:, :2], trail=1, first=1)[0][0])
    assert torch.equal(got[2], _draw([planes[0][2:]], "planar8", t, trail=2, first=2)[0][0])


def test_two_equal_points_draw_a_disc_of_the_line_radius():
    _, planes = _canvas()
    seg = _draw(planes, "planar8", _line([(11.25, 9.5), (11.25, 9.5)]), trail=1, width=2.5, dot=-1.0)[0]
    disc = _draw(planes, "planar8", _line([(11.25, 9.5)]), trail=0, dot=1.25)[0]
    assert torch.equal(seg, disc) and not torch.equal(seg, planes[0])


def test_a_negative_radius_draws_nothing_of_its_kind():
    _, planes = _canvas()
    t = _line([(3, 3), (20, 18)])
    both = _draw(planes, "planar8", t, trail=1, alpha=1.0)[0]
    assert torch.equal(_draw(planes, "planar8", t, trail=1, width=-1.0, dot=-1.0)[0], planes[0])
    line = _draw(planes, "planar8", t, trail=1, dot=-1.0, alpha=1.0)[0]
    dot = _draw(planes, "planar8", t, trail=1, width=-1.0, alpha=1.0)[0]
    assert torch.equal(dot, _draw(planes, "planar8", t, trail=0, alpha=1.0)[0])
    assert not torch.equal(line, planes[0]) and not torch.equal(dot, planes[0]) and not torch.equal(line, dot)
    changed = lambda a: a != planes[0]
    assert torch.equal(changed(both).any(dim=1), (changed(line) | changed(dot)).any(dim=1))              # the union, drawn once
    with pytest.raises(ValueError):
        _draw(planes, "planar8", t, dot=16.1)
    with pytest.raises(ValueError):
        _draw(planes, "planar8", t, width=32.2)


def test_column_order_is_part_of_the_rule():
    for fmt in ("planar8", "nv12"):
        _, planes = _canvas(fmt=fmt)
        t = torch.tensor([[[4.0, 4.0], [18.0, 4.0]], [[18.0, 18.0], [4.0, 18.0]]]).view(1, 2, 2, 2)       # they cross on pixel (11, 11)
        colors = torch.tensor([[255, 0, 0], [0, 0, 255]], dtype=torch.uint8)
        a = _draw(planes, fmt, t, colors=colors, alpha=0.6)
        b = _draw(planes, fmt, t.flip(2), colors=colors.flip(0), alpha=0.6)
        assert any(not torch.equal(x, y) for x, y in zip(a, b))
        # at full opacity and full coverage the later column wins
        if fmt == "planar8":
            assert _draw(planes, fmt, t, colors=colors, alpha=1.0, width=4.0)[0][0, :, 11, 11].tolist() == [0, 0, 255]
            assert _draw(planes, fmt, t.flip(2), colors=colors.flip(0), alpha=1.0, width=4.0)[0][0, :, 11, 11].tolist() == [255, 0, 0]


@pytest.mark.parametrize("fmt", FORMATS)
def test_nothing_outside_the_image_is_written(fmt):
    h, w = 9, 13
    bufs = buffers(fmt, 2, h, w, 11)
    before = [b.clone() for b in bufs]
    planes = views(bufs, fmt, h, w)
    t = torch.tensor([[-3.0, -2.0], [20.0, 14.0], [-4.0, 12.0]]).view(1, 3, 1, 2)
    _draw(planes, fmt, t, trail=2, width=6.0, dot=6.0, alpha=1.0, inplace=True)
    assert any(not torch.equal(a, b) for a, b in zip(bufs, before)) and outside_untouched(bufs, before, fmt, h, w)
    if fmt in ("rgba32", "bgra32"):
        assert bool((planes[0][..., :3] != before[0][:, :h, :w, :3]).any())


def _light(case):                                                   # (300 tracks with 33 points each: once per size on the CPU, as nv12)
    return not (case[6] == 300 and case[7] == 32 and case[0] != "nv12")


@pytest.mark.parametrize("case", [c for c in format_cases() + grid_cases() if _light(c)], ids=case_id)
def test_the_gpu_cases_are_not_vacuous(case):
    """the seeds of tests/test_draw_gpu.py's grid: the twin's output on the cases shows partial coverage, overlap, partial chroma
    coverage and a changed fraction of 2 % .. 60 % (test_draw_gpu.py asserts the same of every case on the device; tracks and
    coverage do not depend on the format)"""
    fmt, h, w = case[0], case[3], case[4]
    bufs, trajs, vis, kw = case_inputs(case)
    planes = views(bufs, fmt, h, w)
    after = drivers.draw_tracks_torch(planes, fmt, trajs, vis, **kw)
    after = [after] if torch.is_tensor(after) else after
    ok, what = not_vacuous(case, planes, after, trajs, kw)
    assert ok, what


# ----------------------------------------------------------------------------------------------------------- TrackPainter
@pytest.mark.parametrize("fmt", ["nv12", "bgr24"])
def test_painter_push_by_push_is_one_whole_video_call(fmt):
    """three pushes of 3, 4 and 3 frames; identity 1 leaves after the first, identity 4 joins in the second: the painter's bytes are
    those of one draw_tracks_torch over the video with trajs by identity (NaN outside each life)"""
    h, w, T, K, trail = 20, 28, 10, 5, 4
    g = torch.Generator().manual_seed(9)
    trajs = torch.rand(1, 1, K, 2, generator=g) * torch.tensor([w - 8.0, h - 8.0]) + 4 + torch.randn(1, T, K, 2, generator=g).cumsum(1) * 1.5
    vis = torch.randn(1, T, K, generator=g)
    trajs[0, 3:, 1] = NAN                                           # retired on frame 2
    trajs[0, :4, 4] = NAN                                           # born on frame 4
    style = dict(width=1.5, dot=2.0, alpha=0.8, alpha_occ=0.3, vis_thr=0.4, matrix="bt601", range="full")
    bufs = buffers(fmt, T, h, w, 12)
    planes = views(bufs, fmt, h, w)
    want = drivers.draw_tracks_torch(planes, fmt, trajs, vis, colors=drivers.track_colors(torch.arange(K)), trail=trail, **style)
    want = [want] if torch.is_tensor(want) else want
    painter = drivers.TrackPainter((h, w), trail=trail, engine="torch", **style)
    got = []
    for (a, b), ids in zip(((0, 3), (3, 7), (7, 10)), ([0, 1, 2, 3], [0, 2, 3, 4], [0, 2, 3, 4])):
        out = painter.paint([p[a:b] for p in planes], fmt, a, trajs[:, a:b][:, :, ids], vis[:, a:b][:, :, ids], ids=torch.tensor(ids),
                            inplace=False)
        got.append([out] if torch.is_tensor(out) else out)
    for k in range(len(planes)):
        assert torch.equal(torch.cat([p[k] for p in got]), want[k])
    assert any(not torch.equal(a, b) for a, b in zip(want, planes))
    with pytest.raises(ValueError):
        painter.paint([p[:1] for p in planes], fmt, 3, trajs[:, :1], vis[:, :1], ids=torch.arange(K))   # frame 3 after frame 9
    # stable columns without ids; the trail runs across the pushes
    stable = drivers.TrackPainter((h, w), trail=trail, engine="torch", **style)
    t2 = trajs[:, :, [0, 2, 3]]
    want2 = drivers.draw_tracks_torch(planes, fmt, t2, None, trail=trail, **style)
    want2 = [want2] if torch.is_tensor(want2) else want2
    parts = []
    for a, b in ((0, 5), (5, 10)):
        out = stable.paint([p[a:b] for p in planes], fmt, a, t2[:, a:b], inplace=False)
        parts.append([out] if torch.is_tensor(out) else out)
    assert all(torch.equal(torch.cat([p[k] for p in parts]), want2[k]) for k in range(len(planes)))
    with pytest.raises(ValueError):
        stable.paint([p[:1] for p in planes], fmt, 10, trajs[:, :1])                                    # five columns after three


# ------------------------------------------------------------------------------------------------- the library's checks
E_ARG = -1
GOOD = dict(format=4, matrix=1, range=0, F=2, h=10, w=12, p0=0x1000, pitch0=12, step0=120, p1=0x2000, pitch1=12, step1=60, p2=None,
            pitch2=0, step2=0, trajs=0x3000, vis=None, G=5, n=3, first=1, src_h=10, src_w=12, colors=0x4000, trail=4, line8=8, dot8=24,
            alpha_vis=256, alpha_occ=90, vis_logit=0.0, workspace=0x5000, workspace_bytes=1 << 20, stream=None)


def _rc(lib, **change):
    a = dict(GOOD, **change)
    return lib.pips_tracks_draw(*[a[k] for k in GOOD])


def test_tracks_draw_rejects_bad_arguments_ahead_of_any_launch():
    """every PIPS_E_ARG case of the header through the loaded library: the pointers are never followed (nothing is launched), so
    this runs without a device; a call that launches nothing -- F = 0 or n = 0 -- returns PIPS_OK"""
    from pips_amd import _lib
    lib = _lib.load()
    assert lib.pips_abi_version() == 3
    need = lib.pips_draw_workspace_bytes(2, 3, 4)
    assert need == 4 * 2 * 3 * (2 * 4 + 10) and lib.pips_draw_workspace_bytes(0, 3, 4) == 0
    assert lib.pips_draw_workspace_bytes(2, 3, 33) == 0 and lib.pips_draw_workspace_bytes(-1, 3, 4) == 0
    assert _rc(lib, F=0) == 0 and _rc(lib, n=0) == 0 and _rc(lib, F=0, first=5) == 0
    assert _rc(lib, n=0, p0=None, trajs=None, colors=None, workspace=None, workspace_bytes=0) == 0
    bad = [dict(format=6), dict(format=7), dict(format=9), dict(format=-1), dict(matrix=2), dict(range=-1), dict(range=2), dict(F=-1),
           dict(n=-1), dict(h=0), dict(w=0), dict(src_h=0), dict(src_w=0), dict(h=8193, step0=8193 * 12, step1=4097 * 12),
           dict(w=8193, pitch0=8193, pitch1=8194, step0=81930, step1=8194 * 5), dict(trail=-1), dict(trail=33), dict(line8=129),
           dict(dot8=129), dict(alpha_vis=257), dict(alpha_vis=-1), dict(alpha_occ=257), dict(alpha_occ=-1), dict(first=-1),
           dict(first=4), dict(G=2), dict(pitch0=11), dict(pitch1=11), dict(step0=119), dict(step1=59), dict(p0=None), dict(p1=None),
           dict(trajs=None), dict(colors=None), dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=0x5004),
           dict(format=5), dict(format=5, p2=0x6000, pitch2=5, step2=30), dict(format=5, p2=0x6000, pitch2=6, step2=29),
           dict(format=8), dict(format=8, p2=0x6000, pitch2=12, step2=119), dict(format=2, pitch0=47), dict(format=0, pitch0=35)]
    for change in bad:
        assert _rc(lib, **change) == E_ARG, change
        assert lib.pips_last_error().decode().startswith("tracks_draw:"), change
    # a matrix or range is looked at for the YCbCr formats alone; negative radii are legal
    assert _rc(lib, format=0, matrix=7, range=7, pitch0=36, step0=360, F=0) == 0
    assert _rc(lib, F=0, line8=-5, dot8=-1, h=8192, w=8192, pitch0=8192, pitch1=8192) == 0


def test_python_layers_reject_bad_arguments():
    _, planes = _canvas()
    t = _line([(3, 3), (20, 18)])
    for kw in (dict(trail=33), dict(trail=-1), dict(first=2), dict(alpha=1.01), dict(alpha_occ=-0.1), dict(vis_thr=1.0), dict(size=(0, 4)),
               dict(matrix="bt2020")):
        with pytest.raises(ValueError):
            _draw(planes, "planar8", t, **kw)
    with pytest.raises(ValueError):
        drivers.draw_tracks_torch(planes, "p010", t)
    with pytest.raises(ValueError):
        drivers.draw_tracks_torch(planes, "planar8", t[0])
    with pytest.raises(ValueError):
        drivers.draw_tracks_torch(planes, "planar8", t, colors=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        drivers.TrackPainter((8, 8), trail=40)
    with pytest.raises(ValueError):
        drivers.TrackPainter((8, 8), engine="eager")
    with pytest.raises(ValueError):
        drivers.TrackPainter((8, 8), colour="red")
    assert set(ops.DRAW_FORMATS) == set(FORMATS) and ops.DRAW_FORMATS["planar8"] == 8
