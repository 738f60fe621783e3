"""pips_frames_warp_fill alone: microseconds per output frame for stabilised frames whose border is filled from neighbouring frames,
HIP events around ``reps`` back-to-back calls after a warm-up of each case; every figure ``repeats`` times in one session, the
three routes of a case in alternating order, with its median.
  - surfaces: 1080x1920 NV12, P010 and RGBA32, and 2160x3840 NV12, in calls of ``--frames`` (8) frames;
  - maps: candidate 0 is tools/warp_bench.py's rotation of one degree about the centre with a shift of (3.5, -2.25) px; K = 1, 3 and
    5, neighbour k differing from it by a further +-0.5 k' degrees and +-4 k' px (k' = 1, 1, 2, 2), read from the frames before and
    behind;
  - three routes per case, measured in the same session: the fill call; pips_frames_warp on the same surfaces under candidate 0
    (what the fill's fast path executes); and the route open before the fill call existed -- K ops.warp_frames calls into K
    full-size temporaries, the coverage masks of every plane from the same integers in torch, and a chain of torch.where per plane;
  - beside them the share of tiles on the fast path (the kernel's criterion restated on Python ints for frame 0; every frame of a
    case has the same rows) and the share of plane-0 samples each slot supplied, from the source map.
The library calls go straight to the C entry points with buffers allocated once.  Every case is first compared with
drivers.warp_frames_fill_torch (run on the GPU) on its first frame, bytes and map: a time of wrong bytes is no time.  Prints a table
and one JSON line; no pass mark.
usage: python tools/warp_fill_bench.py [--reps 100 --repeats 3 --frames 8]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import _lib, drivers, ops  # noqa: E402
from warp_bench import CASES, _surfaces, _time  # noqa: E402

KS = (1, 3, 5)
EXTRA = ((0.0, 0.0, 0.0), (0.5, 4.0, -4.0), (-0.5, -4.0, 4.0), (1.0, 8.0, 8.0), (-1.0, -8.0, -8.0))     # degrees, px, px beside candidate 0
OFFSETS = (0, -1, 1, -2, 2)


def _forward(h, w, deg, sx, sy):
    cx, cy = (w - 1) / 2, (h - 1) / 2
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [c, -s, cx - c * cx + s * cy + sx, s, c, cy - s * cx - c * cy + sy]


def _tables(F, K, h, w):
    """cand (F,K) and coef (F,K,6): slot k of frame j reads frame j + OFFSETS[k] (-1 outside the call)"""
    rows = [_forward(h, w, 1.0 + d, 3.5 + sx, -2.25 + sy) for d, sx, sy in EXTRA[:K]]
    coef = drivers.warp_coefficients(torch.tensor(rows, dtype=torch.float64), (h, w))
    cand = [[j + o if 0 <= j + o < F else -1 for o in OFFSETS[:K]] for j in range(F)]
    return torch.tensor(cand, dtype=torch.int32), coef.unsqueeze(0).expand(F, K, 6).contiguous()


def _pos(m, x, y, chroma):
    if chroma:
        return ((m[0] * (4 * x + 1) + m[1] * (4 * y + 1) + 512 * m[2] - 2 ** 24 + 2 ** 17) >> 26,
                (m[3] * (4 * x + 1) + m[4] * (4 * y + 1) + 512 * m[5] - 2 ** 24 + 2 ** 17) >> 26)
    return (m[0] * x + m[1] * y + 256 * m[2] + 32768) >> 24, (m[3] * x + m[4] * y + 256 * m[5] + 32768) >> 24


def _fast_share(row, fmt, h, w):
    """the share of tiles whose candidate-0 box lies inside every plane: warp_fill_kernel's fast-path test on Python ints"""
    def inside(chroma, tx, ty, tw, th, pw, ph):
        pts = [_pos(row, x, y, chroma) for x, y in ((tx, ty), (tx + tw - 1, ty), (tx, ty + th - 1), (tx + tw - 1, ty + th - 1))]
        return min(p[0] for p in pts) >= 0 and min(p[1] for p in pts) >= 0 and max(p[0] for p in pts) + 1 < pw and max(p[1] for p in pts) + 1 < ph
    tw, th = ops.WARP_TILE_W, ops.WARP_TILE_H
    tiles = [(x0, y0) for y0 in range(0, h, th) for x0 in range(0, w, tw)]
    yuv = fmt in ("nv12", "i420", "p010", "i010")
    fast = sum(inside(False, x0, y0, tw, th, w, h) and (not yuv or inside(True, x0 // 2, y0 // 2, tw // 2, th // 2, (w + 1) // 2, (h + 1) // 2))
               for x0, y0 in tiles)
    return fast / len(tiles)


def _fill_call(lib, fmt, planes, out, cand, coef, smap, stream):
    F, h, w = planes[0].shape[:3]
    args = ops.draw_surfaces(planes, fmt) + ops.draw_surfaces(out, fmt)
    head = (ops.DRAW_FORMATS_EX[fmt], 1, 0, 0, 0, F, F, cand.shape[1], h, w)

    def call():
        rc = lib.pips_frames_warp_fill(*head, *args, C.c_void_p(cand.data_ptr()), C.c_void_p(coef.data_ptr()),
                                       C.c_void_p(smap.data_ptr()), smap.stride(1), smap.stride(0), stream)
        assert rc == 0, lib.pips_last_error()
    return call


def _warp_call(lib, fmt, planes, out, coef0, stream):
    F, h, w = planes[0].shape[:3]
    args = ops.draw_surfaces(planes, fmt) + ops.draw_surfaces(out, fmt)
    head = (ops.DRAW_FORMATS_EX[fmt], 1, 0, 0, 0, F, h, w)

    def call():
        rc = lib.pips_frames_warp(*head, *args, C.c_void_p(coef0.data_ptr()), stream)
        assert rc == 0, lib.pips_last_error()
    return call


def _old_route(fmt, planes, cand, coef):
    """the route open before: K warps into full-size temporaries, coverage masks in torch, torch.where per plane"""
    F, h, w = planes[0].shape[:3]
    dev = planes[0].device
    K = cand.shape[1]
    rows = coef[0].tolist()                                                  # (every frame of the bench has the same rows)
    idx = cand.to(dev, torch.int64).clamp(min=0)
    valid = (cand >= 0).to(dev)
    per_slot = [coef[:, k].contiguous() for k in range(K)]

    def call():
        outs = [ops.warp_frames([p[idx[:, k]] for p in planes], fmt, per_slot[k], "constant") for k in range(K)]
        res = outs[0]                                                        # candidate 0 under the border rule
        for k in reversed(range(1, K)):
            for i, p in enumerate(outs[k]):
                ph, pw = p.shape[1:3]
                cov = drivers._warp_covers(ph, pw, rows[k], i > 0, dev).unsqueeze(0) & valid[:, k].view(F, 1, 1)
                res[i] = torch.where(cov if p.dim() == 3 else cov.unsqueeze(-1), p, res[i])
        if K > 1:                                                            # (the first in list order stays)
            for i, p in enumerate(outs[0]):
                ph, pw = p.shape[1:3]
                cov = drivers._warp_covers(ph, pw, rows[0], i > 0, dev).unsqueeze(0)
                res[i] = torch.where(cov if p.dim() == 3 else cov.unsqueeze(-1), p, res[i])
        return res
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F = a.frames
    rows, notes = {}, []
    for fmt, h, w in CASES:
        g = torch.Generator().manual_seed(h + F)
        planes = _surfaces(fmt, F, h, w, g, dev)
        out = [torch.empty_like(p) for p in planes]
        smap = torch.empty(F, h, w, dtype=torch.uint8, device=dev)
        reps = max(a.reps * 8 // F // (4 if h > 1080 else 1), 5)
        for K in KS:
            cand, coef = _tables(F, K, h, w)
            cand, coef = cand.to(dev), coef.to(dev)
            tag = f"{h}p {fmt} F{F} K{K}"
            fill = _fill_call(lib, fmt, planes, out, cand, coef, smap, stream)
            warp = _warp_call(lib, fmt, planes, [torch.empty_like(p) for p in planes], coef[:, 0].contiguous(), stream)
            old = _old_route(fmt, planes, cand, coef)
            fill()
            torch.cuda.synchronize()
            hi = min(max(OFFSETS[:K]), F - 1) + 1                               # a time of wrong bytes is no time: frame 0 against the twin
            want, wmap = drivers.warp_frames_fill_torch([p[:hi] for p in planes], fmt, cand[:1], coef[:1], source=True)
            want = [want] if torch.is_tensor(want) else want
            assert all(torch.equal(o[:1], x) for o, x in zip(out, want)) and torch.equal(smap[:1], wmap), tag
            share = torch.bincount(smap.flatten().to(torch.int64), minlength=256).double() / smap.numel()
            notes.append(f"{tag}: {_fast_share(coef[0, 0].tolist(), fmt, h, w):.1%} of the tiles on the fast path; plane-0 samples by slot "
                         + " ".join(f"{k}: {float(share[k]):.2%}" for k in range(K)) + f" none: {float(share[255]):.2%}")
            routes = [("pips_frames_warp_fill", fill, reps), ("pips_frames_warp, candidate 0", warp, reps),
                      (f"{K} warps + masks + torch.where", old, max(reps // 10, 2))]
            for r in range(a.repeats):
                for name, fn, n in (routes if r % 2 == 0 else routes[::-1]):
                    rows.setdefault(f"{tag}: {name}, us/frame", []).append(_time(fn, n, warm=2) / F)
        del planes, out, smap
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(dev), "config": f"{a.reps} calls per figure at 8 frames of 1080p (fewer for larger calls), {a.repeats} repeats"}
    print(f"device: {res['device']}")
    print(f"{'run':84s} {'(repeats)':>36s} {'median':>10s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:84s} {' '.join(f'{u:11.2f}' for u in us):>36s} {med:10.2f}")
        res[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    for n in notes:
        print(n)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
