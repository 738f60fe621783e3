"""pips_object_masks and pips_masks_tint alone: microseconds per frame, by tools/motion_layers_bench.py's method -- HIP events
around ``reps`` back-to-back calls after a warm-up of each shape, every figure ``repeats`` times in one session, with its median;
the library calls go straight to the C entry points with buffers allocated once.
  - masks of one frame at 368 x 496 from tracks of the same size and at 1080 x 1920 from 368 x 496 tracks; n = 256 and 2048 tracks
    spread evenly over the frame, a rectangle of them labelled 1, the others 0, one in twenty 255; vote 1 and 3; the radius 1.5 x
    the mean track spacing sqrt(h w / n) of the shape;
  - the tint of one 1080 x 1920 frame on NV12 and on RGBA32 with the n = 2048, vote = 1 mask: the object alone (opacity 0 for
    label 0, as object_colors makes it) and every label tinted;
  - beside each the route open before these entries, in the same session: per frame the squared distances from the pixel grid to
    the tracks in float32, in chunks of pixels, ``topk`` for the nearest, ``gather`` for their labels (``mode`` for the vote) --
    and for the tint float blending per plane (the chroma weights by a 2 x 2 average pool).  HIP events around ``slow_reps`` runs;
  - ``--kernels``: 21 calls per shape and nothing else -- the run to put under a kernel trace
    (rocprofv3 --kernel-trace --stats -d DIR -- python tools/masks_bench.py --kernels);
  - ``--reduce TRACE.db``: needs no GPU.  Reads the ``kernels`` view of the SQLite database that trace wrote, drops the first call
    of each shape and prints, per shape, the median over the other 20 calls of each kernel's time, and its byte time: h w bytes
    written by the raster kernel; the mask read plus the surface read and written by the tint kernel (every label tinted).
Every shape is compared with the torch twin first (drivers.object_masks_torch, drivers.tint_masks_torch, on the device): a time of
wrong masks is no time.  Prints a table and one JSON line.
usage: python tools/masks_bench.py [--reps 200 --repeats 3 --slow-reps 5] [--kernels | --reduce TRACE.db]"""
import argparse
import ctypes as C
import json
import math
import os
import re
import sqlite3
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from motion_bench import _time  # noqa: E402
from pips_amd import _lib, drivers, ops  # noqa: E402

SRC = (368, 496)
MASK_SHAPES = [(size, n, vote) for size in ((368, 496), (1080, 1920)) for n in (256, 2048) for vote in (1, 3)]
TINT_SHAPES = [(fmt, every) for fmt in ("nv12", "rgba32") for every in (False, True)]
TINT_SIZE, TINT_N = (1080, 1920), 2048
TRACE_CALLS = 21


def _radius8(size, n):
    return min(int(math.floor(8 * 1.5 * math.sqrt(size[0] * size[1] / n) + 0.5)), ops.MASK_RADIUS8_MAX)


def _tracks(n, g):
    """n tracks of one row in SRC coordinates, jittered about an even spread; labels 1 inside the middle ninth, 0 outside, 255 for
    one in twenty -> (rows (1,n,2) float32, labels (1,n) uint8)"""
    H, W = SRC
    xy = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)])
    inside = (xy[:, 0] > W / 3) & (xy[:, 0] < 2 * W / 3) & (xy[:, 1] > H / 3) & (xy[:, 1] < 2 * H / 3)
    lab = inside.to(torch.uint8)
    lab[torch.rand(n, generator=g) < 0.05] = ops.MASK_NONE
    return xy.view(1, n, 2).float(), lab.view(1, n)


def _masks(lib, rows, lab, size, vote, stream):
    """one pips_object_masks call on device rows, buffers allocated once -> (call, mask)"""
    n, (h, w) = rows.shape[1], size
    out = torch.empty(1, h, w, dtype=torch.uint8, device=rows.device)
    nbytes = ops.object_masks_workspace_bytes(1, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rows.device)
    p = [C.c_void_p(t.data_ptr()) for t in (rows, lab, out, ws)]
    r8 = _radius8(size, n)

    def call():
        rc = lib.pips_object_masks(p[0], p[1], 1, n, 0, 1, SRC[0], SRC[1], h, w, r8, vote, p[2], w, h * w, p[3], nbytes, stream)
        assert rc == 0, lib.pips_last_error()
    return call, out, ws


def _old_masks(rows, lab, size, radius8, vote, chunk=1 << 16):
    """the route of before: float32 squared distances from chunks of the pixel grid to the tracks, topk, gather (mode for a vote)"""
    (h, w), dev = size, rows.device
    s = torch.tensor([w / SRC[1], h / SRC[0]], device=dev)
    part = lab[0] != ops.MASK_NONE
    pos, l = ((rows[0] + 0.5) * s - 0.5)[part], lab[0][part].long()
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xx.flatten(), yy.flatten()], dim=1)
    out = torch.empty(h * w, dtype=torch.uint8, device=dev)
    r2 = (radius8 / 8.0) ** 2
    for a in range(0, h * w, chunk):
        d2 = ((grid[a:a + chunk, None, :] - pos[None]) ** 2).sum(dim=2)
        v, i = d2.topk(vote, dim=1, largest=False)
        near = torch.where(v <= r2, l[i], ops.MASK_NONE)
        out[a:a + chunk] = (near[:, 0] if vote == 1 else near.mode(dim=1).values).to(torch.uint8)
    return out.view(1, h, w)


def _surfaces(fmt, size, g, dev):
    h, w = size
    if fmt == "nv12":
        return [torch.randint(0, 256, (1, h, w), generator=g, dtype=torch.uint8).to(dev),
                torch.randint(0, 256, (1, h // 2, w // 2, 2), generator=g, dtype=torch.uint8).to(dev)]
    return [torch.randint(0, 256, (1, h, w, 4), generator=g, dtype=torch.uint8).to(dev)]


def _tint(lib, fmt, planes, mask, colors, alpha, stream):
    """one pips_masks_tint call on device surfaces -> call"""
    h, w = mask.shape[1:]
    args = ops.draw_surfaces(planes, fmt)
    table = (C.c_int * alpha.numel())(*alpha.reshape(-1).tolist())
    pm, pc = C.c_void_p(mask.data_ptr()), C.c_void_p(colors.data_ptr())

    def call():
        rc = lib.pips_masks_tint(ops.DRAW_FORMATS[fmt], 1, 0, 1, h, w, *args, pm, w, h * w, pc, table, alpha.shape[1], stream)
        assert rc == 0, lib.pips_last_error()
    return call


def _old_tint(planes, fmt, mask, colors, alpha):
    """the route of before: float blending per plane, the chroma weights by a 2 x 2 average pool"""
    l = mask[0].long().clamp(max=colors.shape[1])
    A = torch.cat([alpha[0].float() / 256.0, alpha.new_zeros(1).float()])[l]                     # (h,w); labels >= C: 0
    comp = (drivers.rgb_to_yuv_torch(colors[0]) if fmt == "nv12" else colors[0].long()).float()
    c = torch.cat([comp, comp.new_zeros(1, 3)])[l]                                                 # (h,w,3)
    if fmt == "nv12":
        y = (planes[0][0].float() * (1 - A) + c[..., 0] * A + 0.5).to(torch.uint8)
        pool = torch.nn.functional.avg_pool2d
        SA = pool(A[None, None], 2)[0, 0]
        Sc = pool((c[..., 1:] * A[..., None]).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
        uv = (planes[1][0].float() * (1 - SA[..., None]) + Sc + 0.5).to(torch.uint8)
        return [y[None], uv[None]]
    out = planes[0].clone()
    out[0, ..., :3] = (planes[0][0, ..., :3].float() * (1 - A[..., None]) + c * A[..., None] + 0.5).to(torch.uint8)
    return [out]


def _tint_tables(every, dev):
    colors = torch.tensor([[[40, 90, 200], [230, 60, 30]]], dtype=torch.uint8, device=dev)
    return colors, torch.tensor([[128 if every else 0, 128]])


def _event_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


RING = 40


def _ring_time(make, pristine):
    """us per call of the in-place calls ``make(planes)()``, each on a fresh copy of ``pristine``: a surface that was tinted before
    is left as it is by the next call (a sample the blend does not change is not stored), which would be another, cheaper run"""
    ring = [[p.clone() for p in pristine] for _ in range(RING + 4)]
    calls = [make(planes) for planes in ring]
    for call in calls[RING:]:
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for call in calls[:RING]:
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / RING


def _reduce(db):
    """the per-kernel table from the kernel trace of a ``--kernels`` run"""
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(re.search(r"mask_prepare_kernel|mask_raster_kernel|masks_tint_kernel", name).group(0), end - start) for name, start, end in rows
            if re.search(r"mask_prepare_kernel|mask_raster_kernel|masks_tint_kernel", name)]
    # the run's first masks (which the tints show) come ahead of the shapes
    want = 2 + 2 * TRACE_CALLS * len(MASK_SHAPES) + TRACE_CALLS * len(TINT_SHAPES)
    assert len(rows) == want, f"{len(rows)} launches in the trace, not {want}"
    rows = rows[2:]
    print(f"us per launch, medians of {TRACE_CALLS - 1} traced calls; byte time: the bytes the rule moves over the kernel's time")
    print(f"{'shape':44s} {'prepare':>9s} {'raster / tint':>14s} {'MB':>7s} {'GB/s':>8s}")
    at = 0
    for (size, n, vote) in MASK_SHAPES:
        seg = rows[at:at + 2 * TRACE_CALLS]
        at += 2 * TRACE_CALLS
        assert [k for k, _ in seg[:2]] == ["mask_prepare_kernel", "mask_raster_kernel"]
        prep = statistics.median(ns for k, ns in seg[2:] if k == "mask_prepare_kernel") / 1e3
        rast = statistics.median(ns for k, ns in seg[2:] if k == "mask_raster_kernel") / 1e3
        mb = size[0] * size[1] / 1e6
        print(f"{f'masks {size[0]}x{size[1]} n{n} vote{vote} r8={_radius8(size, n)}':44s} {prep:9.2f} {rast:14.2f} {mb:7.2f} {mb / rast * 1e3:8.1f}")
    for fmt, every in TINT_SHAPES:
        seg = rows[at:at + TRACE_CALLS]
        at += TRACE_CALLS
        us = statistics.median(ns for _, ns in seg[1:]) / 1e3
        px = TINT_SIZE[0] * TINT_SIZE[1]
        mb = px * (1 + 2 * (1.5 if fmt == "nv12" else 4)) / 1e6
        print(f"{f'tint {fmt} 1080x1920 ' + ('every label' if every else 'object alone'):44s} {'-':>9s} {us:14.2f} {mb:7.2f} {mb / us * 1e3:8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="21 calls per shape and nothing else: the run for a kernel trace")
    ap.add_argument("--reduce", default=None, metavar="TRACE.db", help="print the per-kernel table from the trace of a --kernels run")
    a = ap.parse_args()
    if a.reduce:
        _reduce(a.reduce)
        return
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(5)
    tracks = {n: tuple(t.to(dev) for t in _tracks(n, g)) for n in (256, 2048)}
    call, tint_mask, keep0 = _masks(lib, *tracks[TINT_N], TINT_SIZE, 1, stream)
    call()
    torch.cuda.synchronize()
    surfaces = {fmt: _surfaces(fmt, TINT_SIZE, g, dev) for fmt in ("nv12", "rgba32")}
    if a.kernels:
        for size, n, vote in MASK_SHAPES:
            call, out, keep = _masks(lib, *tracks[n], size, vote, stream)
            for _ in range(TRACE_CALLS):
                call()
            torch.cuda.synchronize()
            print(f"masks {size} n{n} vote{vote}: {TRACE_CALLS} calls", flush=True)
        for fmt, every in TINT_SHAPES:
            colors, alpha = _tint_tables(every, dev)
            for _ in range(TRACE_CALLS):                               # a fresh surface a call: a tinted one would be left as it is
                _tint(lib, fmt, [p.clone() for p in surfaces[fmt]], tint_mask, colors, alpha, stream)()
            torch.cuda.synchronize()
            print(f"tint {fmt} every={every}: {TRACE_CALLS} calls", flush=True)
        return
    rows = {}
    for rep in range(a.repeats):
        for size, n, vote in MASK_SHAPES:
            t, lab = tracks[n]
            r8 = _radius8(size, n)
            name = f"masks {size[0]}x{size[1]} n{n} vote{vote} radius {r8 / 8:.1f} px"
            call, out, keep = _masks(lib, t, lab, size, vote, stream)
            if rep == 0:
                call()
                torch.cuda.synchronize()
                ref = drivers.object_masks_torch(t[None], lab, SRC, out_size=size, radius=r8 / 8.0, vote=vote)
                assert torch.equal(out, ref), f"{name}: {int((out != ref).sum())} bytes differ from the twin"
                assert len(set(out.unique().tolist())) >= 3
                old = _old_masks(t, lab, size, r8, vote)
                agree = float((old == out).float().mean())
                # (float distances; ``mode`` breaks a tie among labels by value, the rule by distance: not every pixel agrees)
                assert agree > (0.99 if vote == 1 else 0.9), f"{name}: the old route agrees on {agree:.3f} of the pixels only"
            rows.setdefault(f"{name}: pips_object_masks, us/frame", []).append(_time(call, a.reps))
            rows.setdefault(f"{name}: chunked distances + topk + gather, us/frame", []).append(
                _event_time(lambda: _old_masks(t, lab, size, r8, vote), a.slow_reps))
        for fmt, every in TINT_SHAPES:
            colors, alpha = _tint_tables(every, dev)
            name = f"tint {fmt} 1080x1920 " + ("every label" if every else "object alone")
            planes = [p.clone() for p in surfaces[fmt]]
            call = _tint(lib, fmt, planes, tint_mask, colors, alpha, stream)
            if rep == 0:
                call()
                torch.cuda.synchronize()
                ref = drivers.tint_masks_torch(surfaces[fmt], fmt, tint_mask, colors, alpha / 256.0)
                ref = [ref] if torch.is_tensor(ref) else ref
                assert all(torch.equal(x, y) for x, y in zip(planes, ref)), f"{name}: bytes differ from the twin"
                assert any(not torch.equal(x, y) for x, y in zip(planes, surfaces[fmt]))
                old = _old_tint(surfaces[fmt], fmt, tint_mask, colors, alpha.to(dev))
                assert all(int((x.int() - y.int()).abs().max()) <= 2 for x, y in zip(old, ref)), f"{name}: the old route is off"
            rows.setdefault(f"{name}: pips_masks_tint, us/frame", []).append(
                _ring_time(lambda planes: _tint(lib, fmt, planes, tint_mask, colors, alpha, stream), surfaces[fmt]))
            d_alpha = alpha.to(dev)
            rows.setdefault(f"{name}: float blending per plane, us/frame", []).append(
                _event_time(lambda: _old_tint(surfaces[fmt], fmt, tint_mask, colors, d_alpha), a.slow_reps))
    out = {"device": torch.cuda.get_device_name(dev),
           "config": f"{a.reps} calls per figure ({RING} for the tint, each on a fresh surface; {a.slow_reps} for the old routes), "
                     f"{a.repeats} repeats, one frame a call"}
    print(f"device: {out['device']}")
    print(f"{'run':92s} {'(repeats)':>40s} {'median':>11s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:92s} {' '.join(f'{u:12.2f}' for u in us):>40s} {med:11.2f}")
        out[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    slower = [k for k in rows if "pips_" in k and statistics.median(rows[k]) >=
              statistics.median(next(v for q, v in rows.items() if q.startswith(k.split(":")[0] + ":") and "pips_" not in q))]
    out["library faster on every shape"] = not slower
    print(json.dumps(out), flush=True)
    assert not slower, slower


if __name__ == "__main__":
    main()
