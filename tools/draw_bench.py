"""pips_tracks_draw and pips_tracks_draw_ex alone: microseconds per frame for drawing tracks onto decoder surfaces in place, HIP
events around ``reps`` back-to-back calls after a warm-up of each shape; every figure ``repeats`` times in one session, with its
median.
  - surfaces 1080x1920 (chunks of 8) and 2160x3840 (chunks of 4), BT.709 limited; NV12 by default, ``--fmt`` takes a comma-separated
    list of nv12, p010 and i010 (the 16-bit formats go through pips_tracks_draw_ex);
  - n = 256 and 2048 tracks in the model's 368x496 coordinates (``size=``), trail 16, from a seeded random walk over the frame;
  - ``--fade linear`` times every format with the linear fade table too (pips_tracks_draw_ex), beside the figure without it; the
    variants of one shape alternate within a repeat;
  - ``--baseline-lib PATH``: another build of the library (the parent commit's, say) whose pips_tracks_draw on NV12 is timed in the
    same session, alternating with this one's;
  - beside each NV12 shape: the same surfaces' import to the model's size (pips_frames_import_ex, antialiased, float32), and the
    memory time of reading and writing the surfaces once (a device copy of both planes).
The library calls go straight to the C entry points with buffers allocated once, so a figure is the launches and nothing of the
wrapper.  A small case (4 tracks, one frame) is compared with drivers.draw_tracks_torch for each variant and size first: a time of
wrong frames is no time.  Drawing in place again and again blends the same tracks deeper into the same pixels; the work per call
stays the same.  Prints a table and one JSON line.
usage: python tools/draw_bench.py [--reps 200 --repeats 3 --fmt nv12,p010,i010 --fade linear --sizes 1080 --baseline-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import _lib, drivers, ops  # noqa: E402

H, W, TRAIL = 368, 496, 16
SIZES = {"1080": ((1080, 1920), 8), "2160": ((2160, 3840), 4)}


def _time(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _walk(G, n, g, dev):
    """n random walks of G rows over the model's frame: starts anywhere, steps of about 2 px (6 to 9 px on the surfaces)"""
    start = torch.rand(1, n, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    return (start + torch.cumsum(torch.randn(G, n, 2, generator=g) * 2.0, dim=0)).to(dev), (torch.randn(G, n, generator=g) * 2.0).to(dev)


def _surfaces(fmt, F, h, w, g, dev):
    """random surfaces of ``fmt``: bytes for nv12, whole 16-bit words (junk in the unused bits) for p010 and i010"""
    if fmt == "nv12":
        return [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in ((F, h, w), (F, h // 2, w // 2, 2))]
    shapes = ((F, h, w), (F, h // 2, w // 2, 2)) if fmt == "p010" else ((F, h, w), (F, h // 2, w // 2), (F, h // 2, w // 2))
    return [torch.randint(-32768, 32768, s, generator=g, dtype=torch.int16).to(dev) for s in shapes]


def _draw(lib, fmt, planes, trajs, vis, colors, first, ws, stream, fade=None):
    """one call of pips_tracks_draw (nv12 without a table) or pips_tracks_draw_ex on ``lib``"""
    F, h, w = planes[0].shape
    G, n = vis.shape
    args = []
    for p in planes:
        args += [C.c_void_p(p.data_ptr()), p.stride(1) * p.element_size(), p.stride(0) * p.element_size()]
    args += [None, 0, 0] * (3 - len(planes))
    head = (ops.DRAW_FORMATS_EX[fmt], ops.IMPORT_MATRICES["bt709"], ops.IMPORT_RANGES["limited"], F, h, w, *args,
            C.c_void_p(trajs.data_ptr()), C.c_void_p(vis.data_ptr()), G, n, first, H, W, C.c_void_p(colors.data_ptr()), TRAIL, 8, 24,
            256, 90, 0.0)
    tail = (C.c_void_p(ws.data_ptr()), ws.numel() * 4, stream)
    ex = fmt != "nv12" or fade is not None
    table = None if fade is None else (C.c_int * TRAIL)(*fade)

    def call():
        rc = lib.pips_tracks_draw_ex(*head, table, *tail) if ex else lib.pips_tracks_draw(*head, *tail)
        assert rc == 0, lib.pips_last_error()
    return call


def _import(lib, planes, dst, stream):
    F, h, w = planes[0].shape
    args = []
    for p in planes:
        args += [C.c_void_p(p.data_ptr()), p.stride(1), p.stride(0)]

    def call():
        rc = lib.pips_frames_import_ex(ops.IMPORT_FORMATS["nv12"], 1, 0, ops.FILTER_TRIANGLE, F, h, w, *args, None, 0, 0,
                                       C.c_void_p(dst.data_ptr()), 0, H, W, stream)
        assert rc == 0, lib.pips_last_error()
    return call


def _baseline(path):
    """another build of the library, with the one entry point this tool times on it"""
    lib = C.CDLL(os.path.abspath(path))
    name, (res, argtypes) = "pips_tracks_draw", _lib.SIGNATURES["pips_tracks_draw"]
    getattr(lib, name).restype, getattr(lib, name).argtypes = res, argtypes
    lib.pips_last_error.restype = C.c_char_p
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fmt", default="nv12", help="comma-separated: nv12, p010, i010")
    ap.add_argument("--fade", default="none", choices=("none", "linear"))
    ap.add_argument("--sizes", default="1080,2160", help="comma-separated: 1080, 2160")
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    fmts = a.fmt.split(",")
    assert all(f in ("nv12", "p010", "i010") for f in fmts) and all(s in SIZES for s in a.sizes.split(","))
    linear = drivers._draw_fade("linear", TRAIL)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    base = _baseline(a.baseline_lib) if a.baseline_lib else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(3)
    rows = {}
    for rep in range(a.repeats):
        for (h, w), F in (SIZES[s] for s in a.sizes.split(",")):
            surfaces = {fmt: _surfaces(fmt, F, h, w, g, dev) for fmt in fmts}
            if rep == 0:                                        # the kernels against the twin at this size, on a case the twin can hold
                t4, v4 = _walk(TRAIL + 1, 4, g, dev)
                for fmt in fmts:
                    for fade in (None, "linear") if a.fade == "linear" else (None,):
                        one = [p[:1].clone() for p in surfaces[fmt]]
                        kw = dict(size=(H, W), first=TRAIL, trail=TRAIL, fade=fade)
                        want = drivers.draw_tracks_torch(one, fmt, t4.unsqueeze(0), v4.unsqueeze(0), **kw)
                        got = drivers.draw_tracks(one, fmt, t4.unsqueeze(0), v4.unsqueeze(0), **kw)
                        assert all(torch.equal(x, y) for x, y in zip(got, want)) and not torch.equal(got[0], one[0])
                        del want, got
            if "nv12" in fmts:
                planes = surfaces["nv12"]
                spare = [torch.empty_like(p) for p in planes]
                small = torch.empty(F, 3, H, W, dtype=torch.float32, device=dev)
                tag = f"nv12 {h}x{w} F{F}"
                rows.setdefault(f"{tag}: import to {H}x{W} f32 (antialiased)", []).append(_time(_import(lib, planes, small, stream), a.reps) / F)

                def copy():
                    for d, s in zip(spare, planes):
                        d.copy_(s)
                rows.setdefault(f"{tag}: read + write the surfaces once (device copy)", []).append(_time(copy, a.reps) / F)
                del spare, small
            for n in (256, 2048):
                trajs, vis = _walk(TRAIL + F, n, g, dev)
                colors = drivers.track_colors(torch.arange(n)).to(dev)
                ws = torch.empty(ops.draw_workspace_bytes(F, n, TRAIL) // 4, dtype=torch.int32, device=dev)
                for fmt in fmts:
                    tag = f"{fmt} {h}x{w} F{F}"
                    call = _draw(lib, fmt, surfaces[fmt], trajs, vis, colors, TRAIL, ws, stream)
                    rows.setdefault(f"{tag}: draw n={n} trail={TRAIL}", []).append(_time(call, a.reps) / F)
                    if base is not None and fmt == "nv12":
                        call = _draw(base, fmt, surfaces[fmt], trajs, vis, colors, TRAIL, ws, stream)
                        rows.setdefault(f"{tag}: draw n={n} trail={TRAIL} (baseline library)", []).append(_time(call, a.reps) / F)
                    if a.fade == "linear":
                        call = _draw(lib, fmt, surfaces[fmt], trajs, vis, colors, TRAIL, ws, stream, linear)
                        rows.setdefault(f"{tag}: draw n={n} trail={TRAIL} fade=linear", []).append(_time(call, a.reps) / F)
            del surfaces
    out = {"device": torch.cuda.get_device_name(dev),
           "config": f"{a.reps} calls per figure, {a.repeats} repeats, tracks in {H}x{W} coordinates, line 2 px, dot 3 px"}
    print(f"device: {out['device']}")
    print(f"{'run':66s} {'us/frame (repeats)':>32s} {'median':>9s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:66s} {' '.join(f'{u:10.2f}' for u in us):>32s} {med:9.2f}")
        out[name] = {"us_per_frame": [round(u, 3) for u in us], "median_us_per_frame": round(med, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
