"""pips_frames_import alone: microseconds per frame, bytes moved and TB/s for chunks of decoder frames, HIP events around ``reps``
back-to-back calls after a warm-up of each shape; every figure three times in one session, with its median.
  - sources 1080x1920 (chunks of 8) and 360x640 (chunks of 24); formats NV12, BGR24 and I420;
  - runs: no resize to uint8 (both sources); fused 1080x1920 -> 360x640 to float32 and to uint8;
  - comparators: (a) the two-step library path -- import at source size as uint8, then pips_resize_frames -- for the fused float
    run; (b) drivers.import_frames_torch on the same device tensors for every run (``reps`` / 10 calls).
The library calls go straight to the C entry points with buffers allocated once, so a figure is the launches and nothing of the
wrapper.  Bytes are the rule's own count: every source byte once, every output byte once (two-step: the uint8 planes written and
read once more); TB/s and the fraction of ``--peak`` (8 TB/s) follow from them.  The outputs are compared with the twin first: a
time of wrong frames is no time.  Prints a table and one JSON line.
``--antialias``: the antialiased downscale instead -- 1080x1920 (chunks of 8) and 2160x3840 (chunks of 4) of ``--fmt`` to the
model's 368x496 as float32, three routes in one run: the fused antialiased import (PIPS_FILTER_TRIANGLE), the fused bilinear
import, and the route there was before -- import at source size as uint8, then torch's F.interpolate(..., antialias=True) on the
device -- each with the source GB/s it achieves (source bytes of a frame over its time).
usage: python tools/import_bench.py [--reps 2000 --repeats 3 --peak 8.0] [--antialias [--fmt nv12|i420|bgr24|p010|i010]]"""
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

SRC_BYTES = {"nv12": 1.5, "i420": 1.5, "bgr24": 3.0, "p010": 3.0, "i010": 3.0}


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


def _planes(fmt, F, h, w, g, dev):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    semi, planar = [(F, h, w), (F, ch, cw, 2)], [(F, h, w), (F, ch, cw), (F, ch, cw)]
    shapes = {"nv12": semi, "i420": planar, "bgr24": [(F, h, w, 3)], "p010": semi, "i010": planar}[fmt]
    if fmt in ops.IMPORT_16BIT:                                 # 16-bit words, every bit random
        return [torch.randint(-32768, 32768, s, generator=g, dtype=torch.int16).to(dev) for s in shapes]
    return [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in shapes]


def _raw(lib, planes, fmt, dst, stream, filt=ops.FILTER_BILINEAR):
    """a closure that launches pips_frames_import_ex on contiguous planes into ``dst`` (F,3,H,W)"""
    F, h, w = planes[0].shape[:3]
    args = []
    for p in planes:
        args += [C.c_void_p(p.data_ptr()), p.stride(1) * p.element_size(), p.stride(0) * p.element_size()]
    args += [None, 0, 0] * (3 - len(planes))
    head = (ops.IMPORT_FORMATS[fmt], ops.IMPORT_MATRICES["bt709"], ops.IMPORT_RANGES["limited"], filt, F, h, w)
    tail = (C.c_void_p(dst.data_ptr()), int(dst.dtype == torch.uint8), dst.shape[2], dst.shape[3], stream)

    def call():
        rc = lib.pips_frames_import_ex(*head, *args, *tail)
        assert rc == 0, lib.pips_last_error()
    return call


def antialias_study(a, lib, stream, dev):
    """--antialias: the three routes to an antialiased (and the one to a bilinear) 368x496 float frame, per source size"""
    g = torch.Generator().manual_seed(2)
    H, W = 368, 496
    fmt = a.fmt
    rows = {}
    for rep in range(a.repeats):
        for (h, w), F in (((1080, 1920), 8), ((2160, 3840), 4)):
            planes = _planes(fmt, F, h, w, g, dev)
            src = SRC_BYTES[fmt] * h * w
            tag = f"{fmt} {h}x{w} F{F} -> {H}x{W} f32"
            small, aa = (torch.empty(F, 3, H, W, dtype=torch.float32, device=dev) for _ in range(2))
            as_u8 = torch.empty(F, 3, h, w, dtype=torch.uint8, device=dev)
            fused_aa, fused = _raw(lib, planes, fmt, aa, stream, ops.FILTER_TRIANGLE), _raw(lib, planes, fmt, small, stream)
            plain = _raw(lib, planes, fmt, as_u8, stream)
            resized = [None]

            def torch_route():
                plain()
                resized[0] = torch.nn.functional.interpolate(as_u8.float(), (H, W), mode="bilinear", antialias=True)
            fused_aa(), fused(), torch_route()
            if rep == 0:
                twin = drivers.import_frames_torch(planes, fmt, (H, W), dtype=torch.float32, antialias=True)
                assert torch.equal(aa.view(torch.int32), twin.view(torch.int32))
                assert torch.equal(small.view(torch.int32), drivers.import_frames_torch(planes, fmt, (H, W), dtype=torch.float32).view(torch.int32))
                print(f"{tag}: max |fused antialiased - torch route| = {float((aa - resized[0]).abs().max()):.5f}")
            for name, fn, nbytes in (("fused antialiased", fused_aa, src + 12 * H * W), ("fused bilinear", fused, src + 12 * H * W),
                                     ("import u8 + torch antialias", torch_route, src + 3 * h * w + 15 * h * w + 12 * H * W)):
                rows.setdefault(f"{tag}: {name}", (src, nbytes, []))[2].append(_time(fn, max(a.reps // 4, 10)) / F)
    out = {"config": f"{max(a.reps // 4, 10)} calls per figure, {a.repeats} repeats, format {fmt}"}
    print(f"{'run':64s} {'src MB/frame':>12s} {'us/frame (repeats)':>30s} {'median':>8s} {'src GB/s':>9s}")
    for name, (src, nbytes, us) in rows.items():
        med = statistics.median(us)
        print(f"{name:64s} {src / 1e6:12.2f} {' '.join(f'{u:9.2f}' for u in us):>30s} {med:8.2f} {src / med * 1e-3:9.1f}")
        out[name] = {"source_bytes_per_frame": int(src), "bytes_moved_per_frame": int(nbytes), "us_per_frame": [round(u, 3) for u in us],
                     "median_us_per_frame": round(med, 3), "source_gb_per_s": round(src / med * 1e-3, 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--peak", type=float, default=8.0, help="HBM bandwidth the fractions refer to, TB/s")
    ap.add_argument("--antialias", action="store_true", help="the antialiased downscale to 368x496: fused, bilinear and the torch route")
    ap.add_argument("--fmt", default="nv12", choices=sorted(SRC_BYTES), help="the source format of --antialias")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if a.antialias:
        return antialias_study(a, lib, stream, dev)
    g = torch.Generator().manual_seed(1)
    H, W = 360, 640
    rows = {}                                                   # name -> (bytes per frame, [us per frame of each repeat])

    def record(name, nbytes, us_per_frame):
        rows.setdefault(name, (nbytes, []))[1].append(us_per_frame)

    for rep in range(a.repeats):
        for (h, w), F in (((1080, 1920), 8), ((360, 640), 24)):
            for fmt in ("nv12", "bgr24", "i420"):
                planes = _planes(fmt, F, h, w, g, dev)
                src = SRC_BYTES[fmt] * h * w
                tag = f"{fmt} {h}x{w} F{F}"
                as_u8 = torch.empty(F, 3, h, w, dtype=torch.uint8, device=dev)
                plain = _raw(lib, planes, fmt, as_u8, stream)
                plain()
                if rep == 0:
                    assert torch.equal(as_u8, drivers.import_frames_torch(planes, fmt))
                record(f"{tag} -> u8: library", src + 3 * h * w, _time(plain, a.reps) / F)
                record(f"{tag} -> u8: torch twin", src + 3 * h * w,
                       _time(lambda: drivers.import_frames_torch(planes, fmt), max(a.reps // 10, 10)) / F)
                if (h, w) == (H, W):
                    continue
                for dt, es in ((torch.float32, 4), (torch.uint8, 1)):
                    small = torch.empty(F, 3, H, W, dtype=dt, device=dev)
                    fused = _raw(lib, planes, fmt, small, stream)
                    fused()
                    name = "f32" if es == 4 else "u8"
                    if rep == 0:
                        twin = drivers.import_frames_torch(planes, fmt, (H, W), dtype=dt)
                        assert torch.equal(small.view(torch.uint8), twin.view(torch.uint8))
                    record(f"{tag} -> {H}x{W} {name}: fused", src + 3 * es * H * W, _time(fused, a.reps) / F)
                    record(f"{tag} -> {H}x{W} {name}: torch twin", src + 3 * es * H * W,
                           _time(lambda: drivers.import_frames_torch(planes, fmt, (H, W), dtype=dt), max(a.reps // 10, 10)) / F)
                    if es == 4:
                        def two_step():
                            plain()
                            rc = lib.pips_resize_frames(C.c_void_p(as_u8.data_ptr()), 1, 3 * F, h, w, C.c_void_p(two.data_ptr()), H, W, stream)
                            assert rc == 0
                        two = torch.empty_like(small)
                        two_step()
                        if rep == 0:
                            assert torch.equal(two.view(torch.uint8), small.view(torch.uint8))
                        record(f"{tag} -> {H}x{W} f32: two-step library", src + 6 * h * w + 12 * H * W, _time(two_step, a.reps) / F)
    out = {"config": f"{a.reps} calls per library figure, {max(a.reps // 10, 10)} per torch figure, {a.repeats} repeats, peak {a.peak} TB/s"}
    print(f"{'run':58s} {'MB/frame':>9s} {'us/frame (repeats)':>30s} {'median':>8s} {'TB/s':>6s} {'of peak':>8s}")
    for name, (nbytes, us) in rows.items():
        med = statistics.median(us)
        tbs = nbytes / med * 1e-6
        print(f"{name:58s} {nbytes / 1e6:9.2f} {' '.join(f'{u:9.2f}' for u in us):>30s} {med:8.2f} {tbs:6.2f} {tbs / a.peak:8.1%}")
        out[name] = {"bytes_per_frame": int(nbytes), "us_per_frame": [round(u, 3) for u in us], "median_us_per_frame": round(med, 3),
                     "tb_per_s": round(tbs, 3), "fraction_of_peak": round(tbs / a.peak, 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
