"""pips_motion_fit alone: microseconds per pair for the consensus similarity between consecutive rows, HIP events around ``reps``
back-to-back calls after a warm-up of each shape; every figure ``repeats`` times in one session, with its median.
  - n = 256 and 2048 tracks, K = 256 hypotheses, thr 2 px, calls of 8 rows (7 pairs) and 64 rows (63 pairs): rows of a scene in
    368x496 coordinates that moves by a similarity of its own per frame, +-0.25 px noise, 30 % of the tracks going their own way;
  - two yardsticks measured in the same run: drivers.motion_table_torch on the same rows on the same GPU (a host clock around a call
    that ends in a synchronise: it reads counts back pair by pair), and pips_tracks_draw of the same rows onto 1080x1920 NV12
    surfaces, one per row (trail 16), in microseconds per frame;
  - ``--tune-lib PATH``: a tuning build of the library (python -m pips_amd._build --tuning).  Its scoring launch is timed in two
    child processes, one after the other, alternating per repeat: as the product runs it (a block per pair and 64 hypotheses: 4
    blocks a pair at K = 256) and with PIPS_MOTION_ONE_BLOCK=1 (a block per pair and 256 hypotheses: one block a pair).
The library calls go straight to the C entry point with buffers allocated once, so a figure is the three launches and nothing of
the wrapper.  Every shape is compared with drivers.motion_table_torch first: a time of wrong models is no time.  Prints a table and
one JSON line.
usage: python tools/motion_bench.py [--reps 500 --repeats 3 --tune-lib pips_amd/libpips_hip_tune.so]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import _lib, drivers, ops  # noqa: E402

H, W, TRAIL, K, THR4, SEED = 368, 496, 16, 256, 8, 1234
SHAPES = [(8, 256), (8, 2048), (64, 256), (64, 2048)]                  # (rows of a call, tracks)
SURFACE = (1080, 1920)


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


def _rows(F, n, g):
    """F rows of n tracks: row f is row f - 1 under a small similarity plus +-0.25 px noise; 30 % of the tracks wander"""
    rows = [torch.rand(n, 2, generator=g, dtype=torch.float64) * torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)]
    wild = torch.rand(n, generator=g) < 0.3
    for _ in range(1, F):
        ang, sc = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([math.radians(2.0), 0.02], dtype=torch.float64)
        a = (1.0 + float(sc)) * complex(math.cos(float(ang)), math.sin(float(ang)))
        p = rows[-1]
        q = torch.stack([a.real * p[:, 0] - a.imag * p[:, 1], a.imag * p[:, 0] + a.real * p[:, 1]], dim=1)
        q = q + (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * 6.0 + (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 0.5
        q[wild] += torch.randn(int(wild.sum()), 2, generator=g, dtype=torch.float64) * 6.0
        rows.append(q)
    return torch.stack(rows).to(torch.float32)


def _fit(lib, trajs, stream):
    """one pips_motion_fit call on device rows, buffers allocated once -> (call, outputs)"""
    F, n = trajs.shape[:2]
    dev = trajs.device
    head = torch.empty(F - 1, 4, dtype=torch.int32, device=dev)
    sums = torch.empty(F - 1, 8, dtype=torch.int64, device=dev)
    model = torch.empty(F - 1, 4, dtype=torch.float64, device=dev)
    flags = torch.empty(F - 1, n, dtype=torch.uint8, device=dev)
    nbytes = ops.motion_workspace_bytes(F, n, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = [C.c_void_p(t.data_ptr()) for t in (trajs, head, sums, model, flags, ws)]

    def call():
        rc = lib.pips_motion_fit(p[0], None, F, n, 0, 0.0, K, THR4, SEED, p[1], p[2], p[3], p[4], p[5], nbytes, stream)
        assert rc == 0, lib.pips_last_error()
    return call, (head, sums, model, flags)


def _draw(lib, trajs, stream, g):
    """pips_tracks_draw of the rows onto one 1080p NV12 surface per row"""
    F, n = trajs.shape[:2]
    dev, (h, w) = trajs.device, SURFACE
    planes = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in ((F, h, w), (F, h // 2, w // 2, 2))]
    colors = drivers.track_colors(torch.arange(n)).to(dev)
    ws = torch.empty(ops.draw_workspace_bytes(F, n, TRAIL) // 4, dtype=torch.int32, device=dev)
    args = []
    for q in planes:
        args += [C.c_void_p(q.data_ptr()), q.stride(1) * q.element_size(), q.stride(0) * q.element_size()]
    head = (ops.DRAW_FORMATS["nv12"], ops.IMPORT_MATRICES["bt709"], ops.IMPORT_RANGES["limited"], F, h, w, *args, None, 0, 0,
            C.c_void_p(trajs.data_ptr()), None, F, n, 0, H, W, C.c_void_p(colors.data_ptr()), TRAIL, 8, 24, 256, 90, 0.0,
            C.c_void_p(ws.data_ptr()), ws.numel() * 4, stream)

    def call():
        rc = lib.pips_tracks_draw(*head)
        assert rc == 0, lib.pips_last_error()
    return call, (planes, colors, ws)


def _fit_times(reps, check):
    """microseconds per pair of the bound library's pips_motion_fit on every shape (seeded rows: the same in every process)"""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for F, n in SHAPES:
        trajs = _rows(F, n, torch.Generator().manual_seed(100 * F + n)).to(dev)
        call, got = _fit(lib, trajs, stream)
        if check:
            call()
            torch.cuda.synchronize()
            ref = drivers.motion_table_torch(trajs.cpu(), None, 0, 0.0, K, THR4, SEED)
            assert torch.equal(got[0].cpu().long(), ref[0]) and torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[3].cpu(), ref[3])
            assert torch.equal(got[2].cpu().view(torch.int64), ref[2].view(torch.int64)) and int(ref[0][:, 1].min()) >= n // 4
        out[f"F{F} n{n}"] = _time(call, reps) / (F - 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tune-lib", default=None)
    ap.add_argument("--fit-only", action="store_true", help="(the child processes of --tune-lib) the fit of the bound library, as JSON")
    a = ap.parse_args()
    if a.fit_only:
        print(json.dumps(_fit_times(a.reps, check=True)), flush=True)
        return
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = {}
    for rep in range(a.repeats):
        for name, us in _fit_times(a.reps, check=rep == 0).items():
            rows.setdefault(f"{name} K{K}: pips_motion_fit, us/pair", []).append(us)
        for F, n in SHAPES:
            g = torch.Generator().manual_seed(100 * F + n)
            trajs = _rows(F, n, g).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                drivers.motion_table_torch(trajs, None, 0, 0.0, K, THR4, SEED)
            torch.cuda.synchronize()
            rows.setdefault(f"F{F} n{n} K{K}: motion_table_torch on the GPU, us/pair", []).append((time.perf_counter() - t0) * 1e6 / 3 / (F - 1))
            call, keep = _draw(lib, trajs, stream, g)
            rows.setdefault(f"F{F} n{n}: pips_tracks_draw 1080p NV12 trail {TRAIL}, us/frame", []).append(_time(call, max(a.reps // 10, 20)) / F)
            del keep
        if a.tune_lib:
            for hook, tag in (("0", "4 blocks a pair (as the product)"), ("1", "one block a pair")):
                env = dict(os.environ, PIPS_LIB_PATH=os.path.abspath(a.tune_lib), PIPS_MOTION_ONE_BLOCK=hook)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--fit-only", "--reps", str(a.reps)], env=env,
                                     capture_output=True, text=True, timeout=300)
                assert res.returncode == 0, res.stderr[-2000:]
                for name, us in json.loads(res.stdout.strip().splitlines()[-1]).items():
                    rows.setdefault(f"{name} K{K}: tuning build, {tag}, us/pair", []).append(us)
    out = {"device": torch.cuda.get_device_name(dev),
           "config": f"{a.reps} calls per figure, {a.repeats} repeats, K={K} hypotheses, thr {THR4 / 4} px, rows in {H}x{W} coordinates"}
    print(f"device: {out['device']}")
    print(f"{'run':74s} {'(repeats)':>36s} {'median':>10s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:74s} {' '.join(f'{u:11.2f}' for u in us):>36s} {med:10.2f}")
        out[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
