"""pips_motion_layers alone: microseconds per pair for L motion layers between consecutive rows, by tools/motion_bench.py's method --
HIP events around ``reps`` back-to-back calls after a warm-up of each shape, every figure ``repeats`` times in one session, with
its median; the library calls go straight to the C entry point with buffers allocated once.
  - n = 256 and 2048 tracks, K = 256 hypotheses, thr 2 px, min_in 8, calls of 8 rows (7 pairs) and 64 rows (63 pairs), L = 1 and 4:
    motion_bench's rows (a scene in 368x496 coordinates that moves by a similarity of its own per frame, 30 % of the tracks going
    their own way), of which a fifth and an eighth of the tracks also move by a shift of their own: two layers to find;
  - beside it pips_motion_fit on the same rows (layer 0 alone, three launches);
  - beside it the route a host had before pips_motion_layers: per pair and layer one ops.motion_fit on a two-row slice, with torch
    masking between the calls (the inliers of a layer that has a model get NaN positions, by torch.where on the device: nothing is
    read back in between).  A host clock around ``slow_reps`` runs that end in a synchronise.  ops.motion_fit allocates its outputs
    and workspace on every call, as a host on this route would through the Python wrapper: the figure is that of the route as
    open in Python, an upper figure for a C host that keeps its buffers;
  - ``--kernels``: 21 L = 4 calls per shape and nothing else -- the run to put under a kernel trace
    (rocprofv3 --kernel-trace --stats -d DIR -- python tools/motion_layers_bench.py --kernels);
  - ``--reduce TRACE.db [--bench BENCH.txt]``: needs no GPU.  Reads the ``kernels`` view of the SQLite database that trace wrote,
    drops the first call of each shape and prints, per shape, the median over the other 20 calls of each kernel's time summed over
    its launches in a call; with the saved output of a plain run of this tool (its JSON line) also the call's untraced time and the
    launch floor of a call: its time at L = 4 minus L times the score and select kernels' own time.
Every shape is compared with drivers.motion_layers_table_torch first, and the old route's labels with the library's: a time of
wrong layers is no time.  Prints a table and one JSON line.
usage: python tools/motion_layers_bench.py [--reps 500 --repeats 3 --slow-reps 2] [--kernels | --reduce TRACE.db [--bench BENCH.txt]]"""
import argparse
import ctypes as C
import json
import os
import re
import sqlite3
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from motion_bench import K, SEED, SHAPES, THR4, _rows, _time  # noqa: E402
from pips_amd import _lib, drivers, ops  # noqa: E402

LAYERS, MIN_IN = (1, 4), 8
SHIFTS = ((9.0, 0.0), (0.0, -10.0))                                      # px a frame, of a fifth and an eighth of the tracks


def _layer_rows(F, n, g):
    """motion_bench's rows with two groups of tracks that move by a constant shift of their own a frame on top of the camera"""
    rows = _rows(F, n, g).double()
    steps = torch.arange(F, dtype=torch.float64).view(F, 1, 1)
    a, b = n // 5, n // 5 + n // 8
    rows[:, :a] += steps * torch.tensor(SHIFTS[0], dtype=torch.float64)
    rows[:, a:b] += steps * torch.tensor(SHIFTS[1], dtype=torch.float64)
    return rows.to(torch.float32)


def _layers(lib, trajs, L, stream):
    """one pips_motion_layers call on device rows, buffers allocated once -> (call, outputs)"""
    F, n = trajs.shape[:2]
    dev, P = trajs.device, trajs.shape[0] - 1
    out = (torch.empty(P, L, 4, dtype=torch.int32, device=dev), torch.empty(P, L, 8, dtype=torch.int64, device=dev),
           torch.empty(P, L, 4, dtype=torch.float64, device=dev), torch.empty(P, L, 4, dtype=torch.int32, device=dev),
           torch.empty(P, n, dtype=torch.uint8, device=dev), torch.empty(P, L, L, dtype=torch.int32, device=dev))
    nbytes = ops.motion_layers_workspace_bytes(F, n, K, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = [C.c_void_p(t.data_ptr()) for t in (trajs, *out, ws)]

    def call():
        rc = lib.pips_motion_layers(p[0], None, None, F, n, 0, 0.0, K, THR4, SEED, L, MIN_IN, p[1], p[2], p[3], p[4], p[5], p[6], p[7],
                                    nbytes, stream)
        assert rc == 0, lib.pips_last_error()
    return call, out + (ws,)


def _fit(lib, trajs, stream):
    F, n = trajs.shape[:2]
    dev = trajs.device
    out = (torch.empty(F - 1, 4, dtype=torch.int32, device=dev), torch.empty(F - 1, 8, dtype=torch.int64, device=dev),
           torch.empty(F - 1, 4, dtype=torch.float64, device=dev), torch.empty(F - 1, n, dtype=torch.uint8, device=dev))
    nbytes = ops.motion_workspace_bytes(F, n, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = [C.c_void_p(t.data_ptr()) for t in (trajs, *out, ws)]

    def call():
        rc = lib.pips_motion_fit(p[0], None, F, n, 0, 0.0, K, THR4, SEED, p[1], p[2], p[3], p[4], p[5], nbytes, stream)
        assert rc == 0, lib.pips_last_error()
    return call, out + (ws,)


def _old_route(trajs, L):
    """the layers by the entry points of before: per pair and layer one ops.motion_fit on a two-row slice, the inliers of a layer
    with a model masked out by torch ops on the device between the calls -> layer (P,n) uint8"""
    F, n = trajs.shape[:2]
    labels = torch.full((F - 1, n), 255, dtype=torch.uint8, device=trajs.device)
    for f in range(1, F):
        cur = trajs[f - 1:f + 1].clone()
        for l in range(L):
            head, _, _, flags = ops.motion_fit(cur, None, f - 1, 0.0, K, THR4, (SEED + l * drivers.MOTION_LAYER_SEED) & 0xFFFFFFFF)
            if l == 0:
                labels[f - 1] = torch.where(flags[0] >= 1, 254, 255).to(torch.uint8)
            take = (flags[0] == 2) & (head[0, 1] >= (2 if l == 0 else MIN_IN))
            labels[f - 1] = torch.where(take, torch.full_like(labels[f - 1], l), labels[f - 1])
            cur = torch.where(take.view(1, n, 1), torch.full_like(cur, float("nan")), cur)
    return labels


TRACE_CALLS, TRACE_LAUNCHES = 21, 1 + 2 * 4 + 1
KERNELS = ("motion_compact_kernel", "motion_score_kernel", "motion_layers_select_kernel", "motion_overlap_kernel")


def _reduce(db, bench):
    """the per-kernel table of an L = 4 call from the kernel trace of a ``--kernels`` run (and the untraced call from ``bench``)"""
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(re.search(r"motion_\w+", name).group(0), end - start) for name, start, end in rows if "motion_" in name]
    assert len(rows) == len(SHAPES) * TRACE_CALLS * TRACE_LAUNCHES, f"{len(rows)} motion launches in the trace"
    calls = {}
    if bench:
        line = [text for text in open(bench).read().splitlines() if text.startswith("{")][-1]
        calls = {k: v["median"] for k, v in json.loads(line).items() if isinstance(v, dict)}
    print(f"us per call at L = 4, medians of {TRACE_CALLS - 1} traced calls: 1 compact, 4 score, 4 select, 1 overlap launch")
    print(f"{'shape':12s} {'compact':>9s} {'4 x score':>10s} {'4 x select':>11s} {'overlap':>9s} {'all ten':>9s} {'call, untraced':>15s} "
          f"{'call - 4 x (score + select)':>28s}")
    for s, (F, n) in enumerate(SHAPES):
        per = TRACE_CALLS * TRACE_LAUNCHES
        seg = rows[s * per:(s + 1) * per]
        med = {}
        for k in KERNELS:
            each = [sum(ns for name, ns in seg[c * TRACE_LAUNCHES:(c + 1) * TRACE_LAUNCHES] if name == k) / 1e3 for c in range(1, TRACE_CALLS)]
            med[k] = statistics.median(each)
        whole = statistics.median(sum(ns for _, ns in seg[c * TRACE_LAUNCHES:(c + 1) * TRACE_LAUNCHES]) / 1e3 for c in range(1, TRACE_CALLS))
        us = calls.get(f"F{F} n{n} K{K} L4: pips_motion_layers, us/pair")
        call = f"{us * (F - 1):15.2f}" if us is not None else f"{'-':>15s}"
        floor = f"{us * (F - 1) - med[KERNELS[1]] - med[KERNELS[2]]:28.2f}" if us is not None else f"{'-':>28s}"
        print(f"{f'F{F} n{n}':12s} {med[KERNELS[0]]:9.2f} {med[KERNELS[1]]:10.2f} {med[KERNELS[2]]:11.2f} {med[KERNELS[3]]:9.2f} {whole:9.2f} "
              f"{call} {floor}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="one L = 4 call per shape and nothing else: the run for a kernel trace")
    ap.add_argument("--reduce", default=None, metavar="TRACE.db", help="print the per-kernel table from the trace of a --kernels run")
    ap.add_argument("--bench", default=None, metavar="BENCH.txt", help="(with --reduce) the saved output of a plain run: the untraced call")
    a = ap.parse_args()
    if a.reduce:
        _reduce(a.reduce, a.bench)
        return
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if a.kernels:
        for F, n in SHAPES:
            call, keep = _layers(lib, _layer_rows(F, n, torch.Generator().manual_seed(100 * F + n)).to(dev), 4, stream)
            for _ in range(TRACE_CALLS):
                call()
            torch.cuda.synchronize()
            print(f"F{F} n{n} K{K} L4: {TRACE_CALLS} calls", flush=True)
        return
    rows = {}
    for rep in range(a.repeats):
        for F, n in SHAPES:
            trajs = _layer_rows(F, n, torch.Generator().manual_seed(100 * F + n)).to(dev)
            name = f"F{F} n{n} K{K}"
            for L in LAYERS:
                call, got = _layers(lib, trajs, L, stream)
                if rep == 0:
                    call()
                    torch.cuda.synchronize()
                    ref = drivers.motion_layers_table_torch(trajs.cpu(), None, 0, 0.0, K, THR4, SEED, L, MIN_IN)
                    assert all(torch.equal(got[k].cpu().long(), ref[k].long()) for k in (0, 1, 3, 4, 5))
                    assert torch.equal(got[2].cpu().view(torch.int64), ref[2].view(torch.int64))
                    assert L == 1 or int((ref[0][:, 1:3, 2] >= 0).sum()) == 2 * (F - 1)        # the two planted layers are found
                    assert torch.equal(_old_route(trajs, L).cpu(), ref[4])
                rows.setdefault(f"{name} L{L}: pips_motion_layers, us/pair", []).append(_time(call, a.reps) / (F - 1))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.slow_reps):
                    _old_route(trajs, L)
                torch.cuda.synchronize()
                rows.setdefault(f"{name} L{L}: ops.motion_fit per pair and layer + torch masking, us/pair", []).append(
                    (time.perf_counter() - t0) * 1e6 / a.slow_reps / (F - 1))
            call, keep = _fit(lib, trajs, stream)
            rows.setdefault(f"{name}: pips_motion_fit, us/pair", []).append(_time(call, a.reps) / (F - 1))
    out = {"device": torch.cuda.get_device_name(dev),
           "config": f"{a.reps} calls per figure ({a.slow_reps} for the old route), {a.repeats} repeats, K={K} hypotheses, thr {THR4 / 4} px, "
                     f"min_in {MIN_IN}"}
    print(f"device: {out['device']}")
    print(f"{'run':84s} {'(repeats)':>36s} {'median':>10s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:84s} {' '.join(f'{u:11.2f}' for u in us):>36s} {med:10.2f}")
        out[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
