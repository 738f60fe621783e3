"""Several streamed videos at once: V sequential drivers.StreamTracker runs against one drivers.MultiStreamTracker.

360x640 frames, stride 4, T = 100 frames per stream, 256 query points per stream (a 16 x 16 grid) split over frames
0/33/66/99, seeded synthetic uint8 frames made on the host (one seed per stream), 4 frames per stream per push, rings of 24
slots, library rounds everywhere.  For each V of --streams (default 1, 4, 8) three modes are timed on one GPU, alternating,
after a warm-up of each:
  sequential    V StreamTracker(rounds="library") runs, one after the other (the baseline: the same commit)
  multi         one MultiStreamTracker(rounds="library"): per-stream encoder passes, one round for all streams
  multi_joint   the same with joint_encode=True: shared encoder passes
A figure is the median of --reps (3) calls; the whole comparison is repeated --runs (5) times and every run's medians are
printed with their own median.  The outputs of ``multi`` are compared with the sequential ones as bit patterns; ``multi_joint``
reports its largest difference instead.  The library's rounds per call are counted, and the fp32 GEMM routes of the mixer at
the row counts 8 * 256 * k, k = 1..V, reported (the batched rounds leave route 0 where the sequential ones stay on it).
Prints one JSON line per V."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pips_amd import Pips, _lib, drivers  # noqa: E402
from pips_amd.weights import init_state_dict  # noqa: E402
from tools.stream_bench import H, W, STRIDE, N, SLOTS, frames, queries  # noqa: E402

PUSH = 4
MODES = ("sequential", "multi", "multi_joint")


def pushes(hosts):
    T = hosts[0].shape[1]
    return [[h[:, t0:t0 + PUSH] for h in hosts] for t0 in range(0, T, PUSH)]


def run(mode, m, qs, hosts):
    """-> per stream (trajs (1,T,N,2), vis (1,T,N))"""
    if mode == "sequential":
        return [drivers.track_stream(m, [w[v] for w in pushes(hosts)], q, iters=6, slots=SLOTS, rounds="library")
                for v, q in enumerate(qs)]
    lists = [[w[v] for w in pushes(hosts)] for v in range(len(hosts))]
    return drivers.track_streams(m, lists, qs, iters=6, slots=SLOTS, rounds="library", joint_encode=mode == "multi_joint")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def routes(V):
    """fp32 routes of the mixer's four GEMMs at the row counts of a round over the queries of k streams"""
    lib = _lib.load()
    out = {}
    for k in range(1, V + 1):
        n = N * k
        M = 8 * n
        out[str(n)] = [lib.pips_gemm_f32_route(*s) for s in ((M, 512, 544, 0), (M, 2048, 512, 1), (M, 512, 2048, 2), (n, 1040, 512, 0))]
    return out


def compare(m, V, T, reps, runs, dev):
    hosts = [frames(0, T, seed=5 + v) for v in range(V)]
    qs = [queries(dev) for _ in range(V)]
    out, rounds = {}, {}
    real = m.stream_round
    for mode in MODES:                                                   # warm-up: weights, workspaces (and the round count)
        count = [0]

        def counted(*a, **kw):
            count[0] += 1
            return real(*a, **kw)

        m.stream_round = counted
        out[mode] = run(mode, m, qs, hosts)
        rounds[mode] = count[0]
    m.stream_round = real
    meds = {mode: [] for mode in MODES}
    for _ in range(runs):
        ts = {mode: [] for mode in MODES}
        for _ in range(reps):
            for mode in MODES:
                ts[mode].append(timed(lambda: run(mode, m, qs, hosts)))
        for mode in MODES:
            meds[mode].append(round(statistics.median(ts[mode]), 4))

    def bits(t):
        return t.view(torch.int32)

    same = all(torch.equal(bits(a), bits(b)) for s, g in zip(out["sequential"], out["multi"]) for a, b in zip(s, g))
    joint_err = max(float((a[0] - b[0]).nan_to_num(0.0).abs().max()) for a, b in zip(out["sequential"], out["multi_joint"]))
    res = {"config": f"360x640 stride 4, T={T}, N={N} per stream over frames 0/33/66/99, {PUSH} frames per stream per push, "
                     f"slots {SLOTS}, library rounds", "V": V, "reps": reps, "runs": runs}
    for mode in MODES:
        res[f"{mode}_s_runs"] = meds[mode]
        res[f"{mode}_s"] = round(statistics.median(meds[mode]), 4)
        res[f"{mode}_rounds"] = rounds[mode]
    res["multi_over_sequential"] = round(res["multi_s"] / res["sequential_s"], 3)
    res["multi_joint_over_sequential"] = round(res["multi_joint_s"] / res["sequential_s"], 3)
    res["multi_bit_equal"] = same
    res["multi_joint_max_dtraj_px"] = joint_err
    res["f32_routes_by_queries"] = routes(V)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = Pips(S=8, stride=STRIDE)
    m.load_state_dict(init_state_dict(0, tamed=True))
    m = m.to(dev).eval()
    for V in a.streams:
        print(json.dumps(compare(m, V, a.T, a.reps, a.runs, dev)), flush=True)


if __name__ == "__main__":
    main()
