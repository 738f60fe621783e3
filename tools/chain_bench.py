"""Chained tracking at the BASELINE configs[4] geometry with both engines of drivers.track_chained.

100 frames of 360x640, stride 4, 256 points (a 16 x 16 grid) at frame 0, 6 iterations, tamed weights and the seeded synthetic
video of tools/stream_bench.py, the video on the device.  ``engine="torch"`` (the hop's bookkeeping as torch ops) and
``engine="native"`` (one pips_chain_hop call per hop) ALTERNATE on one GPU: a warm-up call of each, then --reps timed pairs, a
host clock around each call between two device synchronisations.  Prints one JSON line: per engine the median, the fastest and
the slowest call; the hops (library calls of the native engine = loop turns of either) and the window forwards of one video;
the encoder pass alone; the difference of the medians per hop; and whether both engines returned the same bits at this size."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pips_amd import Pips, drivers  # noqa: E402
from pips_amd.weights import init_state_dict  # noqa: E402
from stream_bench import H, W, STRIDE, N, frames, queries  # noqa: E402

ITERS = 6


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = Pips(S=8, stride=STRIDE)
    m.load_state_dict(init_state_dict(0, tamed=True))
    m = m.to(dev).eval()
    xy0 = queries(dev)[:, :, 1:].contiguous()
    video = frames(0, a.T).to(dev)
    res = {"config": f"{a.T} frames {H}x{W} stride {STRIDE}, N={N} at frame 0, iters {ITERS}, engines alternating", "reps": a.reps}
    outs, hops = {}, {}
    for e in drivers.ENGINES:                                           # warm-up: weights, workspaces; and the hop logs
        outs[e], hops[e] = drivers.track_chained(m, video, xy0, iters=ITERS, return_hops=True, engine=e)
    torch.cuda.synchronize()
    ts = {e: [] for e in drivers.ENGINES}
    for _ in range(a.reps):
        for e in drivers.ENGINES:
            ts[e].append(timed(lambda: drivers.track_chained(m, video, xy0, iters=ITERS, engine=e))[0])
    for e in drivers.ENGINES:
        res[f"{e}_s"] = {"median": round(statistics.median(ts[e]), 4), "min": round(min(ts[e]), 4), "max": round(max(ts[e]), 4)}
    m.encode(video)
    res["encode_s"] = round(statistics.median(timed(lambda: m.encode(video))[0] for _ in range(a.reps)), 4)
    n_hops = max(len(h) for h in hops["torch"])
    res["hops"] = n_hops
    res["window_forwards"] = sum(len(h) for h in hops["torch"])
    res["torch_minus_native_us_per_hop"] = round((res["torch_s"]["median"] - res["native_s"]["median"]) / n_hops * 1e6, 1)
    res["same_hops"] = hops["torch"] == hops["native"]
    res["same_bits"] = bool(torch.equal(outs["torch"].view(torch.int32), outs["native"].view(torch.int32)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
