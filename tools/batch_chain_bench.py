"""V sequential drivers.track_chained calls against ONE drivers.track_chained_batch call over the same V videos.

Per video: 100 frames of 360x640, stride 4, 20 points at frame 0 (a 4 x 5 grid), 6 iterations, tamed weights, the seeded
synthetic video of tools/stream_bench.py with a seed per video, videos on the device.  For V = 1, 4, 16 and both engines the
sequential loop and the batch call ALTERNATE on one GPU: a warm-up of each, then --reps timed pairs, a host clock around each
between two device synchronisations.  Prints one JSON line per (V, engine): the medians, their ratio, and whether the batch
returned the bits and the hops of the loop -- promised only while no mixer GEMM of the batched row count takes the fp32
route 2 (pips_gemm_f32_route), whose partial sums are added in another order."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pips_amd import Pips, _lib, drivers  # noqa: E402
from pips_amd.weights import init_state_dict  # noqa: E402
from stream_bench import H, W, STRIDE, frames  # noqa: E402

ITERS, POINTS = 6, 20


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def points(dev):
    gy, gx = torch.meshgrid(torch.linspace(40, H - 41, 4), torch.linspace(40, W - 41, 5), indexing="ij")
    return torch.stack([gx.reshape(-1), gy.reshape(-1)], -1).unsqueeze(0).to(dev)


def routes(n):
    """the fp32 routes of the mixer's four GEMM shapes at n particles"""
    lib = _lib.load()
    M = 8 * n
    return [lib.pips_gemm_f32_route(*s) for s in ((M, 512, 544, 0), (M, 2048, 512, 1), (M, 512, 2048, 2), (n, 1040, 512, 0))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--videos", type=int, nargs="+", default=[1, 4, 16])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = Pips(S=8, stride=STRIDE)
    m.load_state_dict(init_state_dict(0, tamed=True))
    m = m.to(dev).eval()
    xy0 = points(dev)
    videos = [frames(0, a.T, seed=5 + v).to(dev) for v in range(max(a.videos))]
    for V in a.videos:
        vs, xs = videos[:V], [xy0] * V

        def loop(e, hops=False):
            return [drivers.track_chained(m, v, x, iters=ITERS, return_hops=hops, engine=e) for v, x in zip(vs, xs)]

        def batch(e, hops=False):
            return drivers.track_chained_batch(m, vs, xs, iters=ITERS, return_hops=hops, engine=e)

        for e in drivers.ENGINES:
            ref, got = loop(e, True), batch(e, True)                      # warm-up, and the outputs to compare
            ts = {"loop": [], "batch": []}
            for _ in range(a.reps):
                ts["loop"].append(timed(lambda: loop(e))[0])
                ts["batch"].append(timed(lambda: batch(e))[0])
            med = {k: statistics.median(v) for k, v in ts.items()}
            r = routes(V * POINTS)
            print(json.dumps({
                "config": f"{V} videos x {a.T} frames {H}x{W} stride {STRIDE}, {POINTS} points each at frame 0, iters {ITERS}",
                "engine": e, "reps": a.reps, "loop_s": round(med["loop"], 4), "batch_s": round(med["batch"], 4),
                "loop_over_batch": round(med["loop"] / med["batch"], 3), "hops_longest_chain": max(len(h) for _, hs in ref for h in hs),
                "f32_routes_at_first_hop": r, "bits_promised": 2 not in r,
                "same_hops": all(g[1] == q[1] for g, q in zip(got, ref)),
                "same_bits": all(torch.equal(g[0].view(torch.int32), q[0].view(torch.int32)) for g, q in zip(got, ref))}), flush=True)


if __name__ == "__main__":
    main()
