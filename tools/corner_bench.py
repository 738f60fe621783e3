"""pips_corner_table alone: microseconds per call and per frame for chunks of F frames of HxW with cells of ``cell`` px, uint8 and
float32 frames, HIP events around ``reps`` back-to-back calls after a warm-up of each shape.  Prints one JSON line.
usage: python tools/corner_bench.py [--H 360 --W 640 --cell 32 --chunks 8 24 --reps 2000]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import drivers, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=360)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--chunks", type=int, nargs="+", default=[8, 24])
    ap.add_argument("--reps", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    res = {"config": f"{a.H}x{a.W}, cell {a.cell}, {a.reps} calls per figure", "bytes_in_per_frame_u8": 3 * a.H * a.W,
           "bytes_out_per_frame": 12 * ((a.H - 1) // a.cell + 1) * ((a.W - 1) // a.cell + 1)}
    for F in a.chunks:
        host = torch.randint(0, 256, (F, 3, a.H, a.W), generator=g, dtype=torch.uint8)
        for name, frames in (("u8", host.to(dev)), ("f32", host.float().to(dev))):
            table = ops.corner_table(frames, a.cell)
            if name == "u8" and F == a.chunks[0]:                     # the bits first: a time of a wrong table is no time
                assert torch.equal(table.cpu().view(torch.int32), drivers.corner_table_torch(host, a.cell).view(torch.int32))
            for _ in range(20):
                ops.corner_table(frames, a.cell)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                ops.corner_table(frames, a.cell)
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.reps
            res[f"F{F}_{name}_us_per_call"] = round(us, 2)
            res[f"F{F}_{name}_us_per_frame"] = round(us / F, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
