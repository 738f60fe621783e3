"""pips_cut_table alone, and pips_corner_table on the same frames as the yardstick: microseconds per call and per frame for chunks
of F frames of HxW, uint8 and float32 frames, HIP events around ``reps`` back-to-back calls after a warm-up of each shape.  Prints
one JSON line.  (The encoder at the same sizes: tools/encode_bench.py in the same session.)
usage: python tools/cut_bench.py [--H 360 --W 640 --cell 32 --chunks 8 24 --reps 2000]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import drivers, ops  # noqa: E402


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
    res = {"config": f"{a.H}x{a.W}, {a.reps} calls per figure, corner table with cell {a.cell}", "bytes_in_per_frame_u8": 3 * a.H * a.W,
           "bytes_out_per_frame": 4 * (512 + 1)}
    for F in a.chunks:
        host = torch.randint(0, 256, (F, 3, a.H, a.W), generator=g, dtype=torch.uint8)
        host[F - 1] = 200                                                # a flat frame: every pixel of a region in one bin
        for name, frames in (("u8", host.to(dev)), ("f32", host.float().to(dev))):
            hist, dist = ops.cut_table(frames)
            if F == a.chunks[0]:                                         # the integers first: a time of a wrong table is no time
                ref_h, ref_d = drivers.cut_table_torch(host)
                assert torch.equal(hist.cpu().long(), ref_h) and torch.equal(dist.cpu().long(), ref_d)
            prev = hist[-1].clone()
            for what, fn in (("cut", lambda: ops.cut_table(frames, prev)), ("corner", lambda: ops.corner_table(frames, a.cell))):
                us = _time(fn, a.reps)
                res[f"F{F}_{name}_{what}_us_per_call"] = round(us, 2)
                res[f"F{F}_{name}_{what}_us_per_frame"] = round(us / F, 3)
        flat = host[F - 1:].expand(F, 3, a.H, a.W).contiguous().to(dev)  # every frame flat: the case that would serialise
        res[f"F{F}_u8_cut_flat_us_per_call"] = round(_time(lambda: ops.cut_table(flat, prev), a.reps), 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
