"""pips_object_masks_guided alone: microseconds per frame, by tools/masks_bench.py's method -- HIP events around ``reps``
back-to-back calls after a warm-up of each shape, every figure ``repeats`` times in one session, with its median; the library
calls go straight to the C entry points with buffers allocated once.
  - masks of one frame at 368 x 496 from tracks of the same size and at 1080 x 1920 from 368 x 496 tracks (masks_bench's tracks: n =
    256 and 2048 spread evenly, a rectangle of them labelled 1, the others 0, one in twenty 255); the radius 1.5 x the mean track
    spacing sqrt(h w / n) of the shape, reach = floor(5 radius + 0.5), edge = 4; the guide a blocky luma -- 60, 110 or 160 on cells
    of 97 x 83 pixels -- with noise of +-2;
  - beside each, in the same session: (a) pips_object_masks at vote 1 on the same tracks and radius -- the price of the edge term
    is the ratio to it -- and (b) drivers.object_masks_guided_torch on the same GPU, the route open to a user without the kernel
    (HIP events around ``slow_reps`` runs);
  - the launches of a guided call -- the prepare launch and ceil(floor(reach / 5) / GUIDED_HALO) relaxation launches -- are printed
    with each shape.
Every shape is compared with the torch twin first (on the device): a time of wrong masks is no time.  Prints a table and one JSON
line; nothing is asserted about the ratios.
usage: python tools/masks_guided_bench.py [--reps 100 --repeats 3 --slow-reps 3]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from masks_bench import SRC, _event_time, _masks, _tracks  # noqa: E402
from motion_bench import _time  # noqa: E402
from pips_amd import _lib, drivers, ops  # noqa: E402

SHAPES = [(size, n) for size in ((368, 496), (1080, 1920)) for n in (256, 2048)]
EDGE = 4


def _radius(size, n):
    return 1.5 * math.sqrt(size[0] * size[1] / n)


def _guide(size, g, dev):
    h, w = size
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return ((60 + ((xx // 97 + yy // 83) % 3) * 50) + torch.randint(-2, 3, (h, w), generator=g)).to(torch.uint8)[None].to(dev)


def _guided(lib, rows, lab, guide, size, reach, stream):
    """one pips_object_masks_guided call on device rows, buffers allocated once -> (call, mask, workspace)"""
    n, (h, w) = rows.shape[1], size
    out = torch.empty(1, h, w, dtype=torch.uint8, device=rows.device)
    nbytes = ops.object_masks_guided_workspace_bytes(1, n, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rows.device)
    p = [C.c_void_p(t.data_ptr()) for t in (rows, lab, guide, out, ws)]

    def call():
        rc = lib.pips_object_masks_guided(p[0], p[1], 1, n, 0, 1, SRC[0], SRC[1], h, w, EDGE, reach, p[2], w, h * w, p[3], w, h * w, p[4],
                                          nbytes, stream)
        assert rc == 0, lib.pips_last_error()
    return call, out, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(5)
    tracks = {n: tuple(t.to(dev) for t in _tracks(n, g)) for n in (256, 2048)}
    guides = {size: _guide(size, g, dev) for size in ((368, 496), (1080, 1920))}
    rows, launches = {}, {}
    for rep in range(a.repeats):
        for size, n in SHAPES:
            t, lab = tracks[n]
            radius = _radius(size, n)
            reach = int(math.floor(5 * radius + 0.5))
            name = f"{size[0]}x{size[1]} n{n} radius {radius:.1f} px reach {reach}"
            launches[name] = 1 + ops.guided_launches(reach)
            call, out, keep = _guided(lib, t, lab, guides[size], size, reach, stream)
            twin = lambda: drivers.object_masks_guided_torch(t[None], lab, guides[size], SRC, out_size=size, radius=radius, edge=EDGE)
            if rep == 0:
                call()
                torch.cuda.synchronize()
                ref = twin()
                assert torch.equal(out, ref), f"{name}: {int((out != ref).sum())} bytes differ from the twin"
                assert len(set(out.unique().tolist())) >= 3
            rows.setdefault(f"{name}: pips_object_masks_guided, us/frame", []).append(_time(call, a.reps))
            plain, _, keep2 = _masks(lib, t, lab, size, 1, stream)
            rows.setdefault(f"{name}: (a) pips_object_masks vote 1, us/frame", []).append(_time(plain, a.reps))
            rows.setdefault(f"{name}: (b) object_masks_guided_torch on the GPU, us/frame", []).append(_event_time(twin, a.slow_reps))
    out = {"device": torch.cuda.get_device_name(dev),
           "config": f"{a.reps} calls per figure ({a.slow_reps} for the torch twin), {a.repeats} repeats, one frame a call, edge {EDGE}, "
                     f"tile {ops.GUIDED_TILE}, halo {ops.GUIDED_HALO}"}
    print(f"device: {out['device']}; {out['config']}")
    print(f"{'run':100s} {'(repeats)':>40s} {'median':>11s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:100s} {' '.join(f'{u:12.2f}' for u in us):>40s} {med:11.2f}")
        out[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    print(f"{'shape':60s} {'launches':>9s} {'guided / (a)':>13s} {'(b) / guided':>13s}")
    for name, k in launches.items():
        med = {key.split(": ")[1][:3]: statistics.median(v) for key, v in rows.items() if key.startswith(name + ":")}
        ratio_a, ratio_b = med["pip"] / med["(a)"], med["(b)"] / med["pip"]
        print(f"{name:60s} {k:9d} {ratio_a:13.2f} {ratio_b:13.1f}")
        out[name] = {"launches": k, "guided over (a)": round(ratio_a, 2), "(b) over guided": round(ratio_b, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
