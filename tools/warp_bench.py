"""pips_frames_warp alone: microseconds per frame for resampling decoder surfaces through a per-frame affine map, HIP events around
``reps`` back-to-back calls after a warm-up of each case; every figure ``repeats`` times in one session, with its median.
  - surfaces: 1080x1920 NV12, P010 and RGBA32, and 2160x3840 NV12, in calls of 8 and 64 frames;
  - maps: a rotation of one degree about the centre with a shift of (3.5, -2.25) px -- every tile's source box is staged in LDS --
    and a 4x zoom-out about the centre (four source pixels a pixel: every tile reads its taps from global memory; most of the
    output is border).  ops.warp_staged is asked which path the tile at (0, 0) takes and the answer is printed;
  - two yardsticks measured in the same run on the same GPU: a stock torch comparator -- the planes to float32, F.affine_grid +
    F.grid_sample (bilinear, align_corners=False) per plane, rounded back into the format -- and the antialiased import of the same
    surfaces to 368x496 float32 (pips_frames_import_ex);
  - the byte time of a case: the bytes of the surfaces read once and written once at the 6.3 TB/s a float4 copy reaches on this
    GPU, beside each figure.
The library calls go straight to the C entry point with buffers allocated once, so a figure is the launch and nothing of the
wrapper.  Every case is first compared with drivers.warp_frames_torch on its first and last frame: a time of wrong bytes is no
time.  Prints a table, the ratio to the torch comparator for every case (the tool fails when the kernel is not faster on one), and
one JSON line.
usage: python tools/warp_bench.py [--reps 100 --repeats 3 --frames 8 64]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F_  # noqa: E402
import _tunelib  # noqa: E402,F401
from pips_amd import _lib, drivers, ops  # noqa: E402

CASES = [("nv12", 1080, 1920), ("p010", 1080, 1920), ("rgba32", 1080, 1920), ("nv12", 2160, 3840)]
MODEL = (368, 496)
HBM_TBS = 6.3


def _time(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _maps(h, w):
    """name -> the forward affine row (six floats, surface pixels) whose inverse the kernel applies"""
    cx, cy = (w - 1) / 2, (h - 1) / 2
    c, s = math.cos(math.radians(1.0)), math.sin(math.radians(1.0))
    return {"rotation 1 deg + shift": [c, -s, cx - c * cx + s * cy + 3.5, s, c, cy - s * cx - c * cy - 2.25],
            "zoom-out 4x": [0.25, 0.0, cx - 0.25 * cx, 0.0, 0.25, cy - 0.25 * cy]}


def _surfaces(fmt, F, h, w, g, dev):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "rgba32":
        return [torch.randint(0, 256, (F, h, w, 4), generator=g, dtype=torch.uint8).to(dev)]
    shapes = [(F, h, w), (F, ch, cw, 2)]
    if fmt == "nv12":
        return [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in shapes]
    words = [torch.randint(0, 1024, s, generator=g) << 6 for s in shapes]
    return [(v - ((v & 0x8000) << 1)).to(torch.int16).to(dev) for v in words]                       # (the bits of the uint16 words)


def _bytes(planes):
    return sum(p[0].numel() * p.element_size() for p in planes)


def _library(lib, fmt, planes, out, coef, stream):
    F, h, w = planes[0].shape[:3]
    args = ops.draw_surfaces(planes, fmt) + ops.draw_surfaces(out, fmt)
    head = (ops.DRAW_FORMATS_EX[fmt], 1, 0, 0, 0, F, h, w)

    def call():
        rc = lib.pips_frames_warp(*head, *args, C.c_void_p(coef.data_ptr()), stream)
        assert rc == 0, lib.pips_last_error()
    return call


def _theta(coef, h, w):
    """the kernel's integer rows as F.affine_grid's normalised matrices (align_corners=False)"""
    m = coef.to(torch.float64).cpu()
    a, b, c, d, e, f = m[:, 0] / 2 ** 24, m[:, 1] / 2 ** 24, m[:, 2] / 2 ** 16, m[:, 3] / 2 ** 24, m[:, 4] / 2 ** 24, m[:, 5] / 2 ** 16
    rows = [torch.stack([a, b * h / w, (a * (w - 1) + b * (h - 1) + 2 * c + 1) / w - 1], dim=1),
            torch.stack([d * w / h, e, (d * (w - 1) + e * (h - 1) + 2 * f + 1) / h - 1], dim=1)]
    return torch.stack(rows, dim=1).to(torch.float32)


def _torch_warp(fmt, planes, theta):
    """the stock comparator: float planes, affine_grid + grid_sample per plane, back to the format"""
    def sample(x):                                                          # (F,C,rows,cols) float32
        grid = F_.affine_grid(theta, list(x.shape), align_corners=False)
        return F_.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    if fmt == "rgba32":
        rgb = sample(planes[0][..., :3].permute(0, 3, 1, 2).float())
        out = torch.empty_like(planes[0])
        out[..., :3] = (rgb + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
        out[..., 3] = 255
        return [out]
    if fmt == "nv12":
        y = sample(planes[0].unsqueeze(1).float())
        uv = sample(planes[1].permute(0, 3, 1, 2).float())
        return [(y[:, 0] + 0.5).clamp(0, 255).to(torch.uint8), (uv + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()]
    val = lambda p: ((p.to(torch.int32) & 0xFFFF) >> 6).float()
    def word(v):                                                            # the bits of the uint16 words
        v = (v + 0.5).clamp(0, 1023).to(torch.int32) << 6
        return (v - ((v & 0x8000) << 1)).to(torch.int16)
    y = sample(val(planes[0]).unsqueeze(1))
    uv = sample(val(planes[1]).permute(0, 3, 1, 2))
    return [word(y[:, 0]), word(uv).permute(0, 2, 3, 1).contiguous()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, notes, ratios = {}, [], {}
    for fmt, h, w in CASES:
        for F in a.frames:
            g = torch.Generator().manual_seed(h + F)
            planes = _surfaces(fmt, F, h, w, g, dev)
            out = [torch.empty_like(p) for p in planes]
            nbytes = 2 * _bytes(planes)
            byte_us = nbytes / (HBM_TBS * 1e12) * 1e6
            reps = max(a.reps * 8 // F // (4 if h > 1080 else 1), 5)
            tag = f"{h}p {fmt} F{F}"
            for name, fwd in _maps(h, w).items():
                coef = drivers.warp_coefficients(torch.tensor([fwd] * F, dtype=torch.float64), (h, w)).to(dev)
                staged = ops.warp_staged(coef[0].tolist(), fmt)
                call = _library(lib, fmt, planes, out, coef, stream)
                call()
                torch.cuda.synchronize()
                for f in (0, F - 1):                                        # a time of wrong bytes is no time
                    want = drivers.warp_frames_torch([p[f:f + 1] for p in planes], fmt, coef[f:f + 1])
                    want = [want] if torch.is_tensor(want) else want
                    assert all(torch.equal(o[f:f + 1], x) for o, x in zip(out, want)), (tag, name, f)
                theta = _theta(coef, h, w).to(dev)
                key = f"{tag}, {name} ({'staged' if staged else 'direct'})"
                for _ in range(a.repeats):
                    rows.setdefault(f"{key}: pips_frames_warp, us/frame", []).append(_time(call, reps) / F)
                    rows.setdefault(f"{key}: torch grid_sample, us/frame", []).append(
                        _time(lambda: _torch_warp(fmt, planes, theta), max(reps // 10, 2), warm=1) / F)
                ratios[key] = statistics.median(rows[f"{key}: torch grid_sample, us/frame"]) / \
                    statistics.median(rows[f"{key}: pips_frames_warp, us/frame"])
                del theta
            notes.append(f"{tag}: {nbytes / 1e6:.2f} MB in + out a frame, byte time {byte_us:.2f} us at {HBM_TBS} TB/s")
            for _ in range(a.repeats):
                rows.setdefault(f"{tag}: antialiased import to {MODEL[0]}x{MODEL[1]} float32, us/frame", []).append(
                    _time(lambda: ops.import_frames(planes, fmt, size=MODEL, dtype=torch.float32, antialias=True), max(reps // 2, 3)) / F)
            del planes, out
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(dev), "config": f"{a.reps} calls per figure at 8 frames of 1080p (fewer for larger calls), {a.repeats} repeats"}
    print(f"device: {res['device']}")
    print(f"{'run':92s} {'(repeats)':>36s} {'median':>10s}")
    for name, us in rows.items():
        med = statistics.median(us)
        print(f"{name:92s} {' '.join(f'{u:11.2f}' for u in us):>36s} {med:10.2f}")
        res[name] = {"repeats": [round(u, 3) for u in us], "median": round(med, 3)}
    for n in notes:
        print(n)
    print("torch grid_sample / pips_frames_warp, by case:")
    for key, r in ratios.items():
        print(f"  {key:70s} {r:8.1f}x")
    res["ratio_torch_over_kernel"] = {k: round(v, 2) for k, v in ratios.items()}
    print(json.dumps(res), flush=True)
    slow = [k for k, r in ratios.items() if r <= 1.0]
    assert not slow, f"the kernel is not faster than the torch comparator on {slow}"


if __name__ == "__main__":
    main()
