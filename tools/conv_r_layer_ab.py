"""Per-layer A/B of the fp32 encoder's layer-1 convolutions: the staged pair  inorm_apply mode 0 + the convolution the shape selects
(conv3x3_f32_t4_kernel<0> on large maps)  against  conv3x3_c64_f32_r_kernel normalising while it stages (pips_conv_nhwc_f32_r),
on the same raw map.  Device-event times over `reps` calls, `runs` runs per side, alternating; one line per geometry with the
tiles per compute unit that PIPS_CONV_F32_R_MINPCT (conv_f32_r.hip) is read against.
usage: python tools/conv_r_layer_ab.py [out.txt] [reps=20] [runs=3]"""
import ctypes as C
import sys

import _tunelib  # noqa: F401  (first: binds pips_amd to PIPS_LIB_PATH if set)
import torch

from pips_amd import _lib, ops

DEV = "cuda:0"
#        name                         F   H    W
GEOMS = [("8 x 128x160 input",        8,  64,  80),
         ("8 x 192x256 input",        8,  96, 128),
         ("8 x 256x320 input",        8, 128, 160),
         ("8 x 256x512 input",        8, 128, 256),
         ("headline 8 x 368x496",     8, 184, 248),
         ("config 4: 32 x 360x640",  32, 180, 320)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    lib = _lib.load()
    cus = lib.pips_device_cus()
    lines = ["# us per layer, %d runs of %d calls each, alternating; %d compute units" % (runs, reps, cus),
             "# geometry                  tiles/CU | apply<0>            | shape-selected conv  | LDS-resident conv + in_norm | pair - new"]
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(DEV)
    b = torch.randn(64, generator=g).to(DEV)
    for name, F, H, W in GEOMS:
        x = torch.randn(F, H, W, 64, generator=g).to(DEV)
        nrm = torch.stack([torch.randn(F, 64, generator=g) * 0.1, 0.5 + torch.rand(F, 64, generator=g)], -1).to(DEV)
        xa, o1, o2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        parts_r = 4 * ((H + 3) // 4) * ((W + 31) // 32)
        cap = max(2 * ((H * W + 63) // 64) + 4, parts_r)
        stats = torch.zeros(F, cap, 64, 4, device=DEV)
        tiles = C.c_int(0)
        st = ops._stream()
        p = _lib.ptr

        def apply0():
            _lib.check(lib.pips_inorm_apply(p(x), p(nrm), None, None, 0, p(xa), F, H * W, 64, 0, st), "apply")

        def conv_old():
            _lib.check(lib.pips_conv_nhwc_f32(p(xa), F, H, W, 64, p(w), p(b), 64, 3, 1, 1, p(o1), p(stats), C.byref(tiles), st), "conv")

        def conv_new():
            _lib.check(lib.pips_conv_nhwc_f32_r(p(x), p(nrm), F, H, W, 64, p(w), p(b), 64, 3, 1, 1, p(o2), p(stats), cap,
                                                C.byref(tiles), st), "conv_r")
        for fn in (apply0, conv_old, conv_new):
            fn()
        torch.cuda.synchronize()
        assert torch.equal(o1, o2), name
        ta, to, tn = [], [], []
        for _ in range(runs):
            ta.append(timed(apply0, reps)); to.append(timed(conv_old, reps)); tn.append(timed(conv_new, reps))

        def f3(v):
            return " ".join("%6.1f" % t for t in v)
        gain = [a + o - n for a, o, n in zip(ta, to, tn)]
        lines.append("%-28s %7.2f | %s | %s | %s        | %s" % (name, 2.0 * parts_r / 4 * F / cus, f3(ta), f3(to), f3(tn), f3(gain)))
        print(lines[-1], flush=True)
    txt = "\n".join(lines) + "\n"
    if out_path:
        open(out_path, "w").write(txt)


if __name__ == "__main__":
    main()
