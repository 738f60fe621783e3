"""Per-layer durations of the encoder convolutions that igemm_f32_kernel<..., true> or conv_f32_e_kernel runs, out of a
`rocprofv3 --kernel-trace --output-format csv` trace of the plain bench.py command: the launches of those two kernels in order,
folded by their position inside a forward (13 per forward at the headline geometry), mean and spread over the forwards.
usage: python tools/conv_layer_times.py <kernel_trace.csv> [layers per forward = 13]"""
import csv
import statistics
import sys

# the 13 launches of a headline forward (8 frames of 368 x 496) in launch order: name, output pixels per frame, K, N
LAYERS = [("L2 3x3 s2 64->96", 92 * 124, 576, 96), ("L2 1x1 s2 64->96", 92 * 124, 64, 96),
          ("L3 3x3 s2 96->128", 46 * 62, 864, 128), ("L3 3x3 128->128 a", 46 * 62, 1152, 128), ("L3 1x1 s2 96->128", 46 * 62, 96, 128),
          ("L3 3x3 128->128 b", 46 * 62, 1152, 128), ("L3 3x3 128->128 c", 46 * 62, 1152, 128),
          ("L4 3x3 s2 128->128", 23 * 31, 1152, 128), ("L4 3x3 128->128 a", 23 * 31, 1152, 128), ("L4 1x1 s2 128->128", 23 * 31, 128, 128),
          ("L4 3x3 128->128 b", 23 * 31, 1152, 128), ("L4 3x3 128->128 c", 23 * 31, 1152, 128), ("final 1x1 256->128", 46 * 62, 256, 128)]
PEAK_TF, FRAMES = 157.3, 8


def main():
    per = int(sys.argv[2]) if len(sys.argv) > 2 else len(LAYERS)
    rows = []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            n = r["Kernel_Name"]
            if ("igemm_f32_kernel" in n and "true>" in n) or "conv_f32_e_kernel" in n:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n))
    rows.sort()
    assert rows and len(rows) % per == 0, "%d launches are no multiple of %d" % (len(rows), per)
    total = 0.0
    for k in range(per):
        d = [(e - s) / 1e3 for s, e, _ in rows[k::per]][3:]             # the warm-up forwards left out
        name, m, kk, n = LAYERS[k] if per == len(LAYERS) else ("layer %d" % k, 0, 0, 0)
        kern = rows[k][2].replace("void pips::", "").split("(")[0]
        mean = statistics.mean(d)
        total += mean
        tiles = -(-m // 64) * -(-n // 64) * FRAMES
        frac = 2.0 * m * kk * n * FRAMES / (mean * 1e-6) / 1e12 / PEAK_TF if m else 0.0
        print("%-20s M=%5d K=%4d N=%3d  64x64 tiles %4d  %7.2f us (min %7.2f max %7.2f, %d forwards)  %.2f of peak  %s" %
              (name, m, kk, n, tiles, mean, min(d), max(d), len(d), frac, kern))
    print("total %.1f us per forward" % total)


if __name__ == "__main__":
    main()
