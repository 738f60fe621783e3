"""References and bounds of the encoder's stage kernels (tests/test_encoder_stages.py on the CPU, tests/test_encoder_stages_gpu.py
on the GPU): pure torch, importable without a device, nothing here calls the library.  Every reference is the operation in fp64;
every bound is per element and derived from the arithmetic of a correct fp32 (or fp32-then-bf16) implementation, so an excess
is a finding and not noise.  u = 2^-24 is the unit roundoff of fp32.

stem        conv2d (7x7, stride 2, pad 3) of 2 (x / 255) - 1, the scaling formed in fp32 as the kernel forms it and then
            widened.  K = 147 products and the bias summed in any order: |err| <= 160 u (conv(|x|, |w|) + |b|).  bf16 mode: x and
            w rounded to bf16 (RNE) ahead of the fp64 sum; the store adds half a bf16 ulp of the result.
apply       t1 = (x - m) r, t2 = the shortcut term of the mode, y = relu(t2 + relu(t1)) from the same fp32 {mean, rstd}: three
            roundings per term, |err| <= 4 u (|t1| + |t2|) (+ half a bf16 ulp of y on bf16 maps).
resize      bilinear, align_corners=True.  The source coordinate scale * y carries at most three fp32 roundings of relative size
            u on a value <= size - 1, a coordinate error moves the result by at most the neighbour difference <= 2 max|src|,
            on two axes: |err| <= 2^-22 (Hs + Ws) max|src| (+ half a bf16 ulp).
avgpool     ((a + b) + c + d) / 4: three roundings, |err| <= 3 u (|a| + |b| + |c| + |d|) / 4.
finalize    fp64 inside: only the rounding of the two results shows.  mean within 2^-23 |mean|, rstd within 2^-22 relative.
mirror      bit equality with round-to-nearest-even.
"""
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
EPS = 1e-5                   # nn.InstanceNorm2d(eps=1e-5)


def bf16_half_ulp(ref):
    """half a bf16 ulp (8 significant bits) at |ref|: 2^(floor(log2 |ref|) - 8); 0 at 0"""
    a = ref.abs().double()
    h = torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -126))) - 8)
    return torch.where(a > 0, h, torch.zeros_like(h))


def worst(err, bound):
    """max err / bound; an error where the bound is zero counts as infinite"""
    err, bound = err.double(), bound.double()
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    return float(r.max())


def bf16_rne_bits(x):
    """fp32 tensor (no NaN) -> int32 tensor of the 16 bf16 bits of its round-to-nearest-even, by integer arithmetic"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def bf16_bits(t):
    """the bits of a bfloat16 tensor as int32 in 0..65535"""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bf16_truncate(x):
    """wrong implementation: the bf16 store that drops the low 16 bits instead of rounding"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


# ----------------------------------------------------------------------------------------------- stem
def stem_out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_parts(H, W):
    """partials per frame: one per wave of the 4-row x 64-column tiles (encoder.hip: stem_tiles_m)"""
    Ho, Wo = stem_out_hw(H, W)
    return ((Ho + 3) // 4) * ((Wo + 63) // 64) * 4


def stem_frames(Fr, H, W, seed=7):
    """(Fr, 3, H, W) integer frames 0..255 as float"""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    return torch.randint(0, 256, (Fr, 3, H, W), generator=g).float()


def stem_scale(rgbs):
    """2 (x / 255) - 1 in fp32, nets/pips.py:436"""
    return 2.0 * (rgbs.float() / 255.0) - 1.0


def conv7s2_nhwc64(x, w, b):
    """conv2d(x (F,3,H,W), w (64,3,7,7), b, stride 2, padding 3) in fp64 as 49 matrix products -> NHWC (F,Ho,Wo,64): the form
    that runs where the operands are (F.conv2d has no fp64 kernel on every device); test_encoder_stages.py pins it to F.conv2d"""
    x, w = x.double(), w.double()
    Fr, Ci, H, W = x.shape
    Ho, Wo = stem_out_hw(H, W)
    xp = torch.zeros(Fr, Ci, H + 6, W + 6, dtype=torch.float64, device=x.device)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    xp = xp.permute(0, 2, 3, 1)
    out = torch.zeros(Fr, Ho, Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for i in range(7):
        for j in range(7):
            out += xp[:, i:i + 2 * (Ho - 1) + 1:2, j:j + 2 * (Wo - 1) + 1:2] @ w[:, :, i, j].t()
    return out + b.double()


def stem_ref(rgbs, w, b, bf16=False):
    """-> (ref, mag), fp64 NHWC (F,Ho,Wo,64): the reference map and the magnitude sum conv(|x|, |w|) + |b| of its bound.
    bf16: x and w rounded to bf16 (RNE) first, as autocast's cast of the convolution's operands does."""
    x, w = stem_scale(rgbs), w.float()
    if bf16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    return conv7s2_nhwc64(x, w, b), conv7s2_nhwc64(x.abs(), w.abs(), b.abs())


def stem_bound(ref, mag, bf16=False):
    b = 160 * U24 * mag
    return b + bf16_half_ulp(ref) if bf16 else b


def drop_stem_tap(w, co=5, ci=1, kh=6, kw=0):
    """wrong implementation: one filter tap of one output channel never multiplied"""
    w = w.clone()
    w[co, ci, kh, kw] = 0
    return w


def map_stats64(m):
    """fp64 NHWC map (F,H,W,C) -> (F,C,2) fp64 {mean, 1 / sqrt(biased variance + eps)}"""
    var, mean = torch.var_mean(m.double(), dim=(1, 2), unbiased=False)
    return torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], dim=-1)


def map_stats32(m):
    """the yardstick: torch's own fp32 var_mean of an fp32 map"""
    var, mean = torch.var_mean(m.float(), dim=(1, 2), unbiased=False)
    return torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], dim=-1)


def stats_gate(got, ref64, yard32):
    """{mean, rstd} (F,C,2) against the fp64 values, judged by the error of the yardstick on the same values: per quantity
    |got - ref| <= 4 max|yard - ref| + 2^-22 |ref|.  Returns (ratio of the worst error to max|yard - ref|, ok) per quantity."""
    out = []
    for q in range(2):
        g, r, y = got[..., q].double(), ref64[..., q].double(), yard32[..., q].double()
        yard = float((y - r).abs().max())
        err = (g - r).abs()
        ok = bool((err <= 4 * yard + 2.0 ** -22 * r.abs()).all())
        out.append((float(err.max()) / max(yard, 1e-300), ok))
    return out


# ----------------------------------------------------------------------------------------------- instance-norm apply
APPLY_MODES = {"f32": (0, 1, 2), "bf16": (0, 1, 2, 3)}


def apply_case(Fr, HW, C, bf16, seed=11, device="cpu"):
    """x, res (Fr, HW, C) and st, rst (Fr, C, 2): statistics distinct per (frame, channel), mean ~ N(0, 1) and rstd
    log-uniform in [0.5, 20], so that a frame or channel mix-up is an O(1) error; x spread about its mean by a few 1 / rstd.
    bf16: the maps are bfloat16 tensors."""
    g = torch.Generator().manual_seed(seed + 7 * HW + C + 1000 * Fr)

    def stats():
        mean = torch.randn(Fr, C, generator=g)
        rstd = 0.5 * torch.exp(torch.rand(Fr, C, generator=g) * math.log(40.0))
        return torch.stack([mean, rstd], dim=-1)

    st, rst = stats(), stats()
    x = st[:, None, :, 0] + 1.5 * torch.randn(Fr, HW, C, generator=g) / st[:, None, :, 1]
    res = rst[:, None, :, 0] + 1.5 * torch.randn(Fr, HW, C, generator=g) / rst[:, None, :, 1]
    if bf16:
        x, res = x.bfloat16(), res.bfloat16()
    return x.to(device), st.to(device), res.to(device), rst.to(device)


def apply_ref(x, st, res, rst, mode, bf16=False):
    """-> (ref, bound), fp64 (F, HW, C), from the fp32 {mean, rstd} and the maps as given"""
    x, st = x.double(), st.double()
    t1 = (x - st[:, None, :, 0]) * st[:, None, :, 1]
    if mode == 0:
        t2 = torch.zeros_like(t1)
    elif mode == 1:
        t2 = res.double()
    else:
        rst = rst.double()
        t2 = (res.double() - rst[:, None, :, 0]) * rst[:, None, :, 1]
        if mode == 3:
            t2 = torch.relu(t2)
    ref = torch.relu(t2 + torch.relu(t1))
    bound = 4 * U24 * (t1.abs() + t2.abs())
    return ref, bound + bf16_half_ulp(ref) if bf16 else bound


def apply_f32(x, st, res, rst, mode):
    """the operation in plain fp32 torch arithmetic (the CPU proof that the bound passes a correct stage)"""
    x, st = x.float(), st.float()
    o = torch.relu((x - st[:, None, :, 0]) * st[:, None, :, 1])
    if mode == 0:
        return o
    r = res.float()
    if mode >= 2:
        r = (r - rst[:, None, :, 0].float()) * rst[:, None, :, 1].float()
        if mode == 3:
            r = torch.relu(r)
    return torch.relu(r + o)


# ----------------------------------------------------------------------------------------------- resize
RESIZE_SHAPES = (((53, 75), (13, 18)), ((14, 19), (13, 18)), ((7, 10), (13, 18)), ((13, 18), (13, 18)), ((13, 10), (13, 18)),
                 ((2, 3), (16, 17)), ((5, 7), (1, 1)))
RESIZE_CHANNELS = ((64, 0), (96, 64), (128, 160), (128, 288))       # (C, coff) of the four layers in the 416-channel map
RESIZE_CDST = 416


def resize_ref(src, size, align_corners=True):
    """src NHWC (F,Hs,Ws,C) -> fp64 NHWC (F,Hd,Wd,C)"""
    out = F.interpolate(src.double().permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=align_corners)
    return out.permute(0, 2, 3, 1)


def resize_bound(src, ref, bf16=False):
    Hs, Ws = src.shape[1:3]
    b = torch.full_like(ref, 2.0 ** -22 * (Hs + Ws) * float(src.double().abs().max()))
    return b + bf16_half_ulp(ref) if bf16 else b


# ----------------------------------------------------------------------------------------------- avg pool
def avgpool_ref(src):
    """src NHWC fp32 -> (ref, bound) fp64 NHWC (F,H//2,W//2,C)"""
    s = src.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(s, 2, stride=2).permute(0, 2, 3, 1)
    mag = F.avg_pool2d(s.abs(), 2, stride=2).permute(0, 2, 3, 1)           # 0.25 (|a| + |b| + |c| + |d|)
    return ref, 3 * U24 * mag


def avgpool_last_odd_row(src):
    """wrong implementation: on an odd height the windows start at row 1, so the last row is pooled and the first is not"""
    H = src.shape[1]
    return F.avg_pool2d(src[:, H % 2:].permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------------------------- finalize
PART_MAX = 64


def finalize_partials(Fr, parts, C, kind, device="cpu", seed=3):
    """Pivoted partials (Fr, parts, C, 4) fp32 {sum(x - p), sum((x - p)^2), p, n} formed in fp64 from real per-part data and
    rounded: n random in 1..64 pixels per part, about a quarter of the parts empty (n = 0; what an empty part holds besides
    is noise: 1e30 in all three), the first part of a channel never empty (the finalize takes its pivot as the reference,
    as it may in the encoder), p = the part's first pixel as fp32.
    kind "wide": per channel mean ~ 3 N(0, 1), std log-uniform in [1e-2, 10]; "flat": mean 200, std 1e-3."""
    g = torch.Generator(device=device).manual_seed(seed + parts * 131 + Fr * 17 + C)
    rows = []
    for _ in range(Fr):                                                       # frame by frame: (parts, C, 64) fp64 at a time
        if kind == "wide":
            mu = 3 * torch.randn(C, generator=g, device=device, dtype=torch.float64)
            sd = torch.exp(torch.rand(C, generator=g, device=device, dtype=torch.float64) * math.log(1e3)) * 1e-2
        else:
            mu = torch.full((C,), 200.0, device=device, dtype=torch.float64)
            sd = torch.full((C,), 1e-3, device=device, dtype=torch.float64)
        x = mu[None, :, None] + sd[None, :, None] * torch.randn(parts, C, PART_MAX, generator=g, device=device, dtype=torch.float64)
        n = torch.randint(1, PART_MAX + 1, (parts, C), generator=g, device=device)
        empty = torch.rand(parts, C, generator=g, device=device) < 0.25
        empty[0] = False
        n = torch.where(empty, torch.zeros_like(n), n)
        live = torch.arange(PART_MAX, device=device)[None, None, :] < n[:, :, None]
        p = x[:, :, 0].float()
        d = torch.where(live, x - p.double()[:, :, None], torch.zeros_like(x))
        row = torch.stack([d.sum(-1).float(), (d * d).sum(-1).float(), p, n.float()], dim=-1)
        rows.append(torch.where(empty[:, :, None].expand_as(row) & (torch.arange(4, device=device) < 3), torch.full_like(row, 1e30), row))
    return torch.stack(rows)


def finalize_ref(partials):
    """(F, parts, C, 4) fp32 -> (F, C, 2) fp64 {mean, rstd}: the fp64 evaluation of those partials.  The mean first (sums of
    n p + s), then the sum of squares about THAT mean, sum[q + 2 (p - mean) s + n (p - mean)^2]: no cancellation beyond the
    data's own spread, and no choice of reference pivot shared with the kernel."""
    st = partials.double()
    s, q, p, n = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
    live = n > 0
    z = torch.zeros_like(s)
    s, q, p = torch.where(live, s, z), torch.where(live, q, z), torch.where(live, p, z)
    N = n.sum(dim=1)
    mean = (n * p + s).sum(dim=1) / N
    d = torch.where(live, p - mean[:, None, :], z)
    s1 = (s + n * d).sum(dim=1) / N                                           # ~ 0: the residual of the mean
    var = (q + 2 * d * s + n * d * d).sum(dim=1) / N - s1 * s1
    return torch.stack([mean + s1, 1.0 / torch.sqrt(var.clamp_min(0) + EPS)], dim=-1)


def finalize_bounds(ref):
    """(F, C, 2): 2^-23 |mean| and 2^-22 rstd"""
    return torch.stack([2.0 ** -23 * ref[..., 0].abs(), 2.0 ** -22 * ref[..., 1].abs()], dim=-1)


def finalize_like_kernel(partials):
    """a correct finalize in the kernel's own form (everything re-based on the first part's pivot, fp64, rounded to fp32)"""
    st = partials.double()
    s, q, p, n = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
    live = n > 0
    z = torch.zeros_like(s)
    r = p[:, :1]
    d = torch.where(live, p - r, z)
    s, q = torch.where(live, s, z), torch.where(live, q, z)
    N = n.sum(dim=1)
    m1 = (s + n * d).sum(dim=1) / N
    var = ((q + d * (2 * s + n * d)).sum(dim=1) / N - m1 * m1).clamp_min(0)
    return torch.stack([(r[:, 0] + m1).float(), (1.0 / torch.sqrt(var + EPS)).float()], dim=-1)


# ----------------------------------------------------------------------------------------------- bf16 mirror
def mirror_plants():
    """fp32 values whose bf16 rounding has a case of its own: exact ties (low half 0x8000) on an even and on an odd kept
    mantissa, one below and one above a tie, the largest finite bf16, fp32 subnormals (and the smallest normal), +-0; each
    in both signs"""
    bits = [0x3F808000, 0x3F818000,                      # ties: kept mantissa even (stays), odd (goes up)
            0x3F807FFF, 0x3F817FFF, 0x3F808001, 0x3F818001,
            0x40FF8000, 0x40FE8000, 0x3FFF8000,          # ties that carry into the exponent / the last mantissa step
            0x7F7F0000, 0x7F7F7FFF,                      # the largest finite bf16, and the largest fp32 that rounds to it
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00400000, 0x00800000, 0x00807FFF,
            0x00000000]
    bits = bits + [b | 0x80000000 for b in bits]
    return torch.tensor([b - (1 << 32) if b >> 31 else b for b in bits], dtype=torch.int32).view(torch.float32)
