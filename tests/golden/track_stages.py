"""Inputs, references, bounds, fp32 emulations and wrong implementations of the tracker-side stage kernels that are no gather and
no GEMM (tests/test_track_stages.py on the CPU, tests/test_track_stages_gpu.py on the GPU): pure torch / numpy, importable
without a device, nothing here calls the library.  Conventions of encoder_stages.py and mixer_stages.py: every reference is the
operation in fp64, every bound is per element (per row for the score-map terms) and comes from the arithmetic of a correct fp32
implementation, never from the kernel under test.  u = 2^-24.

point sample    ps_twin: point_sample_kernel in numpy float32, operation by operation, no fused multiply-add (bit gate).  ps_ref:
                the blend in fp64 with the twin's fp32 weights widened; four products and three sums, every one rounded once, the
                first product under three sums: |err| <= 6 u sum |w| |v|.
embedding       embed_ref: dx = fl(c - c[s = 0]), arg = fl(val * freq) in fp32 (freq = (i >> 1) * 31.25, exact), sin / cos of that
                fp32 argument in fp64.  No error of sinf / cosf is stated by the project or the toolchain: embed_gate is the
                yardstick rule, 4 x the worst error of torch's own fp32 sin / cos on the same arguments + 2^-24.
score map U     upsum_ref: the fp64 sum over the four levels of encoder_stages.resize_ref (bilinear, align_corners=True); bound =
                the four levels' encoder_stages.resize_bound, taken frame by frame, + 3 u sum |level terms| (three sums).
score terms     terms_ref: score_p = sum_c U f / sqrt(128), a = -label score, loss = b + log(exp(-b) + exp(a - b)), b = relu(a),
                in fp64 per pixel, then the two sums.  Per row:
                  score       d_p = (128 + 2) u sum_c |U f| / sqrt(128)   (128 products in any order, sqrtf(128), the division)
                                    (+ sum_c dU |f| / sqrt(128) where U itself carries a bound dU)
                  pixel loss  e_p = sigmoid(a_p + d_p) d_p + 2^-23 + 8 u loss_p: the loss has slope sigmoid(a) <= 1; the
                              logarithm's argument lies in [1, 2], where its rounding (u) and expf's error on the term <= 1
                              (<= 1 ulp) are absolute and pass through a slope 1 / t <= 1 -- an ABSOLUTE 2^-23, which is all that
                              is left of the loss below a = -16.6, where fp32 returns exactly 0 as the reference's fp32 does;
                              logf's own error, the sum b + log and what exceeds 2^-23 near a = 0 are relative, 8 u loss_p
                  positive    e_p of the target pixel (the block sum adds zeros to it)
                  negative    sum of e_p + (ceil(HW / 256) + 10) u sum loss_p: a thread's running sum, six shuffle steps, two
                              more sums
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from encoder_stages import U24, resize_bound, resize_ref, worst          # noqa: F401  (re-exported)
from mixer_stages import sum32                                           # noqa: F401

C = 128
SQRT_C = math.sqrt(float(C))
F32 = np.float32


# ----------------------------------------------------------------------------------------------- point sample
PS_SHAPES = ((2, 8, 33, 16, 20), (2, 5, 7, 17, 25), (1, 1, 1, 8, 8), (1, 12, 4, 46, 62))     # (B, S, N, H8, W8)
PS_WRONG = ("clamped_weights", "swapped_w01_w10", "frame_1", "fma")


def ps_maps(B, S, H8, W8, seed=31):
    """(B*S, H8, W8, 128) fp32 level-0 maps, every frame of every clip different"""
    g = torch.Generator().manual_seed(seed + 1000 * S + 10 * H8 + W8 + B)
    return torch.randn(B * S, H8, W8, C, generator=g)


def ps_specials(H8, W8):
    """(K, 2) fp32 positions with a case of their own; the first PS_INTEGERS are integers inside the map"""
    below = lambda v: float(np.nextafter(F32(v), F32(0)))
    return torch.tensor([[3.0, 5.0], [7.0, 6.0], [0.0, 0.0], [W8 - 1.0, H8 - 1.0], [W8 - 1.0, 0.0],      # the pixel's bits
                         [-5.0, -7.5], [W8 + 6.0, H8 + 2.0],                                              # clamped indices, unclamped weights
                         [-0.25, -0.25], [2.75, -0.25], [below(5.0), below(3.0)], [below(1.0), 2.5],
                         [1.0e6, -1.0e6], [-1.0e6, 1.0e6], [2.0 ** 24 + 1, 2.5], [1.5, 2.0 ** 24 + 1]], dtype=torch.float32)


PS_INTEGERS = 5


def ps_positions(B, N, H8, W8, seed=37):
    """(B, N, 2) fp32 random positions, a few of them just outside the map"""
    g = torch.Generator().manual_seed(seed + 100 * N + H8 + B)
    return torch.rand(B, N, 2, generator=g) * torch.tensor([W8 + 1.0, H8 + 1.0]) - 1.0


def _ps_parts(level0, S, xy, wrong=None):
    lv = level0.numpy() if isinstance(level0, torch.Tensor) else np.asarray(level0)
    xy = xy.numpy() if isinstance(xy, torch.Tensor) else np.asarray(xy)
    assert lv.dtype == F32 and xy.dtype == F32
    B = xy.shape[0]
    H, W = lv.shape[1:3]
    x, y = xy[..., 0], xy[..., 1]
    xw, yw = (np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)) if wrong == "clamped_weights" else (x, y)
    one = F32(1)
    x0f, y0f = np.floor(x), np.floor(y)
    x0w, y0w = np.floor(xw), np.floor(yw)
    x1w, y1w = x0w + one, y0w + one                                       # (x0f + 1 no longer differs from x0f at 2^24)
    xi0 = np.clip(x0f.astype(np.int64), 0, W - 1)
    xi1 = np.clip(x0f.astype(np.int64) + 1, 0, W - 1)
    yi0 = np.clip(y0f.astype(np.int64), 0, H - 1)
    yi1 = np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    w00, w01 = (x1w - xw) * (y1w - yw), (xw - x0w) * (y1w - yw)
    w10, w11 = (x1w - xw) * (yw - y0w), (xw - x0w) * (yw - y0w)
    if wrong == "swapped_w01_w10":
        w01, w10 = w10, w01
    f = (np.arange(B) * S + (1 if wrong == "frame_1" else 0))[:, None]
    ws = [w[..., None].astype(F32) for w in (w00, w01, w10, w11)]
    vs = [lv[f, yi0, xi0], lv[f, yi0, xi1], lv[f, yi1, xi0], lv[f, yi1, xi1]]
    assert all(w.dtype == F32 for w in ws) and all(v.dtype == F32 for v in vs)
    return ws, vs


def ps_twin(level0, S, xy, wrong=None):
    """point_sample_kernel in numpy float32 -> (B, N, 128) fp32 tensor.  wrong: one of PS_WRONG; "fma" contracts the blend into
    fma(w, v, acc) (emulated in fp64: the product of two fp32 numbers is exact there, the sum is rounded to fp64 and then to
    fp32 -- a double rounding that differs from a hardware fma in about one case in 2^29)."""
    ws, vs = _ps_parts(level0, S, xy, None if wrong == "fma" else wrong)
    if wrong == "fma":
        o = ws[0] * vs[0]
        for w, v in zip(ws[1:], vs[1:]):
            o = (w.astype(np.float64) * v.astype(np.float64) + o.astype(np.float64)).astype(F32)
    else:
        o = ws[0] * vs[0] + ws[1] * vs[1]
        o = o + ws[2] * vs[2]
        o = o + ws[3] * vs[3]
    assert o.dtype == F32
    return torch.from_numpy(np.ascontiguousarray(o))


def ps_ref(level0, S, xy):
    """-> (ref, bound) fp64 (B, N, 128): the blend in fp64 with the twin's fp32 weights widened; 6 u sum |w| |v|"""
    ws, vs = _ps_parts(level0, S, xy)
    ref = sum(w.astype(np.float64) * v.astype(np.float64) for w, v in zip(ws, vs))
    mag = sum(np.abs(w.astype(np.float64)) * np.abs(v.astype(np.float64)) for w, v in zip(ws, vs))
    return torch.from_numpy(ref), torch.from_numpy(6 * U24 * mag)


# ----------------------------------------------------------------------------------------------- embedding tail
EMB_WINDOWS = (1, 5, 8, 12, 32)
EMB_H8, EMB_W8 = 17, 24
EMB_DISP = (0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 0.5, -0.5, float(EMB_W8), -float(EMB_W8), 1.0e3, -1.0e3, 1.0e4, -1.0e4, 3.0e5, -3.0e5)
EMB_BASES = ((0.0, 0.0), (3.25, 5.5), (EMB_W8 - 1.0, EMB_H8 - 1.0))


def embed_coords(S, N):
    """(N*S, 2) fp32 particle-major positions: particle n sits at EMB_BASES[n] in frame 0; frame s >= 1 is displaced by
    EMB_DISP[k] in x and EMB_DISP[k + 7] in y, k running over the rows.  A displacement of -0.0 from a base of +0.0 is the
    coordinate -0.0, so that dx = (-0.0) - (+0.0) = -0.0."""
    co = torch.zeros(N, S, 2)
    k = 0
    D = len(EMB_DISP)
    for n in range(N):
        bx, by = EMB_BASES[n % len(EMB_BASES)]
        co[n, 0] = torch.tensor([bx, by])
        for s in range(1, S):
            for a, (b, d) in enumerate(((bx, EMB_DISP[k % D]), (by, EMB_DISP[(k + 7) % D]))):
                co[n, s, a] = -0.0 if (d == 0 and math.copysign(1.0, d) < 0 and b == 0) else b + d
            k += 1
    return co.reshape(N * S, 2)


def embed_ref(coords, times, S):
    """coords (M, 2) fp32 particle-major, times (S) fp32 -> dict(flow (M, 3) fp32 = the bits of columns 516:519, arg (M, 192)
    fp32, ref (M, 192) fp64 = columns 324:516, zero (M, 192) bool: arg == 0)"""
    co = coords.float().reshape(-1, S, 2)
    d = co - co[:, :1]                                                    # fp32, one rounding
    t = times.float().reshape(1, S, 1).expand(co.shape[0], S, 1)
    flow = torch.cat([d, t], dim=-1).reshape(-1, 3)
    i = torch.arange(64)
    freq = (i >> 1).float() * 31.25
    arg = (flow[:, :, None] * freq[None, None, :]).reshape(-1, 192)       # fp32, one rounding
    a64 = arg.double()
    ref = torch.where((i & 1).bool().repeat(3)[None, :], torch.cos(a64), torch.sin(a64))
    return dict(flow=flow, arg=arg, ref=ref, zero=arg == 0)


def embed_yardstick(r, device="cpu"):
    """worst |torch fp32 sin / cos - fp64| on the reference's fp32 arguments, evaluated on `device`"""
    a = r["arg"].to(device)
    odd = (torch.arange(192, device=device) % 2).bool()[None, :]
    got = torch.where(odd, torch.cos(a), torch.sin(a)).cpu().double()
    return float((got - r["ref"]).abs().max())


def embed_gate(yard_cpu, yard_dev):
    return 4 * max(yard_cpu, yard_dev) + U24


# ----------------------------------------------------------------------------------------------- score map: U
UP_SHAPES = ((2, 8, 8), (3, 17, 25), (2, 9, 23), (16, 64, 66))            # (F, H8, W8)


def up_levels(Fr, H8, W8, seed=41, device="cpu"):
    """four independent (not pooled) channel-last levels (F, H8 >> l, W8 >> l, 128) fp32, frame f scaled by 2^f"""
    g = torch.Generator().manual_seed(seed + 100 * H8 + W8 + Fr)
    sc = torch.exp2(torch.arange(Fr).float())[:, None, None, None]
    return [(torch.randn(Fr, H8 >> l, W8 >> l, C, generator=g) * sc).to(device) for l in range(4)]


def upsum_ref(levels, drop_level=None, align_corners=True):
    """-> (ref, bound) fp64 (F, H8, W8, 128).  drop_level / align_corners=False: the wrong implementations."""
    size = levels[0].shape[1:3]
    ref = torch.zeros(levels[0].shape, dtype=torch.float64, device=levels[0].device)
    mag, bound = torch.zeros_like(ref), torch.zeros_like(ref)
    for l, lv in enumerate(levels):
        if l == drop_level:
            continue
        r = resize_ref(lv, size, align_corners=align_corners)
        ref += r
        mag += r.abs()
        for f in range(lv.shape[0]):                                      # frame by frame: the frames differ by powers of two
            bound[f:f + 1] += resize_bound(lv[f:f + 1], r[f:f + 1])
    return ref, bound + 3 * U24 * mag


# ----------------------------------------------------------------------------------------------- score map: terms
TERM_SHAPES = ((1, 8, 3, 8, 8), (2, 5, 2, 17, 25), (1, 12, 1, 16, 20), (1, 1, 2, 46, 62))     # (B, S, N, H8, W8)
TERM_FAMILIES = ("dense", "large", "small", "impulse")
TERM_WRONG = ("label_sign", "target_among_negatives", "xy_swapped", "pitch_H8", "frame_S8", "clip_wrong_N", "log1p_exp", "no_sqrt_C")
K_LOSS = 8


def term_case(family, B, S, N, H8, W8, seed=43):
    """-> U (B*S, H8, W8, 128), ffeats (B*N*S, 128) fp32.  dense: U = 11 randn, f = randn: scores of std 11, both softplus
    branches; large: std 57, |score| up to ~200; small: 1e-3; impulse: frame f holds ONE non-zero value 2^(f mod 5) at pixel
    (7 f + 3) mod HW, channel (5 f + 1) mod 128, and row m a one-hot feature 4.0 at the channel of its own frame."""
    g = torch.Generator().manual_seed(seed + 1000 * S + 10 * H8 + W8 + N + TERM_FAMILIES.index(family))
    Fr, M, HW = B * S, B * N * S, H8 * W8
    if family == "impulse":
        U = torch.zeros(Fr, HW, C)
        f = torch.arange(Fr)
        U[f, (7 * f + 3) % HW, (5 * f + 1) % C] = torch.exp2((f % 5).float())
        ff = torch.zeros(M, C)
        fr = term_frames(B, S, N)
        ff[torch.arange(M), (5 * fr + 1) % C] = 4.0
        return U.reshape(Fr, H8, W8, C), ff
    scale = {"dense": 11.0, "large": 57.0, "small": 1.0e-3}[family]
    return torch.randn(Fr, H8, W8, C, generator=g) * scale, torch.randn(M, C, generator=g)


def term_frames(B, S, N):
    """frame b * S + s of mixer row m = (b * N + n) * S + s"""
    m = torch.arange(B * N * S)
    return (m // (S * N)) * S + m % S


def term_special_pixels(H8, W8):
    HW = H8 * W8
    px = [0, HW - 1, W8 - 1, HW - W8] + [p for p in (255, 256, 257) if p < HW]
    return list(dict.fromkeys(px))


def term_targets(B, S, N, H8, W8, family="dense", seed=47):
    """-> list of (M, 3) fp32 tables {x, y, use}: rows walk over the special pixels (0, HW - 1, the other two corners, 255, 256,
    257), then a table of random pixels; on the impulse family every other row of the last table aims at its frame's impulse.
    use = 0 on a quarter of the rows, with in-map positions."""
    M, HW = B * N * S, H8 * W8
    g = torch.Generator().manual_seed(seed + M + HW)
    sp = term_special_pixels(H8, W8)
    tables = []
    m = torch.arange(M)
    for t in range((len(sp) + M - 1) // M + 1):
        if t * M < len(sp):
            p = torch.tensor([sp[(t * M + i) % len(sp)] for i in range(M)])
        else:
            p = torch.randint(0, HW, (M,), generator=g)
            if family == "impulse":
                p = torch.where(m % 2 == 0, (7 * term_frames(B, S, N) + 3) % HW, p)
        use = ((m + t) % 4 != 3).float()
        tables.append(torch.stack([(p % W8).float(), (p // W8).float(), use], dim=-1))
    return tables


def softplus_stable(a):
    b = a.clamp_min(0)
    return b + torch.log(torch.exp(-b) + torch.exp(a - b))


def term_scores(U, ff, B, S, N, dtype=torch.float64, order=None, frames=None, scale=True):
    """(M, HW) scores sum_c U f (/ sqrt(128)); fp32 with `order`: every product and sum rounded, sums in that order (sum32)"""
    Fr = U.shape[0]
    Uf = U.reshape(Fr, -1, C).to(dtype)
    ff = ff.to(dtype)
    frames = term_frames(B, S, N) if frames is None else frames
    out = torch.zeros(ff.shape[0], Uf.shape[1], dtype=dtype)
    for f in frames.unique().tolist():
        idx = (frames == f).nonzero()[:, 0]
        if order is None:
            out[idx] = ff[idx] @ Uf[f].t()
        else:
            out[idx] = sum32(Uf[f][None, :, :] * ff[idx][:, None, :], order)
    if scale:
        out = out / (torch.sqrt(torch.tensor(float(C), dtype=dtype)) if dtype == torch.float32 else SQRT_C)
    return out


def _target_pixel(tgt, W8):
    return tgt[:, 1].long() * W8 + tgt[:, 0].long()


def terms_ref(U, ff, tgt, B, S, N, H8, W8, dU=None):
    """-> dict(pos, neg, bpos, bneg) fp64 (M,): the two terms of every row and their bounds (module docstring); rows with
    use = 0 are 0 with bound 0.  U, ff: fp32, or fp64 values with dU the bound U carries (fp64, U's shape)."""
    HW = H8 * W8
    sc = term_scores(U, ff, B, S, N)
    d = (C + 2) * U24 * term_scores(U.abs(), ff.abs(), B, S, N)
    if dU is not None:
        d = d + term_scores(dU, ff.abs(), B, S, N)
    pt = _target_pixel(tgt, W8)
    is_t = torch.arange(HW)[None, :] == pt[:, None]
    a = torch.where(is_t, -sc, sc)
    loss = softplus_stable(a)
    e = torch.sigmoid(a + d) * d + 2.0 ** -23 + K_LOSS * U24 * loss
    use = (tgt[:, 2] > 0).double()
    z = torch.zeros_like(loss)
    ln, en = torch.where(is_t, z, loss), torch.where(is_t, z, e)
    pos, bpos = torch.where(is_t, loss, z).sum(1), torch.where(is_t, e, z).sum(1)
    neg = ln.sum(1)
    bneg = en.sum(1) + ((HW + 255) // 256 + 10) * U24 * neg
    return dict(pos=pos * use, neg=neg * use, bpos=bpos * use, bneg=bneg * use)


def pixel_sum32(t, order):
    """fp32 sum over the pixels (last axis) by a reduction at most ceil(HW / 256) + 10 deep, the only kind the negative term's
    bound covers: "pair" a binary tree over all pixels; "seq" the kernel's shape -- lane i adds pixels i, i + 256, ... one by
    one, then a tree over the 256 lanes.  (One running sum over all HW pixels is HW - 1 deep: on the impulse family, where
    every pixel's loss is the same log 2, it reached 1.28 of the bound at HW = 425.)"""
    if order == "pair":
        return sum32(t, "pair")
    n = t.shape[-1]
    t = F.pad(t.float(), (0, -n % 256)).reshape(*t.shape[:-1], -1, 256)
    return sum32(sum32(t.transpose(-1, -2), "seq"), "pair")


def terms32(U, ff, tgt, B, S, N, H8, W8, order, wrong=None):
    """score_terms_kernel's formula in fp32 torch arithmetic, the channel sums in `order` ("seq" / "pair"), the pixel sums by
    pixel_sum32(order) -> (M, 2) fp32 {positive, negative}.  wrong: one of TERM_WRONG."""
    HW = H8 * W8
    M = ff.shape[0]
    m = torch.arange(M)
    frames = None
    if wrong == "frame_S8":
        frames = ((m // (8 * N)) * S + m % 8).clamp_max(U.shape[0] - 1)
    elif wrong == "clip_wrong_N":
        frames = ((m // (S * (N + 1))) * S + m % S).clamp_max(U.shape[0] - 1)
    sc = term_scores(U, ff, B, S, N, torch.float32, order, frames, scale=wrong != "no_sqrt_C")
    x, y = tgt[:, 0].long(), tgt[:, 1].long()
    pt = y * W8 + x
    if wrong == "xy_swapped":
        pt = (x * W8 + y).clamp_max(HW - 1)
    elif wrong == "pitch_H8":
        pt = (y * H8 + x).clamp_max(HW - 1)
    is_t = torch.arange(HW)[None, :] == pt[:, None]
    a = torch.where(is_t, sc, -sc) if wrong == "label_sign" else torch.where(is_t, -sc, sc)
    loss = torch.log(1.0 + torch.exp(a)) if wrong == "log1p_exp" else softplus_stable(a)
    assert loss.dtype == torch.float32
    z = torch.zeros_like(loss)
    pos = torch.where(is_t, loss, z).sum(1)
    neg = pixel_sum32(torch.where(is_t, z, loss), order)
    if wrong == "target_among_negatives":
        neg = neg + softplus_stable(torch.where(is_t, sc, z).sum(1))
    use = (tgt[:, 2] > 0).float()
    return torch.stack([pos * use, neg * use], dim=-1)


def terms_worst(got, r):
    """(worst positive error / bound, worst negative error / bound) of (M, 2) terms; a value that is not finite counts as infinite"""
    g = got.double().nan_to_num(nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
    return worst((g[:, 0] - r["pos"]).abs(), r["bpos"]), worst((g[:, 1] - r["neg"]).abs(), r["bneg"])


# ----------------------------------------------------------------------------------------------- target selection
def oracle_selection(trajs_map, vis_g, valids, H8, W8):
    """score_map_loss's own selection (oracle/pips_oracle.py::score_map_loss, nets/pips.py:62-69) on trajs_map (B,S,N,2) in map
    pixels -> (x, y, ind) of the B*S*N heat maps in (b, s, n) order"""
    xy = trajs_map.reshape(-1, 2).round().long()
    x, y = xy[:, 0], xy[:, 1]
    ind = (x >= 0) & (x <= (W8 - 1)) & (y >= 0) & (y <= (H8 - 1)) & (valids.reshape(-1) > 0) & (vis_g.reshape(-1) > 0)
    return x, y, ind


def selection_probes(H8, W8, stride):
    """(trajs_g (1, S, N, 2) in image pixels, vis_g, valids): k + 0.5 on even and odd k (half to even), negatives, -0.5,
    W8 - 0.5, W8 - 1, both map edges in y, and every position once with valids = 0 and once with vis_g = 0"""
    xs = [0.5, 1.5, 2.5, 3.5, -0.5, -0.49, -1.0, -3.0, W8 - 0.5, W8 - 1.0, W8 - 1.5, W8 - 0.51, float(W8), 4.0, 0.0]
    ys = [0.5, 1.5, 2.5, -0.5, H8 - 0.5, H8 - 1.0, H8 - 1.5, float(H8), 2.0, 0.0]
    pts = torch.tensor([[x, y] for x in xs for y in ys]) * stride
    n = pts.shape[0]
    tg = pts.reshape(1, 1, n, 2).repeat(1, 3, 1, 1)
    vis, val = torch.ones(1, 3, n), torch.ones(1, 3, n)
    val[0, 1], vis[0, 2] = 0.0, 0.0
    return tg, vis, val


# ----------------------------------------------------------------------------------------------- per-iteration wiring
WIRING_CASE = "s8_trained_i6"
_wiring = {}


def pyramid_nhwc(pyramid):
    """oracle pyramid, a list of (B, S, C, h, w) -> channel-last (B*S, h, w, C) levels"""
    return [p.reshape(-1, *p.shape[2:]).permute(0, 2, 3, 1).contiguous() for p in pyramid]


def pm(t):
    """(B, S, N, X) -> particle-major (B*N*S, X)"""
    B, S, N, X = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N * S, X).contiguous()


def wiring_refs():
    """The evaluation branch on cases.TRAINED_CASES[WIRING_CASE] (B = 2, N = 16, 136 x 200, 6 iterations, trained-like tamed
    weights) from the fp64 and the fp32 oracle, computed once: per iteration the fp64 terms of the fp64 oracle's
    taps["iters"][it]["ffeats_in"] with their stage bound (U's own bound carried through), and the yardstick: the error of the
    fp32 oracle's terms (its own forward, O.dense_score_maps, the softplus in fp32) against those values -- relative for the
    negative term, absolute for the positive one.  gate = 4 x yardstick + stage bound."""
    if _wiring:
        return _wiring
    import cases as G
    from oracle import pips_oracle as O
    from pips_amd.pips import _score_map_targets
    case = G.TRAINED_CASES[WIRING_CASE]
    B, N, S, iters, stride = case["B"], case["N"], 8, case["iters"], case["stride"]
    H8, W8 = case["H"] // stride, case["W"] // stride
    sd = G.case_state_dict(case)
    xys, rgbs, _, _ = G.make_inputs(case)
    tg, vg, va = G.make_targets(case)
    tgt = _score_map_targets(tg, vg, va, float(stride), H8, W8)
    used = tgt[:, 2] > 0
    t64, t32 = {}, {}
    O.forward(O.to_dtype(sd, torch.float64), xys.double(), rgbs.double(), iters=iters, stride=stride, taps=t64)
    O.forward(sd, xys, rgbs, iters=iters, stride=stride, taps=t32)
    U64, dU = upsum_ref(pyramid_nhwc(t64["pyramid"]))
    dU = dU + U24 * U64.abs()                                             # the stored U is an fp32 number
    pt = _target_pixel(tgt, W8)
    is_t = torch.arange(H8 * W8)[None, :] == pt[:, None]
    its = []
    for it in range(iters):
        r = terms_ref(U64, pm(t64["iters"][it]["ffeats_in"]), tgt, B, S, N, H8, W8, dU=dU)
        fcp = O.dense_score_maps(t32["pyramid"], t32["iters"][it]["ffeats_in"])                      # (B,S,N,H8,W8) fp32
        sc = pm(fcp.reshape(B, S, N, H8 * W8))
        loss = softplus_stable(torch.where(is_t, -sc, sc))
        z = torch.zeros_like(loss)
        pos32, neg32 = torch.where(is_t, loss, z).sum(1).double(), torch.where(is_t, z, loss).sum(1).double()
        y_neg = float(((neg32 - r["neg"]).abs() / r["neg"].clamp_min(1e-300))[used].max())
        y_pos = float((pos32 - r["pos"]).abs()[used].max())
        r.update(yard_neg_rel=y_neg, yard_pos_abs=y_pos, gate_neg=4 * y_neg * r["neg"] + r["bneg"], gate_pos=(4 * y_pos + r["bpos"]) * used.double())
        its.append(r)
    _wiring.update(case=case, sd=sd, xys=xys, rgbs=rgbs, tgt=tgt, used=used, B=B, N=N, S=S, H8=H8, W8=W8, iters=iters, stride=stride, its=its)
    return _wiring
