"""Inputs, references and bounds of the mixer's and the update's stage kernels (tests/test_mixer_stages.py on the CPU,
tests/test_mixer_stages_gpu.py on the GPU): pure torch, importable without a device, nothing here calls the library.  The
conventions are those of encoder_stages.py: every reference is the operation in fp64 (formulas of oracle/pips_oracle.py::mixer
and ::update_step), every bound is per element and comes from the arithmetic of a correct implementation, never from the kernel
under test.  u = 2^-24.

normalised values   the yardstick rule of the encoder stage tests: torch's own fp32 F.layer_norm / F.group_norm on the same
                    operands against fp64; the gate is 4x its worst error plus a floor of 4 u of the value and 8 u of the
                    magnitudes it is formed from (ln_floor).
sums of products    K products and a bias summed in any order: (K + 8) u times the fp64 magnitude sum (|b| + sum |w| |h|), plus
                    the operands' own gates carried through sum |w|.
GELU                |gelu'| <= 1.13; the project's stated absolute errors (csrc/common.h): 4.8e-7 for gelu_exact, 5.1e-6 for
                    gelu_bf16out2 before its rounding.
bf16 roundings      the reference rounds (RNE) where the kernels round: token-MLP weights, LN1(x), the hidden units, the stored
                    stream.  A rounding is a step function: a value whose distance to a rounding tie is below its own
                    pre-rounding gate may legitimately land on either neighbour, a whole bf16 ulp apart.  round_slack() marks
                    exactly those operands and the bound carries one ulp of each through the weights behind it; an operand away
                    from a tie gets nothing (14 % of the outputs carry such an allowance on the centred rows, and the
                    fp32 emulations with the fast GELU's error in either direction reach 0.98 of the bound there: the ties are
                    real).  A bf16 OUTPUT adds half a bf16 ulp.

Token rows differ in kind (token_rows): token t has its own scale 2^(t mod 5 - 2) and its own mean, so a statistic handed to
another token misses the bounds by orders of magnitude (test_mixer_stages.py proves it for every pair).
"""
import torch
import torch.nn.functional as F

from encoder_stages import U24, bf16_half_ulp, worst          # noqa: F401  (re-exported)

D = 512
C = 128
EPS = 1e-5
GELU_LIP = 1.13              # max |d gelu / dx| = 1.1290
GELU_F32_ABS = 4.8e-7        # gelu_exact, csrc/common.h
GELU_BF16OUT_ABS = 5.1e-6    # gelu_bf16out2 before its rounding, csrc/common.h
MD = "delta_block.to_delta"
LAYERS = (0, 5, 11)

# The largest per-row |mean| / std over the 25 LayerNorm inputs of the fp64 oracle's mixer (taps["ln_in"] of
# oracle/pips_oracle.py::mixer).  Measured maxima: cases.mixer_rows(64) on init_state_dict(0) 1.4223 (raw and tamed alike: the
# mixer's weights are the same), on trained_like_state_dict(0) 1.3375; the mixer inputs of the golden forwards: s8_raw_i3
# (init weights, 3 iterations) 0.8234, s8_trained_i6 (trained-like, 6 iterations) 0.7970.  The first LayerNorm sees 0.08 .. 0.17,
# the ratio grows to ~1.3 by layer 7 and stays.  No trained checkpoint is at hand, hence the 4x margin of SHIFTS;
# 64 is a fixed probe.  tests/test_mixer_stages.py::test_shift_range_is_the_oracles recomputes the first figure.
R = 1.43
SHIFTS = (0.0, R, 4 * R)
SHIFT_PROBE = 64.0

WINDOWS = ((1, 2), (5, 3), (12, 2), (16, 1), (17, 2), (32, 1))        # (S, P): both SMAX instantiations, their edges, PIPS_S_MAX


def delta_stride(S):
    return (S * (C + 2) + 3) & ~3


def bf16r(x):
    """fp64 / fp32 -> the bf16 round-to-nearest-even of the value, as fp64"""
    return x.float().bfloat16().double()


def bf16_ulp(x):
    return 2 * bf16_half_ulp(x)


def round_slack(v, delta):
    """How far the bf16 rounding of a value within delta of v (fp64) can be from bf16r(v): 0 where every such value rounds the
    same way (delta is below v's distance to the nearest tie), else delta + one bf16 ulp (|rn(a) - rn(b)| <= |a - b| + ulp)."""
    v = v.double()
    to_tie = bf16_half_ulp(v) - (v - bf16r(v)).abs()
    return torch.where(delta < to_tie, torch.zeros_like(v), delta + bf16_ulp(v.abs() + delta))


# ----------------------------------------------------------------------------------------------- inputs
def token_means(S):
    """per-token mean offset in units of the token's std: distinct for every token, about 0"""
    return 0.02 * (torch.arange(S, dtype=torch.float64) - S / 2)


def token_scales(S):
    return torch.exp2((torch.arange(S) % 5 - 2).double())


def token_rows(P, S, family="centred", r=0.0, seed=5, width=D):
    """(P, S, width) fp32 rows.  Every row is noise with per-channel structure (a channel profile of scale 0.5 .. 1.5 and a
    ramp), standardised exactly (fp64: mean 0, std 1), then row (p, t) = scale_t (z + r + token_means[t]).
    family "centred": r = 0;  "shifted": the row mean sits r stds from 0;  "hot": centred, plus one channel per row, a
    different one for every (p, t), at 60 stds."""
    assert family in ("centred", "shifted", "hot")
    g = torch.Generator().manual_seed(seed + 1000 * S + 17 * P + width)
    c = torch.arange(width, dtype=torch.float64)
    z = torch.randn(P, S, width, generator=g, dtype=torch.float64) * (1.0 + 0.5 * torch.sin(0.37 * c)) + 0.3 * (c / width - 0.5)
    z = (z - z.mean(-1, keepdim=True)) / z.std(-1, unbiased=False, keepdim=True)
    shift = (r if family == "shifted" else 0.0) + token_means(S)
    x = token_scales(S)[None, :, None] * (z + shift[None, :, None])
    if family == "hot":
        p, t = torch.meshgrid(torch.arange(P), torch.arange(S), indexing="ij")
        x[p, t, (7 * t + 13 * p + 3) % width] = 60.0 * token_scales(S)[t]
    return x.float()


def update_inputs(B, N, S, seed=11, pad=1.0e3):
    """-> delta (B*N, delta_stride(S)), ffeats (B*N, S, 128), coords, coords0 (B*N, S, 2), particle-major fp32.  Delta rows
    are token-distinct (token_rows on 130 channels, a mean of 0.3 stds per token step on top); the floats between S*130 and
    the stride hold pad + their index."""
    BN = B * N
    g = torch.Generator().manual_seed(seed + 100 * S + BN)
    d = token_rows(BN, S, "centred", seed=seed, width=C + 2).double()
    d = d + (0.3 * (torch.arange(S, dtype=torch.float64) - S / 2) * token_scales(S))[None, :, None]
    delta = torch.empty(BN, delta_stride(S), dtype=torch.float64)
    delta[:, :S * (C + 2)] = d.reshape(BN, -1)
    npad = delta_stride(S) - S * (C + 2)
    delta[:, S * (C + 2):] = pad + torch.arange(BN * npad, dtype=torch.float64).reshape(BN, npad)
    ffeats = torch.randn(BN, S, C, generator=g)
    coords = torch.rand(BN, S, 2, generator=g) * 40
    coords0 = coords + 0.5 + 0.01 * torch.arange(BN * S * 2).reshape(BN, S, 2)
    return delta.float(), ffeats, coords, coords0.float()


# ----------------------------------------------------------------------------------------------- weights
def mix_weights(sd, layer):
    """the tensors one token-mixing launch of layer `layer` (0-based) reads, fp32"""
    k = f"{MD}.{layer + 1}"
    w = dict(g1=sd[f"{k}.0.norm.weight"], b1=sd[f"{k}.0.norm.bias"], w0=sd[f"{k}.0.fn.0.weight"][:, :, 0], b0=sd[f"{k}.0.fn.0.bias"],
             w3=sd[f"{k}.0.fn.3.weight"][:, :, 0], b3=sd[f"{k}.0.fn.3.bias"], g2=sd[f"{k}.1.norm.weight"], b2=sd[f"{k}.1.norm.bias"])
    return {n: t.float() for n, t in w.items()}


def final_ln(sd):
    return sd[f"{MD}.13.weight"].float(), sd[f"{MD}.13.bias"].float()


# ----------------------------------------------------------------------------------------------- LayerNorm
def ln64(x, g, b):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) * g.double() + b.double()


def ln_floor(x, g):
    """8 u of the magnitudes a LayerNorm's result is formed from, (|x| + |mean|) rstd |g|: one u per rounding on the way from
    the operands to the result whatever the summation order -- the mean (its sum and its scaling: it is a rounded fp32 number,
    so x - mean carries u |mean|, and on rows whose mean is r stds from zero that alone is r u of the normalised value), the
    difference, rstd (sum of squares, scaling, + eps, square root, reciprocal) and the two products"""
    x = x.double()
    m = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + EPS)
    return 8 * U24 * (x.abs() + m.abs()) * rstd * g.double().abs()


def ln_ref(x, g, b):
    """-> (ref, gate), fp64: the LayerNorm of the fp32 (or bf16) rows x and the yardstick gate: 4 max|F.layer_norm_fp32 - ref|
    + the floor 4 u |ref| + ln_floor"""
    ref = ln64(x, g, b)
    yard = F.layer_norm(x.float(), (x.shape[-1],), g.float(), b.float()).double()
    return ref, 4 * float((yard - ref).abs().max()) + 4 * U24 * ref.abs() + ln_floor(x, g)


def ln_mean_ref(x, g, b):
    """-> (ref (P, 512), gate): LayerNorm per token, mean over the tokens; the yardstick is torch's fp32 of the same, the
    floor the mean over the tokens of ln_ref's"""
    n = ln64(x, g, b)
    ref = n.mean(1)
    yard = F.layer_norm(x.float(), (x.shape[-1],), g.float(), b.float()).mean(1).double()
    return ref, 4 * float((yard - ref).abs().max()) + (4 * U24 * n.abs() + ln_floor(x, g)).mean(1)


def row_half_ulp(ref):
    """half a bf16 ulp at the largest value of each row: the size of the rounding noise the row's bf16 form carries, the
    yardstick of the fixed probe (an error of a LayerNorm's statistics is common to the row, not relative to each element)"""
    return bf16_half_ulp(ref.abs().amax(-1, keepdim=True)).expand_as(ref)


# ----------------------------------------------------------------------------------------------- token mixing
def token_mix_ref(x, w, bf16=False, dn=None):
    """One token-mixing step on x (P, S, 512) (fp32, or the values of a bf16 stream) -> (y, bound), fp64: the new residual
    stream y = x + b3 + w3 gelu(b0 + w0 LN1(x)) over the token axis and its per-element bound BEFORE any rounding of y.
    bf16: the matrix-core contract -- w0, w3, LN1(x) and the hidden units rounded to bf16, everything else as it is.
    dn: the pre-rounding gate of LN1(x); default the yardstick gate."""
    S = x.shape[1]
    n, gate = ln_ref(x, w["g1"], w["b1"])
    dn = gate if dn is None else dn
    w0, w3 = w["w0"].double(), w["w3"].double()
    b0, b3 = w["b0"].double(), w["b3"].double()
    if bf16:
        w0, w3 = bf16r(w0), bf16r(w3)
        dn = round_slack(n, dn)
        n = bf16r(n)
    h = torch.einsum("jt,ptc->pjc", w0, n) + b0[None, :, None]
    dh = torch.einsum("jt,ptc->pjc", w0.abs(), dn) + (S + 8) * U24 * (torch.einsum("jt,ptc->pjc", w0.abs(), n.abs()) + b0.abs()[None, :, None])
    u = F.gelu(h)
    du = GELU_LIP * dh + (GELU_BF16OUT_ABS if bf16 else GELU_F32_ABS) + 4 * U24 * u.abs()
    if bf16:
        flip = round_slack(u, du)
        du = du + torch.where(flip > 0, bf16_ulp(u.abs() + du), torch.zeros_like(u))
        u = bf16r(u)
    xd = x.double()
    y = xd + b3[None, :, None] + torch.einsum("tj,pjc->ptc", w3, u)
    mag = xd.abs() + b3.abs()[None, :, None] + torch.einsum("tj,pjc->ptc", w3.abs(), u.abs())
    return y, torch.einsum("tj,pjc->ptc", w3.abs(), du) + (4 * S + 8) * U24 * mag


def stored_bf16_bound(ref, pre):
    """bound of a value stored as bf16 whose pre-rounding gate is `pre`: half a bf16 ulp (at |ref| + pre: the rounding
    happens on the implementation's side of a binade edge) + pre"""
    return bf16_half_ulp(ref.abs() + pre) + pre


# ----------------------------------------------------------------------------------------------- state update
def update_ref(sd, delta, ffeats, coords, coords0, S, stride):
    """-> dict of (ref, bound) pairs, fp64, particle-major: ffeats (BN,S,128), coords (BN,S,2), traj_pm (BN,S,2) px, and
    vis (BN,S) with its bound.  oracle.update_step's formulas + the vis_predictor Linear."""
    BN = delta.shape[0]
    d = delta[:, :S * (C + 2)].reshape(BN, S, C + 2)
    df = d[:, :, 2:]
    g, b = sd["norm.weight"].float(), sd["norm.bias"].float()
    hn = ln64(df, g, b)
    yard = F.group_norm(df.reshape(-1, C).float(), 1, g, b, eps=EPS).reshape(BN, S, C).double()
    dhn = 4 * float((yard - hn).abs().max()) + 4 * U24 * hn.abs()
    W, bu = sd["ffeat_updater.0.weight"].double(), sd["ffeat_updater.0.bias"].double()
    acc = hn @ W.t() + bu
    dacc = dhn @ W.abs().t() + (C + 8) * U24 * (hn.abs() @ W.abs().t() + bu.abs())
    ge = F.gelu(acc)
    nf = ge + ffeats.double()
    dnf = GELU_LIP * dacc + GELU_F32_ABS + 4 * U24 * (ge.abs() + ffeats.double().abs())
    co = coords.double() + d[:, :, :2].double()
    dco = 2 * U24 * (coords.double().abs() + d[:, :, :2].double().abs())
    co[:, 0] = coords0.double()[:, 0]
    dco[:, 0] = 0
    wv, bv = sd["vis_predictor.0.weight"].double()[0], sd["vis_predictor.0.bias"].double()[0]
    vis, dvis = vis_ref(sd, nf)
    return dict(ffeats=(nf, dnf), coords=(co, dco), traj=(co * stride, (dco + U24 * co.abs()) * stride),
                vis=(vis, dvis + dnf @ wv.abs()))


def vis_ref(sd, ffeats):
    """vis_predictor on features (..., 128) as given -> (ref, bound) fp64: 128 products and a bias in any order"""
    wv, bv = sd["vis_predictor.0.weight"].double()[0], sd["vis_predictor.0.bias"].double()[0]
    f = ffeats.double()
    return f @ wv + bv, (C + 8) * U24 * (f.abs() @ wv.abs() + bv.abs())


def to_bsn(t, B, N):
    """particle-major (B*N, S, ...) -> (B, S, N, ...)"""
    return t.reshape(B, N, *t.shape[1:]).transpose(1, 2)


# ----------------------------------------------------------------------------------------------- fp32 emulations (CPU proofs)
def sum32(t, order):
    """fp32 sum over the last axis in a fixed order: "seq" ascending one by one, "pair" a binary tree"""
    t = t.float()
    if order == "seq":
        acc = torch.zeros_like(t[..., 0])
        for i in range(t.shape[-1]):
            acc = acc + t[..., i]
        return acc
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def ln_stats32(x, order, one_pass=False):
    """fp32 {mean, rstd} (..., 1) of the rows: two passes (mean, then centred squares) or the one-pass form
    var = max(sum x^2 / n - mean^2, 0)"""
    x = x.float()
    n = x.shape[-1]
    m = (sum32(x, order) * (1.0 / n))[..., None]
    if one_pass:
        v = torch.clamp_min(sum32(x * x, order)[..., None] * (1.0 / n) - m * m, 0.0)
    else:
        v = sum32((x - m) ** 2, order)[..., None] * (1.0 / n)
    return m, 1.0 / torch.sqrt(v + 1e-5)


def ln32(x, g, b, order, one_pass=False, stats=None):
    m, r = ln_stats32(x, order, one_pass) if stats is None else stats
    return (x.float() - m) * (r * g.float()) + b.float()


def dot32(w, h, bias, order, eq):
    """bias + sum over the contracted axis of w * h in fp32 in a fixed order; eq as in token_mix_ref"""
    if eq == "jt,ptc->pjc":
        prod = w.float()[None, :, :, None] * h.float()[:, None, :, :]           # (p, j, t, c)
        return bias.float()[None, :, None] + sum32(prod.transpose(2, 3), order)
    raise ValueError(eq)


def token_mix32(x, w, order, bf16=False, one_pass=False, stats1=None, gelu_shift=0.0):
    """The step in fp32 arithmetic with sums in `order`; bf16: operands rounded where the matrix-core kernel rounds them.
    stats1: {mean, rstd} to use for LayerNorm 1 instead of the rows' own (planted errors).  gelu_shift: added to the hidden
    units before a bf16 rounding (the allowance of the fast GELU, in either direction)."""
    rb = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    n = rb(ln32(x, w["g1"], w["b1"], order, one_pass, stats1))
    h = dot32(rb(w["w0"]), n, w["b0"], order, "jt,ptc->pjc")
    u = rb(F.gelu(h.double()).float() + gelu_shift)
    o = dot32(rb(w["w3"]), u, w["b3"], order, "jt,ptc->pjc")
    return x.float() + o
