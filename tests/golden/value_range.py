"""Builders and gates of the value-range tests (tests/test_value_range.py on the CPU, tests/test_value_range_gpu.py on the
GPU): pure torch / numpy, importable without a device.

Three families.
A. The GELU as a function: a one-hot A selects W[n, m % K] as the pre-activation of output (m, n) exactly, so a GEMM with the
   GELU epilogue evaluates the kernel's GELU on a chosen sweep.  Gate per bucket of x: 2 * E_ref + 2^-24, E_ref the error of
   F.gelu in fp32 against F.gelu in fp64 on the same bucket.
B. bf16 stores: a zero accumulator plus an fp32 addend of chosen bit patterns, compared bit for bit with torch's RNE.
C. Mixed scales: power-of-two scales per row / input channel of A and per output channel of W and the bias; outputs judged
   element by element against the componentwise forward bound gamma * (|A||W|^T + |b| + |R|).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24              # unit roundoff of fp32
BF16_HALF_ULP = 2.0 ** -8     # relative half ulp of bf16 (8 significant bits)
FLUSH = 2.0 ** -126           # below this an fp32 value is subnormal: flushing it is mode-dependent
GELU_TMAX = float(np.float32(5.65685425))
GELU_SLOPE = 1.13             # max |gelu'| = 1.1290 (at x = sqrt(2))

# ----------------------------------------------------------------------------------------------- A. the GELU sweep
BUCKETS = ((-12.0, -5.7), (-5.7, -3.0), (-3.0, -0.5), (-0.5, 0.5), (0.5, 3.0), (3.0, 12.0))
BUCKET_NAMES = tuple(f"[{lo:g}, {hi:g}{']' if hi == 12.0 else ')'}" for lo, hi in BUCKETS) + ("|x| > 12",)


def bucket_index(x):
    """bucket number (0..5 as BUCKETS, 6 = |x| > 12) of every element of x"""
    x = x.double()
    idx = torch.full(x.shape, 6, dtype=torch.long, device=x.device)
    for i, (lo, hi) in enumerate(BUCKETS):
        inside = (x >= lo) & ((x <= hi) if hi == 12.0 else (x < hi))
        idx = torch.where(inside, torch.full_like(idx, i), idx)
    return idx


def bf16_values(limit=64.0):
    """every bf16 value with |x| <= limit as fp32 (34 050 for limit = 64: zeros and subnormals included)"""
    hi = torch.arange(0, 0x7F80, dtype=torch.int32)                    # positive finite bf16 bit patterns
    pos = (hi << 16).view(torch.float32)
    pos = pos[pos <= limit]
    return torch.cat([pos, -pos])


def _neighbours(v, n=2):
    """the fp32 value v and its n fp32 neighbours on either side"""
    out, lo, hi = [np.float32(v)], np.float32(v), np.float32(v)
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return [float(t) for t in out]


def gelu_specials():
    """+-0, tiny, subnormal, large values and the clamp of the polynomial GELU with its fp32 neighbours, in both signs"""
    pos = [0.0, 1e-30, 1e-40, 20.0, 1e4] + _neighbours(GELU_TMAX)
    pos = torch.tensor(pos, dtype=torch.float64).float()
    return torch.cat([pos, -pos])


def gelu_sweep_f32(slots):
    """The sweep of the fp32 and split routes for a W of ``slots`` = N * K entries: the specials, every bf16 value with
    |x| <= 64 and a dense uniform grid on [-12, 12] in the rest."""
    fixed = torch.cat([gelu_specials(), bf16_values()])
    if slots < fixed.numel() + 1024:
        raise ValueError(f"{slots} slots do not hold the {fixed.numel()} fixed points of the sweep and a grid")
    grid = torch.linspace(-12.0, 12.0, slots - fixed.numel(), dtype=torch.float64).float()
    return torch.cat([fixed, grid])


def gelu_sweep_bf16(slots):
    """The sweep of the bf16 routes: the 34 050 bf16 values, tiled over the slots."""
    v = bf16_values()
    if slots < v.numel():
        raise ValueError(f"{slots} slots do not hold the {v.numel()} bf16 values")
    return v.repeat((slots + v.numel() - 1) // v.numel())[:slots].contiguous()


def onehot_operands(M, N, K, sweep):
    """(A, W): A[m, m % K] = 1, W (N, K) = the sweep -- the pre-activation of output (m, n) is W[n, m % K] exactly"""
    A = torch.zeros(M, K)
    A[torch.arange(M), torch.arange(M) % K] = 1.0
    return A, sweep.reshape(N, K).contiguous()


def selected(W, M):
    """(M, N) matrix of the pre-activations the one-hot A selects.  A sum 0 + ... + x + ... + 0 of IEEE numbers is x, except
    that -0 comes out as +0 (the other terms are +0)."""
    K = W.shape[1]
    sel = W.t()[torch.arange(M, device=W.device) % K]
    return torch.where(sel == 0, torch.zeros_like(sel), sel).contiguous()


def bitwise_equal(out, expect):
    """two fp32 tensors agree bit for bit (a -0 is not a +0, a flushed subnormal is not its value)"""
    return torch.equal(out.view(torch.int32), expect.view(torch.int32))


def planes_to_f32(planes):
    """int16 bf16 planes (3, ...) of the split path -> the fp32 value they sum to"""
    return (planes.to(torch.int32) << 16).view(torch.float32).double().sum(dim=0).float()


_EREF = {}


def gelu_eref():
    """E_ref per bucket: max |F.gelu(x_fp32) - F.gelu(x_fp64)| over the 1 M point sweep of the fp32 routes (2048 x 512),
    on the CPU.  Measured with torch 2.x: 3.4e-8, 1.1e-6, 9.3e-7, 3.5e-8, 1.1e-6, 1.2e-6."""
    if not _EREF:
        x = gelu_sweep_f32(2048 * 512)
        err = (F.gelu(x).double() - F.gelu(x.double())).abs()
        idx = bucket_index(x)
        for i in range(7):
            _EREF[i] = float(err[idx == i].max())
    return dict(_EREF)


def gelu_gate_f32(x):
    """per-element bound of an fp32 GELU output at pre-activation x: 2 * E_ref(bucket of x) + 2^-24.  The factor 2: a
    kernel as good as the reference must not fail on the reference's noise; 2^-24: beyond the clamp the kernels return a
    constant of about -4.4e-8 where E_ref is 3e-8."""
    e = gelu_eref()
    table = torch.tensor([e[i] for i in range(7)], dtype=torch.float64, device=x.device)
    return 2.0 * table[bucket_index(x)] + U24


def gelu_gate_bf16(x, ref64):
    """the same for a bf16 output: half a bf16 ulp of the reference on top of the fp32 bound"""
    return BF16_HALF_ULP * ref64.abs() + gelu_gate_f32(x)


def gelu_ref64(x):
    return F.gelu(x.double())


def bucket_maxima(err, x):
    """{bucket name: max of err over the bucket} (buckets without a point are left out)"""
    idx = bucket_index(x)
    return {BUCKET_NAMES[i]: float(err[idx == i].max()) for i in range(7) if bool((idx == i).any())}


def rounding_safe(x, ref64):
    """elements whose bf16 rounding no admissible fp32 error can change: bf16(ref64 - d) == bf16(ref64 + d), d the fp32 bound"""
    d = gelu_gate_f32(x)
    lo, hi = (ref64 - d).float().bfloat16(), (ref64 + d).float().bfloat16()
    return lo.view(torch.int16) == hi.view(torch.int16)


# numpy fp32 emulations of the kernels' GELU texts (common.h: gelu_exact / gelu_bf16out2) and of wrong variants of them
GELU_A8 = (3.208326405e-07, -6.917509381e-06, 6.041429151e-05, -2.428356966e-04, -5.105399032e-05, 6.989960559e-03,
           -5.246259645e-02, -4.592153430e-01, -1.151104689e+00)
GELU_A5 = (2.554670494e-05, -6.529359078e-04, 7.452824686e-03, -5.192063601e-02, -4.602978599e-01, -1.150685204e+00)


def gelu_emulated(x, coeffs=GELU_A8, tmax=GELU_TMAX):
    """max(x, 0) - 0.5 * t * exp2(t * P(t)), t = min(|x|, tmax), every operation rounded to fp32"""
    f = np.float32
    xn = x.numpy().astype(np.float32)
    t = np.minimum(np.abs(xn), f(tmax))
    q = np.full_like(t, f(coeffs[0]))
    for c in coeffs[1:]:
        q = (q.astype(np.float64) * t + np.float64(f(c))).astype(np.float32)              # one fused multiply-add
    w = (t * np.exp2((q * t).astype(np.float32)).astype(np.float32)).astype(np.float32)
    out = (w.astype(np.float64) * -0.5 + np.maximum(xn, f(0))).astype(np.float32)
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------------------------- B. bf16 rounding
def rne_expected(addend):
    """bf16 bits of (+0 accumulator) + addend rounded to nearest even, as int16 (0 + -0 is +0 in IEEE arithmetic)"""
    return (torch.zeros_like(addend) + addend).bfloat16().view(torch.int16)


def rne_patterns(n, seed=0):
    """n fp32 values for the bf16 store test: every exact tie of a sample of bf16 neighbours over all normal exponents in
    both signs with its two fp32 neighbours, values within a bf16 ulp of the largest finite bf16 (RNE overflows to inf
    above the tie), +-0, subnormals (at most 0.1 % of n) and random finite normal bit patterns in the rest."""
    exps = torch.arange(1, 255, dtype=torch.int64)
    mant = torch.tensor([0x00, 0x01, 0x02, 0x03, 0x2A, 0x55, 0x7E, 0x7F], dtype=torch.int64)
    hi = ((exps[:, None] << 7) | mant[None, :]).reshape(-1)                     # upper halves: even and odd last bits
    low = torch.tensor([0x7FFF, 0x8000, 0x8001], dtype=torch.int64)
    ties = ((hi[:, None] << 16) | low[None, :]).reshape(-1)
    top = torch.tensor([0x7F7F0000, 0x7F7F0001, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0x7F7EFFFF, 0x7F7E8000],
                       dtype=torch.int64)
    zero = torch.tensor([0], dtype=torch.int64)
    nsub = min(64, n // 2000)                                                  # per sign
    g = torch.Generator().manual_seed(seed)
    sub = torch.randint(1, 1 << 23, (nsub,), generator=g, dtype=torch.int64)
    if nsub >= 4:
        sub[:4] = torch.tensor([1, 0x7FFFFF, 0x8000, 0x18000])
    pos = torch.cat([ties, top, zero, sub])
    fixed = torch.cat([pos, pos | 0x80000000])
    if n < fixed.numel():
        raise ValueError(f"{n} values do not hold the {fixed.numel()} fixed patterns")
    rnd = torch.randint(0, 1 << 32, (n - fixed.numel(),), generator=g, dtype=torch.int64)
    e = (rnd >> 23) & 0xFF
    rnd = torch.where((e == 0) | (e == 255), (rnd & ~(0xFF << 23)) | (127 << 23), rnd)       # finite and normal
    bits = torch.cat([fixed, rnd])
    bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    vals = bits.view(torch.float32)
    assert bool(torch.isfinite(vals).all())
    return vals[torch.randperm(n, generator=g)].contiguous()


def rne_check(out_bits, addend):
    """(ok per element, excused, cap): bit equality with torch's RNE at |addend| >= 2^-126; below it the RNE value or a
    zero of the same sign.  ``excused`` counts the elements that used the second form, ``cap`` the subnormals fed."""
    want = rne_expected(addend)
    same = out_bits == want
    sub = (addend != 0) & (addend.abs() < FLUSH)
    zero_same_sign = (out_bits & 0x7FFF) == 0
    zero_same_sign &= (out_bits < 0) == (addend.view(torch.int32) < 0)
    ok = same | (sub & zero_same_sign)
    return ok, int((sub & ~same).sum()), int(sub.sum())


def bf16_truncate(x):
    """wrong store: the upper 16 bits of the fp32 pattern"""
    return (x.view(torch.int32) >> 16).to(torch.int16)


def bf16_ties_away(x):
    """wrong store: nearest, ties away from zero (add half an ulp to the magnitude, truncate)"""
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b & 0x7FFFFFFF) + 0x8000) >> 16 | ((b >> 31) << 15)
    return torch.where(r >= (1 << 15), r - (1 << 16), r).to(torch.int16)


# ----------------------------------------------------------------------------------------------- C. mixed scales
def pow2_scales(n, g, pin=True):
    """2^round(U(-10, 10)) per channel; ``pin``: channel 0 carries 2^10 and the last two 2^-10, so that every case has the
    whole range whatever its seed."""
    s = torch.exp2(torch.round(torch.rand(n, generator=g) * 20.0 - 10.0))
    if pin and n >= 4:
        s[0], s[-1], s[-2] = 2.0 ** 10, 2.0 ** -10, 2.0 ** -10
    return s


def gamma(K, split=False):
    """Constant of the componentwise forward bound of a K-term fp32 dot product plus bias and residual adds, (K + 3) u.
    Split path: its three dropped cross terms are each at most 2^-16 * 2^-8 of a product, 3 * 2^-24 per product -> K + 12
    covers them beside the summation error."""
    return (K + (12 if split else 3)) * U24


def forward_bound(mag, K, ref64=None, split=False, out_bf16=False):
    """|out - ref| <= gamma * mag, mag = |A||W|^T + |b| (+ |R|) in fp64; half a bf16 ulp of the reference on a bf16 output"""
    b = gamma(K, split) * mag
    if out_bf16:
        b = b + BF16_HALF_ULP * ref64.abs()
    return b


def gelu_forward_bound(x64, mag, K, out_bf16=False, pre_bf16=False):
    """bound of gelu(A W^T + b) at fp64 pre-activation x64: the pre-activation's own bound (and, on the kernel that rounds it
    to bf16 first, half a bf16 ulp of it) through the GELU's slope (<= 1.13), plus the GELU gate of family A"""
    dx = gamma(K) * mag + (BF16_HALF_ULP * x64.abs() if pre_bf16 else 0.0)
    ref = F.gelu(x64)
    b = GELU_SLOPE * dx + gelu_gate_f32(x64)
    return b + BF16_HALF_ULP * ref.abs() if out_bf16 else b


def conv_ref64(x, w, b, k, s, p):
    """NHWC convolution in fp64 as k*k matrix products: x (F, H, W, Cin), w (Cout, k, k, Cin), b (Cout) or None ->
    (F, Ho, Wo, Cout).  With |x|, |w|, |b| it gives the magnitude sum of the forward bound."""
    x, w = x.double(), w.double()
    Fr, H, Wd, Cin = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (Wd + 2 * p - k) // s + 1
    xp = torch.zeros(Fr, H + 2 * p, Wd + 2 * p, Cin, dtype=torch.float64, device=x.device)
    xp[:, p:p + H, p:p + Wd] = x
    out = torch.zeros(Fr, Ho, Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for i in range(k):
        for j in range(k):
            out += xp[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] @ w[:, i, j].t()
    return out if b is None else out + b.double()


def stats_gate(s1, s2, y):
    """InstanceNorm partial sums per (frame, channel) against the map y (F, H, W, C) in fp64:
    |s1 - sum y| <= 1e-5 * sum |y| and |s2 - sum y^2| <= 1e-5 * sum y^2.  Returns the two err / bound maxima."""
    y = y.double()
    r1 = (s1 - y.sum(dim=(1, 2))).abs() / (1e-5 * y.abs().sum(dim=(1, 2)))
    r2 = (s2 - (y * y).sum(dim=(1, 2))).abs() / (1e-5 * (y * y).sum(dim=(1, 2)))
    return float(r1.max()), float(r2.max())


def rel_err_global(a, b):
    """the suite's older yardstick (tests/test_kernels_gpu.py: _rel_err): one norm for the whole tensor"""
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def gemm_case(M, N, K, epi, seed, bf16_operands=False):
    """Operands of tests/test_kernels_gpu.py's GEMM tests (unit-normal A, W / sqrt(K), bias, residual) and their scales:
    dict with A, W, b, R (or None), sa (M), sw (N)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if epi == 2 else None
    if bf16_operands:
        A, W = A.bfloat16().float(), W.bfloat16().float()
    return dict(A=A, W=W, b=b, R=R, sa=pow2_scales(M, g), sw=pow2_scales(N, g))


def conv_case(Fr, H, Wd, Cin, Cout, k, seed, bf16_operands=False):
    """Operands of the convolution tests, NHWC / (Cout, k, k, Cin), and their scales: x, w, b, sx (Cin), sw (Cout)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Fr, H, Wd, Cin, generator=g)
    w = torch.randn(Cout, k, k, Cin, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    if bf16_operands:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    return dict(x=x, w=w, b=b, sx=pow2_scales(Cin, g), sw=pow2_scales(Cout, g))
