"""The gates of tests/test_value_range_gpu.py are meaningful: on the same inputs torch's own fp32 arithmetic passes every
one of them, and host-emulated wrong kernels fail them -- most of them while passing the yardsticks the suite applied
before (one global norm at 2e-6, half a bf16 ulp).  Builders and gates: tests/golden/value_range.py.  No GPU."""
import math

import torch
import torch.nn.functional as F

import value_range as V


# ------------------------------------------------------------------------------------------------ A. the GELU
def test_onehot_construction_is_exact():
    """A[m, m % K] = 1 selects W[n, m % K]: exactly in fp32, in bf16 (the sweep is bf16-representable) and on the split
    path (the three bf16 planes of a sweep value sum back to it)."""
    M, N, K = 1093, 130, 512
    A, W = V.onehot_operands(M, N, K, V.gelu_sweep_f32(N * K))
    assert V.bitwise_equal(A @ W.t(), V.selected(W, M))
    Ab, Wb = V.onehot_operands(M, 132, K, V.gelu_sweep_bf16(132 * K))
    assert torch.equal(Wb.bfloat16().float(), Wb) and torch.equal(Ab.bfloat16().float(), Ab)
    assert V.bitwise_equal(Ab @ Wb.t(), V.selected(Wb, M))
    x = W.reshape(-1)
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    normal = x.abs() >= 2.0 ** -100          # below, the remainders are subnormal (tests/test_kernels_gpu.py: test_split_bf16x3_is_exact)
    assert torch.equal((h.double() + m.double() + l.double()).float()[normal], x[normal])
    # the sweep holds what the issue lists
    assert V.bf16_values().numel() == 34050
    s = V.gelu_specials()
    for v in (0.0, 1e-30, 1e-40, 20.0, 1e4, V.GELU_TMAX):
        assert bool((s == torch.tensor(v, dtype=torch.float64).float()).any()) and bool((s == -torch.tensor(v, dtype=torch.float64).float()).any())
    assert float(x.abs().max()) <= 1e4 and int(V.bucket_index(x).unique().numel()) == 7


def test_gelu_gate_holds_for_the_reference_and_the_intended_arithmetic():
    e = V.gelu_eref()
    print("E_ref per bucket: " + ", ".join(f"{V.BUCKET_NAMES[i]} {e[i]:.2e}" for i in range(7)))
    assert all(e[i] < 2e-6 for i in range(7)) and e[0] < 1e-7 and e[3] < 1e-7
    x = V.gelu_sweep_f32(2048 * 512)
    ref = V.gelu_ref64(x)
    gate = V.gelu_gate_f32(x)
    assert bool(((F.gelu(x).double() - ref).abs() <= gate).all())
    # the kernels' formula in emulated fp32: 2.5e-7 overall, 4.4e-8 beyond the clamp
    err = (V.gelu_emulated(x).double() - ref).abs()
    worst = V.bucket_maxima(err, x)
    print("emulated gelu_exact: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()), f"; max err / gate {float((err / gate).max()):.2f}")
    assert float(err.max()) <= 2.5e-7 and worst[V.BUCKET_NAMES[0]] <= 4.4e-8 and worst[V.BUCKET_NAMES[6]] <= 4.4e-8
    assert bool((err <= gate).all())
    # bf16 outputs: either polynomial, rounded once, passes the bf16 gate on the bf16 sweep
    xb = V.bf16_values()
    rb = V.gelu_ref64(xb)
    for out in (F.gelu(xb).bfloat16(), V.gelu_emulated(xb).bfloat16(), V.gelu_emulated(xb, V.GELU_A5).bfloat16()):
        assert bool(((out.double() - rb).abs() <= V.gelu_gate_bf16(xb, rb)).all())


def _old_gelu_gate(fn):
    """what the suite saw of a GELU before: a GEMM whose pre-activations are about N(0, 2), one global norm at 2e-6"""
    pre = torch.randn(1 << 20, generator=torch.Generator().manual_seed(0)) * math.sqrt(2.0)
    return V.rel_err_global(fn(pre).double(), V.gelu_ref64(pre)) < 2e-6


def test_wrong_gelus_fail_the_new_gate_and_pass_the_old():
    x = V.gelu_sweep_f32(2048 * 512)
    ref, gate = V.gelu_ref64(x), V.gelu_gate_f32(x)
    c = list(V.GELU_A8)
    c[6] = -5.247259645e-02                   # -5.246259645e-02: one unit in the fourth digit
    mutants = {
        "clamp at 5.0": lambda t: V.gelu_emulated(t, tmax=5.0),
        "degree-5 polynomial on an fp32 output": lambda t: V.gelu_emulated(t, V.GELU_A5),
        "one coefficient off in its fourth digit": lambda t: V.gelu_emulated(t, tuple(c)),
    }
    for name, fn in mutants.items():
        err = (fn(x).double() - ref).abs()
        ratio = float((err / gate).max())
        print(f"{name}: max err / gate {ratio:.2f}, old gate passes: {_old_gelu_gate(fn)}")
        assert ratio > 1.0, name
        assert _old_gelu_gate(fn), name


def test_rounding_safe_subset():
    """The bit-exact form of the bf16 GELU check holds where bf16(ref - d) == bf16(ref + d), d the fp32 gate.  d is an
    ABSOLUTE bound of 1.3e-7 .. 2.5e-6; 88 % of the bf16 values lie below 2^-9, where it exceeds a bf16 ulp of the result, so
    over the whole sweep the subset is 12.6 %.  Over the values a GEMM produces in bulk, 1/16 <= x <= 64, it is above 95 %."""
    xb = V.bf16_values()
    rb = V.gelu_ref64(xb)
    safe = V.rounding_safe(xb, rb)
    bulk = (xb >= 2.0 ** -4)
    print(f"rounding-safe: {float(safe.float().mean()):.3f} of the sweep, {float(safe[bulk].float().mean()):.3f} of 1/16 <= x <= 64 "
          f"({int(bulk.sum())} values), {float(safe[xb.abs() >= 2.0 ** -4].float().mean()):.3f} of |x| >= 1/16")
    assert float(safe[bulk].float().mean()) >= 0.95
    assert int(safe.sum()) >= 4000
    # on the subset the intended arithmetic IS the rounding of the reference
    want = rb.float().bfloat16().view(torch.int16)
    for coeffs in (V.GELU_A8, V.GELU_A5):
        got = V.gelu_emulated(xb, coeffs).bfloat16().view(torch.int16)
        assert bool((got == want)[safe & (xb.abs() >= 2.0 ** -4)].all())


# ------------------------------------------------------------------------------------------------ B. bf16 stores
def test_rne_patterns_and_wrong_roundings():
    for n in (16384, 1024 * 512):
        p = V.rne_patterns(n, seed=n)
        assert p.numel() == n and bool(torch.isfinite(p).all())
        sub = (p != 0) & (p.abs() < V.FLUSH)
        assert 0 < int(sub.sum()) <= n // 1000
        bits = p.view(torch.int32)
        assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any())                  # +0 and -0
        assert int(((bits & 0xFFFF) == 0x8000).sum()) >= 2 * 254 * 8                          # exact ties, both signs
        assert bool(torch.isinf(p.bfloat16().float()).any())                                 # above the largest bf16: RNE gives inf
        ref = (torch.zeros_like(p) + p).bfloat16().view(torch.int16)                          # torch's own conversion
        ok, excused, cap = V.rne_check(ref, p)
        assert bool(ok.all()) and excused == 0 and cap == int(sub.sum())
        flushed = torch.where(sub, torch.zeros_like(p) * p, torch.zeros_like(p) + p).bfloat16().view(torch.int16)   # subnormals -> zero of their sign
        ok, excused, cap = V.rne_check(flushed, p)
        assert bool(ok.all()) and excused <= cap
        # the gate the suite applied to bf16 stores: half a bf16 ulp of the reference (+ 2e-5)
        finite = torch.isfinite(p.bfloat16().float()) & (p.abs() < 3e38)
        old = lambda b: bool((((b.to(torch.int32) << 16).view(torch.float32).double() - p.double()).abs()[finite]
                              <= (p.double().abs() * 2.0 ** -8 + 2e-5)[finite]).all())
        trunc, away = V.bf16_truncate(p), V.bf16_ties_away(p)
        assert not bool(V.rne_check(trunc, p)[0].all()) and not bool(V.rne_check(away, p)[0].all())
        assert old(ref) and old(away)          # a wrong tie is invisible to the old gate
        print(f"n = {n}: truncation differs at {int((trunc != ref).sum())}, ties-away at {int((away != ref).sum())}; "
              f"old gate passes truncation: {old(trunc)}")


# ------------------------------------------------------------------------------------------------ C. mixed scales
def _gemm_ref(c, bf16_operands=False):
    A = c["A"] * c["sa"][:, None]
    Ws, bs = c["W"] * c["sw"][:, None], c["b"] * c["sw"]
    Rs = None if c["R"] is None else c["R"] * c["sa"][:, None] * c["sw"]
    ref = A.double() @ Ws.double().t() + bs.double()
    mag = A.double().abs() @ Ws.double().abs().t() + bs.double().abs()
    if Rs is not None:
        ref, mag = ref + Rs.double(), mag + Rs.double().abs()
    return A, Ws, bs, Rs, ref, mag


def test_torch_fp32_passes_the_mixed_scale_gates():
    for (M, N, K, epi) in ((77, 130, 64, 0), (256, 1040, 512, 0), (200, 132, 96, 2), (128, 256, 2048, 2)):
        for bf16_operands in (False, True):
            c = V.gemm_case(M, N, K, epi, seed=M * 7 + N, bf16_operands=bf16_operands)
            A, Ws, bs, Rs, ref, mag = _gemm_ref(c)
            out = A @ Ws.t() + bs + (0 if Rs is None else Rs)
            err = (out.double() - ref).abs()
            assert bool((err <= V.forward_bound(mag, K, ref)).all()), (M, N, K)
            unscaled = A @ c["W"].t() + c["b"] + (0 if Rs is None else c["R"] * c["sa"][:, None])
            assert float(((unscaled * c["sw"]).double() - ref).abs().max() / ref.abs().max()) < 1e-5      # the same problem
            ob = out.bfloat16()
            assert bool(((ob.double() - ref).abs() <= V.forward_bound(mag, K, ref, out_bf16=True)).all())
    # GELU epilogue
    c = V.gemm_case(256, 512, 512, 1, seed=11)
    A, Ws, bs, _, pre, mag = _gemm_ref(c)
    out = F.gelu(A @ Ws.t() + bs)
    assert bool(((out.double() - F.gelu(pre)).abs() <= V.gelu_forward_bound(pre, mag, 512)).all())
    # convolutions and their InstanceNorm sums
    for (Fr, H, W, Cin, Cout, k, s, p) in ((2, 23, 31, 64, 96, 3, 2, 1), (1, 16, 20, 96, 128, 1, 2, 0), (2, 20, 13, 64, 64, 3, 1, 1)):
        c = V.conv_case(Fr, H, W, Cin, Cout, k, seed=Cin + Cout + k)
        x, ws, bs = c["x"] * c["sx"], c["w"] * c["sw"][:, None, None, None], c["b"] * c["sw"]
        ref = V.conv_ref64(x, ws, bs, k, s, p)
        mag = V.conv_ref64(x.abs(), ws.abs(), bs.abs(), k, s, p)
        torch64 = F.conv2d(x.double().permute(0, 3, 1, 2), ws.double().permute(0, 3, 1, 2), bs.double(), stride=s, padding=p)
        assert float((torch64.permute(0, 2, 3, 1) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())    # conv_ref64 is conv2d
        out = F.conv2d(x.permute(0, 3, 1, 2), ws.permute(0, 3, 1, 2), bs, stride=s, padding=p).permute(0, 2, 3, 1)
        assert bool(((out.double() - ref).abs() <= V.forward_bound(mag, k * k * Cin, ref)).all())
        r1, r2 = V.stats_gate(out.sum(dim=(1, 2)).double(), (out * out).sum(dim=(1, 2)).double(), ref)
        assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


def test_misplaced_bias_and_statistics_fail_only_the_elementwise_gates():
    M, N, K = 256, 1040, 512
    c = V.gemm_case(M, N, K, 0, seed=M * 7 + N)
    A, Ws, bs, _, ref, mag = _gemm_ref(c)
    small = c["sw"] <= 2.0 ** -8
    small[0] = False
    assert int(small.sum()) >= 8
    shifted = torch.where(small, torch.roll(c["b"], 1) * c["sw"], bs)          # the neighbour's bias in the small columns
    out = A @ Ws.t() + shifted
    err = (out.double() - ref).abs()
    assert V.rel_err_global(out.double(), ref) < 2e-6                           # invisible under one global norm
    bad = ~(err <= V.forward_bound(mag, K, ref))
    assert bool(bad.any()) and not bool(bad[:, ~small].any())
    # a channel's sum taken from its neighbour, in the two smallest channels
    Fr, H, W, Cin, Cout, k = 2, 20, 13, 64, 64, 3
    c = V.conv_case(Fr, H, W, Cin, Cout, k, seed=5)
    x, ws, bs = c["x"] * c["sx"], c["w"] * c["sw"][:, None, None, None], c["b"] * c["sw"]
    ref = V.conv_ref64(x, ws, bs, k, 1, 1)
    s1, s2 = ref.sum(dim=(1, 2)), (ref * ref).sum(dim=(1, 2))
    assert max(V.stats_gate(s1, s2, ref)) == 0.0
    wrong = s1.clone()
    wrong[:, -1] = s1[:, -2]                                                      # both scaled by 2^-10, the largest by 2^10
    assert V.rel_err_global(wrong, s1) < 1e-5
    assert V.stats_gate(wrong, s2, ref)[0] > 1.0
