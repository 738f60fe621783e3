"""The nine convolution kernels under impulse, mixed-scale and low-variance probes (builders and gates:
tests/golden/conv_probes.py; the gates are proven on the CPU in tests/test_conv_probes.py).  Everything under test is called
through pips_amd.ops; torch on the device forms the operands and the fp64 references.

A. impulse response: every output is one weight times a power of two or zero -- equality; statistics within 4 n u.
B. mixed power-of-two scales: every element within (K + 3) u (conv(|x|, |w|) + |b|) (+ half a bf16 ulp on bf16 maps),
   output-channel scaling exact, statistics per (frame, channel).
C. bias >> std: mean and variance from the pivoted partials, and per part: pivot inside the part's range, n its pixel count.

Rows (conv_probes.ROWS).  Families A, B and C visit every row -- igemm_64, igemm_416, igemm_s2, igemm_1x1 (igemm_f32_kernel),
t4_cfg0, t4_cfg0_tiny, t4_cfg1, t4_cfg2, t4_linear (conv3x3_f32_t4), x3_small, x3_128row, x3_256row (split bf16 x 3),
bf16_igemm, maps_igemm, maps_s2, maps_1x1_f32out (gemm_bf16_kernel<CONV>), c64_lds, c64_pp (conv_bf16_c64.hip), c96_t4c
(conv_bf16_t4c.hip + its statistics kernel) -- except c64_pp_norm, the ping-pong kernel with in_norm, which has its own two
exact-staging cases (a) and (b) of family A; (b) is judged by family B's bound.

A route is recognised from the number of statistics partials per frame the call reports, against the kernel that
conv_probes.predict names for this device's compute units; where that is not the kernel the row is meant for (another
device size), the numbers are still checked and only the route assertion is left out.  Every test prints its route."""
import pytest
import torch

import conv_probes as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = [r.id for r in P.ROWS if not r.norm]


def _cus():
    from pips_amd import _lib
    return _lib.load().pips_device_cus()


def _run(r, x, w, b, nrm=None):
    from pips_amd import ops
    if r.entry == "f32":
        return ops.conv_nhwc(x, w, b, r.k, r.s, r.p, want_stats=True)
    if r.entry == "x3":
        return ops.conv_nhwc_x3(x, ops.split_bf16x3(w), b, r.k, r.s, r.p, want_stats=True)
    if r.entry == "bf16":
        return ops.conv_nhwc_bf16(x, w.bfloat16(), b, r.k, r.s, r.p, want_stats=True)
    return ops.conv_nhwc_bf16_maps(x.bfloat16(), w.bfloat16(), b, r.k, r.s, r.p, in_norm=nrm, out_bf16=r.out_bf16, want_stats=True)


def _route(tag, r, stats):
    """the kernel that took the call: the partition conv_probes.predict names for this device must be the one reported"""
    route = P.predict(r, _cus())
    assert stats.shape[1] == route.parts, f"{tag}: {stats.shape[1]} partials per frame, {route.name} writes {route.parts}"
    if route.name == r.route:
        print(f"{tag}: route {route.name}, {route.parts} partials per frame")
    else:
        print(f"{tag}: route {route.name} on {_cus()} compute units (the row is meant for {r.route}): route assertion left out")
    Ho, Wo = P.out_hw(r)
    return route, int(P.part_sizes(route, Ho, Wo).max())


def _sums(stats):
    from pips_amd import ops
    return ops.partial_sums(stats)


def _check_exact(tag, r, out, stats, exp):
    route, n = _route(tag, r, stats)
    same = out.float() == exp
    assert bool(same.all()), (f"{tag}: {int((~same).sum())} of {same.numel()} outputs differ from the selected weight, "
                              f"max |diff| {float((out.float() - exp).abs().max()):.3g}, first at {[int(t[0]) for t in (~same).nonzero(as_tuple=True)]}")
    s1, s2 = _sums(stats)
    b1, b2 = P.exact_stats_bound(exp, n)
    e = exp.double()
    assert bool(((s1 - e.sum(dim=(1, 2))).abs() <= b1).all()) and bool(((s2 - (e * e).sum(dim=(1, 2))).abs() <= b2).all()), tag
    return route


# ============================================================================================ A. impulse response
@pytest.mark.parametrize("rid", ALL)
def test_impulse_response(rid):
    """zero bias (a tensor: the assembly routes need one), impulses 2^e on the lattice, one phase per frame: out == expected
    on every route, the split route included (with x = 2^e only the leading plane of x is non-zero, and every partial sum of
    the three bf16 planes of a weight is an fp32 number)"""
    r = P.ROW[rid]
    w = P.impulse_weights(r, DEV)
    b = torch.zeros(r.Cout, device=DEV)
    for call in range(P.impulse_calls(r)):
        x = P.impulse_map(r, call, DEV)
        exp = P.impulse_expected(r, call, w, DEV)
        out, stats = _run(r, x, w, b)
        _check_exact(f"impulse {rid} call {call}", r, out, stats, exp)


@pytest.mark.parametrize("case", ["a", "b"])
def test_impulse_normalise_on_load(case):
    """The ping-pong 64 -> 64 kernel with in_norm, staged exactly (rstd a power of two, mean in quarters).
    (a) background = mean (stages to 0), impulses mean + 2^e / rstd, a third of the sites mean - 2^e / rstd (ReLU deletes
        them): out == expected.
    (b) background = mean + 1 / rstd (stages to 1 inside the image): against the fp64 convolution of a map of ones with
        zero padding, element by element -- taps outside the image stay 0 and are not normalised."""
    r = P.ROW["c64_pp_norm"]
    w = P.impulse_weights(r, DEV)
    nrm = P.norm_params(r, DEV)
    if case == "a":
        x = P.impulse_map_prenorm(r, 0, nrm, DEV)
        exp = P.impulse_expected(r, 0, w, DEV, drop_neg=True)
        out, stats = _run(r, x, w, torch.zeros(r.Cout, device=DEV), nrm)
        _check_exact("impulse c64_pp_norm (a)", r, out, stats, exp)
        return
    b = torch.randn(r.Cout, generator=torch.Generator().manual_seed(3)).to(DEV)
    out, stats = _run(r, P.ones_map_prenorm(r, nrm), w, b, nrm)
    _route("ones c64_pp_norm (b)", r, stats)
    ref, mag = P.ref_and_mag(r, torch.ones(r.F, r.H, r.W, r.Cin, device=DEV), w, b)
    err, bound = (out.double() - ref).abs(), P.element_bound(r, ref, mag)
    print(f"ones c64_pp_norm (b): max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ============================================================================================ B. mixed scales
@pytest.mark.parametrize("rid", ALL)
def test_mixed_scales(rid):
    r = P.ROW[rid]
    c = P.mixed_case(r, DEV)
    x, w, b, sw = c["x"], c["w"], c["b"], c["sw"]
    ws, bs = w * sw[:, None, None, None], b * sw
    out_s, st = _run(r, x, ws, bs)
    tag = f"mixed scales {rid}"
    route, n = _route(tag, r, st)
    out_u, _ = _run(r, x, w, b)
    assert torch.equal(out_s.double(), out_u.double() * sw.double()), f"{tag}: scaling W and bias by powers of two changed the digits"
    ref, mag = P.ref_and_mag(r, x, ws, bs)
    err, bound = (out_s.double() - ref).abs(), P.element_bound(r, ref, mag)
    s1, s2 = _sums(st)
    if route.name == "c96_t4c":
        o = out_s.double()
        b1, b2 = P.stats_bounds_stored(out_s, n)
        e1, e2 = (s1 - o.sum(dim=(1, 2))).abs(), (s2 - (o * o).sum(dim=(1, 2))).abs()
    else:
        b1, b2 = P.stats_bounds_accum(r, ref, mag, n)
        e1, e2 = (s1 - ref.sum(dim=(1, 2))).abs(), (s2 - (ref * ref).sum(dim=(1, 2))).abs()
    print(f"{tag}: max err / bound {float((err / bound).max()):.3f}; statistics per (frame, channel) "
          f"{float((e1 / b1).max()):.3f} (sum), {float((e2 / b2).max()):.3f} (sum of squares)")
    assert bool((err <= bound).all())
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())


# ============================================================================================ C. |mean| >> std
@pytest.mark.parametrize("rid", ALL)
def test_low_variance_statistics(rid):
    """one bias for every channel, far above the map's std (64 and 1/16 on fp32 maps: ratio 2^10; 4 and 1/4 on bf16 maps:
    ratio 2^4).  Mean and variance per (frame, channel) from the partials, and every part's pivot and n."""
    r = P.ROW[rid]
    c = P.lowvar_case(r, DEV)
    out, st = _run(r, c["x"], c["w"], c["b"])
    tag = f"low variance {rid} (bias / std {c['ratio']:g})"
    route, n = _route(tag, r, st)
    Ho, Wo = P.out_hw(r)
    s1, s2 = _sums(st)
    mean, var = P.mean_var_from_sums(s1, s2, Ho * Wo)
    if P.stats_of_stored(r, route):
        m = out.double()
        mean64, var64 = m.mean(dim=(1, 2)), m.var(dim=(1, 2), unbiased=False)
        gate_v, gate_m = P.variance_gate_stored(n) * var64, P.U24 * mean64.abs()
        bad = P.check_partials(st, route, Ho, Wo, m)
    else:
        ref, mag = P.ref_and_mag(r, c["x"], c["w"], c["b"])
        el = (r.k * r.k * r.Cin + 3) * P.U24 * mag
        delta = el.amax(dim=(1, 2))
        mean64, var64 = ref.mean(dim=(1, 2)), ref.var(dim=(1, 2), unbiased=False)
        gate_v, gate_m = P.variance_gate_accum(delta, var64.sqrt(), n) * var64, delta + P.U24 * mean64.abs()
        bad = P.check_partials(st, route, Ho, Wo, ref, widen=el)
    ev, em = (var - var64).abs(), (mean - mean64).abs()
    print(f"{tag}: variance err / gate {float((ev / gate_v).max()):.3g}, mean err / gate {float((em / gate_m).max()):.3g}, "
          f"std {float(var64.sqrt().mean()):.4f}")
    assert bad == [], f"{tag}: {bad}"
    assert bool((ev <= gate_v).all()) and bool((em <= gate_m).all())


_ORACLE = {}


def _encoder_oracle(kind, weights_raw):
    """fp32 and fp64 oracle maps of frames 0 and 11 of the clip (InstanceNorm is per frame: a frame's map does not depend
    on the others), computed once per frame kind"""
    if kind not in _ORACLE:
        from oracle import pips_oracle as O
        rgbs = P.low_variance_frames(kind, 16, 184, 248)
        x = 2 * (rgbs[[0, 11]] / 255.0) - 1.0
        _ORACLE[kind] = (rgbs, O.encoder(weights_raw, x, 8), O.encoder(O.to_dtype(weights_raw, torch.float64), x.double(), 8))
    return _ORACLE[kind]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", ["low_contrast", "letterbox", "flat_with_dot"])
def test_encoder_low_variance_frames_assembly_route(kind, split, weights_raw, arenas):
    """test_kernels_gpu.py::test_encoder_low_variance_frames at 16 x 184 x 248, where layer 1 is 45 tiles x 16 frames -- the
    fp32 assembly convolutions on 256 compute units -- and in the split mode.  Same yardstick: HIP against the fp64 oracle
    within 4x the fp32 oracle's own error against fp64, plus 1e-5."""
    from pips_amd import ops
    rgbs, ref32, ref64 = _encoder_oracle(kind, weights_raw)
    pyr = ops.encoder_fwd(arenas["raw"], rgbs.to(DEV), 8, split=split)
    got = ops.pyramid_levels(pyr, 16, 184, 248, 8)[0][[0, 11]].cpu().permute(0, 3, 1, 2)
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    print(f"{kind} split={split}: HIP vs fp64 {err:.2e}, fp32 reference arithmetic vs fp64 {floor:.2e}, |map| {float(ref64.abs().max()):.1f}")
    assert err < 4 * floor + 1e-5


# ============================================================================================ assembly route == igemm, bitwise
@pytest.mark.parametrize("H,W,Cin,Cout", [(93, 125, 64, 64), (93, 125, 96, 96), (45, 63, 416, 256)])
def test_assembly_route_is_bitwise_igemm(H, W, Cin, Cout):
    """conv_f32_t4.hip's header: the assembly route's map is bitwise igemm_f32_kernel's.  One frame alone takes igemm (too few
    tiles); the same content as frame 3 of a 16-frame and of a 19-frame call takes the assembly route in both block orders.
    The statistics partitions differ by design: their combined sums agree within n u."""
    g = torch.Generator().manual_seed(H + Cin)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    x19 = torch.randn(19, H, W, Cin, generator=g).to(DEV)
    one = P._r("one", "f32", "igemm_f32", 1, H, W, Cin, Cout)
    out1, st1 = _run(one, x19[3:4].contiguous(), w, b)
    r1, n1 = _route("bitwise: one frame", one, st1)
    a1, a2 = _sums(st1)
    o = out1.double()
    for frames in (16, 19):
        many = P._r("many", "f32", f"f32_t4_cfg{(64, 96, 416).index(Cin)}", frames, H, W, Cin, Cout)
        out, st = _run(many, x19[:frames].contiguous(), w, b)
        rm, nm = _route(f"bitwise: frame 3 of {frames}", many, st)
        if r1.name == "igemm_f32" and rm.name == many.route:
            pass
        else:
            print("bitwise: the two calls do not take the two kernels on this device; the comparison still holds")
        assert torch.equal(out[3:4], out1)
        s1, s2 = _sums(st[3:4])
        n = max(n1, nm)
        assert bool(((s1 - a1).abs() <= n * P.U24 * o.abs().sum(dim=(1, 2))).all())
        assert bool(((s2 - a2).abs() <= n * P.U24 * (o * o).sum(dim=(1, 2))).all())
