"""Value range of the matrix kernels and their epilogues, route by route (builders and gates: tests/golden/value_range.py;
the same gates are proven meaningful on the CPU in tests/test_value_range.py).

A. the GELU of every route as a function, against F.gelu in fp64 at exactly known pre-activations;
B. bf16 stores against torch's round-to-nearest-even, bit for bit;
C. operands with mixed power-of-two scales, judged element by element against the componentwise forward bound.

Every case asserts the route it is meant for before it looks at a number; shapes are the smallest of a short list that
take the route on the device at hand.

Measured on an MI355X (256 compute units), err / bound maxima -- see DESIGN.md section 2 for the table."""
import pytest
import torch

import value_range as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GELU, RES = 1, 2


def _lib():
    from pips_amd import _lib
    return _lib.load()


def _first(shapes, takes):
    """the first (smallest) shape of the list that takes the wanted route on this device"""
    for s in shapes:
        if takes(*s):
            return s
    raise AssertionError(f"none of {shapes} takes the route on a device of {_lib().pips_device_cus()} compute units")


def _f32_shape(route, epi):
    """(M, N, K) for pips_gemm_f32 on the given route.  M >= 2 K: every slot of W is selected at least twice."""
    lib = _lib()
    if route == 1:      # 128 x 128 assembly tiles: from 3/4 tile per compute unit
        shapes = [(m, 2048, 512) for m in (1024, 1536, 2048, 3072, 4096)]
    elif route == 2:    # 64 x 64 assembly tiles, K split over the waves: 0.75 .. 2 tiles per compute unit
        shapes = [(m, 512, 256) for m in (512, 1024, 1536, 2048, 3072, 4096)]
    else:
        shapes = [(1024, 512, 512)]
    return _first(shapes, lambda M, N, K: lib.pips_gemm_f32_route(M, N, K, epi) == route)


# ============================================================================================ A. the GELU as a function
def _run_f32(path, A, W, epi, R=None):
    from pips_amd import ops
    bias = torch.zeros(W.shape[0], device=DEV)              # the assembly routes need a bias
    if path == "x3":
        return ops.gemm_x3(A, ops.split_bf16x3(W), bias, epi, R)
    return ops.gemm(A, W, bias, epi, R)


def _check_gelu(tag, out, pre, gate_fn, K):
    """out (M, N) against F.gelu in fp64 at the selected pre-activations, and rows of equal m % K against each other"""
    ref = V.gelu_ref64(pre)
    err = (out.double() - ref).abs()
    gate = gate_fn(pre, ref)
    worst = V.bucket_maxima(err, pre)
    ratio = float((err / gate).max())
    print(f"GELU {tag}: max err / gate {ratio:.3f}; per bucket " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert bool((err <= gate).all()), (tag, ratio, worst)
    M = out.shape[0]
    assert M > K
    bits = out.view(torch.int32) if out.dtype == torch.float32 else out.view(torch.int16)
    assert torch.equal(bits[K:], bits[: M - K]), f"{tag}: the GELU of a value depends on where in the tile it sits"


@pytest.mark.parametrize("path,route,ragged", [
    ("f32", 0, False),      # igemm_f32_kernel, full tiles: gelu_exact2
    ("f32", 0, True),       # ragged M and N: gelu_exact in the vector and the scalar edge path
    ("f32", 1, False),      # gemm_f32_t4u_kernel: asm_emit.gelu4, nine coefficients; 1 M points
    ("x3", 0, False),       # split path, full tiles
    ("x3", 0, True),        # split path, ragged: gemm_tail.h
])
def test_gelu_function_f32(path, route, ragged):
    lib = _lib()
    M, N, K = (1093, 130, 512) if ragged else _f32_shape(route, GELU)
    if path == "f32":
        assert lib.pips_gemm_f32_route(M, N, K, GELU) == route and lib.pips_gemm_f32_route(M, N, K, RES) == route
    A, W = V.onehot_operands(M, N, K, V.gelu_sweep_f32(N * K))
    A, W = A.to(DEV), W.to(DEV)
    Wx = W
    if path == "x3":
        # the three planes sum back to W exactly, except below 2^-110 where the remainders are subnormal and only the
        # leading plane is kept (tests/test_kernels_gpu.py: test_split_bf16x3_is_exact): what the planes hold is the operand
        from pips_amd import ops
        Wx = V.planes_to_f32(ops.split_bf16x3(W))
        big = W.abs() >= 2.0 ** -100
        assert torch.equal(Wx[big], W[big]) and float((Wx - W).abs().max()) < 2.0 ** -100 * 2.0 ** -8
    pre = V.selected(Wx, M)
    ident = _run_f32(path, A, W, RES, torch.zeros(M, N, device=DEV))
    print(f"identity {path} route {route} {M}x{N}x{K}: {int((ident.view(torch.int32) != pre.view(torch.int32)).sum())} of {M * N} not bitwise")
    assert V.bitwise_equal(ident, pre)
    out = _run_f32(path, A, W, GELU)
    _check_gelu(f"{path} route {route} {M}x{N}x{K}", out, pre, lambda x, r: V.gelu_gate_f32(x), K)


def test_identity_f32_route2():
    """gemm_f32_t4e_kernel has the residual epilogue only: the one-hot product with R = 0 returns W bit for bit"""
    M, N, K = _f32_shape(2, RES)
    A, W = V.onehot_operands(M, N, K, V.gelu_sweep_f32(N * K))
    A, W = A.to(DEV), W.to(DEV)
    out = _run_f32("f32", A, W, RES, torch.zeros(M, N, device=DEV))
    pre = V.selected(W, M)
    print(f"identity f32 route 2 {M}x{N}x{K}: {int((out.view(torch.int32) != pre.view(torch.int32)).sum())} of {M * N} not bitwise")
    assert V.bitwise_equal(out, pre)


def _bf16_shape(route, epi, out_bf16):
    lib = _lib()
    if route == 4:      # 256 x 256 tiles, K = 512: from 3/4 tile per compute unit
        shapes = [(m, 2048, 512) for m in (1024, 2048, 3072, 4096, 6144, 8192)]
    elif route == 3:    # 128 x 256 tiles: from half a tile per compute unit
        shapes = [(m, 512, 128) for m in (1024, 2048, 4096, 8192, 16384)]
    else:
        shapes = [(1024, 512, 512)]
    return _first(shapes, lambda M, N, K: lib.pips_gemm_bf16_route(M, N, K, epi, 1, out_bf16) == route)


@pytest.mark.parametrize("route,out_bf16,ragged", [
    (0, False, False),      # register-staged kernel, fp32 C: gelu_exact2
    (0, True, False),       # bf16 C: epilogue_full_tile<..., OUT_BF16>
    (0, True, True),        # ragged: gelu_exact + the edge path's bf16 store
    (4, True, False),       # gemm_bf16_t4_gelu_kernel: asm_emit.gelu4, six coefficients
])
def test_gelu_function_bf16(route, out_bf16, ragged):
    from pips_amd import ops
    lib = _lib()
    M, N, K = (1093, 132, 512) if ragged else _bf16_shape(route, GELU, int(out_bf16))
    assert lib.pips_gemm_bf16_route(M, N, K, GELU, 1, int(out_bf16)) == route
    A, W = V.onehot_operands(M, N, K, V.gelu_sweep_bf16(N * K))
    A, W = A.to(DEV).bfloat16(), W.to(DEV)
    pre = V.selected(W, M)
    bias = torch.zeros(N, device=DEV)
    if route == 0:          # the same kernel with the residual epilogue and R = 0 (route 4 is GELU only)
        assert lib.pips_gemm_bf16_route(M, N, K, RES, 1, 0) == 0
        ident = ops.gemm_bf16(A, W.bfloat16(), bias, epi=RES, R=torch.zeros(M, N, device=DEV), out_bf16=False)
        print(f"identity bf16 route 0 {M}x{N}x{K}: {int((ident.view(torch.int32) != pre.view(torch.int32)).sum())} of {M * N} not bitwise")
        assert V.bitwise_equal(ident, pre)
    out = ops.gemm_bf16(A, W.bfloat16(), bias, epi=GELU, out_bf16=out_bf16)
    gate = (lambda x, r: V.gelu_gate_bf16(x, r)) if out_bf16 else (lambda x, r: V.gelu_gate_f32(x))
    _check_gelu(f"bf16 route {route} out {'bf16' if out_bf16 else 'fp32'} {M}x{N}x{K}", out, pre, gate, K)
    if out_bf16:
        # where no admissible fp32 error can change the rounding, the stored bf16 is THE rounding of the reference
        ref = V.gelu_ref64(pre)
        safe = V.rounding_safe(pre, ref)
        want = ref.float().bfloat16().view(torch.int16)
        bad = int(((out.view(torch.int16) != want) & safe).sum())
        print(f"bf16 route {route}: {int(safe.sum())} of {safe.numel()} outputs rounding-safe, {bad} of them not the RNE value")
        assert bad == 0


@pytest.mark.parametrize("res_bf16", [False, True])
def test_identity_bf16_route3(res_bf16):
    """gemm_bf16_t4_res_kernel in both of its forms (fp32 R and C; EPI_RES_BF16: bf16 R and C): residual only, so the one-hot
    product with R = 0 returns the bf16 sweep bit for bit -- the only identity test this kernel gets."""
    from pips_amd import ops
    lib = _lib()
    epi = RES | (ops.EPI_RES_BF16 if res_bf16 else 0)
    M, N, K = _bf16_shape(3, epi, int(res_bf16))
    assert lib.pips_gemm_bf16_route(M, N, K, epi, 1, int(res_bf16)) == 3
    A, W = V.onehot_operands(M, N, K, V.gelu_sweep_bf16(N * K))
    A, W = A.to(DEV).bfloat16(), W.to(DEV)
    R = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16 if res_bf16 else torch.float32)
    out = ops.gemm_bf16(A, W.bfloat16(), torch.zeros(N, device=DEV), epi=RES, R=R, out_bf16=res_bf16)
    pre = V.selected(W, M)
    print(f"identity bf16 route 3 ({'bf16' if res_bf16 else 'fp32'} R/C) {M}x{N}x{K}: "
          f"{int((out.float().view(torch.int32) != pre.view(torch.int32)).sum())} of {M * N} not bitwise")
    assert V.bitwise_equal(out.float(), pre)


# ============================================================================================ B. bf16 stores round to nearest even
@pytest.mark.parametrize("M,N,K", [(1024, 512, 128), (1093, 132, 128)])       # full tiles; ragged tiles
def test_bf16_store_rne_register_staged(M, N, K):
    """W = 0 and bias = 0: the accumulator is +0 and the stored bf16 is the rounding of the fp32 residual alone"""
    from pips_amd import ops
    assert _lib().pips_gemm_bf16_route(M, N, K, RES, 1, 1) == 0
    R = V.rne_patterns(M * N, seed=M).reshape(M, N).to(DEV)
    A = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).to(DEV).bfloat16()
    W = torch.zeros(N, K, device=DEV, dtype=torch.bfloat16)
    out = ops.gemm_bf16(A, W, torch.zeros(N, device=DEV), epi=RES, R=R, out_bf16=True)
    ok, excused, cap = V.rne_check(out.view(torch.int16), R)
    print(f"bf16 store {M}x{N}: {int((~ok).sum())} of {M * N} not RNE; {excused} subnormals flushed (of {cap} fed)")
    assert cap <= M * N // 1000 and excused <= cap
    assert bool(ok.all())


def test_bf16_store_rne_route3_bf16_stream():
    """EPI_RES_BF16 on gemm_bf16_t4_res_kernel<true>: R is bf16, so the fp32 patterns ride in the bias (W = 0, R = 0)"""
    from pips_amd import ops
    lib = _lib()
    epi = RES | ops.EPI_RES_BF16
    M, N, K = _first([(m, 16384, 128) for m in (128, 256, 512, 1024)],
                     lambda M, N, K: lib.pips_gemm_bf16_route(M, N, K, epi, 1, 1) == 3)
    bias = V.rne_patterns(N, seed=3).to(DEV)
    A = torch.randn(M, K, generator=torch.Generator().manual_seed(2)).to(DEV).bfloat16()
    W = torch.zeros(N, K, device=DEV, dtype=torch.bfloat16)
    out = ops.gemm_bf16(A, W, bias, epi=RES, R=torch.zeros(M, N, device=DEV, dtype=torch.bfloat16), out_bf16=True)
    ok, excused, cap = V.rne_check(out.view(torch.int16), bias.expand(M, N).contiguous())
    print(f"bf16 store route 3 {M}x{N}: {int((~ok).sum())} of {M * N} not RNE; {excused // M} subnormals flushed (of {cap // M} fed)")
    assert cap // M <= N // 1000 and excused <= cap
    assert bool(ok.all())


# ============================================================================================ C. mixed scales
def _report(tag, err, bound):
    ratio = float((err / bound).max())
    print(f"mixed scales {tag}: max err / bound {ratio:.3f}")
    return ratio


def _gemm_mixed(path, M, N, K, epi, run, split=False, out_bf16=False, bf16_operands=False, pre_bf16=False):
    """One GEMM with the row scale on A in both launches and the output-channel scale on W, bias and R in the second: the
    second is the first times the column scale, exactly (epilogues without a GELU); the scaled output within the bound."""
    c = V.gemm_case(M, N, K, epi, seed=M * 7 + N, bf16_operands=bf16_operands)
    A = (c["A"] * c["sa"][:, None]).to(DEV)
    W, b, sw = c["W"].to(DEV), c["b"].to(DEV), c["sw"].to(DEV)
    R = None if c["R"] is None else (c["R"] * c["sa"][:, None]).to(DEV)
    if out_bf16 and R is not None and path == "bf16_stream":
        R = R.bfloat16().float()
    Ws, bs, Rs = W * sw[:, None], b * sw, None if R is None else R * sw
    out_s = run(A, Ws, bs, Rs).double()
    pre = A.double() @ Ws.double().t() + bs.double()
    mag = A.double().abs() @ Ws.double().abs().t() + bs.double().abs()
    if epi == GELU:
        ref = torch.nn.functional.gelu(pre)
        bound = V.gelu_forward_bound(pre, mag, K, out_bf16=out_bf16, pre_bf16=pre_bf16)
    else:
        ref = pre if Rs is None else pre + Rs.double()
        mag = mag if Rs is None else mag + Rs.double().abs()
        bound = V.forward_bound(mag, K, ref, split=split, out_bf16=out_bf16)
        out_u = run(A, W, b, R).double()
        assert torch.equal(out_s, out_u * sw.double()), f"{path} {M}x{N}x{K}: scaling W, bias and R by powers of two changed the digits"
    err = (out_s - ref).abs()
    ratio = _report(f"{path} {M}x{N}x{K} epi {epi}", err, bound)
    assert bool((err <= bound).all()), ratio


@pytest.mark.parametrize("M,N,K,epi,route", [
    (2048, 512, 544, 0, 0),       # input projection: full tiles
    (77, 130, 64, 0, 0),          # ragged M and N
    (256, 1040, 512, 0, 0),       # head: N not a tile multiple
    (2048, 2176, 512, 2, 1),      # assembly, 128 x 128 tiles, residual form
    (2048, 512, 2048, 2, 2),      # assembly, 64 x 64 tiles, K split over the waves
    (2048, 2048, 512, 1, 1),      # assembly, GELU
])
def test_mixed_scales_gemm_f32(M, N, K, epi, route):
    from pips_amd import ops
    assert _lib().pips_gemm_f32_route(M, N, K, epi) == route
    _gemm_mixed(f"f32 route {route}", M, N, K, epi, lambda A, W, b, R: ops.gemm(A, W, b, epi, R))


@pytest.mark.parametrize("M,N,K,epi", [
    (2048, 512, 544, 0),          # full tiles
    (77, 132, 96, 2),             # ragged: gemm_tail.h's element-wise epilogue
    (16500, 1040, 512, 0),        # 256-row tiles with ragged M and N edges
])
def test_mixed_scales_gemm_split(M, N, K, epi):
    from pips_amd import ops
    _gemm_mixed("split", M, N, K, epi, lambda A, W, b, R: ops.gemm_x3(A, ops.split_bf16x3(W), b, epi, R), split=True)


@pytest.mark.parametrize("M,N,K,epi,out_bf16,route", [
    (4096, 512, 544, 0, False, 0),        # input projection: fp32 A rounded on staging, 32-element K blocks
    (1280, 2048, 512, 1, True, 0),        # register-staged, GELU, bf16 C
    (1000, 384, 128, 2, True, 0),         # bf16 residual stream on ragged tiles
    (8192, 512, 2048, 2, False, 3),       # gemm_bf16_t4_res_kernel<false>
    (8192, 512, 2048, 2, True, 3),        # gemm_bf16_t4_res_kernel<true>: EPI_RES_BF16
    (6144, 2048, 512, 1, True, 4),        # gemm_bf16_t4_gelu_kernel
])
def test_mixed_scales_gemm_bf16(M, N, K, epi, out_bf16, route):
    from pips_amd import ops
    stream = epi == RES and out_bf16
    a_bf16 = epi != 0
    flag = epi | (ops.EPI_RES_BF16 if stream else 0)
    assert _lib().pips_gemm_bf16_route(M, N, K, flag, int(a_bf16), int(out_bf16)) == route

    def run(A, W, b, R):
        A = A.bfloat16() if a_bf16 else A
        R = R.bfloat16() if (stream and R is not None) else R
        return ops.gemm_bf16(A, W.bfloat16(), b, epi=epi, R=R, out_bf16=out_bf16).float()
    _gemm_mixed("bf16_stream" if stream else f"bf16 route {route}", M, N, K, epi, run, out_bf16=out_bf16, bf16_operands=True,
                pre_bf16=route == 4)


def _conv_mixed(tag, c, k, s, p, run, parts_ok, split=False, out_bf16=False, stats_of_stored=False):
    """One convolution with the input-channel scale on the map in both launches and the output-channel scale on the weights
    and the bias in the second: outputs and pivoted partials of the second are those of the first times the scale, exactly."""
    x = (c["x"] * c["sx"]).to(DEV)
    w, b, sw = c["w"].to(DEV), c["b"].to(DEV), c["sw"].to(DEV)
    ws, bs = w * sw[:, None, None, None], b * sw
    out_s, st_s = run(x, ws, bs)
    assert parts_ok(st_s.shape[1]), f"{tag}: {st_s.shape[1]} statistics partials per frame: another kernel took the layer"
    out_u, st_u = run(x, w, b)
    assert torch.equal(out_s.double(), out_u.double() * sw.double()), f"{tag}: scaling W and bias by powers of two changed the digits"
    K = k * k * x.shape[-1]
    ref = V.conv_ref64(x, ws, bs, k, s, p)
    mag = V.conv_ref64(x.abs(), ws.abs(), bs.abs(), k, s, p)
    err = (out_s.double() - ref).abs()
    bound = V.forward_bound(mag, K, ref, split=split, out_bf16=out_bf16)
    ratio = _report(tag, err, bound)
    assert bool((err <= bound).all()), ratio
    from pips_amd import ops
    s1, s2 = ops.partial_sums(st_s)
    r1, r2 = V.stats_gate(s1, s2, out_s if stats_of_stored else ref)
    print(f"mixed scales {tag}: InstanceNorm partials err / bound {r1:.3f} (sum), {r2:.3f} (sum of squares)")
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("F_,H,W,Cin,Cout,k,s,p", [
    (16, 93, 125, 64, 64, 3, 1, 1),      # conv_f32_t4.hip, 64 -> 64 (256-pixel tiles), odd size, frames % 8 == 0
    (5, 181, 183, 64, 64, 3, 1, 1),      # the same, frames % 8 != 0: the linear block order
    (8, 93, 125, 96, 96, 3, 1, 1),       # 96 -> 96: 128-pixel tiles, three channel blocks
    (8, 45, 63, 416, 256, 3, 1, 1),      # 416 -> 256: four column tiles
    (2, 46, 62, 64, 96, 3, 2, 1),        # igemm_f32_kernel, stride 2
    (2, 23, 31, 96, 128, 1, 2, 0),       # 1 x 1 shortcut
])
def test_mixed_scales_conv_f32(F_, H, W, Cin, Cout, k, s, p):
    from pips_amd import ops
    cus = _lib().pips_device_cus()
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    px, ncol = (256, 1) if Cin == 64 else (128, 4 if Cin == 416 else 1)
    t4 = k == 3 and s == 1 and (Cin, Cout) in ((64, 64), (96, 96), (416, 256)) and F_ * ncol * ((H * W + px - 1) // px) * 2 >= 5 * cus
    assert t4 == (k == 3 and s == 1)
    if t4:      # one partial per wave (px / 4 pixels)
        parts_ok = lambda n: n == (H * W + px // 4 - 1) // (px // 4)
    else:       # igemm_f32_kernel: m tiles x wave rows
        parts_ok = lambda n: n in (2 * ((Ho * Wo + 63) // 64), 2 * ((Ho * Wo + 127) // 128), 4 * ((Ho * Wo + 127) // 128))
    c = V.conv_case(F_, H, W, Cin, Cout, k, seed=Cin + Cout + k)
    _conv_mixed(f"conv f32 {F_}x{H}x{W} {Cin}->{Cout} k{k} s{s}", c, k, s, p,
                lambda x, w, b: ops.conv_nhwc(x, w, b, k, s, p, want_stats=True), parts_ok)


@pytest.mark.parametrize("F_,H,W,Cin,Cout,k,s,p,rows", [
    (2, 46, 62, 64, 64, 3, 1, 1, 64),
    (8, 92, 124, 96, 96, 3, 1, 1, 256),      # the 256-row split tile (four wave rows)
])
def test_mixed_scales_conv_split(F_, H, W, Cin, Cout, k, s, p, rows):
    from pips_amd import ops
    c = V.conv_case(F_, H, W, Cin, Cout, k, seed=Cin + Cout + k)
    wave_rows = 4 if rows == 256 else 2
    _conv_mixed(f"conv split {F_}x{H}x{W} {Cin}->{Cout}", c, k, s, p,
                lambda x, w, b: ops.conv_nhwc_x3(x, ops.split_bf16x3(w), b, k, s, p, want_stats=True),
                lambda n: n == wave_rows * ((H * W + rows - 1) // rows), split=True)


@pytest.mark.parametrize("F_,H,W,Cin,Cout,kernel", [
    (16, 92, 124, 64, 64, "c64"),        # conv_bf16_c64.hip: weights and halo patch in LDS
    (24, 93, 125, 96, 96, "t4c"),        # conv_bf16_t4c.hip, odd size
    (2, 46, 62, 64, 64, "igemm"),        # too few tiles: implicit GEMM on bf16 maps
    (8, 92, 124, 96, 96, "igemm"),       # Cout = 96 on a 128-wide tile
])
def test_mixed_scales_conv_bf16_maps(F_, H, W, Cin, Cout, kernel):
    from pips_amd import ops
    cus = _lib().pips_device_cus()
    c = V.conv_case(F_, H, W, Cin, Cout, 3, seed=F_ + H + Cin + 3, bf16_operands=True)
    tiles4 = ((H + 3) // 4) * 4
    if kernel == "c64":         # one partial per wave of a 4-row tile, 64 or 32 columns wide
        parts_ok = lambda n: n in (((W + 63) // 64) * tiles4, ((W + 31) // 32) * tiles4)
    elif kernel == "t4c":       # one partial per 256-pixel tile
        assert F_ * ((H * W + 255) // 256) >= 4 * cus
        parts_ok = lambda n: n == (H * W + 255) // 256
    else:
        parts_ok = lambda n: n in (2 * ((H * W + 63) // 64), 2 * ((H * W + 127) // 128))

    def run(x, w, b):
        return ops.conv_nhwc_bf16_maps(x.bfloat16(), w.bfloat16(), b, 3, 1, 1, out_bf16=True, want_stats=True)
    # conv_bf16_t4c.hip takes its statistics from the stored bf16 map (tests/test_kernels_gpu.py), the others from the accumulators
    _conv_mixed(f"conv bf16 maps {kernel} {F_}x{H}x{W} {Cin}->{Cout}", c, 3, 1, 1, run, parts_ok, out_bf16=True,
                stats_of_stored=kernel == "t4c")
