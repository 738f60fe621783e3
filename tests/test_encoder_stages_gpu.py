"""The encoder's stage kernels alone, each against the operation in fp64 with the derived per-element bound of
tests/golden/encoder_stages.py (the bounds are proven on the CPU in tests/test_encoder_stages.py): the stems
(stem_conv_kernel / stem_conv_bf16_kernel, four instantiations each) with their statistics partials, inorm_apply_kernel<0..2>
and inorm_apply_bf16_kernel<0..3>, resize_into_kernel and its bf16 form, avgpool2_kernel, both finalize kernels on partials
built on the host, pyramid_mirror_kernel, and stem -> finalize -> apply against the oracle's enc_stem tap.  Everything under
test is called through pips_amd.ops; torch on the device forms operands and fp64 references.  Shapes are the smallest that
reach the path named beside them."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import encoder_stages as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_ARG = -1


def _lib():
    from pips_amd import _lib
    return _lib.load()


def _stem_w(sd):
    return sd["fnet.conv1.weight"].float(), sd["fnet.conv1.bias"].float()


# ============================================================================================ stem
def _walk_frames(bf16):
    """frames of 176 x 128 (22 tiles each) whose work items outnumber the persistent grid -- 512 blocks (fp32), three per
    compute unit (bf16) -- so that blocks walk to a second tile: 24 frames (528 items), and 36 on 256 compute units
    (792 items against 768 blocks; 35 would already walk, with two blocks); more where the device has more compute units"""
    grid = 3 * _lib().pips_device_cus() if bf16 else 512
    return max(grid // 22 + 1, 36 if bf16 else 24)


# name: (frames, H, W, base pointer one element past an aligned allocation)
STEM_CASES = {
    "a_37x150_rows": (3, 37, 150, False),      # W % 4 != 0: the row-by-row form; Ho = 19: the last tile is one wave short; Wo = 75: two column tiles, the second 11 wide
    "b_37x152_quads": (3, 37, 152, False),     # the quad-load form
    "c_37x152_unaligned": (3, 37, 152, True),  # W % 4 == 0 on an unaligned base: the row-by-row form (another tap order than b: the bound, not b's bits)
    "d_5x9_padding": (3, 5, 9, False),         # every tap of every pixel is padding-adjacent
    "e_176x128_walk": (None, 176, 128, False),  # the persistent walk
}
_STEM_REF = {}


def _stem_reference(Fr, H, W, bf16, sd):
    """frames, fp64 reference, magnitude sum, fp64 statistics and the fp32 yardstick's statistics: once per (shape, mode)"""
    key = (Fr, H, W, bf16)
    if key not in _STEM_REF:
        w, b = _stem_w(sd)
        rgbs = E.stem_frames(Fr, H, W)
        ref, mag = E.stem_ref(rgbs.to(DEV), w.to(DEV), b.to(DEV), bf16)
        x = E.stem_scale(rgbs)
        m32 = F.conv2d(x.bfloat16().float() if bf16 else x, w.bfloat16().float() if bf16 else w, b, stride=2, padding=3)
        _STEM_REF[key] = (rgbs, ref, mag, E.map_stats64(ref), E.map_stats32(m32.permute(0, 2, 3, 1)).to(DEV))
    return _STEM_REF[key]


def _offset_by_one(t):
    """the same values seen from a base one element past an aligned allocation"""
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 256 == 0 and v.is_contiguous() and v.data_ptr() == buf.data_ptr() + t.element_size()
    return v


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(STEM_CASES))
def test_stem(case, bf16, weights_raw, arenas):
    """Raw conv1 map within 160 u (conv(|x|, |w|) + |b|) (+ half a bf16 ulp) of the fp64 convolution, element by element
    (measured on an MI355X: fp32 0.018 .. 0.038 of the bound, i.e. 3 .. 6 u; bf16 0.987 .. 0.994: the rounding of the store).
    Statistics: {mean, rstd} finalized from the kernel's partials against the fp64 mean and biased variance of the (in bf16
    mode: unrounded) reference map; yardstick = fp32 torch.var_mean on torch's fp32 convolution against the same fp64
    values, gate 4x that + 2^-22 relative.  Measured on an MI355X, worst error / yardstick's worst error, {mean, rstd}:
    a fp32 1.07 / 0.72, bf16 1.00 / 1.00; b and c fp32 1.00 / 1.07, bf16 1.00 / 0.97; d fp32 1.12 / 1.23, bf16 1.00 / 0.94;
    e fp32 0.99 / 0.67, bf16 1.01 / 0.85.
    Exact: the counts of a (frame, channel) add up to Ho Wo, empty partials exist when Ho % 4 != 0, and uint8 frames give the
    bits of the same values as float on the same route."""
    from pips_amd import ops
    Fr, H, W, unaligned = STEM_CASES[case]
    Fr = _walk_frames(bf16) if Fr is None else Fr
    rgbs, ref, mag, st64, st_yard = _stem_reference(Fr, H, W, bf16, weights_raw)
    Ho, Wo = E.stem_out_hw(H, W)
    xf, x8 = rgbs.to(DEV), rgbs.to(torch.uint8).to(DEV)
    if unaligned:
        xf, x8 = _offset_by_one(xf), _offset_by_one(x8)
        assert xf.data_ptr() % 16 != 0 and x8.data_ptr() % 4 != 0
    out, stats = ops.encoder_stem(arenas["raw"], xf, bf16=bf16)
    out8, stats8 = ops.encoder_stem(arenas["raw"], x8, bf16=bf16)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (Fr, Ho, Wo, 64) and out.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert tuple(stats.shape) == (Fr, E.stem_parts(H, W), 64, 4)
    ratio = E.worst((out.double() - ref).abs(), E.stem_bound(ref, mag, bf16))
    print(f"stem {case} {'bf16' if bf16 else 'f32'} F={Fr}: worst element at {ratio:.3f} of its bound")
    assert ratio <= 1.0
    assert torch.equal(out8, out) and torch.equal(stats8, stats)
    n = stats[..., 3]
    assert bool((n.sum(dim=1) == Ho * Wo).all())
    assert bool((n == 0).any()) == (Ho % 4 != 0)
    got = ops.inorm_finalize(stats)
    (rm, okm), (rr, okr) = E.stats_gate(got, st64, st_yard)
    print(f"stem {case} {'bf16' if bf16 else 'f32'} statistics: mean at {rm:.2f} x, rstd at {rr:.2f} x the fp32 yardstick's error")
    assert okm and okr


# ============================================================================================ instance-norm apply
APPLY = [("f32", m) for m in E.APPLY_MODES["f32"]] + [("bf16", m) for m in E.APPLY_MODES["bf16"]]


def _apply_check(tag, Fr, HW, Cc, maps, mode):
    from pips_amd import ops
    bf16 = maps == "bf16"
    x, st, res, rst = E.apply_case(Fr, HW, Cc, bf16, device=DEV)
    got = ops.inorm_apply(x, st, res if mode >= 1 else None, rst if mode >= 2 else None, mode)
    assert got.dtype == x.dtype and got.shape == x.shape
    ref, bound = E.apply_ref(x, st, res, rst, mode, bf16)
    ratio = E.worst((got.double() - ref).abs(), bound)
    assert ratio <= 1.0, f"{tag}: worst element at {ratio:.3f} of 4 u (|t1| + |t2|){' + half a bf16 ulp' if bf16 else ''}"


@pytest.mark.parametrize("Cc", [64, 96, 128, 256])
@pytest.mark.parametrize("maps,mode", APPLY)
def test_inorm_apply(maps, mode, Cc):
    """F = 3 frames with statistics distinct per (frame, channel); HW straddles the bf16 kernel's chunk sizes: 64 pixels
    (C = 256), 128 (C = 128), 168 (C = 96: 252 threads, 21 pixels per step) and 256 (C = 64)"""
    for HW in (1, 70, 167, 168, 169, 257):
        _apply_check(f"apply {maps} mode {mode} C={Cc} HW={HW}", 3, HW, Cc, maps, mode)


@pytest.mark.parametrize("mode", E.APPLY_MODES["f32"])
def test_inorm_apply_f32_grid_stride(mode):
    """5 x 4800 x 256: 1 536 000 float4 against the fp32 kernel's 4096 x 256 threads -- the second pass of its grid-stride loop"""
    assert 5 * 4800 * 256 // 4 > 4096 * 256
    _apply_check(f"apply f32 mode {mode} grid-stride", 5, 4800, 256, "f32", mode)


# ============================================================================================ resize
def _sentinel(shape, dtype):
    return torch.full(shape, -12288.0, dtype=dtype, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _resize_check(tag, Fr, hs, hd, Cc, coff, maps):
    from pips_amd import ops
    bf16 = maps == "bf16"
    g = torch.Generator().manual_seed(17 + hs[0] * 100 + hs[1] + Cc + coff)
    src = torch.randn(Fr, hs[0], hs[1], Cc, generator=g)
    src = (src.bfloat16() if bf16 else src).to(DEV)
    dst = _sentinel((Fr, hd[0], hd[1], E.RESIZE_CDST), src.dtype)
    before = dst.clone()
    ops.resize_into(src, dst, coff)
    inside = torch.zeros(E.RESIZE_CDST, dtype=torch.bool, device=DEV)
    inside[coff:coff + Cc] = True
    assert torch.equal(_bits(dst)[..., ~inside], _bits(before)[..., ~inside]), f"{tag}: channels outside [{coff}, {coff + Cc}) were written"
    got = dst[..., coff:coff + Cc]
    if hs == hd:
        assert torch.equal(_bits(got), _bits(src)), f"{tag}: the identity size is not a copy"
    ref = E.resize_ref(src, hd)
    ratio = E.worst((got.double() - ref).abs(), E.resize_bound(src, ref, bf16))
    assert ratio <= 1.0, f"{tag}: worst element at {ratio:.3f} of 2^-22 (Hs + Ws) max|src|{' + half a bf16 ulp' if bf16 else ''}"
    return ratio


@pytest.mark.parametrize("maps", ["f32", "bf16"])
@pytest.mark.parametrize("hs,hd", E.RESIZE_SHAPES, ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in E.RESIZE_SHAPES])
def test_resize_into(hs, hd, maps):
    """down, nearly the identity, up, the identity (a bit-exact copy), one inactive axis, 2 x 3 up, and one output pixel (scale
    0); the four layers' (C, coff) into a 416-channel map pre-filled with a sentinel that must survive outside [coff, coff + C)"""
    worst = max(_resize_check(f"resize {maps} {hs}->{hd} C={Cc}@{coff}", 3, hs, hd, Cc, coff, maps) for Cc, coff in E.RESIZE_CHANNELS)
    print(f"resize {maps} {hs}->{hd}: worst element at {worst:.3f} of its bound")


@pytest.mark.parametrize("maps", ["f32", "bf16"])
def test_resize_into_grid_stride(maps):
    """12 x (23, 31) -> (46, 62) x 128: 1 095 168 float4 against 4096 x 256 threads -- the second pass of the fp32 kernel's loop"""
    assert 12 * 46 * 62 * 128 // 4 > 4096 * 256
    _resize_check(f"resize {maps} grid-stride", 12, (23, 31), (46, 62), 128, 160, maps)


# ============================================================================================ avg pool
@pytest.mark.parametrize("Fr,H,W", [(3, 13, 18), (3, 16, 16), (3, 3, 5), (3, 2, 2), (12, 92, 124)])
def test_avgpool2(Fr, H, W):
    """odd sizes drop the last row / column; (12, 92, 124): the second pass of the grid-stride loop"""
    from pips_amd import ops
    g = torch.Generator().manual_seed(23 + H)
    src = torch.randn(Fr, H, W, 128, generator=g).to(DEV)
    got = ops.avgpool2(src)
    ref, bound = E.avgpool_ref(src)
    assert tuple(got.shape) == tuple(ref.shape) == (Fr, H // 2, W // 2, 128)
    assert Fr == 3 or got.numel() // 4 > 4096 * 256
    ratio = E.worst((got.double() - ref).abs(), bound)
    assert ratio <= 1.0, f"avgpool {H}x{W}: worst element at {ratio:.3f} of 3 u (|a| + |b| + |c| + |d|) / 4"


# ============================================================================================ finalize
@pytest.mark.parametrize("Fr", [1, 16, 17])
@pytest.mark.parametrize("parts", [1, 7, 2049, 4100])
def test_inorm_finalize(parts, Fr):
    """Partials built on the host from per-part data (n in 0..64, a quarter of the parts empty and filled with noise, the
    first never empty).  F <= 16: inorm_finalize_pivot_kernel<256>, whose loop steps by 2048 partials -- 2049 and 4100 take
    its second and third trip; F = 17: inorm_finalize_pivot16_kernel (step 256).  mean within 2^-23 |mean|, rstd within
    2^-22 relative of the fp64 evaluation of the same partials, on a wide-spread set and on mean 200 / std 1e-3."""
    from pips_amd import ops
    for Cc in (16, 64, 96):
        for kind in ("wide", "flat"):
            st = E.finalize_partials(Fr, parts, Cc, kind, device=DEV)
            got = ops.inorm_finalize(st)
            ref = E.finalize_ref(st)
            assert tuple(got.shape) == (Fr, Cc, 2)
            ratio = E.worst((got.double() - ref).abs(), E.finalize_bounds(ref))
            assert ratio <= 1.0, f"finalize F={Fr} parts={parts} C={Cc} {kind}: worst at {ratio:.3f} of (2^-23 |mean|, 2^-22 rstd)"
            if kind == "flat" and parts >= 7:
                assert float((got[..., 0] - 200).abs().max()) < 1e-3


# ============================================================================================ bf16 mirror
def test_pyramid_mirror_rounding():
    """3 frames of 136 x 200 at stride 8 (levels 17x25, 8x12, 4x6, 2x3): the mirror is levels.bfloat16() bit for bit -- ties on
    even and odd kept mantissas, neighbours of ties, the largest finite bf16, fp32 subnormals, +-0 -- and nothing behind it
    is written"""
    from pips_amd import ops
    lib = _lib()
    Fr, H, W, stride = 3, 136, 200, 8
    n, total = lib.pips_pyramid_mirror_offset(Fr, H, W, stride), lib.pips_pyramid_floats(Fr, H, W, stride)
    g = torch.Generator().manual_seed(29)
    pyr = _sentinel((total,), torch.float32)
    pyr[:n] = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())).to(DEV)
    plants = E.mirror_plants().to(DEV)
    levels = ops.pyramid_levels(pyr, Fr, H, W, stride)
    assert [tuple(l.shape[1:3]) for l in levels] == [(17, 25), (8, 12), (4, 6), (2, 3)]
    for l in levels:                                   # at the head, at the tail and at an odd offset inside every level
        flat = l.view(-1)
        for at in (0, flat.numel() - plants.numel(), flat.numel() // 2 + 3):
            flat[at:at + plants.numel()] = plants
    before = pyr.clone()
    ops.pyramid_mirror(pyr, Fr, H, W, stride)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pyr[:n]), _bits(before[:n])) and torch.equal(_bits(pyr[n + n // 2:]), _bits(before[n + n // 2:]))
    got = pyr[n:n + n // 2].view(torch.bfloat16)
    assert got.numel() == n
    want = before[:n].bfloat16()
    bad = E.bf16_bits(got) != E.bf16_bits(want)
    assert not bool(bad.any()), (f"{int(bad.sum())} of {n} mirror elements differ from .bfloat16(), first at {int(bad.nonzero()[0])}: "
                                 f"{float(before[int(bad.nonzero()[0])]):.9g}")
    assert torch.equal(E.bf16_bits(got).cpu(), E.bf16_rne_bits(before[:n].cpu()))      # and from round-to-nearest-even in integers


# ============================================================================================ composition
@pytest.mark.parametrize("H,W", [(106, 150), (128, 160)])
def test_stem_finalize_apply_is_the_oracles_stem_tap(H, W, weights_raw, arenas):
    """stem -> finalize -> apply mode 0 on 2 frames against taps["enc_stem"] of the oracle run in fp64; yardstick = the oracle's own
    fp32 tap against its fp64 tap, gate 4x that + 1e-6.  Measured on an MI355X: 2.15e-06 against 2.40e-06 (0.90 x) at 106 x 150, 2.34e-06 against
    2.41e-06 (0.97 x) at 128 x 160, on maps of |value| up to 4.7."""
    from oracle import pips_oracle as O
    from pips_amd import ops
    g = torch.Generator().manual_seed(3)
    rgbs = torch.randint(0, 256, (2, 3, H, W), generator=g).float()
    x = 2 * (rgbs / 255.0) - 1.0
    t32, t64 = {}, {}
    O.encoder(weights_raw, x, 8, t32)
    O.encoder(O.to_dtype(weights_raw, torch.float64), x.double(), 8, t64)
    ref = t64["enc_stem"].permute(0, 2, 3, 1)
    yard = float((t32["enc_stem"].permute(0, 2, 3, 1).double() - ref).abs().max())
    raw, stats = ops.encoder_stem(arenas["raw"], rgbs.to(DEV))
    got = ops.inorm_apply(raw, ops.inorm_finalize(stats))
    err = float((got.cpu().double() - ref).abs().max())
    print(f"stem tap {H}x{W}: HIP vs fp64 {err:.2e}, the oracle's fp32 tap vs fp64 {yard:.2e} ({err / yard:.2f} x), |map| {float(ref.abs().max()):.1f}")
    assert err <= 4 * yard + 1e-6


# ============================================================================================ return codes
def test_stage_entry_points_reject_bad_arguments(arenas):
    """PIPS_E_ARG ahead of any launch -- the outputs keep their sentinel -- for null pointers, a C off its alignment, a mode
    outside its range, mode 3 on fp32 maps, and coff + C > Cdst"""
    from pips_amd import _lib as L, ops
    lib = L.load()
    p, st = L.ptr, ops._stream()
    arena = arenas["raw"]
    rgbs = torch.zeros(1, 3, 16, 16, device=DEV)
    out = _sentinel((1, 8, 8, 64), torch.float32)
    stats = _sentinel((1, lib.pips_encoder_stem_parts(16, 16), 64, 4), torch.float32)
    parts = C.c_int(-7)
    assert lib.pips_encoder_stem_parts(16, 16) == 2 * 1 * 4 and lib.pips_encoder_stem_parts(0, 16) == 0
    stem = lambda a, r, o, s, F_=1, H=16, W=16, flags=0: lib.pips_encoder_stem(a, r, F_, H, W, flags, o, s, C.byref(parts), st)
    for rc in (stem(None, p(rgbs), p(out), p(stats)), stem(p(arena), None, p(out), p(stats)), stem(p(arena), p(rgbs), None, p(stats)),
               stem(p(arena), p(rgbs), p(out), None), stem(p(arena), p(rgbs), p(out), p(stats), F_=0),
               stem(p(arena), p(rgbs), p(out), p(stats), W=0), stem(p(arena), p(rgbs), p(out), p(stats), flags=ops.FLAG_SPLIT_BF16)):
        assert rc == E_ARG and lib.pips_last_error()
    assert parts.value == -7

    x = torch.zeros(1, 4, 64, device=DEV)
    xb = x.bfloat16()
    y, yb = _sentinel((1, 4, 64), torch.float32), _sentinel((1, 4, 64), torch.bfloat16)
    s2 = torch.ones(1, 64, 2, device=DEV)
    app = lambda x_, s_, r_, rs_, mode, y_, Cc=64, bf=0, F_=1, HW=4: lib.pips_inorm_apply(x_, s_, r_, rs_, mode, y_, F_, HW, Cc, bf, st)
    for rc in (app(None, p(s2), None, None, 0, p(y)), app(p(x), None, None, None, 0, p(y)), app(p(x), p(s2), None, None, 0, None),
               app(p(x), p(s2), None, None, 1, p(y)),                 # mode 1 without a shortcut
               app(p(x), p(s2), p(x), None, 2, p(y)),                 # mode 2 without the shortcut's statistics
               app(p(x), p(s2), p(x), p(s2), 3, p(y)),                # mode 3 on fp32 maps
               app(p(x), p(s2), p(x), p(s2), -1, p(y)), app(p(xb), p(s2), p(xb), p(s2), 4, p(yb), bf=1),
               app(p(xb), p(s2), p(xb), None, 3, p(yb), bf=1),
               app(p(x), p(s2), None, None, 0, p(y), Cc=62),          # C off its alignment: 4 for fp32 maps, 8 for bf16 maps
               app(p(xb), p(s2), None, None, 0, p(yb), Cc=60, bf=1),
               app(p(x), p(s2), None, None, 0, p(y), F_=0), app(p(x), p(s2), None, None, 0, p(y), HW=0)):
        assert rc == E_ARG and lib.pips_last_error()

    src, srcb = torch.zeros(1, 4, 4, 64, device=DEV), torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.bfloat16)
    dst, dstb = _sentinel((1, 8, 8, 416), torch.float32), _sentinel((1, 8, 8, 416), torch.bfloat16)
    rsz = lambda s_, d_, Cc=64, Cdst=416, coff=0, bf=0, Hs=4: lib.pips_resize_into(s_, 1, Hs, 4, Cc, d_, 8, 8, Cdst, coff, bf, st)
    for rc in (rsz(None, p(dst)), rsz(p(src), None), rsz(p(src), p(dst), coff=356), rsz(p(src), p(dst), Cdst=60),
               rsz(p(src), p(dst), coff=-4), rsz(p(src), p(dst), Cc=62), rsz(p(src), p(dst), coff=2), rsz(p(src), p(dst), Cdst=418),
               rsz(p(srcb), p(dstb), Cc=60, bf=1), rsz(p(srcb), p(dstb), coff=4, bf=1), rsz(p(srcb), p(dstb), coff=360, bf=1),
               rsz(p(src), p(dst), Hs=0)):
        assert rc == E_ARG and lib.pips_last_error()

    pool_out = _sentinel((1, 2, 2, 64), torch.float32)
    pool = lambda s_, d_, H=4, W=4, Cc=64, F_=1: lib.pips_avgpool2(s_, F_, H, W, Cc, d_, st)
    for rc in (pool(None, p(pool_out)), pool(p(src), None), pool(p(src), p(pool_out), Cc=62), pool(p(src), p(pool_out), H=1),
               pool(p(src), p(pool_out), W=1), pool(p(src), p(pool_out), F_=0)):
        assert rc == E_ARG and lib.pips_last_error()

    torch.cuda.synchronize()
    for t in (out, stats, y, yb, dst, dstb, pool_out):
        assert bool((t == -12288.0).all()), "a rejected call wrote to its output"
    assert lib.pips_abi_version() == 3
    # and the same calls with good arguments are accepted
    assert stem(p(arena), p(rgbs), p(out), p(stats)) == 0 and parts.value == 8
    assert app(p(xb), p(s2), p(xb), p(s2), 3, p(yb), bf=1) == 0 and rsz(p(src), p(dst), coff=352) == 0 and pool(p(src), p(pool_out)) == 0
    torch.cuda.synchronize()
