"""CPU: the references and bounds of tests/golden/encoder_stages.py, proven before the GPU tests rely on them
(tests/test_encoder_stages_gpu.py).  Each bound must pass a correct implementation of its stage -- torch's own fp32 operator, or
a restatement in fp32 arithmetic -- and must bite: every planted error exceeds it somewhere.  Planted: a truncating bf16 store,
align_corners=False, one dropped stem tap, the statistics of frame f-1 applied to frame f, a pool that takes the last odd row,
one dropped partial in the finalize."""
import pytest
import torch
import torch.nn.functional as F

import encoder_stages as E


def _stem_w(sd):
    return sd["fnet.conv1.weight"].float(), sd["fnet.conv1.bias"].float()


def _conv32(x, w, b):
    return F.conv2d(x, w, b, stride=2, padding=3).permute(0, 2, 3, 1)


_worst = E.worst


def test_stem_reference_is_conv2d(weights_raw):
    """the 49-product form the GPU tests run on the device against F.conv2d in fp64: equal to fp64 summation order"""
    w, b = _stem_w(weights_raw)
    x = E.stem_scale(E.stem_frames(2, 37, 150))
    got = E.conv7s2_nhwc64(x, w, b)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3).permute(0, 2, 3, 1)
    mag = E.conv7s2_nhwc64(x.abs(), w.abs(), b.abs())
    assert tuple(got.shape) == (2, 19, 75, 64) == tuple(ref.shape)
    assert bool(((got - ref).abs() <= 160 * 2.0 ** -53 * mag).all())
    assert E.stem_parts(37, 150) == 5 * 2 * 4 and E.stem_parts(176, 128) == 22 * 4 and E.stem_parts(5, 9) == 4


@pytest.mark.parametrize("H,W", [(37, 150), (37, 152), (5, 9)])
def test_stem_bound_fp32(H, W, weights_raw):
    """torch's fp32 convolution sits at a few u of the magnitude sum (measured 6 u; the gate is 160 u); one dropped tap does not"""
    w, b = _stem_w(weights_raw)
    rgbs = E.stem_frames(3, H, W)
    ref, mag = E.stem_ref(rgbs, w, b)
    bound = E.stem_bound(ref, mag)
    x = E.stem_scale(rgbs)
    ratio = _worst((_conv32(x, w, b).double() - ref).abs(), bound)
    print(f"stem fp32 {H}x{W}: torch fp32 conv at {ratio * 160:.1f} u of the magnitude sum")
    assert ratio <= 1.0
    assert _worst((_conv32(x, E.drop_stem_tap(w), b).double() - ref).abs(), bound) > 1.0


@pytest.mark.parametrize("H,W", [(37, 150), (5, 9)])
def test_stem_bound_bf16(H, W, weights_raw):
    """fp32 accumulation of the bf16 operands rounded once (RNE) passes; the same accumulators truncated do not (45 % of the
    elements at 37 x 150); neither does a dropped tap"""
    w, b = _stem_w(weights_raw)
    rgbs = E.stem_frames(3, H, W)
    ref, mag = E.stem_ref(rgbs, w, b, bf16=True)
    bound = E.stem_bound(ref, mag, bf16=True)
    xb, wb = E.stem_scale(rgbs).bfloat16().float(), w.bfloat16().float()
    acc = _conv32(xb, wb, b)
    ratio = _worst((acc.bfloat16().double() - ref).abs(), bound)
    over = (E.bf16_truncate(acc).double() - ref).abs() > bound
    print(f"stem bf16 {H}x{W}: RNE store at {ratio:.2f} of the bound, truncation over it on {float(over.float().mean()):.0%}")
    assert ratio <= 1.0
    assert bool(over.any()) and (H < 30 or float(over.float().mean()) > 0.3)
    assert _worst((_conv32(xb, E.drop_stem_tap(wb), b).bfloat16().double() - ref).abs(), bound) > 1.0


def test_stem_statistics_gate(weights_raw):
    """{mean, rstd} combined from row-wise pivoted partials of an fp32 map pass the yardstick gate; those of the neighbouring
    frame do not"""
    w, b = _stem_w(weights_raw)
    rgbs = E.stem_frames(3, 37, 150)
    ref, _ = E.stem_ref(rgbs, w, b)
    m32 = _conv32(E.stem_scale(rgbs), w, b)
    m = m32.double()
    p = m[:, :, :1]                                                            # one part per row, pivot = its first pixel
    d = m - p
    parts = torch.stack([d.sum(2), (d * d).sum(2), p[:, :, 0], torch.full_like(p[:, :, 0], m.shape[2])], dim=-1).float()
    got = E.finalize_like_kernel(parts)
    ref64, yard = E.map_stats64(ref), E.map_stats32(m32)
    res = E.stats_gate(got, ref64, yard)
    print("row-wise pivoted partials against the fp64 map: mean %.2f x, rstd %.2f x the error of torch.var_mean in fp32" % (res[0][0], res[1][0]))
    assert res[0][1] and res[1][1]
    bad = E.stats_gate(torch.roll(got, 1, 0), ref64, yard)
    assert not bad[0][1] and not bad[1][1]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("C,HW", [(64, 70), (96, 169)])
def test_apply_bound(C, HW, bf16):
    modes = E.APPLY_MODES["bf16" if bf16 else "f32"]
    x, st, res, rst = E.apply_case(3, HW, C, bf16)
    for mode in modes:
        ref, bound = E.apply_ref(x, st, res, rst, mode, bf16)
        acc = E.apply_f32(x, st, res, rst, mode)
        got = acc.bfloat16() if bf16 else acc
        ratio = _worst((got.double() - ref).abs(), bound)
        print(f"apply mode {mode} C={C} HW={HW} bf16={bf16}: fp32 arithmetic at {ratio:.2f} of the bound")
        assert ratio <= 1.0
        # statistics of frame f-1 on frame f (the map's own, and the shortcut's where the mode reads them)
        wrong = E.apply_f32(x, torch.roll(st, 1, 0), res, rst, mode)
        assert _worst(((wrong.bfloat16() if bf16 else wrong).double() - ref).abs(), bound) > 1.0
        if mode >= 2:
            wrong = E.apply_f32(x, st, res, torch.roll(rst, 1, 0), mode)
            assert _worst(((wrong.bfloat16() if bf16 else wrong).double() - ref).abs(), bound) > 1.0
        if bf16:
            assert _worst((E.bf16_truncate(acc).double() - ref).abs(), bound) > 1.0


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("hs,hd", E.RESIZE_SHAPES)
def test_resize_bound(hs, hd, bf16):
    """torch's fp32 interpolate stays well inside the bound at every shape (fp32 maps: at most 0.15 of it measured, 0.25 asserted);
    align_corners=False is outside it at every shape that is not the identity"""
    g = torch.Generator().manual_seed(5)
    src = torch.randn(3, hs[0], hs[1], 16, generator=g)
    if bf16:
        src = src.bfloat16()
    ref = E.resize_ref(src, hd)
    bound = E.resize_bound(src, ref, bf16)
    acc = F.interpolate(src.float().permute(0, 3, 1, 2), size=hd, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    got = acc.bfloat16() if bf16 else acc
    ratio = _worst((got.double() - ref).abs(), bound)
    print(f"resize {hs}->{hd} bf16={bf16}: torch fp32 interpolate at {ratio:.3f} of the bound")
    assert ratio <= (1.0 if bf16 else 0.25)
    if hs == hd:
        assert torch.equal(got, src)                                           # the identity size is a copy
    else:
        wrong = E.resize_ref(src, hd, align_corners=False)
        assert _worst((wrong - ref).abs(), bound) > 1.0
    if bf16 and hs != hd and hd != (1, 1):                                     # (one output pixel is the source's corner: a bf16 value)
        assert _worst((E.bf16_truncate(acc).double() - ref).abs(), bound) > 1.0


@pytest.mark.parametrize("H,W", [(13, 18), (16, 16), (3, 5), (2, 2)])
def test_avgpool_bound(H, W):
    g = torch.Generator().manual_seed(9)
    src = torch.randn(3, H, W, 128, generator=g)
    ref, bound = E.avgpool_ref(src)
    got = F.avg_pool2d(src.permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (3, H // 2, W // 2, 128)
    assert _worst((got.double() - ref).abs(), bound) <= 1.0
    if H % 2:
        assert _worst((E.avgpool_last_odd_row(src).double() - ref).abs(), bound) > 1.0


@pytest.mark.parametrize("kind", ["wide", "flat"])
@pytest.mark.parametrize("Fr,parts,C", [(2, 1, 16), (2, 7, 16), (1, 2049, 16)])
def test_finalize_bounds(Fr, parts, C, kind):
    """a correct fp64 finalize rounded to fp32 is inside the bounds; with one partial dropped it is not"""
    st = E.finalize_partials(Fr, parts, C, kind)
    n = st[..., 3]
    assert bool((n[:, 0] > 0).all()) and bool((n.sum(1) > 0).all())
    if parts > 100:
        assert 0.2 < float((n == 0).float().mean()) < 0.3
        assert bool((st[..., :3][n == 0] == 1e30).all())
    ref = E.finalize_ref(st)
    bounds = E.finalize_bounds(ref)
    got = E.finalize_like_kernel(st).double()
    assert bool(((got - ref).abs() <= bounds).all())
    if kind == "flat":                                                         # the data's own statistics come back
        assert float((ref[..., 0] - 200).abs().max()) < 1e-3 and float((ref[..., 1] - (1e-6 + E.EPS) ** -0.5).abs().max()) < 30
    if parts > 1:
        t = int(n[0, 1:, 0].argmax()) + 1
        dropped = st.clone()
        dropped[0, t, 0, 3] = 0
        bad = (E.finalize_like_kernel(dropped).double() - ref).abs() > bounds
        assert bool(bad[0, 0].any()) and int(bad.any(-1).sum()) == 1


def test_bf16_rounding_reference():
    """the integer form of round-to-nearest-even is torch's .bfloat16() on the planted values and on random ones; truncation
    differs from it on the planted ties"""
    g = torch.Generator().manual_seed(1)
    x = torch.cat([E.mirror_plants(), torch.randn(4096, generator=g) * torch.exp2(torch.randint(-30, 30, (4096,), generator=g).float())])
    assert torch.equal(E.bf16_rne_bits(x), E.bf16_bits(x.bfloat16()))
    p = E.mirror_plants()
    assert E.bf16_bits(p.bfloat16())[:2].tolist() == [0x3F80, 0x3F82]          # ties to even: down on an even, up on an odd mantissa
    assert int((E.bf16_bits(E.bf16_truncate(p).bfloat16()) != E.bf16_bits(p.bfloat16())).sum()) >= 8
    assert torch.equal(E.bf16_half_ulp(torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0])).float(),
                       torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0]))
