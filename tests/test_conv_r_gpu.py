"""conv_f32_r.hip -- the LDS-resident 64 -> 64 convolution of the fp32 encoder's layer 1 -- through its named entry point
(ops.conv_nhwc_f32_r, any map size) against igemm_f32_kernel (ops.conv_nhwc, route "igemm") on the same input; with in_norm that
input is first passed through ops.inorm_apply mode 0 with the same statistics.  Same K order, one chain per output value: the maps
must be bitwise equal.  The padding probe -- an all-zero map under statistics with mean < 0, so relu((0 - mean) * rstd) > 0
everywhere inside the image -- fails that equality if a tap outside the image is normalised.

Statistics: the kernel's partials (4 ceil(H/4) ceil(W/32) per frame: one per image row of a 4 x 32 tile) through the encoder's own
finalize against fp64 {mean, rstd} of the output map; the bound is 1.5 x the error of igemm_f32_kernel's partials on the same map
(another partition of the same sums; the kernel under test is never its own yardstick).  Both errors are printed.

Containment: output map and partials lie inside poisoned buffers; nothing but the map and the reported parts may change.

The same file holds mode 3 of the apply pass on fp32 maps (pips_inorm_apply_f32, through ops.inorm_apply), bitwise against mode 0
on each operand and relu(a + b) in torch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -7.25e18
GUARD = 3
E_ARG = -1

#        id           F  H  W
CASES = [("2x6x40",   2, 6, 40),      # H no multiple of 4, a ragged second column tile, two frames with different in_norm
         ("1x4x24",   1, 4, 24),      # a single column tile narrower than 32: every tile touches all four borders
         ("3x9x65",   3, 9, 65),      # a one-pixel last column tile, three row tiles (the last of one row), frames % 8 != 0
         ("8x8x64",   8, 8, 64),      # the per-XCD mapping (frames % 8 == 0)
         # more tiles than blocks on a device of 256 compute units (bph = ceil(CUs / 2 F) blocks walk a frame's tiles): the patch
         # prefetch and the tile switch, with and without the per-XCD mapping
         ("1x36x500", 1, 36, 500),    # 144 tiles on 128 blocks per channel half
         ("8x20x130", 8, 20, 130)]    # 25 tiles on 16 blocks, a two-pixel last column tile


def _parts(H, W):
    return 4 * ((H + 3) // 4) * ((W + 31) // 32)


def _operands(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(F, H, W, 64, generator=g)
    w = torch.randn(64, 3, 3, 64, generator=g) / 24.0
    b = torch.randn(64, generator=g)
    mean = torch.randn(F, 64, generator=g) * 0.5
    rstd = 0.5 + torch.rand(F, 64, generator=g)
    return x.to(DEV), w.to(DEV), b.to(DEV), torch.stack([mean, rstd], -1).to(DEV)


def _run_r(x, w, b, nrm):
    """one call of the kernel under test, map and partials inside poisoned buffers -> (map, partials), both cloned"""
    from pips_amd import ops
    F, H, W, _ = x.shape
    n_out, parts = F * H * W * 64, _parts(H, W)
    big = torch.full((n_out + 2 * GUARD * 64,), POISON, device=DEV)
    out = big[GUARD * 64: GUARD * 64 + n_out].view(F, H, W, 64)
    n_st = F * parts * 64 * 4
    sbig = torch.full((GUARD * 256 + F * (parts + GUARD) * 256,), POISON, device=DEV)
    stats = sbig[GUARD * 256:].view(F, parts + GUARD, 64, 4)
    got, st = ops.conv_nhwc_f32_r(x, w, b, in_norm=nrm, out=out, stats=stats)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and st.shape == (F, parts, 64, 4)
    assert bool((big[:GUARD * 64] == POISON).all()) and bool((big[GUARD * 64 + n_out:] == POISON).all()), "written outside the map"
    assert bool((sbig[:GUARD * 256] == POISON).all()) and bool((sbig[GUARD * 256 + n_st:] == POISON).all()), \
        "written outside the reported parts"
    assert not bool((got == POISON).any()) and not bool((st == POISON).any()), "map or partials not wholly written"
    return got.clone(), st.clone()


def _stat_err(mr, out):
    """largest error of {mean, rstd} (F, 64, 2) against fp64 values of the map: (absolute of the mean, relative of rstd)"""
    o = out.double().flatten(1, 2)
    mean64, var64 = o.mean(1), o.var(1, unbiased=False)
    rstd64 = 1.0 / torch.sqrt(var64 + 1e-5)
    return (float((mr[..., 0].double() - mean64).abs().max()), float(((mr[..., 1].double() - rstd64).abs() / rstd64).max()))


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "in_norm"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitwise_igemm_statistics_containment(case, norm):
    from pips_amd import ops
    cid, F, H, W = case
    x, w, b, nrm = _operands(F, H, W, 900 + H + W)
    runs = [("content", x)]
    if norm:
        nrm[..., 0] = torch.where(nrm[..., 0] > 0, -nrm[..., 0], nrm[..., 0]) - 0.125       # mean < 0: the padding probe's condition
        runs.append(("zero map", torch.zeros_like(x)))
    for tag, xin in runs:
        staged = ops.inorm_apply(xin, nrm) if norm else xin
        if norm and tag == "zero map":
            assert bool((staged > 0).all())
        ref, st_i = ops.conv_nhwc(staged, w, b, 3, 1, 1, want_stats=True, route="igemm")
        out, st = _run_r(xin, w, b, nrm if norm else None)
        assert st.shape[1] == _parts(H, W)
        assert torch.equal(out, ref), f"{cid} {tag}: map differs from igemm_f32_kernel's, max {float((out - ref).abs().max()):.3e}"
        out2, st2 = _run_r(xin, w, b, nrm if norm else None)
        assert torch.equal(out, out2) and torch.equal(st, st2), f"{cid} {tag}: two runs differ"
        # pixel counts: every image row of a tile's columns once, nothing for the rows below the image
        n = st[..., 3]
        assert bool((n.sum(1) == H * W).all()) and float(n.max()) == min(32, W)
        e_r = _stat_err(ops.inorm_finalize(st), out)
        e_i = _stat_err(ops.inorm_finalize(st_i), out)
        print(f"{cid} {tag}: |mean err| new {e_r[0]:.3e} igemm {e_i[0]:.3e}; rstd rel err new {e_r[1]:.3e} igemm {e_i[1]:.3e}")
        assert e_r[0] <= 1.5 * e_i[0] and e_r[1] <= 1.5 * e_i[1], f"{cid} {tag}: statistics {e_r} against igemm's {e_i}"


def test_unsupported_shapes_are_refused():
    from pips_amd import _lib, ops
    lib = _lib.load()
    x, w, b, _ = _operands(1, 8, 40, 5)
    out = torch.full((1, 8, 40, 64), POISON, device=DEV)
    stats = torch.full((1, _parts(8, 40), 64, 4), POISON, device=DEV)
    tiles = _lib.C.c_int(0)

    def call(xx, Cin, k, s, p, cap=stats.shape[1]):
        rc = lib.pips_conv_nhwc_f32_r(_lib.ptr(xx), None, 1, 8, 40, Cin, _lib.ptr(w), _lib.ptr(b), 64, k, s, p, _lib.ptr(out),
                                      _lib.ptr(stats), cap, _lib.C.byref(tiles), ops._stream())
        torch.cuda.synchronize()
        return rc
    x96 = torch.zeros(1, 8, 40, 96, device=DEV)
    assert call(x96, 96, 3, 1, 1) == E_ARG                   # Cin != 64
    assert call(x, 64, 3, 2, 1) == E_ARG                     # stride 2
    assert call(x, 64, 1, 1, 0) == E_ARG                     # 1x1
    assert call(x, 64, 3, 1, 1, cap=_parts(8, 40) - 1) == E_ARG      # no room for the parts
    assert bool((out == POISON).all()) and bool((stats == POISON).all()), "a refused call wrote"
    assert call(x, 64, 3, 1, 1) == 0 and tiles.value == _parts(8, 40)


def test_inorm_apply_mode3_fp32():
    """relu(relu(n2(res)) + relu(n(x))) at 2 x 5 x 7 x 64: the same fp32 operations in the same order as mode 0 on each operand
    followed by relu(a + b)"""
    from pips_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, 7, 64, generator=g).to(DEV)
    res = (torch.randn(2, 5, 7, 64, generator=g) * 3 + 1).to(DEV)
    st = torch.stack([torch.randn(2, 64, generator=g), 0.5 + torch.rand(2, 64, generator=g)], -1).to(DEV)
    rst = torch.stack([torch.randn(2, 64, generator=g), 0.5 + torch.rand(2, 64, generator=g)], -1).to(DEV)
    got = ops.inorm_apply(x, st, res, rst, mode=3)
    want = torch.relu(ops.inorm_apply(x, st) + ops.inorm_apply(res, rst))
    assert torch.equal(got, want)
    assert not torch.equal(got, ops.inorm_apply(x, st, res, rst, mode=2))      # the ReLU on the shortcut term is not a no-op here
    # modes 0..2 of the fp32 entry point are pips_inorm_apply's; its refusals come ahead of any launch
    from pips_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    y = torch.full_like(x, -7.25e18)
    for mode, r_, rs_ in ((0, None, None), (1, res, None), (2, res, rst)):
        assert lib.pips_inorm_apply_f32(p(x), p(st), p(r_), p(rs_), mode, p(y), 2, 35, 64, ops._stream()) == 0
        assert torch.equal(y, ops.inorm_apply(x, st, r_, rs_, mode=mode))
    y.fill_(-7.25e18)
    for args in ((p(x), p(st), p(res), None, 3, p(y), 2, 35, 64), (p(x), p(st), None, p(rst), 3, p(y), 2, 35, 64),
                 (p(x), p(st), p(res), p(rst), 4, p(y), 2, 35, 64), (p(x), p(st), p(res), p(rst), 3, p(y), 2, 35, 62),
                 (None, p(st), p(res), p(rst), 3, p(y), 2, 35, 64), (p(x), p(st), p(res), p(rst), 3, p(y), 0, 35, 64)):
        assert lib.pips_inorm_apply_f32(*args, ops._stream()) == E_ARG
    torch.cuda.synchronize()
    assert bool((y == -7.25e18).all())
