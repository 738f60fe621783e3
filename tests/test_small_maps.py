"""CPU: why the library refuses a feature map below 16 x 16, stated by the oracle alone.

The correlation sampler normalises a level's coordinates with ``2 x / (W - 1) - 1`` (nets/pips.py:318-319).  A map with
8 <= H8 < 16 or 8 <= W8 < 16 has a coarsest pyramid level one pixel wide or high: the division is by zero, every tap of that level
is NaN, and the model turns that into NaN positions behind frame 0 and NaN visibilities.  The library therefore accepts a map for
sampling only when all four levels are at least 2 x 2 (H8, W8 >= 16; tests/test_small_maps_gpu.py holds it to that).  Here: the
NaN pattern at the illegal sizes, finiteness at the smallest legal ones, and the table of far-out coordinates -- exactly zero in
every correlation column -- that the GPU tests of the gather routes take as their contract."""
import pytest
import torch

from oracle import pips_oracle as O

ILLEGAL = [(8, 12), (15, 15), (16, 9)]                       # levels 3: 1x1, 1x1, 2x1
LEGAL = [(16, 16), (16, 31), (31, 16), (17, 16)]             # the smallest, and odd sizes around it in either dimension
# coordinates far outside any map, in map pixels: beyond the +-20000 clamp of the tiled gather's window anchors, across its 16-bit
# packing of the anchors (+-70000; 262144 = 2^18; 65541 = 2^16 + 5, which a wrapped anchor would put at x = 5, inside the map),
# beyond its +-1e6 clamp ahead of the int conversion, beyond int32, and up to 1e30 (2 x must stay finite in fp32)
FAR = [(-1e4, 3.0), (5.0, 1e4), (1e6, 1e6), (-1e9, 2.0), (3.0, 1e9), (1e15, -1e15), (1e30, 1e30), (-1e30, 4.0),
       (70000.0, 5.0), (-70000.0, 5.0), (262144.0, 3.0), (65541.0, 5.0)]
DTYPES = [torch.float32, torch.float64]


def _state(H8, W8, N, seed, dtype):
    """(pyramid, ffeats (1,8,N,128), coords (1,8,N,2) inside the map) of random maps"""
    g = torch.Generator().manual_seed(seed)
    fmaps = torch.randn(1, 8, 128, H8, W8, generator=g).to(dtype)
    ffeats = torch.randn(1, 8, N, 128, generator=g).to(dtype)
    coords = (torch.rand(1, 8, N, 2, generator=g) * torch.tensor([W8 - 1.0, H8 - 1.0])).to(dtype)
    return O.build_pyramid(fmaps), ffeats, coords


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("H8,W8", ILLEGAL)
def test_a_one_pixel_level_is_all_nan(H8, W8, dtype):
    """24 rows inside the map: the 49 columns of every level with a dimension of 1 are NaN in every row, all others finite"""
    pyr, ffeats, coords = _state(H8, W8, 3, H8 * W8, dtype)
    sizes = [tuple(p.shape[-2:]) for p in pyr]
    assert sizes[0] == (H8, W8) and min(sizes[3]) == 1 and min(sizes[2]) >= 2
    out = O.corr_sample(pyr, ffeats, coords).reshape(24, 4, 49)
    nan = out.isnan()
    assert int(nan[:, :3].sum()) == 0 and int(nan[:, 3].sum()) == 24 * 49            # 1176 of 1176
    assert bool(torch.isfinite(out[:, :3]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("H8,W8", LEGAL)
def test_the_smallest_legal_maps_are_finite(H8, W8, dtype):
    pyr, ffeats, coords = _state(H8, W8, 3, H8 * W8, dtype)
    assert min(pyr[3].shape[-2:]) == 2
    out = O.corr_sample(pyr, ffeats, coords)
    assert tuple(out.shape) == (1, 8, 3, 196) and bool(torch.isfinite(out).all())
    assert float(out.abs().max()) > 1.0                                              # (windows inside the map: real correlations)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("H8,W8", LEGAL)
def test_far_out_coordinates_give_exact_zeros(H8, W8, dtype):
    """every coordinate of FAR, in each of the 8 frames: all 196 correlation columns are exactly zero (zeros padding: no tap of a
    window that far out touches the map), never NaN, never a wrapped-around sample"""
    pyr, ffeats, _ = _state(H8, W8, len(FAR), 7, dtype)
    coords = torch.tensor(FAR, dtype=dtype).view(1, 1, len(FAR), 2).repeat(1, 8, 1, 1)
    assert bool(torch.isfinite(2 * coords).all())
    out = O.corr_sample(pyr, ffeats, coords)
    assert torch.equal(out, torch.zeros(1, 8, len(FAR), 196, dtype=dtype))


@pytest.mark.parametrize("H8,W8", ILLEGAL)
def test_dense_score_maps_are_finite_below_the_rule(H8, W8):
    """why pips_score_map_prepare keeps its 8 x 8 limit: the dense score maps upsample the levels (align_corners=True) and divide by
    no size - 1 of a level; a one-pixel level is a constant map"""
    pyr, ffeats, _ = _state(H8, W8, 3, 11, torch.float32)
    out = O.dense_score_maps(pyr, ffeats)
    assert tuple(out.shape) == (1, 8, 3, H8, W8) and bool(torch.isfinite(out).all())


def test_forward_is_nan_below_the_rule_and_finite_at_it(weights_tamed):
    """O.forward on tamed weights, two in-frame queries: at 64 x 96 (an 8 x 12 map) every position behind frame 0 and every
    visibility logit is NaN; at 128 x 128 (16 x 16) nothing is"""
    g = torch.Generator().manual_seed(3)
    for (H, W), bad in (((64, 96), True), ((128, 128), False)):
        rgbs = torch.randint(0, 256, (1, 8, 3, H, W), generator=g).float()
        xys = torch.rand(1, 2, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0
        preds, _, vis, _ = O.forward(weights_tamed, xys, rgbs, iters=2, stride=8)
        last = preds[-1]                                                             # (1,8,2,2)
        assert bool(torch.isfinite(last[:, 0]).all())                                # frame 0 is the query itself
        if bad:
            assert bool(last[:, 1:].isnan().all()) and bool(vis.isnan().all())
        else:
            assert all(bool(torch.isfinite(p).all()) for p in preds) and bool(torch.isfinite(vis).all())
