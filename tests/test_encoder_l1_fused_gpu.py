"""The whole exact-fp32 encoder on both sides of the layer-1 route (api.hip: enc_front_f32): at the smallest 8-frame size that
ops.encoder_l1_fused() says takes the LDS-resident 64 -> 64 kernel on this device -- the four layer-1 convolutions normalise their
input while staging it, three normalised half-resolution maps are never stored, block 1 closes with inorm_apply mode 3 -- and at a
size it says is not taken, where the staged sequence runs as before.

Yardsticks are those of tests/test_kernels_gpu.py, restated: the CPU oracle's pyramid at 2e-4 per level (test_encoder_pyramid, its
frame generator), and for a low-variance frame (test_encoder_low_variance_frames' low_contrast kind, here the last of the eight
frames) the oracle's own fp32 error against its fp64 run, times 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STRIDE = 8


def _sizes():
    """(H, W) by area: multiples of 32 from 64 x 96 up"""
    c = [(h, w) for h in range(64, 513, 32) for w in range(96, 1025, 32) if h <= w <= 2 * h]
    return sorted(c, key=lambda s: (s[0] * s[1], s))


def _check(H, W, weights_raw, arenas):
    from oracle import pips_oracle as O
    from pips_amd import ops
    g = torch.Generator().manual_seed(3)
    rgbs = torch.randint(0, 256, (8, 3, H, W), generator=g).float()
    rgbs[7] = (200 + torch.randint(-2, 3, (3, H, W), generator=g)).float()           # |mean| >> std in every channel
    x = 2 * (rgbs / 255.0) - 1.0
    fm = O.encoder(weights_raw, x, STRIDE)
    pyr_ref = O.build_pyramid(fm.unsqueeze(0))
    pyr = ops.encoder_fwd(arenas["raw"], rgbs.to(DEV), STRIDE)
    torch.cuda.synchronize()
    levels = ops.pyramid_levels(pyr, 8, H, W, STRIDE)
    for l, (got, ref) in enumerate(zip(levels, pyr_ref)):
        ref = ref[0].permute(0, 2, 3, 1)
        assert tuple(got.shape) == tuple(ref.shape)
        err = float((got.cpu()[:7] - ref[:7]).abs().max())
        print(f"{H}x{W} level {l}: max |err| {err:.2e}")
        assert err < 2e-4, f"level {l}: {err}"
    ref64 = O.encoder(O.to_dtype(weights_raw, torch.float64), x[7:8].double(), STRIDE)
    floor = float((fm[7:8].double() - ref64).abs().max())
    err = float((levels[0].cpu()[7:8].permute(0, 3, 1, 2).double() - ref64).abs().max())
    print(f"{H}x{W} low-variance frame: HIP vs fp64 {err:.2e}, fp32 reference arithmetic vs fp64 {floor:.2e}")
    assert err < 4 * floor + 1e-5


def test_fused_layer1(weights_raw, arenas):
    from pips_amd import ops
    size = next((s for s in _sizes() if ops.encoder_l1_fused(8, *s)), None)
    assert size is not None, "no size up to 512 x 1024 takes the fused layer-1 path on this device"
    print(f"fused layer 1 from {size[0]} x {size[1]} on {ops._lib.load().pips_device_cus()} compute units")
    _check(size[0], size[1], weights_raw, arenas)


def test_staged_layer1_below_the_threshold(weights_raw, arenas):
    from pips_amd import ops
    size = next((s for s in reversed(_sizes()) if not ops.encoder_l1_fused(8, *s) and s[0] * s[1] <= 128 * 192), None)
    assert size is not None, "every size from 64 x 96 up takes the fused layer-1 path on this device"
    print(f"staged layer 1 at {size[0]} x {size[1]}")
    _check(size[0], size[1], weights_raw, arenas)
