"""conv_f32_e.hip -- the 64 x 64 LDS-DMA convolution body -- against igemm_f32_kernel, both through ops.conv_nhwc with the
route named, and an fp64 reference computed on the CPU from the same inputs.

Frames of a case (conv_probes' families in one map each): a CONTENT frame -- unit-normal channels carrying the mixed powers of
two of conv_probes.scale_exponents, an impulse 2^9 at two opposite corner pixels -- and a LOW-VARIANCE frame -- the same
channel scales on a constant map with 1/32 of noise.  F = 2 cases hold both, F = 1 cases are called once per frame kind.  The
input sits between two guard frames of 1e30 (a tap that reads in front of or behind the image shows up in every output it
touches), the output in front of guard rows of a poison value that must survive.

Per call: the new route's largest error against fp64 is at most 1.5 x igemm_f32_kernel's on the same inputs (two equally valid
summation orders: which one lands closer depends on the input; the kernel under test is never its own yardstick); {mean, rstd}
from the encoder's own finalize kernel agree between the routes to 1e-6 / 1e-5 relative; two runs are bit-equal.

Measured on MI355X: err(new) / err(igemm) 0.31 .. 0.56 over the eight calls (largest: the low-variance frames of the two 1x1
cases), mean within 1.3e-7, rstd within 4.7e-6 (each call prints its figures)."""
import pytest
import torch

import conv_probes as P
import value_range as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -7.25e18
GUARD = 1e30

#        id               F  H   W   Cin  Cout k  s
CASES = [("3x3_s1_128",   2, 13, 19, 128, 128, 3, 1),     # 247 pixels: three full row tiles and a ragged one, every border, two column tiles
         ("3x3_s2_96",    2, 13, 19, 96, 128, 3, 2),      # odd sizes: the last row and column taps fall outside
         ("3x3_s2_64_96", 1, 12, 20, 64, 96, 3, 2),       # 96 columns: one full column tile and a half
         ("1x1_s2_96",    1, 12, 20, 96, 128, 1, 2),      # shortcut
         ("1x1_s1_256",   1, 9, 11, 256, 128, 1, 1)]      # final conv


def _frames(r, kind, g):
    a, _ = P.scale_exponents(r)
    scale = torch.exp2(a.float())
    if kind == "content":
        x = torch.randn(r.H, r.W, r.Cin, generator=g) * scale
        x[0, 0] = 0
        x[0, 0, 5 % r.Cin] = 512.0
        x[r.H - 1, r.W - 1] = 0
        x[r.H - 1, r.W - 1, r.Cin - 3] = 512.0
        return x
    return (1.0 + torch.randn(r.H, r.W, r.Cin, generator=g) / 32) * scale


def _calls(r):
    """[(tag, x (F, H, W, Cin) on the CPU)]"""
    g = torch.Generator().manual_seed(4000 + r.H + r.Cin + r.Cout + r.k)
    if r.F == 2:
        return [("content+lowvar", torch.stack([_frames(r, "content", g), _frames(r, "lowvar", g)]))]
    return [(kind, _frames(r, kind, g)[None]) for kind in ("content", "lowvar")]


def _run(r, xg, w, b, route):
    """one call on `route`: the input inside its guard frames, the output in front of its guard rows"""
    from pips_amd import ops
    Ho, Wo = P.out_hw(r)
    buf = torch.full((r.F + 2, r.H, r.W, r.Cin), GUARD, device=DEV)
    buf[1:r.F + 1] = xg
    big = torch.full((r.F * Ho * Wo + 70, r.Cout), POISON, device=DEV)
    out = big[:r.F * Ho * Wo].view(r.F, Ho, Wo, r.Cout)
    got, st = ops.conv_nhwc(buf[1:r.F + 1], w, b, r.k, r.s, r.p, want_stats=True, route=route, out=out)
    assert got.data_ptr() == big.data_ptr()
    torch.cuda.synchronize()
    assert bool((big[r.F * Ho * Wo:] == POISON).all()), f"{r.id} {route}: rows behind the last pixel were written"
    assert st.shape[1] == 2 * P.cdiv(Ho * Wo, 64), f"{r.id} {route}: {st.shape[1]} partials per frame"
    return got.clone(), st.clone(), ops.inorm_finalize(st)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_new_route_against_igemm_and_fp64(case):
    cid, F, H, W, Cin, Cout, k, s = case
    r = P._r(cid, "f32", "igemm_f32", F, H, W, Cin, Cout, k=k, s=s)
    gw = torch.Generator().manual_seed(77 + Cin + Cout + k)
    w = torch.randn(Cout, k, k, Cin, generator=gw) / (k * k * Cin) ** 0.5
    # |bias| of the order of the content frame's std (the mixed scales reach 2^6) or above: `relative` agreement of the mean is asked
    # where the mean is not itself a difference of large numbers
    b = torch.randn(Cout, generator=gw)
    b = torch.where(b < 0, -1.0, 1.0) * (64.0 + 16.0 * b.abs())
    for tag, x in _calls(r):
        ref = V.conv_ref64(x, w, b, r.k, r.s, r.p)                       # fp64 on the CPU
        xg, wg, bg = x.to(DEV), w.to(DEV), b.to(DEV)
        out_i, st_i, mr_i = _run(r, xg, wg, bg, "igemm")
        out_e, st_e, mr_e = _run(r, xg, wg, bg, "e")
        out_e2, st_e2, _ = _run(r, xg, wg, bg, "e")
        assert torch.equal(out_e, out_e2) and torch.equal(st_e, st_e2), f"{cid} {tag}: two runs differ"
        err_i = float((out_i.cpu().double() - ref).abs().max())
        err_e = float((out_e.cpu().double() - ref).abs().max())
        mean_rel = float(((mr_e[..., 0] - mr_i[..., 0]).abs() / mr_i[..., 0].abs().clamp_min(1e-30)).max())
        rstd_rel = float(((mr_e[..., 1] - mr_i[..., 1]).abs() / mr_i[..., 1].abs()).max())
        print(f"{cid} {tag}: max |err| vs fp64 new {err_e:.3e}, igemm {err_i:.3e}, ratio {err_e / max(err_i, 1e-300):.3f}; "
              f"mean rel {mean_rel:.2e}, rstd rel {rstd_rel:.2e}")
        assert err_e <= 1.5 * err_i, f"{cid} {tag}: {err_e:.3e} > 1.5 x {err_i:.3e}"
        assert mean_rel <= 1e-6 and rstd_rel <= 1e-5, f"{cid} {tag}: statistics differ between the routes"
        n = st_e[..., 3]
        assert torch.equal(n, st_i[..., 3]), f"{cid} {tag}: pixel counts of the parts differ"
