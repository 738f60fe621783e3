"""GPU: the stage and end-to-end parity tests again on TRAINED-LIKE weights (cases.trained_like_state_dict).

pips_amd.weights.init_state_dict starts all 26 affine normalisation pairs at weight = 1, bias = 0, and `x * 1 + 0` hides a
dropped `+ beta`, a `gamma` of the wrong layer, a swapped pair and a permuted channel map alike.  The code that reads those
pairs -- three token-mixing kernels with three different lane-to-channel maps, three final-LayerNorm kernels, two state-update
kernels and the arena packing -- is reached by the rest of the suite with identity affines only.  Here every pair and every
channel is different, and tests/test_oracle_golden.py::test_trained_like_weights_have_teeth shows that no single tensor is
invisible at the inputs used below (the least visible one moves the mixer output by 210x the fp32 gate).

Every comparison is against the CPU oracle on the same dict: in fp64 where the gate is fp32-grade, under
torch.autocast(bfloat16) where the test it mirrors does that.  The gates are those of the tests mirrored (named per test).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_PX = 1e-3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MATMUL = ["exact", "split"]


def _oracle():
    from oracle import pips_oracle as O
    return O


# ------------------------------------------------------------------ module-scoped weights, arenas and oracle results
@pytest.fixture(scope="module")
def sd_raw():
    return G.trained_like_state_dict(0, tamed=False)


@pytest.fixture(scope="module")
def sd_tamed():
    return G.trained_like_state_dict(0, tamed=True)


@pytest.fixture(scope="module")
def arena_raw(sd_raw):
    from pips_amd import ops
    return ops.pack_weights(sd_raw, torch.device(DEV))


@pytest.fixture(scope="module")
def mixer_refs(sd_raw):
    """P -> (x, fp64 oracle, fp32 oracle, autocast oracle or None) on G.mixer_rows(P); each computed once"""
    O = _oracle()
    sd64 = O.to_dtype(sd_raw, torch.float64)
    cache = {}

    def get(P, autocast=False):
        if P not in cache:
            x = G.mixer_rows(P)
            cache[P] = [x, O.mixer(sd64, x.double()), O.mixer(sd_raw, x), None]
        if autocast and cache[P][3] is None:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                cache[P][3] = O.mixer(sd_raw, cache[P][0]).float()
        return cache[P]
    return get


def _pad(x):
    """(P, S, 519) -> the mixer's zero-padded input rows (P*S, 544) on the device"""
    P, S, _ = x.shape
    X = torch.zeros(P * S, 544)
    X[:, :519] = x.reshape(P * S, 519)
    return X.to(DEV)


def _pm(t):
    """(B,S,N,X) -> particle-major (B*N*S, X)."""
    B, S, N, X = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N * S, X).contiguous()


def _model(sd, stride=8, matmul="exact", S=8):
    from pips_amd import Pips
    m = Pips(S=S, stride=stride)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.matmul = matmul
    return m.to(DEV).eval()


def _run(m, xys, rgbs, iters=6):
    out = m(xys.to(DEV), rgbs.to(DEV), iters=iters, return_feat=True)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ mixer, S = 8
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("P", [4, 32, 256, 2048])
def test_mixer(P, split, arena_raw, mixer_refs):
    """tests/test_kernels_gpu.py::test_mixer (token_mix_kernel, ln_mean_kernel) with its gate, against the fp64 oracle."""
    from pips_amd import ops
    x, ref, _, _ = mixer_refs(P)
    out = ops.mixer_fwd(arena_raw, _pad(x), split=split).cpu()
    scale = max(1.0, float(ref.abs().max()))
    e = float((out.double() - ref).abs().max())
    print(f"trained-like mixer P={P} split={split}: err {e:.2e}, gate {1e-4 * scale:.2e}")
    assert e < 1e-4 * scale


@pytest.mark.parametrize("P", [32, 256, 2046, 2048])
def test_mixer_bf16_operands(P, arena_raw, mixer_refs):
    """bf16=True with the fp32 residual stream: token_mix_mfma_kernel<false> (channels g*128 + 4*(lane & 31) + q) and
    ln_mean_kernel<false>.  2048 particles fill the grid; 2046 leave the last block two waves short (`p >= particles` inside a
    block).  Gates of test_mixer_bf16_operands, and the HIP result may be no further from the autocast oracle than
    1.5x the autocast oracle's own distance from the fp32 oracle + 5e-3 (the relative gate of test_mixer_bf16_residual_stream).
    Measured HIP vs autocast oracle / autocast oracle vs fp32 oracle: 0.92x / 0.89x / 0.98x / 0.95x at P = 32 / 256 / 2046 / 2048
    (8.7e-3 .. 1.05e-2 against 9.4e-3 .. 1.13e-2 of the output scale; 4.4e-3 .. 5.8e-3 from the fp64 oracle)."""
    from pips_amd import ops
    x, ref64, ref32, refbf = mixer_refs(P, autocast=True)
    out = ops.mixer_fwd(arena_raw, _pad(x), bf16=True).cpu()
    out32 = ops.mixer_fwd(arena_raw, _pad(x)).cpu()
    scale = max(1.0, float(ref64.abs().max()))
    e = lambda u, v: float((u.double() - v.double()).abs().max()) / scale
    e_f32, e_bf16, e_hip, e_ref = e(out32, ref64), e(out, ref64), e(out, refbf), e(refbf, ref32)
    print(f"trained-like P={P}: bf16-operand mixer rel err {e_bf16:.2e} (fp32 path {e_f32:.2e}); vs autocast oracle {e_hip:.2e}, "
          f"autocast oracle vs fp32 oracle {e_ref:.2e}, ratio {e_hip / e_ref:.2f}")
    assert torch.isfinite(out).all() and tuple(out.shape) == (P, 1040)
    assert e_f32 < 1e-4
    assert 1e-5 < e_bf16 < 3e-2
    assert e_hip <= 1.5 * e_ref + 5e-3


@pytest.mark.parametrize("P", [256, 2046, 2048])
def test_mixer_bf16_residual_stream(P, arena_raw, mixer_refs):
    """stream_bf16=True: token_mix_mfma_kernel<true> and ln_mean_wave_kernel (a lane holds channels 8*lane .. 8*lane + 7).
    Gates of test_mixer_bf16_residual_stream.
    Measured bf16 stream / fp32 stream distance to the autocast oracle: 1.18x / 1.25x / 1.18x at P = 256 / 2046 / 2048
    (1.2e-2 .. 1.3e-2 against 1.0e-2; 9.6e-3 .. 1.1e-2 from the fp32 oracle)."""
    from pips_amd import ops
    x, ref64, ref32, refbf = mixer_refs(P, autocast=True)
    a = ops.mixer_fwd(arena_raw, _pad(x), bf16=True).cpu()
    b = ops.mixer_fwd(arena_raw, _pad(x), bf16=True, stream_bf16=True).cpu()
    scale = max(1.0, float(ref32.abs().max()))
    e = lambda u, v: float((u - v).abs().max()) / scale
    print(f"trained-like bf16 mixer P={P}: fp32 stream vs autocast oracle {e(a, refbf):.2e}, bf16 stream vs autocast oracle {e(b, refbf):.2e} "
          f"(ratio {e(b, refbf) / e(a, refbf):.2f}); vs fp32 oracle {e(a, ref32):.2e} / {e(b, ref32):.2e}; autocast oracle vs fp32 oracle "
          f"{e(refbf, ref32):.2e}; the two forms {e(a, b):.2e}")
    assert torch.isfinite(b).all()
    assert e(b, refbf) < 1.5 * e(a, refbf) + 5e-3 and e(b, ref32) < 3e-2


# ------------------------------------------------------------------ mixer, any window length
@pytest.mark.parametrize("S,P", [(1, 5), (3, 64), (5, 33), (12, 40), (16, 7), (24, 9)])
def test_mixer_any_window_length(S, P):
    """token_mix_any_kernel<SMAX, bf16> / ln_mean_any_kernel<SMAX> on a trained-like Pips(S): gates of
    test_mixer_any_window_length; S = 24 is the SMAX = 32 instantiation, which the identity-affine stage test never reaches."""
    from pips_amd import ops
    O = _oracle()
    sd = G.trained_like_state_dict(0, S=S)
    arena = ops.pack_weights(sd, torch.device(DEV), S=S)
    x = G.mixer_rows(P, S=S, seed=100 * S + P)
    ref = O.mixer(O.to_dtype(sd, torch.float64), x.double())
    assert tuple(ref.shape) == (P, S * 130)
    scale = max(1.0, float(ref.abs().max()))
    for split in (False, True):
        out = ops.mixer_fwd(arena, _pad(x), split=split, S=S).cpu()
        e = float((out.double() - ref).abs().max()) / scale
        print(f"trained-like S={S} P={P} split={split}: rel err {e:.2e}")
        assert tuple(out.shape) == (P, S * 130) and e < 1e-4
    lo = ops.mixer_fwd(arena, _pad(x), bf16=True, S=S).cpu()
    e = float((lo.double() - ref).abs().max()) / scale
    print(f"trained-like S={S} P={P} bf16: rel err {e:.2e}")
    assert 1e-6 < e < 3e-2


# ------------------------------------------------------------------ state update
@pytest.mark.parametrize("want_vis", [True, False])
@pytest.mark.parametrize("B,N", [(2, 19), (1, 1), (1, 257)])
def test_state_update(B, N, want_vis, sd_raw, arena_raw):
    """test_state_update with a GroupNorm pair that is not (1, 0); a single row, and one row past a multiple of 256."""
    from pips_amd import ops
    O = _oracle()
    sd64 = O.to_dtype(sd_raw, torch.float64)
    ffeats, coords, coords0, delta = G.state_update_inputs(B, N)
    ff_ref, co_ref = O.update_step(sd64, ffeats.double(), coords.double(), coords0.double(), delta.double())
    vis_ref = F.linear(ff_ref.reshape(-1, 128), sd64["vis_predictor.0.weight"], sd64["vis_predictor.0.bias"]).reshape(B, 8, N)
    ff = _pm(ffeats).to(DEV)
    co = _pm(coords).to(DEV)
    traj, vis = ops.state_update(arena_raw, delta.reshape(B * N, 1040).to(DEV), ff, co, _pm(coords0).to(DEV), B, N, 8.0,
                                 want_vis=want_vis)
    e_ff = float((ff.cpu().double() - _pm(ff_ref)).abs().max())
    e_co = float((co.cpu().double() - _pm(co_ref)).abs().max())
    print(f"trained-like state update B*N={B * N} want_vis={want_vis}: |dffeat| {e_ff:.2e} (|ffeat| {float(ff_ref.abs().max()):.1f}), |dcoord| {e_co:.2e}")
    assert e_ff < 2e-5
    assert e_co < 1e-5
    assert float((traj.cpu().double() - co_ref * 8.0).abs().max()) < 1e-4
    if want_vis:
        assert float((vis.cpu().double() - vis_ref).abs().max()) < 2e-5
    else:
        assert vis is None
    assert torch.equal(traj.cpu()[:, 0], (coords0 * 8.0)[:, 0])                         # frame 0 locked


# ------------------------------------------------------------------ teacher-forced iterations
@pytest.mark.parametrize("matmul", MATMUL)
def test_teacher_forced_iterations_raw_weights(matmul, sd_raw, arena_raw):
    """test_teacher_forced_iterations_raw_weights on the trained-like raw dict: each iteration recomputed by the HIP stages
    from the fp64 oracle's input state, so a wrong `norm.*` in the update shows at the iteration it happens."""
    from pips_amd import ops
    O = _oracle()
    case = dict(B=1, N=32, H=128, W=160, stride=8, iters=4, tamed=False, border=True)
    xys, rgbs, _, _ = G.make_inputs(case)
    taps = {}
    O.forward(O.to_dtype(sd_raw, torch.float64), xys.double(), rgbs.double(), iters=case["iters"], stride=8, taps=taps)
    B, N, H8, W8 = 1, case["N"], 16, 20
    split = matmul == "split"
    pyr = ops.encoder_fwd(arena_raw, rgbs.reshape(8, 3, 128, 160).to(DEV), 8, split=split)
    pm = lambda t: t.permute(0, 2, 1, 3).reshape(B * N * 8, -1).contiguous()
    coords0 = pm(taps["iters"][0]["coords_in"]).float().to(DEV)
    for i, it in enumerate(taps["iters"]):
        ff, co = pm(it["ffeats_in"]).float().to(DEV), pm(it["coords_in"]).float().to(DEV)
        X = ops.mixer_input_build(pyr, B, H8, W8, ff, co)
        delta = ops.mixer_fwd(arena_raw, X, split=split)
        traj, _ = ops.state_update(arena_raw, delta, ff, co, coords0, B, N, 8.0)
        err = float((traj.cpu().double() - it["coords_out"] * 8.0).abs().max())
        ferr = float((ff.cpu().double() - pm(it["ffeats_out"])).abs().max())
        print(f"trained-like teacher-forced ({matmul}) iteration {i + 1}: max |dtraj| = {err:.2e} px, max |dffeat| = {ferr:.2e}")
        assert err < TOL_PX
        assert ferr < 1e-3


# ------------------------------------------------------------------ full forward, tamed trained-like dict
BORDER_CASE = dict(B=1, N=16, H=128, W=160, stride=8, iters=6, tamed=True, border=True)
CONFIG2_CASE = dict(B=1, N=256, H=368, W=496, stride=8, iters=6, tamed=True)      # BASELINE config 2 geometry


@pytest.fixture(scope="module")
def forward_oracles(sd_tamed):
    """name -> (xys, rgbs, fp64 oracle forward); the config-2 sized one is the expensive part of this module"""
    O = _oracle()
    sd64 = O.to_dtype(sd_tamed, torch.float64)
    cache = {}

    def get(name):
        if name not in cache:
            case = {"border": BORDER_CASE, "config2": CONFIG2_CASE}[name]
            xys, rgbs = G.make_inputs(case)[:2]
            cache[name] = (xys, rgbs, O.forward(sd64, xys.double(), rgbs.double(), iters=case["iters"], stride=case["stride"]))
        return cache[name]
    return get


@pytest.mark.parametrize("matmul", MATMUL)
@pytest.mark.parametrize("name", ["border", "config2"])
def test_forward_against_oracle_tamed(name, matmul, sd_tamed, forward_oracles):
    """test_config2_against_oracle_tamed, and the same on 16 queries with border cases, on the tamed trained-like dict."""
    xys, rgbs, (ref_p, ref_p2, ref_vis, ref_ff) = forward_oracles(name)
    preds, preds2, vis, ffeat, _ = _run(_model(sd_tamed, 8, matmul), xys, rgbs, iters=6)
    err = [float((a.cpu().double() - b).abs().max()) for a, b in zip(preds, ref_p)]
    e_vis, e_ff = float((vis.cpu().double() - ref_vis).abs().max()), float((ffeat.cpu().double() - ref_ff).abs().max())
    print(f"trained-like forward {name} ({matmul}) per-iteration max |dtraj| px:", ["%.2e" % e for e in err], f"vis {e_vis:.2e} ffeat {e_ff:.2e}",
          "max displacement px %.2f" % float((ref_p[-1] - ref_p2[0]).abs().max()))
    assert len(preds) == 6 and max(err) < TOL_PX
    assert e_vis < TOL_PX
    assert e_ff < 2e-4
    for a, b in zip(preds2, ref_p2):
        assert float((a.cpu().double() - b).abs().max()) < TOL_PX


@pytest.mark.parametrize("stream", ["fp32_stream", "bf16_stream"])
@pytest.mark.parametrize("name", ["border", "config2"])
def test_forward_bf16_mode_tamed(name, stream, sd_tamed, forward_oracles):
    """mixer_dtype = encoder_dtype = bfloat16 (both residual-stream forms): the 2e-2 px gate tests/test_config3_gpu.py holds
    the bf16 forward to against the fp32 result."""
    xys, rgbs, (ref_p, _, ref_vis, _) = forward_oracles(name)
    m = _model(sd_tamed, 8)
    m.mixer_dtype = m.encoder_dtype = torch.bfloat16
    m.mixer_stream_dtype = torch.float32 if stream == "fp32_stream" else torch.bfloat16
    preds, _, vis, _, _ = _run(m, xys, rgbs, iters=6)
    err = [float((a.cpu().double() - b).abs().max()) for a, b in zip(preds, ref_p)]
    print(f"trained-like bf16 forward {name} ({stream}) per-iteration max |dtraj| px vs fp64 oracle:", ["%.2e" % e for e in err],
          "vis logits %.2e" % float((vis.cpu().double() - ref_vis).abs().max()))
    assert all(torch.isfinite(p).all() for p in preds) and torch.isfinite(vis).all()
    assert 1e-5 < max(err) < 2e-2


@pytest.mark.parametrize("matmul", MATMUL)
@pytest.mark.parametrize("S", [5, 12, 24])
def test_forward_window_lengths(S, matmul):
    """Pips(S != 8) end to end on a tamed trained-like dict: state_update_any_kernel and ln_mean_any_kernel read `norm.*` / the
    final LayerNorm pair here inside a whole forward (alone: tests/test_mixer_stages_gpu.py).  Gates of
    test_golden_reference_outputs_window_lengths."""
    O = _oracle()
    case = dict(S=S, B=1, N=6, H=128, W=160, stride=8, iters=3, tamed=True, border=True)
    sd = G.trained_like_state_dict(0, S=S, tamed=True)
    xys, rgbs, _, _ = G.make_inputs(case)
    ref_p, ref_p2, ref_vis, ref_ff = O.forward(O.to_dtype(sd, torch.float64), xys.double(), rgbs.double(), iters=3, stride=8)
    preds, preds2, vis, ffeat, _ = _run(_model(sd, 8, matmul, S=S), xys, rgbs, iters=3)
    assert tuple(preds[0].shape) == (1, S, 6, 2) and tuple(vis.shape) == (1, S, 6)
    err = [float((a.cpu().double() - b).abs().max()) for a, b in zip(preds, ref_p)]
    e_vis = float((vis.cpu().double() - ref_vis).abs().max())
    print(f"trained-like S={S} forward ({matmul}) per-iteration max |dtraj| px:", ["%.2e" % e for e in err], f"vis {e_vis:.2e}")
    assert float((preds2[0].cpu().double() - ref_p2[0]).abs().max()) < 1e-5
    assert float((ffeat.cpu().double() - ref_ff).abs().max()) < 2e-4
    assert max(err) < TOL_PX
    assert e_vis < TOL_PX


# ------------------------------------------------------------------ goldens of the unmodified reference
@pytest.mark.parametrize("matmul", MATMUL)
@pytest.mark.parametrize("name", list(G.TRAINED_CASES))
def test_golden_reference_outputs(name, matmul):
    """cases.TRAINED_CASES against the vectors of the unmodified reference (make_golden.py --trained): gates of
    test_golden_reference_outputs, and the three losses of the S = 8 case at 2e-4."""
    case = G.TRAINED_CASES[name]
    S = case.get("S", 8)
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    sd = G.case_state_dict(case)
    xys, rgbs, _, _ = G.make_inputs(case)
    m = _model(sd, case["stride"], matmul, S=S)
    preds, preds2, vis, ffeat, losses = _run(m, xys, rgbs, iters=case["iters"])
    assert losses is None and len(preds) == case["iters"] and len(preds2) == case["iters"] + 4
    trajs = torch.stack(preds).cpu().numpy()
    assert trajs.shape == gold["trajs"].shape and trajs.shape[2] == S
    err = np.abs(trajs - gold["trajs"]).reshape(case["iters"], -1).max(axis=1)
    print(name, matmul, "per-iteration max |dtraj| px:", err)
    assert np.abs(preds2[0].cpu().numpy() - gold["traj0"]).max() < 1e-5
    assert np.abs(ffeat.cpu().numpy() - gold["ffeat"]).max() < 2e-4
    assert err.max() < TOL_PX, err
    assert np.abs(vis.cpu().numpy() - gold["vis"]).max() < TOL_PX
    if os.path.exists(os.path.join(GOLD, name + "_losses.npz")):
        lg = np.load(os.path.join(GOLD, name + "_losses.npz"))
        tg, vg, va = G.make_targets(case)
        out = m(xys.to(DEV), rgbs.to(DEV), iters=case["iters"], trajs_g=tg.to(DEV), vis_g=vg.to(DEV), valids=va.to(DEV))
        for got, key in zip(out[3], ("seq_loss", "vis_loss", "ce_loss")):
            print(name, matmul, key, float(got), float(lg[key]))
            assert abs(float(got) - float(lg[key])) <= 2e-4 * abs(float(lg[key])), key


# ------------------------------------------------------------------ offset residual stream
def _offset_refs(sd_raw, c, autocast):
    O = _oracle()
    sd = dict(sd_raw)
    sd["delta_block.to_delta.0.bias"] = sd_raw["delta_block.to_delta.0.bias"] + c
    x = G.mixer_rows(32)
    ref64, ref32 = O.mixer(O.to_dtype(sd, torch.float64), x.double()), O.mixer(sd, x)
    refbf = None
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            refbf = O.mixer(sd, x).float()
    return sd, x, ref64, ref32, refbf


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("c", [0.0, 8.0, 32.0, 128.0])
def test_mixer_offset_residual_stream(c, split, sd_raw):
    """The mixer's analogue of test_encoder_low_variance_frames: the input projection's bias shifted by c, so that every token
    row enters layer 1 -- and, through the residual adds, every later LayerNorm -- with |mean| >> std, where a sum /
    sum-of-squares variance loses its digits.  Yardstick: the oracle's own fp32 error against its fp64 run at the same c
    (5.8e-7, 1.3e-6, 4.5e-6, 1.7e-5 of the output scale at c = 0, 8, 32, 128); the HIP mixer stays within 4x of it + 1e-5.
    Measured HIP / yardstick at c = 0 / 8 / 32 / 128: exact 1.40x / 1.02x / 0.80x / 0.94x, split 1.02x / 0.91x / 0.83x / 0.85x."""
    from pips_amd import ops
    sd, x, ref64, ref32, _ = _offset_refs(sd_raw, c, False)
    arena = ops.pack_weights(sd, torch.device(DEV))
    out = ops.mixer_fwd(arena, _pad(x), split=split).cpu()
    scale = max(1.0, float(ref64.abs().max()))
    floor = float((ref32.double() - ref64).abs().max()) / scale
    err = float((out.double() - ref64).abs().max()) / scale
    print(f"offset c={c:g} split={split}: HIP vs fp64 {err:.2e}, fp32 oracle vs fp64 {floor:.2e}, ratio {err / floor:.2f}x, |out| {scale:.2f}")
    assert err < 4 * floor + 1e-5


@pytest.mark.parametrize("c", [0.0, 8.0])
def test_mixer_offset_residual_stream_bf16_operands(c, sd_raw):
    """The same for token_mix_mfma_kernel, whose LayerNorm statistics are ONE pass (sum, sum of squares).  Only c = 0 and 8:
    beyond that the reference under autocast is itself lost (autocast oracle vs fp32 oracle 9.8e-3, 7.2e-2, 2.7e-1, 7.1e-1 at
    c = 0, 8, 32, 128) and nothing can be decided.  Gate: HIP vs autocast oracle <= 1.5 x (autocast oracle vs fp32 oracle) + 5e-3.
    Measured HIP / yardstick: 0.92x / 0.98x at c = 0 / 8 (8.7e-3 against 9.4e-3, 7.0e-2 against 7.1e-2); the HIP mixer itself stays
    4.4e-3 / 4.7e-3 from the fp64 oracle -- its fp32 LayerNorm does not lose what the autocast reference loses at c = 8."""
    from pips_amd import ops
    sd, x, ref64, ref32, refbf = _offset_refs(sd_raw, c, True)
    arena = ops.pack_weights(sd, torch.device(DEV))
    out = ops.mixer_fwd(arena, _pad(x), bf16=True).cpu()
    scale = max(1.0, float(ref64.abs().max()))
    e_hip = float((out - refbf).abs().max()) / scale
    e_ref = float((refbf - ref32).abs().max()) / scale
    print(f"offset c={c:g} bf16 operands: HIP vs autocast oracle {e_hip:.2e}, autocast oracle vs fp32 oracle {e_ref:.2e}, ratio {e_hip / e_ref:.2f}x; "
          f"HIP vs fp64 oracle {float((out.double() - ref64).abs().max()) / scale:.2e}")
    assert torch.isfinite(out).all()
    assert e_hip <= 1.5 * e_ref + 5e-3
