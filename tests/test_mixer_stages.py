"""CPU: the references and bounds of tests/golden/mixer_stages.py, proven before the GPU tests rely on them
(tests/test_mixer_stages_gpu.py).  Each bound must pass a correct fp32 implementation of its stage in two summation orders
(sequential and pairwise; with bf16-rounded operands for the matrix-core contract), and must bite.  Planted, each missing a
bound by more than 10x: the statistics of token t' applied to token t (every pair), the LayerNorm scale and shift of layer
d + 1 used in layer d, and the one-pass variance on rows whose mean is 256 stds from zero."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cases as G
import mixer_stages as M

ORDERS = ("seq", "pair")
FAMILIES = (("centred", 0.0), ("shifted", M.R), ("shifted", 4 * M.R), ("hot", 0.0))


@pytest.fixture(scope="module")
def sds():
    return {S: G.trained_like_state_dict(0, S=S) for S in (5, 8)}


def _oracle():
    from oracle import pips_oracle as O
    return O


def test_shift_range_is_the_oracles(weights_raw):
    """M.R against the oracle: the largest per-row |mean| / std over the 25 LayerNorm inputs of the fp64 mixer on
    cases.mixer_rows(64) with the init weights is the largest figure of the provenance note (1.4223)"""
    O = _oracle()
    taps = {}
    O.mixer(O.to_dtype(weights_raw, torch.float64), G.mixer_rows(64).double(), taps)
    assert len(taps["ln_in"]) == 25
    r = max(float((x.mean(-1).abs() / x.std(-1, unbiased=False)).max()) for x in taps["ln_in"])
    print(f"largest |mean|/std over 25 LayerNorm inputs: {r:.4f} (R = {M.R})")
    assert 0.98 * M.R <= r <= M.R
    assert M.SHIFTS == (0.0, M.R, 4 * M.R) and M.SHIFT_PROBE == 64.0


def test_token_rows_are_what_they_say():
    for S in (1, 5, 8, 32):
        for fam, r in FAMILIES + (("shifted", 64.0),):
            x = M.token_rows(3, S, fam, r).double()
            m, s = x.mean(-1), x.std(-1, unbiased=False)
            if fam != "hot":
                assert torch.allclose(s, M.token_scales(S).expand(3, S), rtol=1e-5)
                assert torch.allclose(m / s, (r + M.token_means(S)).expand(3, S), atol=1e-5 * max(1.0, r))
            else:
                assert bool((x.abs().amax(-1) == 60 * M.token_scales(S)).all())
    # every token differs from every other in scale or in mean by at least 0.02 stds
    for S in (5, 8, 12, 32):
        sc, mu = M.token_scales(S), M.token_means(S)
        for t in range(S):
            for t2 in range(t + 1, S):
                assert sc[t] != sc[t2] or abs(float(mu[t] - mu[t2])) >= 0.099


@pytest.mark.parametrize("S,P", [(8, 2), (5, 2)])
def test_bounds_pass_fp32_emulations(S, P, sds):
    """token mixing (fp32 and the bf16 contract, the fast GELU's allowance in both directions), LayerNorm 2, the final
    LayerNorm + mean: fp32 arithmetic in either order stays inside the bounds on every family"""
    sd = sds[S]
    worst_seen = {}
    for layer in (0, 11):
        w = M.mix_weights(sd, layer)
        for fam, r in FAMILIES:
            x = M.token_rows(P, S, fam, r)
            y, by = M.token_mix_ref(x, w)
            yb, bb = M.token_mix_ref(x, w, bf16=True)
            for order in ORDERS:
                got = M.token_mix32(x, w, order)
                worst_seen["x' fp32"] = max(worst_seen.get("x' fp32", 0), M.worst((got.double() - y).abs(), by))
                for shift in (-M.GELU_BF16OUT_ABS, 0.0, M.GELU_BF16OUT_ABS):
                    gb = M.token_mix32(x, w, order, bf16=True, gelu_shift=shift)
                    worst_seen["x' bf16"] = max(worst_seen.get("x' bf16", 0), M.worst((gb.double() - yb).abs(), bb))
                    stored = gb.bfloat16()
                    worst_seen["x' bf16 stored"] = max(worst_seen.get("x' bf16 stored", 0),
                                                       M.worst((stored.double() - yb).abs(), M.stored_bf16_bound(yb, bb)))
                ref, gate = M.ln_ref(got, w["g2"], w["b2"])
                n2 = M.ln32(got, w["g2"], w["b2"], order)
                worst_seen["xn"] = max(worst_seen.get("xn", 0), M.worst((n2.double() - ref).abs(), gate))
                worst_seen["xn bf16"] = max(worst_seen.get("xn bf16", 0),
                                            M.worst((n2.bfloat16().double() - ref).abs(), M.stored_bf16_bound(ref, gate)))
                g, b = M.final_ln(sd)
                ref, gate = M.ln_mean_ref(x, g, b)
                lm = M.sum32(M.ln32(x, g, b, order).transpose(1, 2), order) * (1.0 / S)
                worst_seen["ln_mean"] = max(worst_seen.get("ln_mean", 0), M.worst((lm.double() - ref).abs(), gate))
    print(f"S={S}: worst error / bound of the fp32 emulations: " + ", ".join(f"{k} {v:.2f}" for k, v in worst_seen.items()))
    assert all(v <= 1.0 for v in worst_seen.values()), worst_seen


def test_bf16_bound_is_the_plain_one_away_from_ties(sds):
    """the tie allowance is per operand: most outputs see none, and there the bound is the plain sum-of-products bound plus
    the fast GELU's allowance through sum |w3|"""
    w = M.mix_weights(sds[8], 5)
    x = M.token_rows(4, 8, "centred")
    _, bb = M.token_mix_ref(x, w, bf16=True)
    plain = float(bb.median())
    frac = float((bb > 4 * plain).double().mean())
    print(f"bf16 token-mix bound: median {plain:.2e}, {frac:.1%} of the outputs carry a tie allowance")
    assert plain < 1e-4 and frac < 0.35


@pytest.mark.parametrize("S", [8, 5])
def test_token_swap_misses_every_bound(S, sds):
    """statistics of token t' used for token t, for every pair: the fp32 bounds are missed by more than 100x, the bf16 ones
    (which carry the rounding allowances) by more than 10x, on every row"""
    sd = sds[S]
    w = M.mix_weights(sd, 5)
    g, b = M.final_ln(sd)
    for fam, r in (("centred", 0.0), ("shifted", M.R)):
        x = M.token_rows(2, S, fam, r)
        y, by = M.token_mix_ref(x, w)
        yb, bb = M.token_mix_ref(x, w, bf16=True)
        n2, gate2 = M.ln_ref(x, w["g2"], w["b2"])
        lm, gate_lm = M.ln_mean_ref(x, g, b)
        m, rs = M.ln_stats32(x, "pair")
        lows = []
        for k in range(1, S):                                     # token t takes the statistics of token (t + k) % S
            st = (m.roll(-k, 1), rs.roll(-k, 1))
            per_row = lambda err, bound: (err / bound).amax(-1)
            e32 = per_row((M.token_mix32(x, w, "pair", stats1=st).double() - y).abs(), by)
            eb = per_row((M.token_mix32(x, w, "pair", bf16=True, stats1=st).double() - yb).abs(), bb)
            e2 = per_row((M.ln32(x, w["g2"], w["b2"], "pair", stats=st).double() - n2).abs(), gate2)
            e2b = per_row((M.ln32(x, w["g2"], w["b2"], "pair", stats=st).bfloat16().double() - n2).abs(), M.stored_bf16_bound(n2, gate2))
            elm = ((M.ln32(x, g, b, "pair", stats=st).double().mean(1) - lm).abs() / gate_lm).amax(-1)
            # a swap of LayerNorm 1 moves every token's output through w3; rows are judged one by one all the same
            assert float(e32.min()) > 100 and float(e2.min()) > 100 and float(elm.min()) > 100, (fam, k)
            assert float(eb.min()) > 10 and float(e2b.min()) > 10, (fam, k)
            lows.append((float(e32.min()), float(eb.min()), float(e2.min()), float(e2b.min()), float(elm.min())))
        print(f"S={S} {fam}: least miss over all pairs and rows (x' fp32, x' bf16, xn, xn bf16, ln_mean): "
              + ", ".join(f"{min(v[i] for v in lows):.0f}x" for i in range(5)))


def test_affine_of_the_next_layer_misses_the_bounds(sds):
    sd = sds[8]
    x = M.token_rows(2, 8, "centred")
    for layer in (0, 5):
        w, w_next = M.mix_weights(sd, layer), M.mix_weights(sd, layer + 1)
        y, by = M.token_mix_ref(x, w)
        yb, bb = M.token_mix_ref(x, w, bf16=True)
        wrong1 = dict(w, g1=w_next["g1"], b1=w_next["b1"])
        assert M.worst((M.token_mix32(x, wrong1, "pair").double() - y).abs(), by) > 10
        assert M.worst((M.token_mix32(x, wrong1, "pair", bf16=True).double() - yb).abs(), bb) > 10
        ref, gate = M.ln_ref(x, w["g2"], w["b2"])
        wrong2 = M.ln32(x, w_next["g2"], w_next["b2"], "pair")
        assert M.worst((wrong2.double() - ref).abs(), gate) > 10
        assert M.worst((wrong2.bfloat16().double() - ref).abs(), M.stored_bf16_bound(ref, gate)) > 10


def test_one_pass_variance(sds):
    """The one-pass statistics of token_mix_mfma_kernel in fp32 emulation, pre-rounding error of the normalised values as a
    fraction of the bf16 half-ulp of the row's largest value and of the yardstick gate, per shift and order.  Summed
    pairwise the one-pass form sits at 1.43 of the gate at 4R and 0.27 of the half-ulp at 64 (3.8 at 256), summed one by one at
    12.7 and 1.5 (24 at 256); the kernel's own order (fused squares, 8-term chains, then a tree) is measured on the device.  At 256
    stds it misses the gate by more than 10x in either order (79x / 428x); the two-pass form passes everywhere (<= 0.66)."""
    w = M.mix_weights(sds[8], 5)
    for r in M.SHIFTS + (M.SHIFT_PROBE, 256.0):
        x = M.token_rows(16, 8, "shifted", r)
        ref, gate = M.ln_ref(x, w["g2"], w["b2"])
        half = M.row_half_ulp(ref)
        out = {}
        for one_pass in (False, True):
            errs = [(M.ln32(x, w["g2"], w["b2"], order, one_pass=one_pass).double() - ref).abs() for order in ORDERS]
            out[one_pass] = ([M.worst(e, gate) for e in errs], [float((e / half).max()) for e in errs])
        print(f"shifted({r:g}) seq/pair: two-pass {out[False][0][0]:.2f}/{out[False][0][1]:.2f} of the gate, "
              f"{out[False][1][0]:.1e}/{out[False][1][1]:.1e} of a bf16 half-ulp; one-pass {out[True][0][0]:.2f}/{out[True][0][1]:.2f} of "
              f"the gate, {out[True][1][0]:.1e}/{out[True][1][1]:.1e} of a half-ulp")
        assert max(out[False][0]) <= 1.0
        if r == 256.0:
            assert min(out[True][0]) > 10


def test_references_chain_to_the_oracle_mixer(sds):
    """twelve token_mix_ref steps, the channel mixing between them in plain fp64, ln_mean_ref and the head equal O.mixer"""
    O = _oracle()
    sd = sds[8]
    sd64 = O.to_dtype(sd, torch.float64)
    x0 = G.mixer_rows(3).double()
    ref = O.mixer(sd64, x0)
    x = F.linear(x0, sd64[f"{M.MD}.0.weight"], sd64[f"{M.MD}.0.bias"])
    for d in range(12):
        w = M.mix_weights(sd, d)
        x, _ = M.token_mix_ref(x, w)
        h = M.ln64(x, w["g2"], w["b2"])
        h = F.gelu(F.linear(h, sd64[f"{M.MD}.{d + 1}.1.fn.0.weight"], sd64[f"{M.MD}.{d + 1}.1.fn.0.bias"]))
        x = x + F.linear(h, sd64[f"{M.MD}.{d + 1}.1.fn.3.weight"], sd64[f"{M.MD}.{d + 1}.1.fn.3.bias"])
    pooled, _ = M.ln_mean_ref(x, *M.final_ln(sd))
    out = F.linear(pooled, sd64[f"{M.MD}.15.weight"], sd64[f"{M.MD}.15.bias"])
    assert float((out - ref).abs().max()) < 1e-11 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("S,B,N", [(8, 2, 3), (5, 1, 2), (12, 1, 1)])
def test_update_reference_is_the_oracles(S, B, N):
    O = _oracle()
    sd = G.trained_like_state_dict(0, S=S)
    sd64 = O.to_dtype(sd, torch.float64)
    delta, ff, co, co0 = M.update_inputs(B, N, S)
    assert delta.shape[1] == M.delta_stride(S)
    out = M.update_ref(sd, delta, ff, co, co0, S, 4.0)
    d = delta[:, :S * 130].reshape(B * N, S, 130).double()
    ff_o, co_o = O.update_step(sd64, M.to_bsn(ff, B, N).double(), M.to_bsn(co, B, N).double(), M.to_bsn(co0, B, N).double(), d)
    vis_o = F.linear(ff_o.reshape(-1, 128), sd64["vis_predictor.0.weight"], sd64["vis_predictor.0.bias"]).reshape(B, S, N)
    assert float((M.to_bsn(out["ffeats"][0], B, N) - ff_o).abs().max()) < 1e-12
    assert float((M.to_bsn(out["coords"][0], B, N) - co_o).abs().max()) < 1e-12
    assert float((M.to_bsn(out["vis"][0], B, N) - vis_o).abs().max()) < 1e-12
    # the bounds pass the operation in torch's fp32 and bite on a neighbouring token's statistics
    ff32, co32 = O.update_step(sd, M.to_bsn(ff, B, N), M.to_bsn(co, B, N), M.to_bsn(co0, B, N), d.float())
    assert M.worst((ff32.double() - M.to_bsn(out["ffeats"][0], B, N)).abs(), M.to_bsn(out["ffeats"][1], B, N)) <= 1.0
    assert M.worst((co32.double() - M.to_bsn(out["coords"][0], B, N)).abs(), M.to_bsn(out["coords"][1], B, N)) <= 1.0
    if S > 1:
        df = d[:, :, 2:]                                          # the row's own values with the neighbour's mean and std
        m, s = df.mean(-1, keepdim=True).roll(1, 1), df.std(-1, unbiased=False, keepdim=True).roll(1, 1)
        hn = (df - m) / torch.sqrt(s * s + 1e-5) * sd64["norm.weight"] + sd64["norm.bias"]
        wrong = F.gelu(F.linear(hn, sd64["ffeat_updater.0.weight"], sd64["ffeat_updater.0.bias"])) + ff.double()
        ratio = ((wrong - out["ffeats"][0]).abs() / out["ffeats"][1]).amax(-1)
        assert float(ratio.min()) > 100


def test_stage_entry_points_check_their_arguments():
    """PIPS_E_ARG (-1) ahead of any launch: no device is touched, so this runs without one"""
    from pips_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    BF, ST = 2, 64
    ok_tm = dict(arena=p, layer=0, x=p, xn=p, particles=1, S=8, flags=0)
    bad_tm = [dict(arena=None), dict(x=None), dict(xn=None), dict(particles=0), dict(S=0), dict(S=33), dict(layer=-1), dict(layer=12),
              dict(flags=ST), dict(flags=BF | ST, S=5), dict(flags=16), dict(flags=BF | 4), dict(flags=1)]
    for bad in bad_tm:
        a = dict(ok_tm, **bad)
        rc = lib.pips_token_mix(a["arena"], a["layer"], a["x"], a["xn"], a["particles"], a["S"], a["flags"], None)
        assert rc == -1 and b"token_mix" in lib.pips_last_error(), bad
    ok_lm = dict(arena=p, x=p, out=p, particles=1, S=8, flags=0)
    for bad in [dict(arena=None), dict(x=None), dict(out=None), dict(particles=0), dict(S=0), dict(S=33), dict(flags=ST),
                dict(flags=BF | ST, S=12), dict(flags=16)]:
        a = dict(ok_lm, **bad)
        assert lib.pips_ln_mean(a["arena"], a["x"], a["out"], a["particles"], a["S"], a["flags"], None) == -1, bad
        assert b"ln_mean" in lib.pips_last_error()
    ok_su = dict(arena=p, delta=p, ffeats=p, coords=p, coords0=p, B=1, N=1, S=8, traj=p)
    for bad in [dict(arena=None), dict(delta=None), dict(ffeats=None), dict(coords=None), dict(coords0=None), dict(traj=None),
                dict(B=0), dict(N=0), dict(S=0), dict(S=33)]:
        a = dict(ok_su, **bad)
        assert lib.pips_state_update_s(a["arena"], a["delta"], a["ffeats"], a["coords"], a["coords0"], a["B"], a["N"], a["S"], 8.0,
                                       a["traj"], None, None) == -1, bad
        assert b"state_update" in lib.pips_last_error()
    assert lib.pips_state_update(None, p, p, p, p, 1, 1, 8.0, p, None, None) == -1
    ok_vh = dict(arena=p, ffeats=p, B=1, N=1, S=8, out=p)
    for bad in [dict(arena=None), dict(ffeats=None), dict(out=None), dict(B=0), dict(N=0), dict(S=0), dict(S=33)]:
        a = dict(ok_vh, **bad)
        assert lib.pips_vis_head(a["arena"], a["ffeats"], a["B"], a["N"], a["S"], a["out"], None) == -1, bad
        assert b"vis_head" in lib.pips_last_error()
