"""CPU proofs of the gates of tests/test_gather_probes_gpu.py (builders, reference and bound: tests/golden/gather_probes.py): the
twin geometry is the reference project's sampler, the kernels' formula meets the bound with headroom, the reference project's own
fp32 path meets it, the probes are not vacuous, and twelve stated wrong implementations fail -- five of which the older gate
(max |got - fp64 oracle| < 5e-5, 1e-4 on the bf16 routes, unit-Gaussian data at 17 x 24) lets through.

Measured here (printed by the tests):
  * kernel-formula emulation: error / bound 0.019 .. 0.081 on every family, shape, mode and summation variant (gate 0.5).
  * position allowance of oracle.corr_sample in float32, impulse maps of 33 x 40 at integer and quarter-pixel positions over the
    whole map: 2.60 / 2.02 / 1.09 / 0.55 ulp32 of the position per level; at positions of 4 pixels and more 1.55 / 2.26 / 1.09 /
    0.37 (K_POS = 4).  On the probes' own positions, which include uniform ones near 0, the same path needs 3.7.  The excess is
    at small positions and is the sampler's formulation, not a kernel's: each of its 49 taps runs the fp32 chain
    2c/(size-1) - 1 + 1 on its own, whose rounding is 2^-24 (size - 1) / 2 pixels whatever ix is -- 5 ulp32(1) on a 40-wide map --
    while a kernel has one geometry per row and level, the twin's.  So K_POS stays 4, the gate of the kernels has no such term,
    and the comparisons with the sampler below add gather_probes.chain_slack: with it the fp32 path sits at 0.09 .. 0.43 of the
    bound at K_POS = 2, and the twin at 0.14 .. 0.52 of the position terms against the fp64 sampler.
"""
import functools

import pytest
import torch

import gather_probes as P

SHAPES = {"S1": P.S1, "S2": P.S2}


def _oracle(levels, ffeats, coords, B, S, dtype):
    """oracle.pips_oracle.corr_sample on the probes' layouts -> (M, 196) particle-major"""
    from oracle import pips_oracle as O
    pyr = [lv.reshape(B, S, *lv.shape[1:]).permute(0, 1, 4, 2, 3).to(dtype) for lv in levels]
    ff = P._to_frames(ffeats, B, S)
    N = ff.shape[1]
    out = O.corr_sample(pyr, ff.reshape(B, S, N, 128).to(dtype), P._to_frames(coords, B, S).reshape(B, S, N, 2).to(dtype))
    return P._to_rows(out.reshape(B * S, N, 196), B, S)


@functools.lru_cache(maxsize=None)
def _case(family, shape_id, S=8):
    return P.case(family, P.WIN if shape_id == "WIN" else SHAPES[shape_id], S)


@functools.lru_cache(maxsize=None)
def _ref(family, shape_id, bf16=False, S=8):
    """computed once per (family, shape, mode) and left unchanged"""
    return P.reference(*P.args(_case(family, shape_id, S)), bf16=bf16)


CASES = [(f, s, 8) for s in SHAPES for f in ("A", "A'", "B")] + [("C", "S1", 8)] + [(f, "WIN", S) for S in (5, 12) for f in ("A", "B")]
CASE_IDS = [f"{f}-{s}-S{S}" for f, s, S in CASES]


# ============================================================================================ the reference
@pytest.mark.parametrize("family,shape_id", [("A", "S1"), ("B", "S1"), ("A", "S2"), ("B", "S2")])
def test_twin_equals_fp64_oracle(family, shape_id):
    """The fp64 reference on the twin's fp32 positions equals oracle.corr_sample in fp64 (positions in fp64, every tap normalised on
    its own) to within the POSITION terms alone: one ulp32 of the position (the twin's last product), one chain term, no summation
    term beyond fp64's own (1e-6 of it).  A transcription error in the twin moves a position by far more.  Measured 0.14 .. 0.52."""
    c, r = _case(family, shape_id), _ref(family, shape_id)
    q, bad0 = P.ratios(_oracle(*P.args(c), torch.float64), r, k_pos=1.0, slack=1.0, sum_term=1e-6)
    print(f"twin against the fp64 oracle, {family} {shape_id}: error / position terms per level {[round(float(x), 3) for x in q]}")
    assert int(bad0.sum()) == 0 and float(q.max()) <= 1.0


def test_twin_transcription_error_shows():
    """the same comparison fails for a twin whose positions are 2^-12 pixels off in x: the allowance is tight enough to see it"""
    c = _case("B", "S1")
    r = P.reference(c["levels"], c["ffeats"], c["coords"] + torch.tensor([2.0 ** -12, 0.0]), c["B"], c["S"])
    q, _ = P.ratios(_oracle(*P.args(c), torch.float64), r, k_pos=1.0, slack=1.0, sum_term=1e-6)
    assert float(q.max()) > 1.0


def test_reference_fp32_path_measures_k_pos():
    """oracle.corr_sample in float32 on impulse maps of 33 x 40 at integer and quarter-pixel positions over the whole map: the ulp32
    of position it needs.  Measured 2.60 / 2.02 / 1.09 / 0.55 per level -- the 2.60 at positions below 4 pixels, where the chain's
    rounding (2^-24 (size - 1) / 2 pixels whatever ix is: module docstring) exceeds an ulp32 of the position; from 4 pixels on
    1.55 / 2.26 / 1.09 / 0.37 (asserted <= 2.5: K_POS = 4 is not raised).  Beside one chain term, which is the sampler's own and no
    kernel's, the path needs no ulp32 of position at all (asserted <= 2.5 too)."""
    B, N, H8, W8 = P.S1
    g = torch.Generator().manual_seed(0)
    M = B * N * 8
    co = torch.stack([torch.randint(0, 4 * W8, (M,), generator=g), torch.randint(0, 4 * H8, (M,), generator=g)], 1).float() / 4
    c = dict(_case("A", "S1"), coords=co)
    r = P.reference(*P.args(c))
    o32 = _oracle(*P.args(c), torch.float32)
    raw, need = P.position_ulps(o32, r), P.position_ulps(o32, r, slack=1.0)
    c4 = dict(c, coords=co.clamp_min(4.0))
    far = P.position_ulps(_oracle(*P.args(c4), torch.float32), P.reference(*P.args(c4)))
    print(f"fp32 path of the oracle, impulse maps 33 x 40, integer and quarter-pixel positions: ulp32 of position needed per level "
          f"{[round(float(x), 3) for x in raw]}, at positions of 4 pixels and more {[round(float(x), 3) for x in far]}, beside one chain "
          f"term {[round(float(x), 3) for x in need]} (K_POS = {P.K_POS})")
    assert float(need.max()) <= 2.5 and float(far.max()) <= 2.5
    assert float(raw.max()) >= 0.5                                                 # (the measurement measures something)


@pytest.mark.parametrize("family,shape_id", [("A", "S1"), ("B", "S1"), ("A", "S2"), ("B", "S2")])
def test_reference_fp32_path_passes(family, shape_id):
    """oracle.corr_sample in float32 passes families A and B on the probes' own positions at HALF the kernels' K_POS plus one
    chain term (each of its taps runs the chain on its own: module docstring).  Measured 0.09 .. 0.43."""
    c, r = _case(family, shape_id), _ref(family, shape_id)
    o32 = _oracle(*P.args(c), torch.float32)
    q, bad0 = P.ratios(o32, r, k_pos=P.K_POS / 2, slack=1.0)
    print(f"fp32 oracle, {family} {shape_id}: error / bound per level {[round(float(x), 3) for x in q]}; ulp32 of position it would need "
          f"without the chain term {[round(float(x), 2) for x in P.position_ulps(o32, r)]}")
    assert int(bad0.sum()) == 0 and float(q.max()) <= 1.0


# ============================================================================================ the emulation meets the gate
MODE_CASES = [(f, s, S, bf) for f, s, S in CASES for bf in (False, True) if bf or f != "A'"]       # family A': the bf16 routes only


@pytest.mark.parametrize("fold", [False, True], ids=["div", "fold"])
@pytest.mark.parametrize("family,shape_id,S,bf16", MODE_CASES, ids=[f"{f}-{s}-S{S}-{'bf16' if bf else 'fp32'}" for f, s, S, bf in MODE_CASES])
def test_emulation_passes_with_headroom(family, shape_id, S, bf16, fold):
    """the kernels' formula in fp32 (dots, / sqrtf(128) or the reciprocal folded into the weights, the four-term blend) is within
    HALF the bound on every element, and +0.0 where the bound is 0: the other half is the kernels' other summation orders.
    Measured 0.019 .. 0.081."""
    c, r = _case(family, shape_id, S), _ref(family, shape_id, bf16, S)
    q, bad0 = P.ratios(P.emulate(*P.args(c), bf16=bf16, fold=fold), r)
    print(f"emulation {family} {shape_id} S={S} {'bf16' if bf16 else 'fp32'} {'fold' if fold else 'div'}: error / bound per level "
          f"{[round(float(x), 3) for x in q]}")
    assert int(bad0.sum()) == 0 and float(q.max()) <= 0.5


def test_rescaling_by_powers_of_two_is_exact_in_the_formula():
    """family B2 on the emulation: maps * 2^t[c] with features * 2^-t[c] give the same bits, maps * 2^7 exactly 2^7 times them"""
    c = _case("B", "S2")
    t = P.channel_shift(9)
    for bf16 in (False, True):
        base = P.emulate(*P.args(c), bf16=bf16, fold=True)
        moved = P.emulate([lv * 2.0 ** t for lv in c["levels"]], c["ffeats"] * 2.0 ** -t, c["coords"], c["B"], c["S"], bf16=bf16, fold=True)
        up = P.emulate([lv * 128.0 for lv in c["levels"]], c["ffeats"], c["coords"], c["B"], c["S"], bf16=bf16, fold=True)
        assert torch.equal(up, base * 128.0)
        # (a CPU matrix product may order its sum by the data's alignment, not its values: the same bits or the gate's distance)
        assert torch.equal(moved, base) or float(P.ratios(moved, _ref("B", "S2", bf16))[0].max()) <= 0.5


# ============================================================================================ the probes are not vacuous
def test_probes_are_not_vacuous():
    """Per level and shape at least 20 % of the judged taps have a non-zero reference, and at least 30 % of family A's taps at S1 are
    bound-0 exact zeros (measured 32 % over the four levels: 24 / 30 / 31 / 42 %; non-zero 36 / 33 / 31 / 25 %).  The one level that
    cannot: level 3 of S2 and of the 17 x 24 maps is 2 x 3 pixels, a pitch-3 lattice puts ONE impulse there, which 4 of the 49 taps
    touch; family A is held to 5 % there, family B (every pixel set: at most 12 of 49) to 20 %."""
    for family, shape_id, S in CASES:
        nz, z = P.census(_ref(family, shape_id, family == "A'", S))
        print(f"{family} {shape_id} S={S}: non-zero reference per level {[round(float(x), 3) for x in nz]}, bound-0 zeros "
              f"{[round(float(x), 3) for x in z]} (all levels {float(z.mean()):.3f})")
        tiny = shape_id != "S1" and family in ("A", "A'")
        for l in range(4):
            assert float(nz[l]) >= (0.05 if tiny and l == 3 else 0.20), (family, shape_id, l)
        if family == "A" and shape_id == "S1":
            assert float(z.mean()) >= 0.30 and float(z.min()) >= 0.20
    # the impulses use every channel, the ladder reaches its counts
    lv0 = _case("A", "S1")["levels"][0]
    assert bool((lv0 != 0).any(dim=0).any(dim=0).any(dim=0).all())
    assert int((lv0 != 0).sum(dim=-1).max()) == 1
    c = _case("C", "S1")
    geo = P.geometry(c["coords"], P.level_sizes(33, 40))
    _, key = P.sort_order(geo, P.level_sizes(33, 40), 1, 8)
    tiles_x = 3
    for s, k in enumerate(P.LADDER):
        tile = key[s] // 16
        assert int((tile == 1 * tiles_x + 1).sum()) == k and int((tile == 0).sum()) == 200 - k
        assert len(set((key[s][tile == 0] % 16).tolist())) == min(16, 200 - k)


# ============================================================================================ mutants
MUTANT_FAMILIES = {"tap_order": ("A", "B"), "swap_weights": ("A", "B"), "anchor_l2": ("A", "B"), "no_scale_l3": ("A", "B"),
                   "replicate_border": ("A",), "leak_east": ("A",), "leak_frame": ("A",), "leak_particle": ("A",), "offset_1e-6": ("B",),
                   "feat_truncate": ("A'",), "feat_ties_away": ("A'",), "feat_fp32": ("A'", "B")}
BF16_MUTANTS = ("feat_truncate", "feat_ties_away", "feat_fp32")


@pytest.mark.parametrize("shape_id", list(SHAPES))
@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_mutant_fails_its_family(mutant, shape_id):
    """each wrong implementation, applied to the emulation, misses the gate of each family named for it on at least one element
    (the feature-rounding mutants on the bf16 mode, the others on both modes)"""
    assert set(MUTANT_FAMILIES) == set(P.MUTANTS)
    for family in MUTANT_FAMILIES[mutant]:
        for bf16 in ((True,) if mutant in BF16_MUTANTS else (False, True)):
            c, r = _case(family, shape_id), _ref(family, shape_id, bf16)
            for fold in (False, True):
                q, bad0 = P.ratios(P.emulate(*P.args(c), bf16=bf16, fold=fold, mutant=mutant), r)
                print(f"{mutant} on {family} {shape_id} {'bf16' if bf16 else 'fp32'} {'fold' if fold else 'div'}: error / bound per level "
                      f"{['%.3g' % float(x) for x in q]}, wrong exact zeros {bad0.tolist()}")
                assert float(q.max()) > 1.0, (mutant, family, bf16, fold)


@functools.lru_cache(maxsize=None)
def _old_data():
    """unit-Gaussian maps and features at 17 x 24 with a POOLED pyramid, positions uniform over the map plus a unit Gaussian: the
    data of test_kernels_gpu._random_state (its seed, 5), and the fp64 oracle the present gate compares with.  A float32 normal
    deviate sits on a bf16 tie when its low 16 bits are 0x8000: once in 65 536 draws.  These 32 768 features hold none (asserted), as
    most draws of this size do; with one, the ties-away mutant moves a correlation by up to 2^-7 |f m| / sqrt(128) and the present
    gate sees it or not by the luck of the seed."""
    from oracle import pips_oracle as O
    B, S, N, H8, W8 = 1, 8, 32, 17, 24
    g = torch.Generator().manual_seed(5)
    fmaps = torch.randn(B, S, 128, H8, W8, generator=g)
    ffeats = torch.randn(B, S, N, 128, generator=g)
    coords = torch.rand(B, S, N, 2, generator=g) * torch.tensor([W8 - 1.0, H8 - 1.0]) + torch.randn(B, S, N, 2, generator=g)
    assert int((ffeats.view(torch.int32) & 0xFFFF == 0x8000).sum()) == 0
    pyr = O.build_pyramid(fmaps)
    levels = [p.reshape(B * S, 128, *p.shape[-2:]).permute(0, 2, 3, 1).contiguous() for p in pyr]
    c = dict(levels=levels, ffeats=P._to_rows(ffeats.reshape(B * S, N, 128), B, S), coords=P._to_rows(coords.reshape(B * S, N, 2), B, S),
             B=B, S=S)
    ref = {bf: _oracle([lv.bfloat16() for lv in levels] if bf else levels, c["ffeats"].bfloat16() if bf else c["ffeats"], c["coords"],
                       B, S, torch.float64) for bf in (False, True)}
    return c, ref


@pytest.mark.parametrize("mutant", ["leak_east", "leak_frame", "leak_particle", "offset_1e-6", "feat_ties_away"])
def test_the_present_gate_lets_the_mutant_through(mutant):
    """The gap, written down: on the present data the mutant stays inside the present gate (max |got - fp64 oracle| < 5e-5 on the fp32
    routes, 1e-4 on the bf16 ones) -- a 2^-20 leak moves unit-Gaussian correlations by ~3e-6, random features never sit on a bf16
    tie -- while test_mutant_fails_its_family shows the same mutant missing the new gate."""
    c, ref = _old_data()
    for bf16 in ((True,) if mutant in BF16_MUTANTS else (False, True)):
        gate = 1e-4 if bf16 else 5e-5
        for fold in (False, True):
            clean = float((P.emulate(*P.args(c), bf16=bf16, fold=fold).double() - ref[bf16]).abs().max())
            got = P.emulate(*P.args(c), bf16=bf16, fold=fold, mutant=mutant)
            err = float((got.double() - ref[bf16]).abs().max())
            moved = float((got - P.emulate(*P.args(c), bf16=bf16, fold=fold)).abs().max())
            print(f"{mutant} {'bf16' if bf16 else 'fp32'} {'fold' if fold else 'div'}: {err:.2e} from the fp64 oracle (unmutated {clean:.2e}, "
                  f"gate {gate:.0e}); the mutant moved the result by {moved:.2e}")
            assert clean < gate and err < gate
            if mutant != "feat_ties_away":
                assert moved > 0                                                   # (the mutant is there; no random feature sits on a tie)
