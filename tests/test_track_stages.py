"""CPU: the references and bounds of tests/golden/track_stages.py, proven before the GPU tests rely on them
(tests/test_track_stages_gpu.py).  Each bound must pass a correct fp32 implementation of its stage (the point-sample twin; the
score-map terms with sequential and pairwise sums; torch's fp32 bilinear upsample) and must bite: every listed wrong
implementation misses its gate.  Every test prints error / bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import track_stages as T


def _oracle():
    from oracle import pips_oracle as O
    return O


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ps_calls(B, S, N, H8, W8):
    """the two position sets of a shape: random ones (the shape's N), and the special ones on every clip"""
    sp = T.ps_specials(H8, W8)
    return (("random", T.ps_positions(B, N, H8, W8)), ("special", sp[None].repeat(B, 1, 1).contiguous()))


# ------------------------------------------------------------------ A. point sample
@pytest.mark.parametrize("B,S,N,H8,W8", T.PS_SHAPES)
def test_point_sample_twin_is_the_oracle_and_meets_its_bound(B, S, N, H8, W8):
    """ps_twin equals oracle.pips_oracle.point_sample in float32 bit for bit on every probe (random positions and
    ps_specials: integers, corners, clamped indices, one ulp below an integer, +-1e6, 2^24 + 1), meets 6 u sum |w| |v| against
    the fp64 blend, and returns the pixel's bits at integer positions.  Measured: no element differs; error / bound 0.29 .. 0.43."""
    O = _oracle()
    lv = T.ps_maps(B, S, H8, W8)
    fm0 = lv.reshape(B, S, H8, W8, T.C)[:, 0].permute(0, 3, 1, 2)                    # frame 0 of each clip, (B,C,H,W)
    for name, xy in _ps_calls(B, S, N, H8, W8):
        twin = T.ps_twin(lv, S, xy)
        orc = O.point_sample(fm0, xy[..., 0], xy[..., 1])
        assert orc.dtype == torch.float32
        ndiff = int((_bits(twin) != _bits(orc)).sum())
        ref, bound = T.ps_ref(lv, S, xy)
        q = T.worst((twin.double() - ref).abs(), bound)
        print(f"point sample {(B, S, N, H8, W8)} {name}: twin vs fp32 oracle {ndiff} differing elements; twin error / bound {q:.3f}")
        assert ndiff == 0 and q <= 1.0 and bool(torch.isfinite(twin).all())
        if name == "special":
            ix = xy[0, :T.PS_INTEGERS].long()
            for b in range(B):
                assert torch.equal(_bits(twin[b, :T.PS_INTEGERS]), _bits(lv[b * S, ix[:, 1], ix[:, 0]]))


def test_point_sample_wrong_implementations_miss_the_gate():
    """clamped weights, swapped w01 / w10 and frame s = 1 miss the fp64 gate by orders of magnitude.  The blend contracted into
    FMAs stays inside it on this data (an fma drops roundings: measured 0.36 of the bound) -- only the bit gate sees it (3170 of
    12288 elements differ from the twin)."""
    B, S, N, H8, W8 = T.PS_SHAPES[0]
    lv = T.ps_maps(B, S, H8, W8)
    xy = torch.cat([c for _, c in _ps_calls(B, S, N, H8, W8)], dim=1)
    twin = T.ps_twin(lv, S, xy)
    ref, bound = T.ps_ref(lv, S, xy)
    for wrong in T.PS_WRONG:
        got = T.ps_twin(lv, S, xy, wrong=wrong)
        q = T.worst((got.double() - ref).abs(), bound)
        ndiff = int((_bits(got) != _bits(twin)).sum())
        print(f"point sample, {wrong}: error / bound {q:.3g}; {ndiff} of {got.numel()} elements differ from the twin")
        assert ndiff > 0
        if wrong == "fma":
            assert q <= 1.0
        else:
            assert q > 10.0


# ------------------------------------------------------------------ B. embedding tail
@pytest.mark.parametrize("S", T.EMB_WINDOWS)
def test_embedding_reference_is_the_oracles(S):
    """embed_ref against oracle.embed3d: the same flow bits, the fp64 sin / cos of the fp32 argument within 4 u of the oracle's
    fp32 embedding wherever |arg| < 2^8 (beyond, torch's fp32 sin itself is what the yardstick measures); arg = 0 gives 0 / 1.
    The probe displacements give arguments up to 2.9e8 and every EMB_DISP value is present once S >= 8."""
    O = _oracle()
    N = 3
    co = T.embed_coords(S, N)
    tt = torch.linspace(0, S, S)
    r = T.embed_ref(co, tt, S)
    x = O.mixer_input(torch.zeros(1, S, N, 128), torch.zeros(1, S, N, 196), co.reshape(N, S, 2).transpose(0, 1)[None])
    emb = x.reshape(N * S, 519)[:, 324:]
    assert torch.equal(_bits(emb[:, 192:]), _bits(r["flow"]))
    small = r["arg"].abs() < 256
    e = float((emb[:, :192].double() - r["ref"]).abs()[small].max())
    yard = T.embed_yardstick(r)
    print(f"embedding S={S}: max |arg| {float(r['arg'].abs().max()):.3g}, {int(r['zero'].sum())} zero arguments; oracle fp32 vs reference on "
          f"|arg| < 256: {e:.2e}; torch fp32 sin / cos on the CPU vs fp64, all arguments: {yard:.2e}")
    assert e <= 4 * T.U24
    z = r["zero"]
    odd = (torch.arange(192) % 2).bool()[None, :].expand_as(z)
    assert bool((r["ref"][z & ~odd] == 0).all()) and bool((r["ref"][z & odd] == 1).all())
    if S >= 8:
        d = r["flow"][:, :2].reshape(-1)
        for v in T.EMB_DISP:
            assert bool(((d == v) & (torch.signbit(d) == (np.copysign(1.0, v) < 0))).any()), v
        assert float(r["arg"].abs().max()) > 2.5e8


# ------------------------------------------------------------------ C. score map
@pytest.mark.parametrize("Fr,H8,W8", T.UP_SHAPES[:3])
def test_upsum_bound_passes_fp32_and_bites(Fr, H8, W8):
    """U: torch's fp32 bilinear upsample of the four levels summed in fp32 stays inside the bound; U without level 3 and U with
    align_corners=False miss it.  Measured: fp32 0.025-0.051 of the bound; the wrong ones 3.6e4 and more."""
    levels = T.up_levels(Fr, H8, W8)
    ref, bound = T.upsum_ref(levels)
    acc = torch.zeros_like(levels[0])
    for lv in levels:
        acc = acc + F.interpolate(lv.permute(0, 3, 1, 2), size=(H8, W8), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    q = T.worst((acc.double() - ref).abs(), bound)
    q3 = T.worst((T.upsum_ref(levels, drop_level=3)[0] - ref).abs(), bound)
    qa = T.worst((T.upsum_ref(levels, align_corners=False)[0] - ref).abs(), bound)
    print(f"U {(Fr, H8, W8)}: fp32 torch error / bound {q:.4f}; without level 3 {q3:.3g}; align_corners=False {qa:.3g}")
    assert q <= 1.0 and q3 > 10.0 and qa > 10.0
    # frame f is 2^f times frame-0-like data: the bound scales with the frame, so a small frame is not judged by a large one
    assert float(bound[0].max()) * 2.0 ** (Fr - 1) < 4 * float(bound[Fr - 1].max())


@pytest.fixture(scope="module")
def term_results():
    """(shape, family) -> list over the target tables of (tgt, reference dict, U, ffeats); computed once"""
    cache = {}

    def get(shape, family):
        if (shape, family) not in cache:
            U, ff = T.term_case(family, *shape)
            cache[(shape, family)] = [(tgt, T.terms_ref(U, ff, tgt, *shape), U, ff) for tgt in T.term_targets(*shape, family=family)]
        return cache[(shape, family)]
    return get


@pytest.mark.parametrize("shape", T.TERM_SHAPES)
def test_terms_bound_passes_fp32_emulations(shape, term_results):
    """score_terms_kernel's formula in fp32 with sequential and with pairwise sums stays inside the per-row bounds on every
    family and target table; rows with use = 0 are +0.0.  Measured worst error / bound over the four shapes (positive,
    negative): dense 0.475, 0.002; large 0.458, 0.002; small 0.157, 0.074; impulse 0.212, 0.040."""
    for family in T.TERM_FAMILIES:
        wp = wn = 0.0
        n_off = 0
        for tgt, r, U, ff in term_results(shape, family):
            for order in ("seq", "pair"):
                got = T.terms32(U, ff, tgt, *shape, order)
                off = tgt[:, 2] == 0
                n_off += int(off.sum())
                assert torch.equal(_bits(got[off]), torch.zeros_like(_bits(got[off])))
                p, n = T.terms_worst(got, r)
                wp, wn = max(wp, p), max(wn, n)
        assert n_off > 0
        sc = T.term_scores(U, ff, *shape[:3])
        print(f"terms {shape} {family}: |score| up to {float(sc.abs().max()):.3g}; fp32 emulations error / bound: positive {wp:.3f}, negative {wn:.3f}")
        assert wp <= 1.0 and wn <= 1.0
        if family == "large":
            assert float(sc.abs().max()) > 150


def test_terms_wrong_implementations_miss_the_gate(term_results):
    """every wrong implementation of TERM_WRONG misses a gate on at least one (shape, family); printed: where, and by how much.
    frame_S8 can show only at S != 8, clip_wrong_N only with two clips, log1p_exp only where exp overflows (the large family)."""
    for wrong in T.TERM_WRONG:
        hit = []
        for shape in T.TERM_SHAPES:
            for family in T.TERM_FAMILIES:
                q = 0.0
                for tgt, r, U, ff in term_results(shape, family):
                    q = max(q, *T.terms_worst(T.terms32(U, ff, tgt, *shape, "pair", wrong=wrong), r))
                if q > 1.0:
                    hit.append((shape, family, q))
        print(f"terms, {wrong}: misses the gate on {len(hit)} of {len(T.TERM_SHAPES) * len(T.TERM_FAMILIES)} (shape, family) pairs; "
              f"largest error / bound {max((h[2] for h in hit), default=0):.3g}; e.g. {hit[:2]}")
        assert hit and max(h[2] for h in hit) > 10.0
        if wrong not in ("frame_S8", "clip_wrong_N", "log1p_exp"):         # the others show on every shape (the pitch: where H8 != W8)
            assert {h[0] for h in hit} == {s for s in T.TERM_SHAPES if wrong != "pitch_H8" or s[3] != s[4]}


def test_target_selection_is_the_oracles():
    """pips_amd.pips._score_map_targets against the selection of oracle.score_map_loss: the same used maps, the same pixel on
    every used map; positions at k + 0.5 round half to even, -0.5 is pixel 0 (-0.0 -> 0), W8 - 0.5 is outside on an even W8"""
    from pips_amd.pips import _score_map_targets
    for H8, W8, stride in ((17, 25, 8), (8, 8, 4), (16, 20, 8)):
        tg, vis, val = T.selection_probes(H8, W8, stride)
        tab = _score_map_targets(tg, vis, val, float(stride), H8, W8)
        x, y, ind = T.oracle_selection(tg / float(stride), vis, val, H8, W8)
        n = tg.shape[2]
        order = T.pm(torch.arange(3 * n).reshape(1, 3, n, 1))[:, 0]                # table row m -> (b, s, n) index
        assert torch.equal(tab[:, 2] > 0, ind[order])
        u = ind[order]
        assert torch.equal(tab[u, 0].long(), x[order][u]) and torch.equal(tab[u, 1].long(), y[order][u])
        assert bool(((tab[:, 0] >= 0) & (tab[:, 0] <= W8 - 1) & (tab[:, 1] >= 0) & (tab[:, 1] <= H8 - 1)).all())     # use = 0 rows stay in the map
        print(f"selection {H8}x{W8} stride {stride}: {int(ind.sum())} of {ind.numel()} maps used")
        assert 0 < int(ind.sum()) < ind.numel() and int(ind[2 * n:].sum()) == 0 and int(ind[n:2 * n].sum()) == 0


# ------------------------------------------------------------------ D. per-iteration wiring
def test_wiring_precondition():
    """A condition on the inputs of the GPU wiring test, not a measurement of the kernels: on at least half of the used rows the
    fp64 reference's negative term of iteration it differs from iteration it + 1's, and from iteration 0's, by at least 10 x
    the gate of test 2 (4 x the fp32 oracle's error + the stage bound).  Features taken after the update, or the first
    iteration's, then fail.  Measured: median |difference| / gate 493 .. 910 against the next iteration and 824 .. 2180 against
    iteration 0, 99-100 % of the used rows at 10 x or more; yardstick 7.9e-7 .. 2.9e-6 relative (negative), 3.9e-10 .. 1.4e-8
    absolute (positive: the fp32 formula returns 0 there); the gate is 4.8e-5 .. 8.1e-5 of the negative term on the median row,
    most of it the stage bound's share of U's resize bound."""
    w = T.wiring_refs()
    used, its = w["used"], w["its"]
    assert int(used.sum()) >= w["tgt"].shape[0] // 3
    for it, r in enumerate(its):
        print(f"iteration {it}: fp32-oracle yardstick negative {r['yard_neg_rel']:.2e} relative, positive {r['yard_pos_abs']:.2e} absolute; "
              f"gate / term, median used row: {float((r['gate_neg'] / r['neg'])[used].median()):.2e}; positive term up to "
              f"{float(r['pos'][used].max()):.2e}, its gate {float(r['gate_pos'][used].max()):.2e}")
        for other in ([it + 1] if it + 1 < len(its) else []) + ([0] if it > 0 else []):
            ratio = ((its[other]["neg"] - r["neg"]).abs() / r["gate_neg"].clamp_min(1e-300))[used]
            frac = float((ratio >= 10).double().mean())
            print(f"    against iteration {other}: median |difference| / gate {float(ratio.median()):.3g}, {100 * frac:.0f} % of the used rows at 10 x or more")
            assert frac >= 0.5
