"""GPU: point_sample_kernel, the tail of the mixer input (columns 324:544: sin / cos embedding, flow, time, padding) on every
kernel that writes it, and the evaluation branch (score_upsum_kernel, score_terms_kernel, their use per iteration inside
pips_track_ce), each alone against the operation in fp64 with the references and bounds of tests/golden/track_stages.py
(proven on the CPU by tests/test_track_stages.py, where the listed wrong implementations miss every gate used here).
Every test prints its worst error / bound.

Measured on an MI355X: point_sample_kernel has its twin's bits on every probe (hipcc contracted nothing: the __f*_rn contract holds)
and sits at 0.29 .. 0.43 of the fp64 bound; the embedding's sin / cos are at 0.20 of the yardstick gate and carry the same bits on
all six routes; U at 0.005 .. 0.027 of its bound; the terms at 0.004 .. 0.475 (positive) and 0.001 .. 0.089 (negative); ce_terms are,
bit for bit, the terms of the features held at the start of each iteration in all three matrix modes, and within 0.08 of the gate
against the fp64 oracle.  No kernel needed a change; pips_point_sample and pips_score_map_terms gained the check of H8 and W8."""
import ctypes as C

import pytest
import torch

import track_stages as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
NAN_FILL = 0x7FC12345          # a NaN with a payload: an entry that is written shows
E_ARG = -1


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _nan_filled(*shape):
    return torch.full(shape, NAN_FILL, dtype=I32, device=DEV).view(torch.float32)


def _untouched(t):
    return bool((_bits(t) == NAN_FILL).all())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack(levels, Fr, H8, W8):
    """four (F, H8 >> l, W8 >> l, 128) levels -> packed device pyramid with its bf16 mirror"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    buf = torch.zeros(lib.pips_pyramid_floats(Fr, H8 * 8, W8 * 8, 8), dtype=torch.float32)
    for l, lv in enumerate(levels):
        assert tuple(lv.shape) == (Fr, H8 >> l, W8 >> l, 128)
        off = lib.pips_pyramid_offset(Fr, H8 * 8, W8 * 8, 8, l)
        buf[off:off + lv.numel()] = lv.reshape(-1)
    return ops.pyramid_mirror(buf.to(DEV), Fr, H8 * 8, W8 * 8, 8)


# ------------------------------------------------------------------ A. point sample
@pytest.mark.parametrize("B,S,N,H8,W8", T.PS_SHAPES)
def test_point_sample_bits_and_fp64(B, S, N, H8, W8):
    """point_sample_kernel equals its numpy float32 twin bit for bit (the documented contract: the reference's operation order,
    every product and sum rounded once) and meets 6 u sum |w| |v| against the fp64 blend, on random positions and on
    ps_specials (integers: the pixel's bits; corners; clamped indices with unclamped weights; -0.25; one ulp below an integer;
    +-1e6; 2^24 + 1).  Every frame holds different values: the kernel reads frame b * S.
    Measured on an MI355X: 0 differing elements on every shape and position set; error / bound 0.29 .. 0.43."""
    from pips_amd import ops
    lv = T.ps_maps(B, S, H8, W8)
    d_lv = lv.to(DEV)
    sp = T.ps_specials(H8, W8)
    for name, xy in (("random", T.ps_positions(B, N, H8, W8)), ("special", sp[None].repeat(B, 1, 1).contiguous())):
        got = ops.point_sample(d_lv, B, xy.to(DEV)).cpu()
        twin = T.ps_twin(lv, S, xy)
        ref, bound = T.ps_ref(lv, S, xy)
        ndiff = int((_bits(got) != _bits(twin)).sum())
        q = T.worst((got.double() - ref).abs(), bound)
        print(f"point sample {(B, S, N, H8, W8)} {name}: {ndiff} of {got.numel()} elements differ from the twin; error / bound {q:.3f}")
        assert ndiff == 0 and q <= 1.0
        if name == "special":
            ix = xy[0, :T.PS_INTEGERS].long()
            for b in range(B):
                assert torch.equal(_bits(got[b, :T.PS_INTEGERS]), _bits(lv[b * S, ix[:, 1], ix[:, 0]]))


def test_point_sample_rejects_bad_arguments_and_writes_nothing():
    """PIPS_E_ARG ahead of any launch for an empty map (H8 or W8 below 1), B, S or N below 1 and null pointers: the output,
    pre-filled with a NaN payload, stays untouched; the same call with legal arguments then writes every element."""
    from pips_amd import _lib
    lib = _lib.load()
    p = _lib.ptr
    B, S, N, H8, W8 = 1, 2, 3, 8, 8
    lv = T.ps_maps(B, S, H8, W8).to(DEV)
    xy = T.ps_positions(B, N, H8, W8).to(DEV)
    out = _nan_filled(B, N, 128)
    bad = [(B, S, 0, W8, N), (B, S, H8, 0, N), (B, S, -3, W8, N), (B, S, H8, -1, N), (0, S, H8, W8, N), (B, 0, H8, W8, N), (B, S, H8, W8, 0)]
    for b, s, h, w, n in bad:
        assert lib.pips_point_sample(p(lv), b, s, h, w, p(xy), n, p(out), _stream()) == E_ARG, (b, s, h, w, n)
    for ptrs in ((None, p(xy), p(out)), (p(lv), None, p(out)), (p(lv), p(xy), None)):
        assert lib.pips_point_sample(ptrs[0], B, S, H8, W8, ptrs[1], N, ptrs[2], _stream()) == E_ARG
    torch.cuda.synchronize()
    assert _untouched(out)
    assert lib.pips_point_sample(p(lv), B, S, H8, W8, p(xy), N, p(out), _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ B. embedding tail
def _emb_inputs(S, N, frames=None):
    g = torch.Generator().manual_seed(53 + 10 * S + N)
    Fr = S if frames is None else frames
    levels = [torch.randn(Fr, T.EMB_H8 >> l, T.EMB_W8 >> l, 128, generator=g) for l in range(4)]
    return _pack(levels, Fr, T.EMB_H8, T.EMB_W8), torch.randn(N * S, 128, generator=g).to(DEV)


def _judge_tail(X, r, gate, what):
    """the exact gates and the sin / cos gate of one call; -> the call's worst |sin / cos error|"""
    M = X.shape[0]
    assert torch.equal(_bits(X[:, 516:519]), _bits(r["flow"])), f"{what}: columns 516:519 are the bits of dx, dy, t"
    assert torch.equal(_bits(X[:, 519:544]), torch.zeros(M, 25, dtype=I32)), f"{what}: columns 519:544 are zeros"
    emb = X[:, 324:516]
    z = r["zero"]
    odd = (torch.arange(192) % 2).bool()[None, :].expand_as(z)
    assert bool((emb[z & ~odd] == 0).all()) and bool((emb[z & odd] == 1).all()), f"{what}: sin 0 = 0 and cos 0 = 1 exactly"
    e = float((emb.double() - r["ref"]).abs().max())
    assert e <= gate, f"{what}: sin / cos error {e:.3e} above the gate {gate:.3e}"
    return e


@pytest.mark.parametrize("N", [1, 3])
def test_embedding_tail_every_window_length(N):
    """Columns 324:544 of mixer_input_kernel through pips_mixer_input_build_clips at S = 1, 5, 8, 12, 32 (t = linspace(0, S, S);
    S = 8 is the compile-time-S instantiation, the others the run-time-S one), fp32 and bf16 maps, on displacements of 0, -0.0,
    +-2^-10, +-0.5, +-W8, +-1e3, +-1e4, +-3e5 (arguments up to 2.9e8: Payne-Hanek range reduction).  Exact: flow and time
    bits, zero padding, sin 0 = 0 and cos 0 = 1.  sin / cos: no error bound of OCML's sinf / cosf is stated by the project or
    by the installed toolchain's documents, so the gate is the yardstick rule, 4 x the larger worst error of torch's own fp32
    sin / cos on the same fp32 arguments (on the device, on the CPU) + 2^-24, against the fp64 sin / cos of the fp32 argument.
    Measured on an MI355X, N = 1 and N = 3 alike: worst error of torch's fp32 sin / cos on the device 5.35e-08 / 5.41e-08 / 5.35e-08 /
    5.56e-08 at S = 5 / 8 / 12 / 32, on the CPU 3.30e-08 / 3.46e-08 / 3.35e-08 / 3.47e-08, gates 2.74e-07 .. 2.82e-07; the kernels'
    worst error is the device yardstick's to the digit at every S (5.35e-08 .. 5.56e-08, 0.20 of the gate) on fp32 and bf16
    maps; S = 1 has zero arguments only and is exact (gate 2^-24).  torch.linspace(0, S, S) on the device has the CPU's bits at
    every S."""
    from pips_amd import ops
    for S in T.EMB_WINDOWS:
        co = T.embed_coords(S, N)
        r = T.embed_ref(co, ops.times_table(torch.device(DEV), S).cpu(), S)
        y_cpu, y_dev = T.embed_yardstick(r), T.embed_yardstick(r, DEV)
        gate = T.embed_gate(y_cpu, y_dev)
        pyr, ff = _emb_inputs(S, N)
        win = torch.zeros(N, dtype=I32, device=DEV)
        worst = 0.0
        for bf16 in (False, True):
            X = ops.mixer_input_build_clips(pyr, S, T.EMB_H8, T.EMB_W8, ff, co.to(DEV), win, None, None, None, None, bf16_maps=bf16, S=S).cpu()
            worst = max(worst, _judge_tail(X, r, gate, f"S={S} N={N} bf16_maps={bf16}"))
        same_t = torch.equal(_bits(r["flow"][:S, 2]), _bits(torch.linspace(0, S, S)))
        print(f"embedding tail S={S} N={N}: kernels' worst sin / cos error {worst:.2e}; torch fp32 on the device {y_dev:.2e}, on the CPU {y_cpu:.2e}; "
              f"gate {gate:.2e}; device linspace(0, S, S) {'equals' if same_t else 'DIFFERS from'} the CPU's")


def test_embedding_tail_routes_agree():
    """S = 8, N = 3: columns 324:544 are the same bits on direct fp32 (mixer_input_kernel<8>), direct bf16
    (mixer_input_bf16maps_kernel<8>), tiled fp32 and tiled bf16 (embed_rows_kernel), and on the run-time-S instantiations of both
    direct kernels.  The library picks the compile-time-S kernel whenever S = 8, so the run-time-S kernels are run on windows of
    S = 12 whose first eight rows carry the S = 8 probe and whose time table starts with linspace(0, 8, 8): those rows must be
    the S = 8 bits.  Each route meets the gates of test_embedding_tail_every_window_length on its own.
    Measured on an MI355X: worst sin / cos error 5.41e-08 on each of the six routes, torch's fp32 sin / cos 5.41e-08 on the device and
    3.46e-08 on the CPU, gate 2.76e-07; the six routes differ in no bit of columns 324:544."""
    from pips_amd import _lib, ops
    lib = _lib.load()
    S, N, H8, W8 = 8, 3, T.EMB_H8, T.EMB_W8
    co = T.embed_coords(S, N)
    tt = ops.times_table(torch.device(DEV), S)
    r = T.embed_ref(co, tt.cpu(), S)
    gate = T.embed_gate(T.embed_yardstick(r), T.embed_yardstick(r, DEV))
    pyr, ff = _emb_inputs(S, N)
    d_co = co.to(DEV)
    outs = {}
    for bf16 in (False, True):
        m = "bf16" if bf16 else "f32"
        outs["direct_" + m] = ops.mixer_input_build(pyr, 1, H8, W8, ff, d_co, bf16_maps=bf16).cpu()
        outs["tiled_" + m] = ops.mixer_input_build_tiled(pyr, 1, H8, W8, ff, d_co, out=_nan_filled(N * S, 544), bf16_maps=bf16).cpu()
    # run-time S: windows of 12 rows, the first eight of them the probe
    S2 = 12
    pyr2, ff2 = _emb_inputs(S2, N)
    co2 = torch.cat([co.reshape(N, S, 2), co.reshape(N, S, 2)[:, -1:].expand(N, S2 - S, 2)], dim=1).reshape(N * S2, 2).contiguous().to(DEV)
    tt2 = torch.cat([tt, tt[-1:] + torch.arange(1, S2 - S + 1, device=DEV)]).contiguous()
    win = torch.zeros(N, dtype=I32, device=DEV)
    for bf16 in (False, True):
        X2 = _nan_filled(N * S2, 544)
        rc = lib.pips_mixer_input_build_clips(_lib.ptr(pyr2), 1, S2, S2, H8, W8, _lib.ptr(ff2), _lib.ptr(co2), _lib.ptr(tt2), N, ops._i32(win),
                                              None, None, None, None, 0, ops.FLAG_BF16_MAPS if bf16 else 0, S2, _lib.ptr(X2), _stream())
        _lib.check(rc, "pips_mixer_input_build_clips")
        torch.cuda.synchronize()
        outs["runtime_S_" + ("bf16" if bf16 else "f32")] = X2.cpu().view(N, S2, 544)[:, :S].reshape(N * S, 544)
    worst = {k: _judge_tail(X, r, gate, k) for k, X in outs.items()}
    print("embedding tail, S = 8 routes: worst sin / cos error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; gate {gate:.2e}")
    first = _bits(outs["direct_f32"][:, 324:544])
    for k, X in outs.items():
        assert torch.equal(_bits(X[:, 324:544]), first), f"{k}: columns 324:544 differ from direct_f32's"


# ------------------------------------------------------------------ C. score map: U
@pytest.mark.parametrize("Fr,H8,W8", T.UP_SHAPES)
def test_score_map_prepare(Fr, H8, W8):
    """score_upsum_kernel against the fp64 sum of the four upsampled levels; bound: the four levels' resize bounds (frame by
    frame) + 3 u sum |level terms|.  Levels independent, frame f scaled by 2^f.  (2, 8, 8): level 3 is one pixel; (16, 64, 66):
    the grid-stride loop's second trip.
    Measured on an MI355X, worst error / bound: 0.024 (2, 8, 8), 0.020 (3, 17, 25), 0.027 (2, 9, 23), 0.005 (16, 64, 66)."""
    from pips_amd import ops
    levels = T.up_levels(Fr, H8, W8)
    ref, bound = T.upsum_ref(levels)
    B, S = (2, Fr // 2) if Fr % 2 == 0 else (1, Fr)
    got = ops.score_map_prepare(_pack(levels, Fr, H8, W8), B, S, H8, W8).cpu()
    per_frame = [T.worst((got[f].double() - ref[f]).abs(), bound[f]) for f in range(Fr)]
    print(f"U {(Fr, H8, W8)}: worst error / bound {max(per_frame):.3f} (frame {per_frame.index(max(per_frame))})")
    assert bool(torch.isfinite(got).all()) and max(per_frame) <= 1.0
    if (Fr, H8, W8) == T.UP_SHAPES[-1]:
        assert Fr * H8 * W8 * 32 > 8192 * 256


# ------------------------------------------------------------------ C. score map: terms
@pytest.mark.parametrize("family", T.TERM_FAMILIES)
@pytest.mark.parametrize("shape", T.TERM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_score_map_terms_on_a_given_u(shape, family):
    """score_terms_kernel on a given U against the fp64 formula b + log(exp(-b) + exp(a - b)) per pixel and its two sums, within
    the per-row bounds of track_stages.terms_ref: the positive term an absolute gate (2^-23 + ...), the negative one the sum of
    the per-pixel errors.  Targets: pixels 0, HW - 1, both other corners, 255, 256, 257, random ones; rows with use = 0 are
    +0.0 bit for bit.  Families: dense (scores of std 11), large (|score| up to ~200: finite, relu(a)), small (1e-3), impulse.
    Measured on an MI355X, worst error / bound over the four shapes (positive, negative): dense 0.475, 0.002; large 0.458,
    0.002; small 0.274, 0.089; impulse 0.212, 0.040."""
    from pips_amd import ops
    B, S, N, H8, W8 = shape
    U, ff = T.term_case(family, *shape)
    d_U, d_ff = U.to(DEV), ff.to(DEV)
    wp = wn = 0.0
    n_off = 0
    for tgt in T.term_targets(*shape, family=family):
        got = ops.score_map_terms_u(d_U, B, S, H8, W8, d_ff, tgt.to(DEV)).cpu()
        r = T.terms_ref(U, ff, tgt, *shape)
        off = tgt[:, 2] == 0
        n_off += int(off.sum())
        assert torch.equal(_bits(got[off]), torch.zeros_like(_bits(got[off]))), "rows with use = 0 are +0.0"
        assert bool(torch.isfinite(got).all())
        p, n = T.terms_worst(got, r)
        wp, wn = max(wp, p), max(wn, n)
    print(f"terms {shape} {family}: error / bound positive {wp:.3f}, negative {wn:.3f}")
    assert n_off > 0 and wp <= 1.0 and wn <= 1.0


def test_score_map_rejects_bad_arguments_and_writes_nothing():
    """pips_score_map_prepare (maps below 8 x 8, B or S below 1, null pointers) and pips_score_map_terms (H8, W8, B, S or N below 1,
    null pointers) answer PIPS_E_ARG ahead of any launch: U and the terms, pre-filled with a NaN payload, stay untouched."""
    from pips_amd import _lib
    lib = _lib.load()
    p = _lib.ptr
    B, S, N, H8, W8 = 1, 2, 2, 8, 8
    pyr = _pack(T.up_levels(B * S, H8, W8), B * S, H8, W8)
    U = _nan_filled(B * S, H8, W8, 128)
    for b, s, h, w in ((B, S, 7, W8), (B, S, H8, 7), (B, S, 0, W8), (B, S, H8, -8), (0, S, H8, W8), (B, 0, H8, W8)):
        assert lib.pips_score_map_prepare(p(pyr), b, s, h, w, p(U), _stream()) == E_ARG, (b, s, h, w)
    assert lib.pips_score_map_prepare(None, B, S, H8, W8, p(U), _stream()) == E_ARG
    assert lib.pips_score_map_prepare(p(pyr), B, S, H8, W8, None, _stream()) == E_ARG
    torch.cuda.synchronize()
    assert _untouched(U)
    Ug, ff = T.term_case("dense", B, S, N, H8, W8)
    Ug, ff = Ug.to(DEV), ff.to(DEV)
    tgt = T.term_targets(B, S, N, H8, W8)[0].to(DEV)
    out = _nan_filled(B * N * S, 2)
    for b, s, h, w, n in ((B, S, 0, W8, N), (B, S, H8, 0, N), (B, S, -1, W8, N), (B, S, H8, -1, N), (0, S, H8, W8, N), (B, 0, H8, W8, N),
                          (B, S, H8, W8, 0)):
        assert lib.pips_score_map_terms(p(Ug), b, s, h, w, p(ff), n, p(tgt), p(out), _stream()) == E_ARG, (b, s, h, w, n)
    for ptrs in ((None, p(ff), p(tgt), p(out)), (p(Ug), None, p(tgt), p(out)), (p(Ug), p(ff), None, p(out)), (p(Ug), p(ff), p(tgt), None)):
        assert lib.pips_score_map_terms(ptrs[0], B, S, H8, W8, ptrs[1], N, ptrs[2], ptrs[3], _stream()) == E_ARG
    torch.cuda.synchronize()
    assert _untouched(out)
    assert lib.pips_score_map_terms(p(Ug), B, S, H8, W8, p(ff), N, p(tgt), p(out), _stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ D. the per-iteration wiring
@pytest.fixture(scope="module")
def wiring():
    """the case of track_stages.wiring_refs on the device: weights packed, the pyramid encoded once (fp32 encoder), and the
    pips_track_ce result of every matrix mode run so far"""
    from pips_amd import ops
    w = T.wiring_refs()
    case = w["case"]
    arena = ops.pack_weights(w["sd"], torch.device(DEV))
    rgbs = w["rgbs"].reshape(w["B"] * w["S"], 3, case["H"], case["W"]).to(DEV)
    pyr = ops.encoder_fwd(arena, rgbs, w["stride"])
    runs = {}

    def run(mode):
        if mode not in runs:
            flags = {"exact": 0, "split": ops.FLAG_SPLIT_BF16, "bf16": ops.FLAG_BF16_MIXER}[mode]
            runs[mode] = ops.track_ce(arena, pyr, w["B"], w["H8"], w["W8"], w["xys"].to(DEV), w["stride"], w["iters"], flags, w["tgt"].to(DEV))
            torch.cuda.synchronize()
        return runs[mode]
    return dict(w=w, arena=arena, pyr=pyr, run=run)


@pytest.mark.parametrize("mode", ["exact", "split", "bf16"])
def test_ce_terms_come_from_the_features_ahead_of_the_update(mode, wiring):
    """The loop of pips_track_ce replayed through the stage entry points (point_sample, mixer_input_build, mixer_fwd, state_update):
    the replayed trajectories and initial features equal pips_track_ce's bit for bit, and ce_terms[it] equals, bit for bit,
    pips_score_map_terms on the features the replay held at the START of iteration it -- not those after the update, not
    the first iteration's (tests/test_track_stages.py::test_wiring_precondition: either differs by hundreds of gates).
    Measured on an MI355X: the replay is bit-equal in all three matrix modes."""
    from pips_amd import _lib, ops
    w, arena, pyr = wiring["w"], wiring["arena"], wiring["pyr"]
    B, N, S, H8, W8, stride, iters = (w[k] for k in ("B", "N", "S", "H8", "W8", "stride", "iters"))
    assert _lib.load().pips_gather_route(B, N, H8, W8, 0) == 0                     # the tracker's AUTO route is the direct gather here
    trajs, vis, ffeat0, ce_terms = wiring["run"](mode)
    M = B * N * S
    xy8 = w["xys"].to(DEV) / float(stride)
    level0 = ops.pyramid_levels(pyr, B * S, H8 * stride, W8 * stride, stride)[0]
    f0 = ops.point_sample(level0, B, xy8)
    assert torch.equal(_bits(f0), _bits(ffeat0))
    ff = f0[:, :, None, :].expand(B, N, S, 128).reshape(M, 128).contiguous()
    co = xy8[:, :, None, :].expand(B, N, S, 2).reshape(M, 2).contiguous()
    co0 = co.clone()
    assert torch.equal(_bits(trajs[0]), _bits((co * float(stride)).view(B, N, S, 2).transpose(1, 2)))
    U = ops.score_map_prepare(pyr, B, S, H8, W8)
    tgt = w["tgt"].to(DEV)
    held = []
    for it in range(iters):
        held.append(ff.clone())
        terms = ops.score_map_terms_u(U, B, S, H8, W8, ff, tgt)
        assert torch.equal(_bits(terms), _bits(ce_terms[it])), f"{mode}: ce_terms[{it}] are not the terms of the features at the start of iteration {it}"
        X = ops.mixer_input_build(pyr, B, H8, W8, ff, co)
        delta = ops.mixer_fwd(arena, X, bf16=mode == "bf16", split=mode == "split")
        traj, _ = ops.state_update(arena, delta, ff, co, co0, B, N, float(stride))
        assert torch.equal(_bits(traj), _bits(trajs[it + 1])), f"{mode}: the replayed trajectory of iteration {it} differs"
    # the neighbours are NOT what the library wrote: features after the update / of the first iteration give other bits
    used = w["used"]
    for it in range(1, iters):
        other = ops.score_map_terms_u(U, B, S, H8, W8, held[it - 1], tgt).cpu()
        assert not torch.equal(_bits(other[used]), _bits(ce_terms[it][used.to(DEV)]))
    assert bool(torch.isfinite(ce_terms).all()) and bool((ce_terms[:, (~used).to(DEV)] == 0).all())


def test_ce_terms_against_the_fp64_oracle(wiring):
    """exact mode: ce_terms[it] against the fp64 terms of the fp64 oracle's taps["iters"][it]["ffeats_in"]; gate = 4 x the error of
    the fp32 oracle's own terms against the same values (relative for the negative term, absolute for the positive one) + the
    stage bound (U's bound carried through the scores).  Rows with use = 0 are +0.0.
    Measured on an MI355X, worst error / gate over iterations 0 .. 5: negative 0.020, 0.020, 0.024, 0.037, 0.040, 0.044 (relative
    error 1.1e-06 .. 3.3e-06 beside a yardstick of 8.5e-07 .. 2.9e-06: the stage bound, which carries U's resize bound, is most
    of the gate); positive 0.080, 0.033, 0.011, 0.003, 0.007, 0.050 (yardstick 3.9e-10 .. 1.4e-08 absolute)."""
    w = wiring["w"]
    ce_terms = wiring["run"]("exact")[3].cpu()
    used = w["used"]
    worst_n, worst_p = [], []
    for it, r in enumerate(w["its"]):
        got = ce_terms[it].double()
        assert torch.equal(_bits(ce_terms[it][~used]), torch.zeros_like(_bits(ce_terms[it][~used])))
        worst_n.append(T.worst((got[:, 1] - r["neg"]).abs()[used], r["gate_neg"][used]))
        worst_p.append(T.worst((got[:, 0] - r["pos"]).abs()[used], r["gate_pos"][used]))
        rel = float(((got[:, 1] - r["neg"]).abs() / r["neg"].clamp_min(1e-300))[used].max())
        print(f"ce_terms iteration {it}: negative error / gate {worst_n[-1]:.3f} (relative error {rel:.2e}, yardstick {r['yard_neg_rel']:.2e}); "
              f"positive error / gate {worst_p[-1]:.3f} (yardstick {r['yard_pos_abs']:.2e} absolute)")
    assert max(worst_n) <= 1.0 and max(worst_p) <= 1.0
