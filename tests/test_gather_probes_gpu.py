"""GPU: the four gather routes and the run-time-S instantiations under the impulse, mixed-scale and occupancy probes of
tests/golden/gather_probes.py (reference, bound and their derivation there; tests/test_gather_probes.py proves the gate on the
CPU: the kernels' formula sits at 0.02 .. 0.08 of it, twelve wrong implementations miss it).

Every correlation element of every row is judged against the fp64 reference on the twin's fp32 positions:
|got - ref| <= (n + 8) u blend(A) + 4 (ulp32(ix) Dx + ulp32(iy) Dy), and +0.0 bit for bit where that bound is 0.  Beside it, on
every call: columns 0:128 are the features' bits, columns 519:544 are zeros, and columns 324:519 (embedding, flow, time) are the
same bits on the direct and the tiled route of a mode.  The tiled calls write into a buffer pre-filled with a NaN payload.

Routes: direct_f32 mixer_input_kernel<8>, direct_bf16 mixer_input_bf16maps_kernel<8> (after pyramid_mirror), tiled_f32 bin + table +
embed + gather_tiled_kernel, tiled_bf16 bin + embed + gather_mfma_kernel, win_f32 / win_bf16 the SCT = 0 instantiations of the
direct kernels through pips_mixer_input_build_clips with T = S frames, S in {5, 12}.

Measured on an MI355X, largest error / bound per level: direct routes 0.02 .. 0.08 on the impulse families and 0.007 .. 0.013 on the
mixed-scale ones; tiled routes 0.05 .. 0.12 and 0.01 .. 0.10; run-time-S routes 0.03 .. 0.06 and 0.006 .. 0.009; no wrong exact zero
on any route; family B2 differs in no bit.  No kernel needed a change."""
import pytest
import torch

import gather_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
NAN_FILL = 0x7FC12345          # a NaN with a payload (tests/test_small_maps_gpu.py): an entry that is not written shows
SHAPES = {"S1": P.S1, "S2": P.S2}
ROUTES = ("direct_f32", "direct_bf16", "tiled_f32", "tiled_bf16")


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _pack(levels, F, H8, W8):
    """four (F, H_l, W_l, 128) levels -> packed device pyramid with its bf16 mirror"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    buf = torch.zeros(lib.pips_pyramid_floats(F, H8 * 8, W8 * 8, 8), dtype=torch.float32)
    for l, lv in enumerate(levels):
        assert tuple(lv.shape) == (F, H8 >> l, W8 >> l, 128)
        off = lib.pips_pyramid_offset(F, H8 * 8, W8 * 8, 8, l)
        buf[off:off + lv.numel()] = lv.reshape(-1)
    return ops.pyramid_mirror(buf.to(DEV), F, H8 * 8, W8 * 8, 8)


def _run(route, pyr, c, ffeats=None):
    """one call of a route on the case's coordinates -> X (M, 544) on the CPU"""
    from pips_amd import ops
    B, S, N, H8, W8 = c["B"], c["S"], c["N"], c["H8"], c["W8"]
    ff = (c["ffeats"] if ffeats is None else ffeats).to(DEV)
    co = c["coords"].to(DEV)
    bf16 = route.endswith("bf16")
    if route.startswith("direct"):
        X = ops.mixer_input_build(pyr, B, H8, W8, ff, co, bf16_maps=bf16)
    elif route.startswith("tiled"):
        out = torch.full((B * N * S, 544), NAN_FILL, dtype=I32, device=DEV).view(torch.float32)
        X = ops.mixer_input_build_tiled(pyr, B, H8, W8, ff, co, out=out, bf16_maps=bf16)
    else:
        assert route.startswith("win") and B == 1
        X = ops.mixer_input_build_clips(pyr, S, H8, W8, ff, co, torch.zeros(N, dtype=I32, device=DEV), None, None, None, None,
                                        bf16_maps=bf16, S=S)
    torch.cuda.synchronize()
    return X.cpu()


def _where(got, r, c):
    """the worst element, named by what locates it in the kernels: route-independent text for an assertion message"""
    bound = r["bound"]
    q = torch.where(bound > 0, (got.double() - r["ref"]).abs() / bound.clamp_min(1e-300),
                    ((got != 0) | torch.signbit(got)).double() * float("inf")).nan_to_num(nan=0.0, posinf=1e300)
    m, k = divmod(int(q.argmax()), 196)
    l, t = divmod(k, 49)
    S, N = c["S"], c["N"]
    return (f"worst element: row {m} (clip {m // (N * S)}, particle {(m // S) % N}, frame {m % S}) level {l} tap ix={t // 7} iy={t % 7}, "
            f"position {c['coords'][m].tolist()}, got {float(got[m, k])!r} ref {float(r['ref'][m, k])!r} bound {float(bound[m, k]):.3e}")


@pytest.fixture(scope="module")
def probes():
    """(family, shape id, S) -> inputs, device pyramid, the references of both modes and the outputs of the routes run so far;
    every one computed once and left unchanged"""
    cache = {}

    def get(family, shape_id, S=8):
        key = (family, shape_id, S)
        if key not in cache:
            c = P.case(family, P.WIN if shape_id == "WIN" else SHAPES[shape_id], S)
            cache[key] = dict(c=c, pyr=_pack(c["levels"], c["B"] * S, c["H8"], c["W8"]), ref={}, out={})
        return cache[key]

    def ref(family, shape_id, bf16, S=8):
        e = get(family, shape_id, S)
        if bf16 not in e["ref"]:
            e["ref"][bf16] = P.reference(*P.args(e["c"]), bf16=bf16)
        return e["ref"][bf16]

    def out(family, shape_id, route, S=8):
        e = get(family, shape_id, S)
        if route not in e["out"]:
            e["out"][route] = _run(route, e["pyr"], e["c"])
        return e["out"][route]
    get.ref, get.out = ref, out
    return get


def _judge(X, r, c, what):
    """the gate of the correlation columns and the copies around them; prints the largest error / bound per level"""
    got = X[:, 128:324]
    q, bad0 = P.ratios(got, r)
    _, z = P.census(r)
    print(f"{what}: error / bound per level {[round(float(x), 3) for x in q]}; wrong exact zeros {bad0.tolist()} of "
          f"{[int(x) for x in (z * got.shape[0] * 49).round()]}")
    assert torch.equal(_bits(X[:, :128]), _bits(c["ffeats"])), "columns 0:128 are the features, bit for bit"
    assert torch.equal(_bits(X[:, 519:544]), torch.zeros(X.shape[0], 25, dtype=I32)), "columns 519:544 are zeros"
    assert bool(torch.isfinite(X).all())
    assert int(bad0.sum()) == 0 and float(q.max()) <= 1.0, _where(got, r, c)
    return q


FAMILY_CASES = [(f, s, rt) for f, s in (("A", "S1"), ("A", "S2"), ("A'", "S1"), ("A'", "S2"), ("B", "S1"), ("B", "S2"), ("C", "S1"))
                for rt in ROUTES if rt.endswith("bf16") or f != "A'"]


@pytest.mark.parametrize("family,shape_id,route", FAMILY_CASES, ids=[f"{f}-{s}-{rt}" for f, s, rt in FAMILY_CASES])
def test_route_meets_the_bound(family, shape_id, route, probes):
    """Families A (impulse response: every output a blend of at most four single products, a third of the taps exact zeros inside
    and outside the map), A' (bf16 routes: features on bf16 ties, one fp32 ulp either side, exponents -20..20), B (operand channels
    2^-8 .. 2^8, 4x4 blocks 2^-6 .. 2^6, frames 2^s) and C (family B on the occupancy ladder: 1, 6, 7, 32, 33, 96, 97, 193 particles
    in tile (1, 1), the others in tile (0, 0)) on S1 = (1, 200, 33, 40) and S2 = (2, 40, 16, 31): every element within its bound,
    bound-0 taps +0.0, features / padding / embedding as the module docstring says.
    Measured error / bound, largest element per level: mixer_input_kernel and mixer_input_bf16maps_kernel 0.024 .. 0.073 on A,
    0.036 .. 0.082 on A', 0.007 .. 0.013 on B and C; gather_tiled_kernel and gather_mfma_kernel 0.046 .. 0.111 on A, 0.060 .. 0.116
    on A', 0.010 .. 0.099 on B, 0.038 .. 0.064 on C (the ladder).  Of family A's 99 293 bound-0 taps at S1 and 60 583 at S2 every one
    is +0.0 on every route."""
    e = probes(family, shape_id)
    bf16 = route.endswith("bf16")
    X = probes.out(family, shape_id, route)
    _judge(X, probes.ref(family, shape_id, bf16), e["c"], f"{route} {family} {shape_id}")
    other = probes.out(family, shape_id, ("tiled_" if route.startswith("direct") else "direct_") + route.split("_")[1])
    assert torch.equal(_bits(X[:, 324:519]), _bits(other[:, 324:519])), "columns 324:519: the same bits on the direct and the tiled route"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_powers_of_two_commute_with_the_route(shape_id, route, probes):
    """Family B2: the same call on maps * 2^t[c] with features * 2^-t[c] (t in -10..10 per channel) gives the same 196 correlation
    bits, and on maps * 2^7 alone exactly 2^7 times them.  Powers of two commute with every fp32 and bf16 rounding as long as nothing
    leaves the normal range: family B stores magnitudes within 2^-38 .. 2^24 (gather_probes.mixed_levels), the rescaled operands stay
    within 2^-48 .. 2^34 and their products and sums far inside fp32's 2^+-126.
    Measured: 0 of 313 600 (S1) and 0 of 125 440 (S2) elements differ, on each of the four routes."""
    e = probes("B", shape_id)
    c = e["c"]
    F = c["B"] * c["S"]
    base = probes.out("B", shape_id, route)[:, 128:324]
    t = P.channel_shift(9)
    moved = _run(route, _pack([lv * 2.0 ** t for lv in c["levels"]], F, c["H8"], c["W8"]), c, ffeats=c["ffeats"] * 2.0 ** -t)
    up = _run(route, _pack([lv * 128.0 for lv in c["levels"]], F, c["H8"], c["W8"]), c)
    d1 = int((_bits(moved[:, 128:324]) != _bits(base)).sum())
    d2 = int((_bits(up[:, 128:324]) != _bits(base * 128.0)).sum())
    print(f"{route} B2 {shape_id}: {d1} elements differ under the per-channel rescaling, {d2} under maps * 2^7, of {base.numel()}")
    assert int((base != 0).sum()) > base.numel() // 3
    assert d1 == 0 and d2 == 0


WIN_CASES = [(f, S, bf) for S in (5, 12) for f in ("A", "B") for bf in (False, True)]


@pytest.mark.parametrize("family,S,bf16", WIN_CASES, ids=[f"{f}-S{S}-{'bf16' if bf else 'f32'}" for f, S, bf in WIN_CASES])
def test_runtime_window_length_meets_the_bound(family, S, bf16, probes):
    """win_f32 / win_bf16: the SCT = 0 instantiations of the direct kernels (window lengths other than 8) on their own against fp64:
    pips_mixer_input_build_clips with no clip table, T = S frames, win_start = 0, N = 24, maps 17 x 24, families A and B.
    Measured error / bound, largest element per level: 0.029 .. 0.064 on A, 0.006 .. 0.009 on B, either mode, S = 5 and 12."""
    route = "win_bf16" if bf16 else "win_f32"
    e = probes(family, "WIN", S)
    _judge(probes.out(family, "WIN", route, S), probes.ref(family, "WIN", bf16, S), e["c"], f"{route} {family} S={S}")
