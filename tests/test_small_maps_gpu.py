"""GPU: the smallest maps the library samples, and the ones it refuses.

tests/test_small_maps.py states the reason on the CPU: a map below 16 x 16 has a one-pixel pyramid level, which the reference's
sampler divides by zero on.  Here: (a) the four gather routes -- direct and tiled, fp32 maps and the bf16 mirror -- on 16 x 16,
16 x 31, 31 x 16 and 17 x 16 maps against the fp64 oracle, with coordinates on the pixel boundaries of the 2-wide level and the
far-out table of that file, which crosses every clamp and the 16-bit anchor packing of the tiled kernels; (b) every entry point that
samples windows answers a smaller map with PIPS_E_ARG and writes nothing, and takes 16 x 16; (c) the forward at the smallest legal
frame of either stride against the fp64 oracle."""
import ctypes as C

import pytest
import torch

import cases as G
from test_small_maps import FAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
NAN_FILL = 0x7FC12345          # a NaN with a payload (tests/test_clips_gpu.py): a stray write shows in the bit patterns
E_ARG = -1
TOL_PX = 1e-3


def _oracle():
    from oracle import pips_oracle as O
    return O


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _nan_filled(*shape):
    return torch.full(shape, NAN_FILL, dtype=I32, device=DEV).view(torch.float32)


def _pm(t):
    """(B,S,N,X) -> particle-major (B*N*S, X)."""
    B, S, N, X = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N * S, X).contiguous()


def _pack_pyramid(pyr_ref, B, H8, W8):
    """oracle pyramid list (B,8,C,h,w) -> packed channel-last device buffer with its bf16 mirror"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    F = B * 8
    buf = torch.zeros(lib.pips_pyramid_floats(F, H8 * 8, W8 * 8, 8), dtype=torch.float32)
    for l, p in enumerate(pyr_ref):
        off = lib.pips_pyramid_offset(F, H8 * 8, W8 * 8, 8, l)
        flat = p.reshape(F, 128, p.shape[-2], p.shape[-1]).permute(0, 2, 3, 1).reshape(-1)
        buf[off:off + flat.numel()] = flat
    return ops.pyramid_mirror(buf.to(DEV), F, H8 * 8, W8 * 8, 8)


# ------------------------------------------------------------------ a. the gather routes on the smallest legal maps
SHAPES = [(2, 40, 16, 16), (1, 130, 16, 31), (1, 40, 31, 16), (1, 40, 17, 16)]


def _special_coords(H8, W8, g):
    """the named positions: corners; every multiple of 8 and the fp32 number just below it, in x (y random), in y (x random) and in
    both -- the pixel boundaries of the 2-wide level; windows partly and wholly outside; then FAR -> (coords (K,2), first FAR row)"""
    def edges(size):
        out = []
        for k in range(0, size // 8 + 1):
            v = torch.tensor(8.0 * k)
            out += [float(v), float(torch.nextafter(v, torch.tensor(-1.0)))]
        return out
    rnd = lambda size: float(torch.rand((), generator=g)) * (size - 1.0)
    pts = [(0.0, 0.0), (W8 - 1.0, 0.0), (0.0, H8 - 1.0), (W8 - 1.0, H8 - 1.0)]
    pts += [(x, rnd(H8)) for x in edges(W8)] + [(rnd(W8), y) for y in edges(H8)]
    pts += [(x, y) for x, y in zip(edges(min(H8, W8)), edges(min(H8, W8)))]
    pts += [(-2.0, 1.5), (W8 + 3.5, H8 + 9.0)]
    return torch.tensor(pts + list(FAR), dtype=torch.float32), len(pts)


@pytest.fixture(scope="module")
def gather_cases():
    """(B,N,H8,W8) -> the inputs, the device pyramid and the fp64 oracles, computed once and left unchanged"""
    O = _oracle()
    cache = {}

    def get(shape):
        if shape not in cache:
            B, N, H8, W8 = shape
            g = torch.Generator().manual_seed(H8 * 100 + W8)
            fmaps = torch.randn(B, 8, 128, H8, W8, generator=g)
            ffeats = torch.randn(B, 8, N, 128, generator=g)
            coords = torch.rand(B, 8, N, 2, generator=g) * torch.tensor([W8 - 1.0, H8 - 1.0]) + torch.randn(B, 8, N, 2, generator=g)
            if N > 96:
                coords[0, 1] = torch.tensor([W8 * 0.25, H8 * 0.5]) + torch.rand(N, 2, generator=g)   # a frame in ONE tile: items split at 96
            special, first_far = _special_coords(H8, W8, g)
            K = special.shape[0]
            assert K <= 4 * N
            flat = coords[0, 2:6].reshape(4 * N, 2)                        # frames 2..5 of clip 0, one named position per row
            flat[:K] = special
            coords[0, 2:6] = flat.view(4, N, 2)
            far = torch.zeros(B, 8, N, dtype=torch.bool)
            ff_ = far[0, 2:6].reshape(4 * N)
            ff_[first_far:K] = True
            far[0, 2:6] = ff_.view(4, N)
            assert int(far.sum()) == len(FAR) and bool((coords[far].abs().max(dim=1).values >= 1e4).all())
            assert bool((coords[~far].abs() < 64).all())
            pyr_ref = O.build_pyramid(fmaps)
            c64 = coords.double()
            ref = O.corr_sample([p.double() for p in pyr_ref], ffeats.double(), c64)
            ref_bf = O.corr_sample([p.bfloat16().double() for p in pyr_ref], ffeats.bfloat16().double(), c64)
            ref32 = O.corr_sample(pyr_ref, ffeats, coords)
            emb = O.mixer_input(ffeats, ref32, coords)[..., 324:519]        # (B*N, 8, 195): sin / cos and the raw flow + time
            cache[shape] = dict(ffeats=ffeats, coords=coords, far=_pm(far.unsqueeze(-1))[:, 0], pyr=_pack_pyramid(pyr_ref, B, H8, W8),
                                ref=_pm(ref), ref_bf=_pm(ref_bf), ref32=_pm(ref32.double()), emb=emb.reshape(B * N * 8, 195),
                                far_particle=far.any(dim=1).reshape(B * N).repeat_interleave(8))
        return cache[shape]
    return get


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_routes_on_the_smallest_maps(shape, bf16, gather_cases):
    """direct and tiled gather of one mode against the fp64 oracle (the bf16 mode: on maps and features rounded to bf16): 5e-5 on the
    fp32 correlation columns, 1e-4 on the bf16 ones, 1e-4 route against route (the gates of test_mixer_input_build,
    test_mixer_input_build_tiled and test_mixer_input_build_tiled_bf16_mfma); the far-out rows are 196 exact zeros on both routes;
    features, embedding and padding are the same bits on both routes; the embedding of every particle without a far-out position is
    the oracle's.  The tiled call is the tiled kernels: pips_mixer_input_build_tiled_ex runs them or answers PIPS_E_ARG (a query
    set this thin would go the direct way on its own: pips_gather_route says 0), and its three launches are timed.
    Measured: 1.1e-6 .. 6.9e-6 against the oracle on every route and shape, 3.0e-6 .. 6.9e-6 route against route; the fp32 oracle
    itself stands 2.4e-6 .. 5.1e-6 from its fp64 run.  (Before corr_window zeroed the weights of anchors beyond its clamp, both
    tiled kernels returned 49 NaN taps at level 1 of (1e30, 1e30): the product of two weights of 1.4e22 overflowed.)"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    B, N, H8, W8 = shape
    c = gather_cases(shape)
    ff, co = _pm(c["ffeats"]).to(DEV), _pm(c["coords"]).to(DEV)
    assert lib.pips_gather_route(B, N, H8, W8, ops.FLAG_BF16_MAPS if bf16 else 0) == 0
    Xd = ops.mixer_input_build(c["pyr"], B, H8, W8, ff, co, bf16_maps=bf16).cpu()
    Xt, ms = ops.mixer_input_build_tiled_timed(c["pyr"], B, H8, W8, ff, co, bf16_maps=bf16)
    Xt = Xt.cpu()
    assert ms["bin"] > 0 and ms["embed"] > 0 and ms["gather"] > 0                       # bin, embed and gather kernels ran
    ref = c["ref_bf"] if bf16 else c["ref"]
    gate = 1e-4 if bf16 else 5e-5
    err_d = float((Xd[:, 128:324].double() - ref).abs().max())
    err_t = float((Xt[:, 128:324].double() - ref).abs().max())
    dd = float((Xd[:, 128:324] - Xt[:, 128:324]).abs().max())
    yard = float((c["ref32"] - c["ref"]).abs().max())
    print(f"small map {shape} {'bf16' if bf16 else 'fp32'}: direct {err_d:.2e}, tiled {err_t:.2e} against the fp64 oracle (gate {gate:.0e}); "
          f"route against route {dd:.2e} (gate 1e-4); the fp32 oracle's own distance to fp64 {yard:.2e}")
    assert bool(torch.isfinite(Xd).all()) and bool(torch.isfinite(Xt).all())
    again = ops.mixer_input_build_tiled(c["pyr"], B, H8, W8, ff, co, out=_nan_filled(B * N * 8, 544), bf16_maps=bf16).cpu()
    assert torch.equal(_bits(again), _bits(Xt))                         # into a NaN-payload buffer: every entry is written, the same bits
    far = c["far"]
    assert int(far.sum()) == len(FAR)
    for X in (Xd, Xt):
        assert torch.equal(X[far][:, 128:324], torch.zeros(len(FAR), 196))
        assert torch.equal(X[:, :128], _pm(c["ffeats"])) and torch.equal(X[:, 519:], torch.zeros(X.shape[0], 25))
    assert torch.equal(_bits(Xd[:, :128]), _bits(Xt[:, :128])) and torch.equal(_bits(Xd[:, 324:]), _bits(Xt[:, 324:]))
    near = ~c["far_particle"]
    assert int(near.sum()) >= X.shape[0] // 2
    # sin / cos of arguments up to ~5e4 rad (test_mixer_input_build's gate); the raw flow and the time are copies
    assert float((Xd[near][:, 324:516] - c["emb"][near][:, :192]).abs().max()) < 5e-6
    assert torch.equal(Xd[near][:, 516:519], c["emb"][near][:, 192:])
    assert err_d < gate and err_t < gate and dd < 1e-4


# ------------------------------------------------------------------ b. rejection
T_, N_, ITERS_, L_, R_ = 10, 3, 1, 24, 16


class _Calls:
    """the seven entry points on one map size, every output and workspace buffer pre-filled with a NaN payload; inputs (a random
    pyramid of the map's real size, features, in-map coordinates, a chain / stream state) are real, so that the same calls run at a
    legal size"""

    def __init__(self, m, H8, W8):
        from pips_amd import _lib
        self.lib, P = _lib.load(), _lib.ptr
        lib = self.lib
        g = torch.Generator().manual_seed(H8 * 64 + W8)
        H, W = H8 * 8, W8 * 8
        arena, times = m._aux(torch.device(DEV))
        F = max(T_, R_)
        pyr = torch.randn(lib.pips_pyramid_floats(F, H, W, 8), generator=g).to(DEV) * 0.1
        xy_map = torch.rand(N_ * 8, 2, generator=g) * torch.tensor([W8 - 1.0, H8 - 1.0])
        xy = (torch.rand(N_, 2, generator=g) * torch.tensor([W - 17.0, H - 17.0]) + 8.0).to(DEV)
        ff = torch.randn(N_ * 8, 128, generator=g).to(DEV)
        co = xy_map.to(DEV)
        zero, ones = torch.zeros(N_, dtype=I32, device=DEV), torch.ones(N_, dtype=I32, device=DEV)
        active = torch.arange(N_, dtype=I32, device=DEV)
        self.out = {}

        def buf(name, *shape):
            self.out[name] = _nan_filled(*shape)
            return self.out[name]

        def floats(nbytes):
            return max(int(nbytes) // 4, 1)
        st = _stream()
        X = [buf(f"X{i}", N_ * 8, 544) for i in range(3)]
        nsc = lib.pips_gather_scratch_bytes(1, N_, H8, W8)
        scratch = buf("scratch", floats(nsc))
        nbt = lib.pips_track_workspace_bytes_s(1, N_, 8)
        tws = [buf(f"track_ws{i}", floats(nbt)) for i in range(2)]
        tr = [buf(f"tr{i}", ITERS_ + 1, 1, 8, N_, 2) for i in range(2)]
        vi = [buf(f"vi{i}", 1, 8, N_) for i in range(2)]
        fo = [buf(f"ff{i}", 1, N_, 128) for i in range(2)]
        nbc = lib.pips_chain_workspace_bytes(N_, ITERS_)
        cws = buf("chain_ws", floats(nbc))
        ch = dict(trajs=buf("c_trajs", L_, N_, 2), vis=buf("c_vis", L_, N_), feat=buf("c_feat", N_, 128))
        ch["trajs"][0] = xy                                                # (base 0, cur 0: the start positions the hop reads)
        c_cur = torch.zeros(N_, dtype=I32, device=DEV)
        c_nxt, c_cnt = torch.full((N_,), -77, dtype=I32, device=DEV), torch.full((1,), -1, dtype=I32, device=DEV)
        c_steps = torch.full((N_,), -1, dtype=I32, device=DEV)
        nbs = lib.pips_stream_workspace_bytes(N_, ITERS_)
        sws = buf("stream_ws", floats(nbs))
        s = dict(trajs=buf("s_trajs", L_, N_, 2), vis=buf("s_vis", L_, N_), feat=buf("s_feat", N_, 128))
        s_tq = torch.zeros(N_, dtype=I32, device=DEV)
        s_cur, s_status = torch.zeros(N_, dtype=I32, device=DEV), torch.ones(N_, dtype=I32, device=DEV)      # (as select leaves them)
        s_new = torch.arange(N_, dtype=I32, device=DEV)
        s_counts = torch.tensor([N_, N_, 0, 0], dtype=I32, device=DEV)
        s_steps = torch.full((N_,), -1, dtype=I32, device=DEV)
        s["trajs"][0] = xy                                                 # what pips_stream_select stores for a query that joins
        self.ints = dict(c_cur=c_cur, c_nxt=c_nxt, c_cnt=c_cnt, c_steps=c_steps, s_cur=s_cur, s_status=s_status, s_counts=s_counts,
                         s_steps=s_steps)
        self.keep = [pyr, ff, co, xy, zero, ones, active, s_tq, s_new, arena, times]
        self.calls = {
            "pips_mixer_input_build": lambda: lib.pips_mixer_input_build(P(pyr), 1, 8, H8, W8, P(ff), P(co), P(times), N_, P(X[0]), st),
            "pips_mixer_input_build_tiled": lambda: lib.pips_mixer_input_build_tiled(P(pyr), 1, 8, H8, W8, P(ff), P(co), P(times), N_,
                                                                                     P(X[1]), P(scratch), nsc, st),
            "pips_mixer_input_build_ring": lambda: lib.pips_mixer_input_build_ring(P(pyr), 1, T_, R_, H8, W8, P(ff), P(co), P(times), N_,
                                                                                   P(zero), P(ones), 0, 8, P(X[2]), st),
            "pips_track": lambda: lib.pips_track(P(arena), P(pyr), 1, T_, H8, W8, P(xy), None, None, P(zero), P(times), N_, 8, ITERS_, 0,
                                                 P(tws[0]), nbt, P(tr[0]), P(vi[0]), P(fo[0]), st),
            "pips_track_ring": lambda: lib.pips_track_ring(P(arena), P(pyr), 1, T_, R_, H8, W8, P(xy), None, None, P(zero), P(ones),
                                                           P(times), N_, 8, ITERS_, 0, 8, P(tws[1]), nbt, P(tr[1]), P(vi[1]), P(fo[1]), st),
            "pips_chain_hop": lambda: lib.pips_chain_hop(P(arena), P(pyr), T_, T_, H8, W8, P(times), 8, ITERS_, 0, N_, P(active), N_, 1,
                                                         P(ch["trajs"]), P(ch["vis"]), L_, 0, P(c_cur), None, P(ch["feat"]), P(c_nxt),
                                                         P(c_cnt), P(c_steps), P(cws), nbc, st),
            "pips_stream_round": lambda: lib.pips_stream_round(P(arena), P(pyr), T_, R_, H8, W8, P(times), 8, ITERS_, 0, 0, N_, N_, N_,
                                                               P(s_tq), P(xy), P(s_cur), P(s_status), P(s["feat"]), P(s["trajs"]),
                                                               P(s["vis"]), L_, P(active), P(s_new), P(s_counts), P(s_steps), P(sws),
                                                               nbs, st),
        }

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in {**self.out, **self.ints}.items()}


@pytest.mark.parametrize("H8,W8", [(8, 12), (15, 40), (40, 15)])
def test_maps_with_a_one_pixel_level_are_rejected_and_nothing_is_written(weights_tamed, H8, W8):
    """each of the seven entry points returns PIPS_E_ARG, pips_last_error() names the map, and every output, state and workspace
    buffer keeps its bits"""
    from test_stream_rounds_gpu import _model
    c = _Calls(_model(weights_tamed), H8, W8)
    before = c.snapshot()
    for name, call in c.calls.items():
        assert call() == E_ARG, name
        msg = c.lib.pips_last_error().decode()
        assert f"{H8}x{W8}" in msg and "too small" in msg, (name, msg)
        after = c.snapshot()
        for k in before:
            assert torch.equal(after[k], before[k]), (name, k)


def test_the_same_calls_run_at_16_x_16(weights_tamed):
    """the calls of the rejection test at H8 = W8 = 16 return PIPS_OK and write finite results"""
    from test_stream_rounds_gpu import _model
    c = _Calls(_model(weights_tamed), 16, 16)
    for name, call in c.calls.items():
        assert call() == 0, (name, c.lib.pips_last_error())
    torch.cuda.synchronize()
    for k in ("X0", "X1", "X2", "tr0", "tr1", "vi0", "vi1", "ff0", "ff1"):
        assert bool(torch.isfinite(c.out[k]).all()), k
    assert torch.equal(c.out["X0"][:, :128], c.out["X1"][:, :128]) and float((c.out["X0"] - c.out["X1"]).abs().max()) < 1e-4
    assert int((_bits(c.out["c_trajs"]) != NAN_FILL).sum()) == 8 * N_ * 2                 # the hop wrote one window per query
    assert int((_bits(c.out["s_trajs"]) != NAN_FILL).sum()) == 8 * N_ * 2
    assert bool(torch.isfinite(c.out["c_trajs"][:8]).all()) and bool(torch.isfinite(c.out["s_vis"][:8]).all())


def test_pips_refuses_small_frames_and_takes_the_same_frames_at_stride_4(weights_tamed):
    """Pips.forward on 64 x 96 frames: at stride 8 (an 8 x 12 map) it raises and returns nothing; at stride 4 (16 x 24) it runs and
    is finite.  The sizing queries and the encoder still take 64 x 96 at stride 8."""
    from pips_amd import Pips, _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    rgbs = torch.randint(0, 256, (1, 8, 3, 64, 96), generator=g).float().to(DEV)
    xys = (torch.rand(1, 4, 2, generator=g) * torch.tensor([79.0, 47.0]) + 8.0).to(DEV)
    models = {}
    for stride in (8, 4):
        m = Pips(S=8, stride=stride)
        m.load_state_dict(weights_tamed)
        models[stride] = m.to(DEV).eval()
    out = None
    with pytest.raises(_lib.PipsHipError, match="8x12"):
        out = models[8](xys, rgbs, iters=2)
    assert out is None
    preds, _, vis, _ = models[4](xys, rgbs, iters=2)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in preds) and bool(torch.isfinite(vis).all())
    assert lib.pips_pyramid_floats(8, 64, 96, 8) > 0 and lib.pips_encoder_workspace_bytes(8, 64, 96, 8) > 0
    assert lib.pips_workspace_bytes(1, 8, 64, 96, 4, 8) > 0 and lib.pips_score_map_workspace_bytes(1, 8, 8, 12) > 0
    arena = models[8]._aux(torch.device(DEV))[0]
    pyr = ops.encoder_fwd(arena, rgbs[0], 8)
    torch.cuda.synchronize()
    lv = ops.pyramid_levels(pyr, 8, 64, 96, 8)
    assert tuple(lv[3].shape) == (8, 1, 1, 128) and all(bool(torch.isfinite(l).all()) for l in lv)


# ------------------------------------------------------------------ c. the forward at the smallest legal frame
@pytest.fixture(scope="module")
def smallest_forward_oracles():
    """(H, W, stride) -> (dict, inputs, the fp64 oracle forward, the fp32 oracle's distance to it), computed once"""
    O = _oracle()
    cache = {}

    def get(key):
        if key not in cache:
            H, W, stride = key
            case = dict(B=1, N=6, H=H, W=W, stride=stride, iters=3, tamed=True, border=True)
            sd = G.trained_like_state_dict(0, tamed=True)
            xys, rgbs, _, _ = G.make_inputs(case)
            ref = O.forward(O.to_dtype(sd, torch.float64), xys.double(), rgbs.double(), iters=3, stride=stride)
            p32, _, v32, _ = O.forward(sd, xys, rgbs, iters=3, stride=stride)
            yard = (max(float((a.double() - b).abs().max()) for a, b in zip(p32, ref[0])), float((v32.double() - ref[2]).abs().max()))
            cache[key] = (sd, xys, rgbs, ref, yard)
        return cache[key]
    return get


@pytest.mark.parametrize("matmul", ["exact", "split"])
@pytest.mark.parametrize("H,W,stride", [(128, 128, 8), (64, 64, 4)])
def test_forward_at_the_smallest_legal_frame(H, W, stride, matmul, smallest_forward_oracles):
    """B = 1, N = 6 with border queries, iters = 3, tamed trained-like weights on a 16 x 16 map of either stride, both matrix modes,
    against O.forward in fp64 with the gates of test_forward_window_lengths (TOL_PX on positions and visibilities, 1e-5 on the
    start, 2e-4 on the features); everything finite.  The fp32 oracle's own distance to its fp64 run is printed beside each."""
    from pips_amd import Pips
    sd, xys, rgbs, (ref_p, ref_p2, ref_vis, ref_ff), (yard_p, yard_v) = smallest_forward_oracles((H, W, stride))
    m = Pips(S=8, stride=stride)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.matmul = matmul
    m = m.to(DEV).eval()
    preds, preds2, vis, ffeat, _ = m(xys.to(DEV), rgbs.to(DEV), iters=3, return_feat=True)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in preds) and bool(torch.isfinite(vis).all()) and bool(torch.isfinite(ffeat).all())
    assert all(bool(torch.isfinite(p).all()) for p in ref_p) and bool(torch.isfinite(ref_vis).all())
    err = [float((a.cpu().double() - b).abs().max()) for a, b in zip(preds, ref_p)]
    e_vis = float((vis.cpu().double() - ref_vis).abs().max())
    e_ff = float((ffeat.cpu().double() - ref_ff).abs().max())
    e_0 = float((preds2[0].cpu().double() - ref_p2[0]).abs().max())
    print(f"smallest frame {H}x{W} stride {stride} ({matmul}) per-iteration max |dtraj| px:", ["%.2e" % e for e in err],
          f"vis {e_vis:.2e} (gate {TOL_PX:.0e}), start {e_0:.2e} (1e-5), ffeat {e_ff:.2e} (2e-4); the fp32 oracle against its fp64 run: "
          f"traj {yard_p:.2e} vis {yard_v:.2e}; max displacement px {float((ref_p[-1] - ref_p2[0]).abs().max()):.2f}")
    assert tuple(preds[0].shape) == (1, 8, 6, 2) and len(preds) == 3
    assert e_0 < 1e-5
    assert e_ff < 2e-4
    assert max(err) < TOL_PX
    assert e_vis < TOL_PX
