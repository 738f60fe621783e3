"""GPU: scene cuts in the library.  pips_cut_table is held, as integers, to drivers.cut_table_torch run on the CPU -- uint8 and float32
frames with the float edge values and a flat frame, sizes with empty regions, ragged rows and regions, rows that start off the
16-byte grid, several strips per frame -- with poisoned outputs and workspace tails and its return codes.  End to end on the real
model at 128 x 192 with two scenes of 21 + 19 frames: ``scan="library"`` equals ``scan="torch"``, a covered stream with a cut is its
two scenes tracked apart, and StreamTracker.cut() under library rounds equals torch rounds."""
import ctypes as C

import pytest
import torch

from test_cover_gpu import ECELL, EH, EW, _assert_live, _same_parts, _user
from test_cuts import EDGE, TA, TB, _frames, _pieces, _scenes
from test_stream_rounds_gpu import H_, W_, _assert_route_0, _bits, _model, _queries, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
POISON = -77
GUARD = 64
E_ARG, E_WORKSPACE = -1, -2


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, skip=0):
    return C.c_void_p(t.data_ptr() + skip)


def _table_guarded(lib, src, prev):
    """pips_cut_table on the device frames ``src`` into poisoned buffers with guard words around hist and dist and a poisoned tail
    behind the workspace -> (hist, dist) on the host; guards, tail and inputs are checked"""
    F, _, h, w = src.shape
    before = src.cpu()
    nbytes = lib.pips_cut_workspace_bytes(F, h, w)
    hist = torch.full((F * 512 + 2 * GUARD,), POISON, dtype=I32, device=DEV)
    dist = torch.full((F + 2 * GUARD,), POISON, dtype=I32, device=DEV)
    ws = torch.full((nbytes // 4 + GUARD,), POISON, dtype=I32, device=DEV)
    p = None if prev is None else prev.to(DEV, I32).contiguous()
    keep = None if p is None else p.clone()
    rc = lib.pips_cut_table(_ptr(src), int(src.dtype == torch.uint8), F, h, w, None if p is None else _ptr(p), _ptr(hist, 4 * GUARD),
                            _ptr(dist, 4 * GUARD), _ptr(ws), nbytes, _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    assert bool((hist[:GUARD] == POISON).all()) and bool((hist[GUARD + F * 512:] == POISON).all())
    assert bool((dist[:GUARD] == POISON).all()) and bool((dist[GUARD + F:] == POISON).all())
    assert bool((ws[nbytes // 4:] == POISON).all())
    assert torch.equal(src.cpu(), before) and (p is None or torch.equal(p, keep))              # the inputs are left as they were
    return hist[GUARD:GUARD + F * 512].view(F, 16, 32).cpu(), dist[GUARD:GUARD + F].cpu()


def _check(lib, frames, prev, src=None):
    from pips_amd import drivers, ops
    ref_h, ref_d = drivers.cut_table_torch(frames, prev)                                       # on the CPU
    src = frames.to(DEV) if src is None else src
    got_h, got_d = _table_guarded(lib, src, prev)
    assert torch.equal(got_h.long(), ref_h) and torch.equal(got_d.long(), ref_d), (tuple(frames.shape), frames.dtype)
    via_h, via_d = ops.cut_table(src, None if prev is None else prev.to(DEV))
    assert via_h.dtype == I32 and via_d.dtype == I32 and torch.equal(via_h.cpu(), got_h) and torch.equal(via_d.cpu(), got_d)
    return ref_h, ref_d


# 1x1; 3x5: empty regions; 37x53: ragged rows and regions, element loads; 16x53: 16-byte loads on rows that start at every
# alignment; 64x96: 16-byte loads on aligned rows, six regions a side
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 53), (16, 53), (64, 96)])
def test_cut_table_is_the_torch_form(h, w, dtype):
    from pips_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(h + w)
    prev = torch.randint(0, h * w + 1, (16, 32), generator=g, dtype=I32)
    for F in (0, 1, 5):
        fr = _frames(F, h, w, dtype, 10 * F + w)                                               # edge values and a flat last frame
        for p in (None, prev):
            hist, dist = _check(lib, fr, p)
            assert hist.sum(dim=(1, 2)).tolist() == [h * w] * F
        if F == 5:
            assert int(hist[4].max()) >= max(1, (h // 4) * (w // 4))                          # the flat frame
            assert p is not None and int(dist[0]) > 0 and (h * w < 64 or int(dist[4]) > 0)
    if dtype == torch.float32:
        fr = torch.tensor(EDGE).view(5, 1, 1, 1).expand(5, 3, h, w).contiguous()
        hist, _ = _check(lib, fr, None)
        assert [int(torch.nonzero(hist[f].sum(0))[0, 0]) for f in range(5)] == [0, 0, 31, 31, 31]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_several_strips_per_frame_and_their_sum(dtype):
    """360 x 640, F = 2: 12 strips in each region row, 16-byte loads, the partial sums of both frames; black against white is 2hw"""
    from pips_amd import _lib
    lib = _lib.load()
    assert lib.pips_cut_workspace_bytes(2, 360, 640) == 2 * 4 * 12 * 512
    g = torch.Generator().manual_seed(5)
    fr = torch.randint(0, 256, (2, 3, 360, 640), generator=g, dtype=torch.uint8).to(dtype)
    prev = torch.randint(0, 360 * 640 // 64, (16, 32), generator=g, dtype=I32)
    for p in (None, prev):
        _check(lib, fr, p)
    bw = torch.stack([torch.zeros(3, 360, 640), torch.full((3, 360, 640), 255.0)]).to(dtype)
    assert _check(lib, bw, None)[1].tolist() == [0, 2 * 360 * 640]


@pytest.mark.parametrize("h,w", [(64, 96), (16, 53), (37, 53)])
def test_frames_off_the_16_byte_grid(h, w):
    """the frames as a view 1 and 4 bytes (uint8) and 4 bytes (float32) behind a 16-byte address"""
    from pips_amd import _lib
    lib = _lib.load()
    n = 3 * 3 * h * w
    for dtype, skips in ((torch.uint8, (1, 4)), (torch.float32, (1,))):                       # (skips in elements)
        fr = _frames(3, h, w, dtype, h)
        for skip in skips:
            buf = torch.zeros(n + 64, dtype=dtype, device=DEV)
            lead = (-buf.data_ptr() // buf.element_size()) % (16 // buf.element_size())       # elements up to the grid
            src = buf[lead + skip:lead + skip + n].view(3, 3, h, w)
            src.copy_(fr)
            assert src.data_ptr() % 16 == skip * buf.element_size() and src.is_contiguous()
            _check(lib, fr, None, src=src)


def test_bad_arguments_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    h, w, F = 44, 70, 2
    src = torch.randint(0, 256, (F, 3, h, w), dtype=torch.uint8, device=DEV)
    keep = src.clone()
    nbytes = lib.pips_cut_workspace_bytes(F, h, w)
    assert nbytes == F * 4 * 2 * 512
    hist = torch.full((F * 512,), POISON, dtype=I32, device=DEV)
    dist = torch.full((F,), POISON, dtype=I32, device=DEV)
    ws = torch.full((nbytes // 4,), POISON, dtype=I32, device=DEV)
    prev = torch.zeros(16, 32, dtype=I32, device=DEV)

    def call(**over):
        a = dict(dict(frames=_ptr(src), u8=1, F=F, h=h, w=w, prev=_ptr(prev), hist=_ptr(hist), dist=_ptr(dist), ws=_ptr(ws), bytes=nbytes),
                 **over)
        rc = lib.pips_cut_table(a["frames"], a["u8"], a["F"], a["h"], a["w"], a["prev"], a["hist"], a["dist"], a["ws"], a["bytes"],
                                _stream())
        torch.cuda.synchronize()
        assert bool((hist == POISON).all()) and bool((dist == POISON).all()) and bool((ws == POISON).all()) and torch.equal(src, keep)
        return rc

    for over in (dict(F=-1), dict(h=0), dict(w=0), dict(h=-3), dict(h=(1 << 15) + 1, w=1 << 15), dict(frames=None), dict(hist=None),
                 dict(dist=None), dict(ws=None), dict(F=1 << 25)):
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error()
    for short in (0, 1, nbytes - 1):
        assert call(bytes=short) == E_WORKSPACE
    assert call(F=0) == 0 and call(F=0, frames=None, hist=None, dist=None, ws=None, bytes=0) == 0     # nothing is launched
    assert lib.pips_abi_version() == 3


# ------------------------------------------------------------------ end to end on the device
def _cover(scan, **kw):
    from pips_amd import drivers
    return drivers.Cover(cell=ECELL, vis_thr=0.9, lost_after=2, scan=scan, **kw)


def _scene_video():
    """128 x 192, 21 + 19 frames of noise in [0, 100) / [150, 255]; the condition every test below rests on is asserted first, with the
    torch form alone: within a scene dist / 2hw <= 0.3, across the cut >= 0.7"""
    from pips_amd import drivers
    video = _scenes(EH, EW, 13)
    d = drivers.cut_table_torch(video[0])[1].double() / (2 * EH * EW)
    assert float(d[1:TA].max()) <= 0.3 and float(d[TA + 1:].max()) <= 0.3 and float(d[TA]) >= 0.7
    return video


def _covered(m, chunks, cover, queries, **kw):
    from pips_amd import drivers
    ct = drivers.CoverTracker(m, cover, queries, iters=6, slots=24, record_hops=True, **kw)
    parts = [ct.push(c) for c in chunks] + [ct.finish()]
    return ct, parts


@pytest.mark.parametrize("mode", ["exact", "bf16"])
@pytest.mark.parametrize("kw", [dict(rounds="torch", engine="torch"), dict(rounds="torch", engine="native"), dict(rounds="library")],
                         ids=["torch", "native", "library"])
def test_library_scan_equals_torch_scan_across_a_cut(weights_tamed, kw, mode):
    """a CoverTracker with cut_thr over the two scenes in chunks of 8 (the cut inside the third push): scan="library" hands out,
    push by push, the ids and the bits of scan="torch", with the same cut, births, retirements and hop lists"""
    from pips_amd import drivers
    m = _model(weights_tamed, mode)
    video = _scene_video()
    chunks = [video[:, i:i + 8] for i in range(0, TA + TB, 8)]
    runs = {scan: _covered(m, chunks, _cover(scan, cut_thr=0.5), _user(71).to(DEV), **kw) for scan in drivers.COVER_SCANS}
    (a, pa), (b, pb) = runs["torch"], runs["library"]
    _same_parts(pa, pb)
    assert a.cuts == b.cuts == [TA] and a.born == b.born and a.retired == b.retired and a.hops == b.hops
    assert torch.equal(a.book.prev_hist.cpu().long(), b.book.prev_hist.cpu().long()) and b.book.prev_hist.is_cuda
    cut = [i for i, (f, r) in a.retired.items() if r == "cut"]
    assert cut and all(a.retired[i][0] == TA - 1 for i in cut) and a.born.count(TA) == 6       # every cell of the new scene
    assert sum(p[1].shape[1] for p in pa) == TA + TB
    f0, t, v, ids = pa[2]                                                  # the push that holds the cut
    assert f0 < TA < f0 + t.shape[1] or f0 + t.shape[1] == TA
    assert sum(a.born[i] == TA for i in ids.tolist()) == 6
    _assert_live(pa, a.book, [0, 1], f"cover across a cut {kw} {mode}")


@pytest.mark.parametrize("kw", [dict(rounds="torch", engine="torch"), dict(rounds="library")], ids=["torch", "library"])
def test_a_covered_stream_with_a_cut_is_its_two_scenes_tracked_apart(weights_tamed, kw):
    """the A-part and B-part equalities of tests/test_cuts.py on the real model (fp32, every GEMM on route 0), scan="library": the
    single-scene runs are fed the same pieces, so each frame goes through the same encoder pass"""
    from pips_amd import drivers
    m = _model(weights_tamed)
    video = _scene_video()
    c, T = TA, TA + TB
    ct, parts = _covered(m, [video[:, i:i + 8] for i in range(0, T, 8)], _cover("library", cut_thr=0.5), _user(71).to(DEV), **kw)
    a, pa = _covered(m, _pieces(video, 8, c, 0, c), _cover("library"), _user(71).to(DEV), **kw)
    b, pb = _covered(m, _pieces(video, 8, c, c, T), _cover("library"), None, **kw)
    trajs, vis, born, _ = drivers._by_identity(parts, ct.book)
    ta, va, born_a, _ = drivers._by_identity(pa, a.book)
    tb, vb, born_b, _ = drivers._by_identity(pb, b.book)
    KA, KB = born_a.numel(), born_b.numel()
    _assert_route_0(max(p[3].numel() for p in parts + pa + pb), "exact")       # whoever shares a round: the same bits
    assert ct.cuts == [c] and born.numel() == KA + KB and KB >= 6
    assert born[:KA].tolist() == born_a.tolist() and born[KA:].tolist() == (born_b + c).tolist()
    assert torch.equal(_bits(trajs[:, :c, :KA]), _bits(ta)) and torch.equal(_bits(vis[:, :c, :KA]), _bits(va))
    assert torch.equal(_bits(trajs[:, c:, KA:]), _bits(tb)) and torch.equal(_bits(vis[:, c:, KA:]), _bits(vb))
    assert bool(trajs[:, c:, :KA].isnan().all()) and bool(trajs[:, :c, KA:].isnan().all())
    alive_a = [i for i in range(KA) if i not in a.retired]
    assert alive_a and {i: r for i, r in ct.retired.items() if i < KA} == {**a.retired, **{i: (c - 1, "cut") for i in alive_a}}
    assert {i - KA: (f - c, r) for i, (f, r) in ct.retired.items() if i >= KA} == b.retired
    assert ct.hops[:KA] == a.hops and ct.hops[KA:] == b.hops
    _assert_live(parts, ct.book, [0, 1], f"covered stream with a cut {kw}")


@pytest.mark.parametrize("mode", ["exact", "bf16"])
@pytest.mark.parametrize("slots", [9, 24])
def test_stream_cut_under_library_rounds_equals_torch_rounds(weights_tamed, slots, mode):
    """StreamTracker.cut() after 21 of 40 frames at 128 x 160, chunks of 8 split at the cut, a query waiting behind the cut and two
    added after it: rounds="library" returns the bits, the kept columns and the hop lists of rounds="torch" under both engines, and
    in fp32 (route 0) the columns before the cut are track_stream on the first 21 frames"""
    from pips_amd import drivers
    _assert_route_0(6, mode)
    m = _model(weights_tamed, mode)
    video = _video(TA + TB, H_, W_, seed=81)
    q1, q2 = _queries([0, 3, 11, 25, 20], 82), _queries([21, 30], 83)
    runs = {}
    for name, kw in (("library", dict(rounds="library")), ("torch", dict(rounds="torch", engine="torch")),
                     ("native", dict(rounds="torch", engine="native"))):
        st = drivers.StreamTracker(m, q1.to(DEV), iters=6, slots=slots, record_hops=True, **kw)
        parts = [st.push(p) for p in _pieces(video, 8, TA, 0, TA)]
        f0, t, v, keep = st.cut()
        assert keep.tolist() == [3] and f0 + t.shape[1] == TA == st.emitted and st.trajs.shape[1] == 1 and st.N == 1
        ended = st.cut_hops
        parts.append((f0, t, v))
        assert st.add_queries(q2.to(DEV)).tolist() == [1, 2]
        parts += [st.push(p) for p in _pieces(video, 8, TA, TA, TA + TB)] + [st.finish()]
        assert sum(p[1].shape[1] for p in parts) == TA + TB
        runs[name] = (parts, ended, st.hops)
    for other in ("torch", "native"):
        assert runs["library"][1:] == runs[other][1:], other
        for (f0, t, v), (g0, gt, gv) in zip(runs["library"][0], runs[other][0]):
            assert f0 == g0 and torch.equal(_bits(t), _bits(gt)) and torch.equal(_bits(v), _bits(gv)), other
    if mode == "exact":
        parts, ended, _ = runs["library"]
        n1 = len(_pieces(video, 8, TA, 0, TA)) + 1
        got_t, got_v = torch.cat([p[1] for p in parts[:n1]], dim=1), torch.cat([p[2] for p in parts[:n1]], dim=1)
        cols = [0, 1, 2, 4]
        ref_t, ref_v, ref_h = drivers.track_stream(m, _pieces(video, 8, TA, 0, TA), q1[:, cols].to(DEV), iters=6, slots=slots,
                                                   return_hops=True, rounds="library")
        assert torch.equal(_bits(got_t[:, :, cols]), _bits(ref_t)) and torch.equal(_bits(got_v[:, :, cols]), _bits(ref_v))
        assert [ended[k] for k in cols] == ref_h and bool(got_t[:, :, 3].isnan().all())
