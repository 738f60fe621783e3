"""GPU: every launch split, grid cap and stride loop of DESIGN.md's "Launch seams" crossed once, on the cases made and sized in
tests/test_seams.py.  pips_masks_tint over more frames than one launch's table holds; pips_object_masks, pips_tracks_draw,
pips_tracks_draw_ex and pips_frames_warp at 65535 and 65537 frames of 3 x 5 pixels, whose inputs repeat with a period of 7 frames so
that the twin runs on one period; pips_stream_keep past its rows of blocks, its blocks along a row and the feature mover's stride;
pips_stream_emit / pips_stream_emit_cols past one block and past 64 blocks along a row; the bf16 resize past its 4096 blocks.
Every output is compared bit for bit (the resize: under test_encoder_stages_gpu's fp64 bound) inside poisoned, pitched
allocations that must come back untouched outside the image; workspaces have the size the header states and a poisoned tail; the
inputs come back unchanged; every call goes to the current torch stream."""
import ctypes as C

import pytest
import torch

from test_clips_gpu import LENGTHS_C, NAN_FILL
from test_draw import SENTINEL, outside_untouched, views
from test_draw_ex import WIDE, untouched_outside as untouched_outside_ex
from test_draw_ex_gpu import _dev
from test_encoder_stages_gpu import _resize_check
from test_masks_gpu import GUARD, _guarded, _only_the_image_changed
from test_seams import (DRAW_FADE_INTS, DRAW_INTS, DRAW_TRAIL, EMIT_COLS_M, EMIT_COLS_N, EMIT_L, EMIT_N, FRAME_COUNTS, FRAME_SIZE, JOIN_N_NEW,
                        KEEP_CASES, LIST_COUNTS, MASK_RADIUS8, MASK_VOTES, RESIZE_BF16_STRIDE, TINT_SIZE, V_, WARP_BORDER, WARP_FILL, chain_seam_state, chain_step_reference,
                        draw_frames, draw_reference,
                        emit_cols_list, emit_cols_reference, emit_frames, emit_reference, keep_list, keep_reference, keep_state,
                        mask_reference, mask_seam_inputs, periodic, periodic_index, ring, tint_reference, tint_seam_cases, tint_seam_id,
                        warp_reference, warp_seam_inputs)
from test_stream_rounds_gpu import H_, W_, _bits, _model, _queries, _video
from test_warp import make_surfaces, untouched_outside as warp_untouched_outside, views_like

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
POISON = -77
_cache = {}


def _once(key, make):
    """a reference made once, on the CPU, shared by the cases that need it and never written to"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _first_bad(got, want):
    """the first frames at which two (F, ...) tensors differ"""
    return torch.nonzero((got != want).flatten(1).any(dim=1)).flatten()[:4].tolist()


# ------------------------------------------------------------------------------------------------- tint across launches
@pytest.mark.parametrize("case", tint_seam_cases(), ids=tint_seam_id)
def test_masks_tint_over_more_frames_than_a_launch_holds(case):
    """F frames at TINT_ALPHAS / C frames a launch: the second and third launch's f0, their slice of the opacity table and their rows
    of the colours, against drivers.tint_masks_torch on the CPU"""
    from pips_amd import drivers
    fmt, nlab, F = case
    h, w = TINT_SIZE
    bufs, mbuf, colors, alpha, want = _once(("tint", case), lambda: tint_reference(case))
    flats = [torch.full((2 * GUARD + b.numel(),), SENTINEL, dtype=torch.uint8, device=DEV) for b in bufs + [mbuf]]
    dev = [f[GUARD:GUARD + b.numel()].view(b.shape) for f, b in zip(flats, bufs + [mbuf])]
    for d, b in zip(dev, bufs + [mbuf]):
        d.copy_(b)
    planes, masks = views(dev[:-1], fmt, h, w), dev[-1][:, :h, :w]
    d_colors = colors.to(DEV)
    got = drivers.tint_masks(planes, fmt, masks, d_colors, alpha / 256.0, inplace=True)
    torch.cuda.synchronize()
    got = [got] if torch.is_tensor(got) else got
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, planes))
    for k, (a, b) in enumerate(zip(planes, want)):
        a = a.cpu()
        assert torch.equal(a, b), (tint_seam_id(case), k, int((a != b).sum()), _first_bad(a, b))
    assert outside_untouched([d.cpu() for d in dev[:-1]], bufs, fmt, h, w)            # padding, gaps, the alpha byte
    assert all(bool((f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all()) for f in flats)
    assert torch.equal(dev[-1].cpu(), mbuf) and torch.equal(d_colors.cpu(), colors)


# ------------------------------------------------------------------------------------------------- 65535 frames a launch
@pytest.mark.parametrize("F", FRAME_COUNTS)
@pytest.mark.parametrize("vote", MASK_VOTES)
def test_object_masks_past_the_frames_of_a_launch(vote, F):
    """frame f of the call is frame f % 7 of the twin's period: the records that mask_prepare_kernel writes at f_base + blockIdx.y
    and mask_raster_kernel reads there, and the image it writes at f step"""
    from pips_amd import _lib
    lib = _lib.load()
    h, w = FRAME_SIZE
    rows, lab = mask_seam_inputs()
    n = rows.shape[1]
    rows, lab = periodic(rows, F), periodic(lab, F).to(torch.uint8)
    want = _once(("masks", vote), lambda: mask_reference(vote))
    d_rows, d_lab = rows.to(DEV), lab.to(DEV)
    need = lib.pips_object_masks_workspace_bytes(F, n)
    assert need == 8 * F * n
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    flat, out, pitch, step = _guarded(F, h, w)
    rc = lib.pips_object_masks(d_rows.data_ptr(), d_lab.data_ptr(), F, n, 0, F, h, w, h, w, MASK_RADIUS8, vote, out.data_ptr(), pitch, step,
                               ws.data_ptr(), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    got, want = out.cpu(), want[periodic_index(F)]
    assert torch.equal(got, want), (vote, F, int((got != want).sum()), _first_bad(got, want))
    assert _only_the_image_changed(flat, out)
    assert bool((ws[need:] == 0x5A).all())
    assert torch.equal(d_rows.cpu().view(I32), rows.view(I32)) and torch.equal(d_lab.cpu(), lab)


def _draw_case(fmt, F, faded):
    from pips_amd import ops
    h, w = FRAME_SIZE
    bufs, trajs, vis, colors = draw_frames(fmt, F)
    want, _ = _once(("draw", fmt, faded), lambda: draw_reference(fmt, faded))
    dev_bufs = [_dev(b) for b in bufs]
    planes = views(dev_bufs, fmt, h, w)
    n = trajs.shape[2]
    need = ops.draw_workspace_bytes(F, n, DRAW_TRAIL)
    assert need == 4 * F * n * (2 * DRAW_TRAIL + 10)
    ws = torch.full((need // 4 + 16,), POISON, dtype=I32, device=DEV)
    d_trajs, d_vis, d_colors = trajs[0].to(DEV), vis[0].to(DEV), colors.to(DEV)
    ops.draw_tracks(planes, fmt, d_trajs, d_vis, d_colors, 0, None, DRAW_TRAIL, *DRAW_INTS, 0.0, "bt709", "limited", workspace=ws,
                    fade=list(DRAW_FADE_INTS) if faded else None)
    torch.cuda.synchronize()
    at = periodic_index(F, DRAW_TRAIL)
    for k, (a, b) in enumerate(zip(planes, want)):
        a, b = a.cpu(), b[at]
        assert torch.equal(a, b), (fmt, F, faded, k, int((a != b).sum()), _first_bad(a, b))
    assert untouched_outside_ex([b.cpu() for b in dev_bufs], bufs, fmt, h, w)
    assert bool((ws[need // 4:] == POISON).all())
    assert torch.equal(d_trajs.cpu().view(I32), trajs[0].view(I32)) and torch.equal(d_vis.cpu().view(I32), vis[0].view(I32))
    assert torch.equal(d_colors.cpu(), colors)


@pytest.mark.parametrize("F", FRAME_COUNTS)
@pytest.mark.parametrize("fmt", ["planar8", "nv12"])
def test_tracks_draw_past_the_frames_of_a_launch(fmt, F):
    """pips_tracks_draw: the boxes and records of draw_prepare_kernel at f_base + blockIdx.y and draw_raster_kernel's frame; the
    first DRAW_TRAIL frames, whose trails are cut at row 0, against a twin run of their own"""
    _draw_case(fmt, F, False)


@pytest.mark.parametrize("F", FRAME_COUNTS)
@pytest.mark.parametrize("fmt", ["planar8", "nv12", "p010"])
def test_tracks_draw_ex_past_the_frames_of_a_launch(fmt, F):
    """pips_tracks_draw_ex with the fade table (256, 128): the form of the raster kernel that takes the table as its last argument"""
    _draw_case(fmt, F, True)


@pytest.mark.parametrize("F", FRAME_COUNTS)
@pytest.mark.parametrize("fmt", list(WARP_BORDER))
def test_frames_warp_past_the_frames_of_a_launch(fmt, F):
    """pips_frames_warp: warp_kernel's row of the coefficients and both surfaces at f_base + blockIdx.y"""
    from pips_amd import ops
    h, w = FRAME_SIZE
    coef, (_, period) = warp_seam_inputs(fmt)
    want = _once(("warp", fmt), lambda: warp_reference(fmt))
    s_flats, s_views = make_surfaces(fmt, F, h, w, seed=90, off=1, pad=3, gap=6)
    for v, p in zip(s_views, period):
        v.copy_(periodic(p, F))
    d_flats, d_views = make_surfaces(fmt, F, h, w, seed=None, off=1 if fmt in WIDE else 2, pad=4, gap=10)
    coef = periodic(coef, F).to(I32)
    s_dev, s_planes = views_like(s_flats, s_views, DEV)
    d_dev, d_planes = views_like(d_flats, d_views, DEV)
    d_coef = coef.to(DEV)
    got = ops.warp_frames(s_planes, fmt, d_coef, WARP_BORDER[fmt], WARP_FILL, out=d_planes)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, d_planes))
    at = periodic_index(F)
    for k, (a, b) in enumerate(zip(d_planes, want)):
        a, b = a.cpu(), b[at]
        assert torch.equal(a, b), (fmt, F, k, int((a != b).sum()), _first_bad(a, b))
    assert warp_untouched_outside([f.cpu() for f in d_dev], d_views)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s_dev, s_flats)) and torch.equal(d_coef.cpu(), coef)


# ------------------------------------------------------------------------------------------------- pips_stream_keep
TAIL = 64                                                            # poisoned words behind an output


def _input(t, off):
    """an int32 array on the device, its base on the allocation's own (256-byte) boundary or ``off`` words behind it"""
    buf = torch.full((t.numel() + off,), POISON, dtype=I32, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _output(shape, off):
    """-> (allocation, view): a poisoned output of ``shape`` with ``off`` poisoned words in front of it and TAIL behind"""
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.full((off + numel + TAIL,), POISON, dtype=I32, device=DEV)
    return buf, buf[off:off + numel].view(shape)


def _around(buf, view, off):
    return bool((buf[:off] == POISON).all() and (buf[off + view.numel():] == POISON).all())


KEEP_ORDER = ["n", "keep", "m", "tq", "xy", "cur", "status", "clip", "feat", "trajs", "vis", "L", "tq_out", "xy_out", "cur_out", "status_out",
              "clip_out", "feat_out", "trajs_out", "vis_out", "V", "counts"]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-grid"])
@pytest.mark.parametrize("case", KEEP_CASES, ids=lambda c: "L%d-n%d-m%d" % c)
def test_stream_keep_past_its_rows_columns_and_feature_stride(case, off):
    """rows of blocks beyond KEEP_ROWS_Y (y += ry), more kept columns than 64 blocks hold (j += gridDim.x * SEL_THREADS) and the
    feature mover's stride, with the buffers on the 8- / 16-byte grid and one word off it, with and without a clip table; the keep
    list holds -1 and n.  Every output is poisoned before the call, so a row that is never written shows"""
    from pips_amd import _lib
    lib = _lib.load()
    L, n, m = case
    s = _once(("keep", case), lambda: keep_state(n, L, seed=500 + n))
    keep = keep_list(n, m)
    for clips in (False, True):
        want, want_counts = keep_reference(s, keep, n, clips)
        ins = {k: _input(v, off) for k, v in s.items()}
        d_keep = torch.tensor(keep, dtype=I32, device=DEV)
        shapes = dict(tq_out=(m,), xy_out=(m, 2), cur_out=(m,), status_out=(m,), clip_out=(m,), feat_out=(m, 128), trajs_out=(L, m, 2),
                      vis_out=(L, m), counts=(4 + V_ if clips else 4,))
        outs = {k: _output(shape, off if k != "counts" else 0) for k, shape in shapes.items()}
        a = dict(ins, **{k: v for k, (_, v) in outs.items()}, n=n, m=m, L=L, V=V_ if clips else 0, keep=d_keep)
        if not clips:
            a["clip"] = a["clip_out"] = None
        assert (a["trajs"].data_ptr() % 16, a["trajs_out"].data_ptr() % 16, a["feat"].data_ptr() % 16) == (4 * off,) * 3
        rc = lib.pips_stream_keep(*[(_lib.ptr(a[k]) if torch.is_tensor(a[k]) or a[k] is None else a[k]) for k in KEEP_ORDER], _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.pips_last_error()
        assert outs["counts"][1].tolist() == want_counts, (case, off, clips)
        for name in ("tq", "xy", "cur", "status", "feat", "trajs", "vis") + (("clip",) if clips else ()):
            buf, view = outs[name + "_out"]
            got = view.cpu()
            assert torch.equal(got, want[name]), (case, off, clips, name, int((got != want[name]).sum()),
                                                  torch.nonzero(got != want[name])[:3].tolist())
            assert _around(buf, view, off), (case, off, clips, name)
        if not clips:
            assert bool((outs["clip_out"][0] == POISON).all())
        for name, t in s.items():                                     # every input array is bit-identical afterwards
            assert torch.equal(ins[name].cpu(), t), name
        assert torch.equal(d_keep.cpu(), torch.tensor(keep, dtype=I32))


# ------------------------------------------------------------------------------------------------- pips_stream_emit / _emit_cols
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-grid"])
@pytest.mark.parametrize("n", EMIT_N)
def test_stream_emit_past_one_block_and_past_the_blocks_of_a_row(n, off):
    """L = 17 over the wrapping range: 16-byte pieces on aligned buffers where the row allows them, words otherwise and one word
    off the grid (n = 300: three blocks of words; 8193, 32772 and 32768: emit_row's stride by 64 x 256 threads, and exactly one
    pass).  The outputs are the rows' bits, the emitted rows hold 0x7fc00000, every other row is bit-identical"""
    from pips_amd import _lib
    lib = _lib.load()
    L = EMIT_L
    f0, f1 = emit_frames(L)
    trajs, vis = _once(("ring", n), lambda: ring(L, n, 600 + n))
    want = _once(("emit", n), lambda: emit_reference(trajs, vis, f0, f1))
    d_t, d_v = _input(trajs, off), _input(vis, off)
    (bt, out_t), (bv, out_v) = _output((f1 - f0, n, 2), off), _output((f1 - f0, n), off)
    rc = lib.pips_stream_emit(_lib.ptr(d_t), _lib.ptr(d_v), L, n, f0, f1, _lib.ptr(out_t), _lib.ptr(out_v), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    for name, got, exp in (("out_trajs", out_t, want[0]), ("out_vis", out_v, want[1]), ("trajs", d_t, want[2]), ("vis", d_v, want[3])):
        got = got.cpu()
        assert torch.equal(got, exp), (n, off, name, int((got != exp).sum()), torch.nonzero(got != exp)[:3].tolist())
    assert _around(bt, out_t, off) and _around(bv, out_v, off)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "odd-word"])
@pytest.mark.parametrize("m", EMIT_COLS_M)
def test_stream_emit_cols_past_one_block(m, off):
    """m = 256, 257 and 600 columns of n = 700, -1 and n among them: blockIdx.x * SEL_THREADS + threadIdx.x in the second and third
    block, on 8-byte aligned and on odd-word buffers"""
    from pips_amd import _lib
    lib = _lib.load()
    L, n = EMIT_L, EMIT_COLS_N
    f0, f1 = emit_frames(L)
    trajs, vis = _once(("ring", n), lambda: ring(L, n, 600 + n))
    cols = emit_cols_list(n, m)
    want = emit_cols_reference(trajs, vis, f0, f1, cols)
    d_t, d_v, d_cols = _input(trajs, off), _input(vis, off), torch.tensor(cols, dtype=I32, device=DEV)
    (bt, out_t), (bv, out_v) = _output((f1 - f0, m, 2), off), _output((f1 - f0, m), off)
    assert d_t.data_ptr() % 8 == 4 * off and out_t.data_ptr() % 8 == 4 * off
    rc = lib.pips_stream_emit_cols(_lib.ptr(d_t), _lib.ptr(d_v), L, n, f0, f1, _lib.ptr(d_cols), m, _lib.ptr(out_t), _lib.ptr(out_v), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    for name, got, exp in (("out_trajs", out_t, want[0]), ("out_vis", out_v, want[1]), ("trajs", d_t, want[2]), ("vis", d_v, want[3])):
        got = got.cpu()
        assert torch.equal(got, exp), (m, off, name, int((got != exp).sum()), torch.nonzero(got != exp)[:3].tolist())
    assert _around(bt, out_t, off) and _around(bv, out_v, off) and d_cols.cpu().tolist() == cols


@pytest.mark.parametrize("n", JOIN_N_NEW)
def test_a_round_joins_more_queries_than_one_block_gathers(n, weights_tamed, monkeypatch):
    """stream_join_gather_kernel has ceil(n_new / 256) blocks and is reached through pips_stream_round alone: 256 and 257 queries on
    frame 0 join in one round (the n_new the entry is called with is recorded), and the stream's trajectories, visibilities and hops
    under rounds="library" are those of the torch rounds on the native engine, bit for bit.  Both hop the same list of queries in one
    call, so the GEMMs of both see the same row count and take the same route"""
    from pips_amd import drivers, ops
    joined, real = [], ops._call

    def recorded(name, *args):
        if name == "pips_stream_round":
            joined.append(args[13])
        return real(name, *args)

    m = _model(weights_tamed)
    video = _video(9, H_, W_, seed=46)
    q = _queries([0] * n, seed=47).to(DEV)
    ref, ref_vis, ref_hops = drivers.track_stream(m, [video], q, iters=3, slots=24, return_hops=True, engine="native")
    monkeypatch.setattr(ops, "_call", recorded)
    got, vis, hops = drivers.track_stream(m, [video], q, iters=3, slots=24, return_hops=True, rounds="library")
    assert max(joined) == n and hops == ref_hops
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(_bits(vis), _bits(ref_vis))
    assert tuple(got.shape) == (1, 9, n, 2) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------- single-block list kernels
@pytest.mark.parametrize("n_act", LIST_COUNTS)
def test_chain_step_clips_over_the_chunks_of_its_one_block(n_act):
    """pips_chain_step_clips with sample_feat at 255, 256, 257 and 513 active particles: the offset of next_active carried from
    chunk to chunk and the rows of win_ffeat0 that chunk j0 copies, against test_clips_gpu's torch lines of a hop; steps, window
    starts, the carried features and trajs / vis as bit patterns over the whole NaN-payload buffers"""
    from pips_amd import ops
    s = _once(("chain", n_act), lambda: chain_seam_state(n_act))
    exp = _once(("chain-ref", n_act), lambda: chain_step_reference(s, True, True))
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    frames = torch.tensor(LENGTHS_C, dtype=I32, device=DEV)
    nxt = torch.full((n_act + 8,), POISON, dtype=I32, device=DEV)
    count = torch.full((1,), -1, dtype=I32, device=DEV)
    steps = torch.full((n_act + 8,), POISON, dtype=I32, device=DEV)
    ops.chain_step(d["win_trajs"], d["win_vis"], d["win_ffeat0"], sum(LENGTHS_C), d["active"], n_act, d["trajs"], d["vis"], s["base"], d["cur"],
                   d["dirs"], d["feat"], nxt, count, steps, sample_feat=True, clips=(d["clip"], frames))
    torch.cuda.synchronize()
    bits = lambda t: t.detach().cpu().contiguous().view(I32)
    k = exp["next_active"].numel()
    assert int(count.item()) == k
    assert torch.equal(nxt.cpu()[:k], exp["next_active"]) and bool((nxt.cpu()[k:] == POISON).all())
    assert torch.equal(steps.cpu()[:n_act], exp["steps"]) and bool((steps.cpu()[n_act:] == POISON).all())
    assert torch.equal(d["cur"].cpu(), exp["cur"]) and torch.equal(bits(d["feat"]), bits(exp["feat"]))
    assert torch.equal(bits(d["trajs"]), bits(exp["trajs"])) and torch.equal(bits(d["vis"]), bits(exp["vis"]))
    assert int((bits(exp["trajs"]) != NAN_FILL).sum()) == 8 * n_act * 2
    for name in ("win_trajs", "win_vis", "win_ffeat0", "active", "dirs", "clip"):
        assert torch.equal(bits(d[name]), bits(s[name])), name


# ------------------------------------------------------------------------------------------------- capped element-wise grids
def test_resize_into_bf16_grid_stride():
    """24 x (23, 31) -> (46, 62) x 128 in bf16: 1 095 168 groups of eight channels against resize_into_bf16_kernel's 4096 x 256
    threads -- the second pass of its loop, which test_encoder_stages_gpu's 12 frames (547 584 groups) do not reach"""
    Fr, hs, hd, Cc, coff = RESIZE_BF16_STRIDE
    _resize_check("resize bf16 grid-stride of the bf16 kernel", Fr, hs, hd, Cc, coff, "bf16")
