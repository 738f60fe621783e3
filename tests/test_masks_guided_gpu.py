"""GPU: object masks that follow image edges in the library.  pips_object_masks_guided and pips_guide_plane are held, byte for byte,
to their torch twins run on the CPU (drivers.object_masks_guided_torch, itself held to a heap Dijkstra in
tests/test_masks_guided.py, and drivers.guide_plane_torch) on the cases made and shown to earn their place there.  Outputs are
views of poisoned allocations with 256-byte guard bands whose padding, gaps and bands must come back untouched; mask and guide
have padded pitch and step; the workspace has the size the header states and a poisoned tail; inputs come back unchanged.  The
call is crossed at 65535 frames a launch with a periodic expectation, and end to end the planted scene goes through motion_layers
-> guide_plane -> object_masks_guided -> object_colors -> tint_masks on pitched NV12 to the bytes of the torch route."""
import ctypes as C

import pytest
import torch

from test_draw import SENTINEL, buffers, outside_untouched, views
from test_masks import MEANING_SCENES, meaning_scene
from test_masks_gpu import GUARD, _guarded, _only_the_image_changed
from test_masks_guided import (FRAME_COUNTS, SEAM_EDGE, SEAM_REACH, SEAM_SIZE, guided_case_inputs, guided_cases, guided_id, periodic,
                               seam_inputs, seam_reference, twin)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_want = {}


def _reference(case):
    """the twin's masks of a case, on the CPU, made once and never written to"""
    if case[0] not in _want:
        _want[case[0]] = twin(case)
    return _want[case[0]]


def _guarded_copy(t, pad=(9, 3)):
    """a (F,h,w) uint8 tensor as a view of pitch w + pad[0] and step pitch * (h + pad[1]) inside a poisoned allocation on the device"""
    flat, view, pitch, step = _guarded(*t.shape, pad=pad)
    view.copy_(t)
    return flat, view, pitch, step


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _first_bad(got, want):
    return torch.nonzero((got != want).flatten(1).any(dim=1)).flatten()[:4].tolist()


@pytest.mark.parametrize("case", guided_cases(), ids=guided_id)
def test_object_masks_guided_is_the_twin(case):
    from pips_amd import _lib
    name, h, w, n, edge, reach, F, src, kind, cluster = case
    rows, lab, guide, first = guided_case_inputs(case)
    want = _reference(case)
    G = rows.shape[0]
    src_h, src_w = src or (h, w)
    d_rows, d_lab = rows.to(DEV), lab.to(torch.uint8).to(DEV)
    gflat, d_guide, gpitch, gstep = _guarded_copy(guide)
    gbefore = gflat.clone()
    lib = _lib.load()
    need = lib.pips_object_masks_guided_workspace_bytes(F, n, h, w)
    assert need == (0 if n == 0 else (8 * F * n + 15) // 16 * 16 + 8 * F * h * w)
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    flat, out, pitch, step = _guarded(F, h, w)
    rc = lib.pips_object_masks_guided(d_rows.data_ptr(), d_lab.data_ptr(), G, n, first, F, src_h, src_w, h, w, edge, reach, d_guide.data_ptr(),
                                      gpitch, gstep, out.data_ptr(), pitch, step, ws.data_ptr(), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    got = out.cpu()
    assert torch.equal(got, want), (name, int((got != want).sum()))
    assert _only_the_image_changed(flat, out)
    assert bool((ws[need:] == 0x5A).all())
    assert torch.equal(gflat, gbefore)
    assert torch.equal(d_rows.cpu().view(torch.int32), rows.view(torch.int32)) and torch.equal(d_lab.cpu(), lab.to(torch.uint8))


@pytest.mark.parametrize("case", [c for c in guided_cases() if c[0] in ("two-tiles-across", "n600-clustered", "no-column", "resized")], ids=guided_id)
def test_ops_and_drivers_give_the_same_bytes(case):
    from pips_amd import drivers, ops
    name, h, w, n, edge, reach, F, src, kind, cluster = case
    rows, lab, guide, first = guided_case_inputs(case)
    want = _reference(case)
    rows, lab, guide = rows[:first + F].to(DEV), lab[:first + F].to(DEV), guide.to(DEV)
    got = ops.object_masks_guided(rows, lab.to(torch.uint8), guide, (h, w), src, edge, reach, first)
    assert torch.equal(got.cpu(), want)
    flat, out, _, _ = _guarded(F, h, w, pad=(3, 1))
    _, pitched, _, _ = _guarded_copy(guide, pad=(2, 5))
    ws = torch.full((ops.object_masks_guided_workspace_bytes(F, n, h, w) // 4 + 8,), -77, dtype=torch.int32, device=DEV)
    assert ops.object_masks_guided(rows, lab.to(torch.uint8), pitched, (h, w), src, edge, reach, first, out=out, workspace=ws) is out
    assert torch.equal(out.cpu(), want) and _only_the_image_changed(flat, out) and bool((ws[-8:] == -77).all())
    got = drivers.object_masks_guided(rows[None], lab, pitched, src or (h, w), out_size=(h, w), radius=reach / 5.0, edge=edge, first=first)
    assert got.is_cuda and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("fmt", ["rgb24", "bgr24", "rgba32", "bgra32", "planar8"])
def test_guide_plane_is_the_twin(fmt):
    from pips_amd import drivers, ops
    F, h, w = 2, 33, 70
    bufs = buffers(fmt, F, h, w, 40 + len(fmt), pad=(7, 3))
    want = drivers.guide_plane_torch(views(bufs, fmt, h, w), fmt)
    flats = [torch.full((2 * GUARD + b.numel(),), SENTINEL, dtype=torch.uint8, device=DEV) for b in bufs]
    dev = [f[GUARD:GUARD + b.numel()].view(b.shape) for f, b in zip(flats, bufs)]
    for d, b in zip(dev, bufs):
        d.copy_(b)
    planes = views(dev, fmt, h, w)
    got = drivers.guide_plane(planes, fmt)
    assert got.is_cuda and got.is_contiguous() and torch.equal(got.cpu(), want)
    for pad in ((5, 2), (3, 1)):                                     # rows on and off a dword address
        flat, out, _, _ = _guarded(F, h, w, pad=pad)
        assert ops.guide_plane(planes, fmt, out=out) is out
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want) and _only_the_image_changed(flat, out)
    assert all(torch.equal(d.cpu(), b) for d, b in zip(dev, bufs))
    assert all(bool((f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all()) for f in flats)


def test_return_codes_on_the_device_path():
    from pips_amd import _lib
    lib = _lib.load()
    rows = torch.rand(2, 5, 2, device=DEV) * 8
    lab = torch.zeros(2, 5, dtype=torch.uint8, device=DEV)
    guide = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    flat, out, pitch, step = _guarded(2, 8, 8)
    ws = torch.zeros(2048, dtype=torch.uint8, device=DEV)
    need = lib.pips_object_masks_guided_workspace_bytes(2, 5, 8, 8)
    assert need == 80 + 2 * 4 * 2 * 8 * 8

    def call(p=ws.data_ptr(), nbytes=need, edge=4, reach=240, g=guide.data_ptr(), gpitch=8):
        return lib.pips_object_masks_guided(rows.data_ptr(), lab.data_ptr(), 2, 5, 0, 2, 8, 8, 8, 8, edge, reach, g, gpitch, 64, out.data_ptr(),
                                            pitch, step, p, nbytes, None)
    assert call(nbytes=need - 1) == -1 and lib.pips_last_error().decode().startswith("object_masks_guided: workspace")
    assert call(p=ws.data_ptr() + 8) == -1 and b"16-byte" in lib.pips_last_error()
    assert call(edge=65) == -1 and lib.pips_last_error().decode().startswith("object_masks_guided: edge")
    assert call(reach=32768) == -1 and lib.pips_last_error().decode().startswith("object_masks_guided: reach")
    assert call(g=None) == -1 and lib.pips_last_error().decode().startswith("object_masks_guided: null guide")
    assert call(gpitch=7) == -1 and lib.pips_last_error().decode().startswith("object_masks_guided: guide pitch")
    rgb = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=DEV)
    plane = lambda fmt, gp=pitch: lib.pips_guide_plane(fmt, 2, 8, 8, rgb.data_ptr(), 8, 192, rgb[:, 1].data_ptr(), 8, 192, rgb[:, 2].data_ptr(), 8,
                                                       192, out.data_ptr(), gp, step, None)
    for fmt in (4, 5, 6, 7):
        assert plane(fmt) == -1 and lib.pips_last_error().decode().startswith("guide_plane: format")
    assert plane(8, 7) == -1 and lib.pips_last_error().decode().startswith("guide_plane: guide pitch")
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all()) and bool((ws == 0).all())   # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).any())
    assert plane(8) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and _only_the_image_changed(flat, out)


@pytest.mark.parametrize("F", FRAME_COUNTS)
def test_object_masks_guided_past_the_frames_of_a_launch(F):
    """frame f of the call is frame f % 7 of the twin's period: the records guided_prepare_kernel writes at f_base + blockIdx.y, the
    guide and the key planes guided_relax_kernel reads and writes there (SEAM_REACH takes two launches), the image at f step"""
    from pips_amd import _lib, ops
    lib = _lib.load()
    h, w = SEAM_SIZE
    rows, lab, guide, _ = seam_inputs()
    rows, lab, guide = periodic(rows, F), periodic(lab, F).to(torch.uint8), periodic(guide, F)
    want = periodic(seam_reference(), F)
    assert ops.guided_launches(SEAM_REACH) == 2
    d_rows, d_lab = rows.to(DEV), lab.to(DEV)
    gflat, d_guide, gpitch, gstep = _guarded_copy(guide, pad=(1, 1))
    need = lib.pips_object_masks_guided_workspace_bytes(F, 1, h, w)
    assert need == (8 * F + 15) // 16 * 16 + 8 * F * h * w
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    flat, out, pitch, step = _guarded(F, h, w)
    rc = lib.pips_object_masks_guided(d_rows.data_ptr(), d_lab.data_ptr(), F, 1, 0, F, h, w, h, w, SEAM_EDGE, SEAM_REACH, d_guide.data_ptr(), gpitch,
                                      gstep, out.data_ptr(), pitch, step, ws.data_ptr(), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    got = out.cpu()
    assert torch.equal(got, want), (F, int((got != want).sum()), _first_bad(got, want))
    assert _only_the_image_changed(flat, out)
    assert bool((ws[need:] == 0x5A).all())
    assert torch.equal(d_rows.cpu().view(torch.int32), rows.view(torch.int32)) and torch.equal(d_lab.cpu(), lab)


@pytest.mark.parametrize("F", FRAME_COUNTS)
def test_guide_plane_past_the_rows_of_blocks_of_a_grid(F):
    """guide_plane_kernel's blocks walk the frames blockIdx.y, blockIdx.y + gridDim.y, ...: frame f is frame f % 7 of the period"""
    from pips_amd import drivers, ops
    h, w = SEAM_SIZE
    rgb = seam_inputs()[3]
    want = periodic(drivers.guide_plane_torch([rgb], "planar8"), F)
    d_rgb = periodic(rgb, F).to(DEV)
    flat, out, _, _ = _guarded(F, h, w, pad=(2, 1))
    ops.guide_plane([d_rgb], "planar8", out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, want), (F, _first_bad(got, want))
    assert _only_the_image_changed(flat, out)


def test_end_to_end_on_the_planted_scene():
    """motion_layers -> guide_plane -> object_masks_guided -> object_colors -> tint_masks on pitched NV12 surfaces of the planted
    scene's pair is, byte for byte, the torch route on the CPU.  The Y plane shows the object: luma 150 on the rectangle of its nodes
    grown by 5 px, 90 around it, noise of +-3 -- the guide is that plane as the strided view it is, and the object's mask is the
    rectangle the image shows, not the one halfway to the next tracks that the Voronoi rule draws"""
    from pips_amd import drivers
    H, W = 240, 320
    shift, seed = MEANING_SCENES[0]
    trajs, obj, (x0, y0, x1, y1) = meaning_scene(shift, seed)
    kw = dict(thr=2.0, hypotheses=256, layers=3, min_inliers=8)
    bufs = buffers("nv12", 1, H, W, 21, pad=(64, 8))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    box = (xx >= x0 - 5) & (xx <= x1 + 5) & (yy >= y0 - 5) & (yy <= y1 + 5)
    noise = torch.randint(-3, 4, (H, W), generator=torch.Generator().manual_seed(5))
    bufs[0][0, :H, :W] = (torch.where(box, 150, 90) + noise).to(torch.uint8)
    ref = drivers.motion_layers_torch(trajs[None], **kw)
    ref_guide = drivers.guide_plane_torch(views(bufs, "nv12", H, W), "nv12")
    ref_masks = drivers.object_masks_guided_torch(trajs[None, 1:], ref[2], ref_guide, (H, W))
    colors, alpha = drivers.object_colors(ref[3], alpha=0.6)
    want = drivers.tint_masks_torch(views(bufs, "nv12", H, W), "nv12", ref_masks, colors, alpha)
    mine = int(ref[2][0][obj][0])
    voronoi = drivers.object_masks_torch(trajs[None, 1:], ref[2], (H, W), vote=1)
    miss, miss_voronoi = int(((ref_masks[0] == mine) != box).sum()), int(((voronoi[0] == mine) != box).sum())
    print(f"pixels that differ from the box: guided {miss}, nearest track {miss_voronoi}")
    assert miss_voronoi > 500 and miss <= 0.05 * miss_voronoi

    d_trajs = trajs.to(DEV)
    res = drivers.motion_layers(d_trajs[None], **kw)
    assert torch.equal(res[2].cpu(), ref[2]) and torch.equal(res[3].cpu(), ref[3])
    d_bufs = [b.to(DEV) for b in bufs]
    planes = views(d_bufs, "nv12", H, W)
    guide = drivers.guide_plane(planes, "nv12")
    assert guide.data_ptr() == planes[0].data_ptr() and guide.stride() == planes[0].stride() and not guide.is_contiguous()
    masks = drivers.object_masks_guided(d_trajs[None, 1:], res[2], guide, (H, W))
    assert torch.equal(masks.cpu(), ref_masks), int((masks.cpu() != ref_masks).sum())
    d_colors, d_alpha = drivers.object_colors(res[3], alpha=0.6)
    drivers.tint_masks(planes, "nv12", masks, d_colors, d_alpha, inplace=True)
    torch.cuda.synchronize()
    for a, b in zip(planes, want):
        assert torch.equal(a.cpu(), b), int((a.cpu() != b).sum())
    assert outside_untouched([b.cpu() for b in d_bufs], bufs, "nv12", H, W)
