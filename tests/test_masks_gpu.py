"""GPU: object masks in the library.  pips_object_masks and pips_masks_tint are held, byte for byte, to their torch twins run on the
CPU (drivers.object_masks_torch and drivers.tint_masks_torch, themselves held to plain loops in tests/test_masks.py) on the cases
made there.  Outputs are views of poisoned allocations with 256-byte guard bands whose padding, gaps and bands must come back
untouched; the workspace has a poisoned tail and the size the header states; inputs come back unchanged.  End to end the planted
scene goes through motion_layers -> object_masks -> object_colors -> tint_masks on NV12 to the bytes of the torch route."""
import ctypes

import pytest
import torch

from test_draw import SENTINEL, buffers, outside_untouched, views
from test_masks import (MEANING_SCENES, mask_case_id, mask_case_inputs, mask_cases, meaning_scene, tint_cases, tint_id, tint_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
_want = {}


def _reference(case):
    """the twin's masks of a case, on the CPU, made once and never written to"""
    if case not in _want:
        from pips_amd import drivers
        h, w, n, radius8, vote, F, src, _ = case
        rows, lab, first = mask_case_inputs(case)
        _want[case] = drivers.object_masks_torch(rows[None, :first + F], lab[:first + F], src or (h, w), out_size=(h, w),
                                                 radius=radius8 / 8.0, vote=vote, first=first)
    return _want[case]


def _guarded(F, h, w, pad=(5, 2)):
    """a poisoned allocation with guard bands and the (F,h,w) view of pitch w + pad[0] and step pitch * (h + pad[1]) inside it"""
    pitch = w + pad[0]
    step = pitch * (h + pad[1])
    flat = torch.full((2 * GUARD + F * step,), SENTINEL, dtype=torch.uint8, device=DEV)
    return flat, flat.as_strided((F, h, w), (step, pitch, 1), GUARD), pitch, step


def _only_the_image_changed(flat, view):
    probe = torch.zeros_like(flat, dtype=torch.bool)
    probe.as_strided(view.shape, view.stride(), view.storage_offset())[...] = True
    return bool((flat[~probe] == SENTINEL).all())


@pytest.mark.parametrize("case", mask_cases(), ids=mask_case_id)
def test_object_masks_is_the_twin(case):
    from pips_amd import _lib
    h, w, n, radius8, vote, F, src, _ = case
    rows, lab, first = mask_case_inputs(case)
    want = _reference(case)
    G = rows.shape[0]
    src_h, src_w = src or (h, w)
    d_rows, d_lab = rows.to(DEV), lab.to(torch.uint8).to(DEV)
    lib = _lib.load()
    need = lib.pips_object_masks_workspace_bytes(F, n)
    assert need == 8 * F * n
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    flat, out, pitch, step = _guarded(F, h, w)
    rc = lib.pips_object_masks(d_rows.data_ptr(), d_lab.data_ptr(), G, n, first, F, src_h, src_w, h, w, radius8, vote, out.data_ptr(), pitch,
                               step, ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.pips_last_error()
    got = out.cpu()
    assert torch.equal(got, want), (mask_case_id(case), int((got != want).sum()))
    assert _only_the_image_changed(flat, out)
    assert bool((ws[need:] == 0x5A).all())
    assert torch.equal(d_rows.cpu().view(torch.int32), rows.view(torch.int32)) and torch.equal(d_lab.cpu(), lab.to(torch.uint8))


@pytest.mark.parametrize("case", [c for c in mask_cases() if (c[0], c[1], c[2]) in ((33, 70, 257), (64, 48, 255), (16, 16, 0))], ids=mask_case_id)
def test_ops_and_drivers_give_the_same_bytes(case):
    from pips_amd import drivers, ops
    h, w, n, radius8, vote, F, src, _ = case
    rows, lab, first = mask_case_inputs(case)
    want = _reference(case)
    rows, lab = rows[:first + F].to(DEV), lab[:first + F].to(DEV)
    got = ops.object_masks(rows, lab.to(torch.uint8), (h, w), src, radius8, vote, first)
    assert torch.equal(got.cpu(), want)
    flat, out, _, _ = _guarded(F, h, w, pad=(3, 1))
    ws = torch.full((ops.object_masks_workspace_bytes(F, n) // 4 + 8,), -77, dtype=torch.int32, device=DEV)
    assert ops.object_masks(rows, lab.to(torch.uint8), (h, w), src, radius8, vote, first, out=out, workspace=ws) is out
    assert torch.equal(out.cpu(), want) and _only_the_image_changed(flat, out) and bool((ws[-8:] == -77).all())
    got = drivers.object_masks(rows[None], lab, src or (h, w), out_size=(h, w), radius=radius8 / 8.0, vote=vote, first=first)
    assert got.is_cuda and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("case", tint_cases(), ids=tint_id)
def test_masks_tint_is_the_twin(case):
    from pips_amd import drivers
    fmt, matrix, range_, h, w, C = case
    bufs, mbuf, colors, alpha = tint_inputs(case)
    before = [b.clone() for b in bufs]
    want = drivers.tint_masks_torch(views(bufs, fmt, h, w), fmt, mbuf[:, :h, :w], colors, alpha / 256.0, matrix, range_)
    want = [want] if torch.is_tensor(want) else want
    assert any(not torch.equal(a, b) for a, b in zip(want, views(bufs, fmt, h, w)))
    # the allocations on the device between guard bands
    flats = [torch.full((2 * GUARD + b.numel(),), SENTINEL, dtype=torch.uint8, device=DEV) for b in bufs + [mbuf]]
    dev = [f[GUARD:GUARD + b.numel()].view(b.shape) for f, b in zip(flats, bufs + [mbuf])]
    for d, b in zip(dev, bufs + [mbuf]):
        d.copy_(b)
    planes, masks = views(dev[:-1], fmt, h, w), dev[-1][:, :h, :w]
    d_colors = colors.to(DEV)
    got = drivers.tint_masks(planes, fmt, masks, d_colors, alpha / 256.0, matrix, range_, inplace=True)
    torch.cuda.synchronize()
    got = [got] if torch.is_tensor(got) else got
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, planes))
    for k, (a, b) in enumerate(zip(planes, want)):
        assert torch.equal(a.cpu(), b), (tint_id(case), k, int((a.cpu() != b).sum()))
    assert outside_untouched([d.cpu() for d in dev[:-1]], before, fmt, h, w)          # padding, gaps, the alpha byte
    assert all(bool((f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all()) for f in flats)
    assert torch.equal(dev[-1].cpu(), mbuf) and torch.equal(d_colors.cpu(), colors)


def test_return_codes_on_the_device_path():
    from pips_amd import _lib
    lib = _lib.load()
    rows = torch.rand(2, 5, 2, device=DEV) * 8
    lab = torch.zeros(2, 5, dtype=torch.uint8, device=DEV)
    flat, out, pitch, step = _guarded(2, 8, 8)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    need = lib.pips_object_masks_workspace_bytes(2, 5)
    call = lambda p, nbytes: lib.pips_object_masks(rows.data_ptr(), lab.data_ptr(), 2, 5, 0, 2, 8, 8, 8, 8, 24, 1, out.data_ptr(), pitch, step, p,
                                                   nbytes, None)
    assert call(ws.data_ptr(), need - 1) == -1 and lib.pips_last_error().decode().startswith("object_masks: workspace")
    assert call(ws.data_ptr() + 8, need) == -1 and b"16-byte" in lib.pips_last_error()
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all())                             # nothing was written
    assert call(ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).any())


def test_end_to_end_on_the_planted_scene():
    """motion_layers -> object_masks -> object_colors -> tint_masks on pitched NV12 surfaces of the planted scene's pair is, byte for
    byte, the torch route on the CPU; the object is tinted and the camera layer is not"""
    from pips_amd import drivers
    H, W = 240, 320
    shift, seed = MEANING_SCENES[0]
    trajs, obj, (x0, y0, x1, y1) = meaning_scene(shift, seed)
    kw = dict(thr=2.0, hypotheses=256, layers=3, min_inliers=8)
    bufs = buffers("nv12", 1, H, W, 21, pad=(64, 8))
    ref = drivers.motion_layers_torch(trajs[None], **kw)
    ref_masks = drivers.object_masks_torch(trajs[None, 1:], ref[2], (H, W), vote=3)
    colors, alpha = drivers.object_colors(ref[3], alpha=0.6)
    want = drivers.tint_masks_torch(views(bufs, "nv12", H, W), "nv12", ref_masks, colors, alpha)

    d_trajs = trajs.to(DEV)
    res = drivers.motion_layers(d_trajs[None], **kw)
    assert torch.equal(res[2].cpu(), ref[2]) and torch.equal(res[3].cpu(), ref[3])
    masks = drivers.object_masks(d_trajs[None, 1:], res[2], (H, W), vote=3)
    assert torch.equal(masks.cpu(), ref_masks)
    d_colors, d_alpha = drivers.object_colors(res[3], alpha=0.6)
    d_bufs = [b.to(DEV) for b in bufs]
    planes = views(d_bufs, "nv12", H, W)
    drivers.tint_masks(planes, "nv12", masks, d_colors, d_alpha, inplace=True)
    torch.cuda.synchronize()
    for a, b in zip(planes, want):
        assert torch.equal(a.cpu(), b), int((a.cpu() != b).sum())
    assert outside_untouched([b.cpu() for b in d_bufs], bufs, "nv12", H, W)
    changed = planes[0].cpu() != bufs[0][:, :H, :W]
    assert bool(changed[0, y0:y1, x0:x1].float().mean() > 0.9) and not bool(changed[0, :y0 - 10].any())
