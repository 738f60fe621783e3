"""Thin tensor-level wrappers over the C ABI stage entry points (include/pips_hip.h).

torch is used for device memory and the current stream only; every number is produced by
libpips_hip.so.  These wrappers exist for the parity tests and for callers that keep the
pyramid resident between calls (dense-grid / chained tracking).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .weights import param_table

S = 8
LATENT = 128
KIN_PAD = 544
NOUT = 1040


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    """One entry point of the library on the current stream's device state: look up, call, raise on a non-zero code."""
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _f32(t):
    assert t.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    return t.contiguous().to(torch.float32)


PACK_FP32, PACK_BF16, PACK_SPLIT = 1, 2, 4
EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_RES_BF16 = 0, 1, 2, 0x1000          # include/pips_hip.h: PIPS_EPI_*
# include/pips_hip.h: PIPS_FLAG_*
FLAG_REUSE_MAPS, FLAG_BF16_MIXER, FLAG_BF16_ENCODER, FLAG_RGB_U8 = 1, 2, 4, 8
FLAG_SPLIT_BF16, FLAG_BF16_MAPS, FLAG_BF16_STREAM = 16, 32, 64


def pack_more(arena, sections, S=8):
    """Build further sections (PACK_BF16 / PACK_SPLIT) of an arena whose fp32 section is already packed (for window length S)."""
    with torch.cuda.device(arena.device):
        _call("pips_repack_weights_s", None, 0, _lib.ptr(arena), int(S), int(sections) & ~PACK_FP32, _stream())
        # the arena is shared by every stream that drives the module: the new sections must be complete before another
        # thread's stream can read them (pack_weights synchronises for the same reason)
        torch.cuda.current_stream().synchronize()
    return arena


def pack_weights(state_dict, device, sections=PACK_FP32 | PACK_BF16 | PACK_SPLIT, S=8) -> torch.Tensor:
    """state dict (reference key names/layouts, of a ``Pips(S=S)``) -> packed device arena (pips_repack_weights_s);
    ``sections``: which of the fp32 / bf16-copy / split-plane sections to build now (pack_more adds the others later)."""
    lib = _lib.load()
    table = param_table(S)
    names = list(table.keys())
    missing = [k for k in names if k not in state_dict]
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
    for k in names:           # the C side sees bare pointers: a checkpoint of another window length must not get that far
        if tuple(state_dict[k].shape) != tuple(table[k][0]):
            raise ValueError(f"{k}: shape {tuple(state_dict[k].shape)}, a Pips(S={S}) holds {tuple(table[k][0])}")
    nbytes = lib.pips_weight_arena_bytes_s(int(S))
    if nbytes == 0:
        raise ValueError(f"window length S={S} is outside 1..32")
    with torch.cuda.device(device):
        srcs = [_f32(state_dict[k].detach().to(device)) for k in names]
        arena = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        arr = (C.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
        _call("pips_repack_weights_s", arr, len(srcs), _lib.ptr(arena), int(S), int(sections) | PACK_FP32, _stream())
        torch.cuda.current_stream().synchronize()      # srcs may be temporaries
    return arena


def times_table(device, S=8) -> torch.Tensor:
    # torch.linspace(0, S, S) exactly as nets/pips.py:519 builds it
    return torch.linspace(0, S, S, device=device, dtype=torch.float32)


def pyramid_levels(pyr: torch.Tensor, F: int, H: int, W: int, stride: int):
    """Views (F,H_l,W_l,128) of the packed pyramid buffer."""
    lib = _lib.load()
    out = []
    h, w = H // stride, W // stride
    for l in range(4):
        off = lib.pips_pyramid_offset(F, H, W, stride, l)
        out.append(pyr[off:off + F * h * w * LATENT].view(F, h, w, LATENT))
        h, w = h // 2, w // 2
    return out


def encoder_fwd(arena, rgbs, stride, bf16=False, split=False):
    """rgbs (F,3,H,W) 0..255 -> packed channel-last pyramid buffer.  bf16: bf16 conv operands;
    split: fp32-grade split-bf16 convolutions."""
    lib = _lib.load()
    u8 = rgbs.dtype == torch.uint8                    # decoded frames go in as they are
    rgbs = rgbs.contiguous() if u8 else _f32(rgbs)
    F, _, H, W = rgbs.shape
    with torch.cuda.device(rgbs.device):
        pyr = torch.empty(lib.pips_pyramid_floats(F, H, W, stride), dtype=torch.float32, device=rgbs.device)
        nb = lib.pips_encoder_workspace_bytes(F, H, W, stride)
        ws = torch.empty(nb // 4, dtype=torch.float32, device=rgbs.device)
        flags = (FLAG_BF16_ENCODER if bf16 else 0) | (FLAG_RGB_U8 if u8 else 0) | (FLAG_SPLIT_BF16 if split else 0)
        _call("pips_encoder_fwd_ex", _lib.ptr(arena), _lib.ptr(rgbs), F, H, W, stride, flags, _lib.ptr(pyr), _lib.ptr(ws), nb,
              _stream())
    return pyr


def resize_frames(rgbs, size):
    """uint8 or float frames (..., 3, h, w) -> float32 (..., 3, H, W), values 0..255: the on-device form of the callers'
    ``F.interpolate(rgbs, (H, W), mode='bilinear')`` (demo.py:26-27).  Feed the result to ``Pips.forward``."""
    H, W = int(size[0]), int(size[1])
    h, w = rgbs.shape[-2:]
    src = rgbs.contiguous() if rgbs.dtype == torch.uint8 else _f32(rgbs)
    planes = src.numel() // (h * w)
    out = torch.empty(tuple(rgbs.shape[:-2]) + (H, W), dtype=torch.float32, device=rgbs.device)
    with torch.cuda.device(rgbs.device):
        _call("pips_resize_frames", _lib.ptr(src), 1 if src.dtype == torch.uint8 else 0, planes, h, w, _lib.ptr(out), H, W,
              _stream())
    return out


# include/pips_hip.h: PIPS_FMT_*, PIPS_MATRIX_*, PIPS_RANGE_*, PIPS_FILTER_*
IMPORT_FORMATS = {"rgb24": 0, "bgr24": 1, "rgba32": 2, "bgra32": 3, "nv12": 4, "i420": 5, "p010": 6, "i010": 7}
IMPORT_16BIT = ("p010", "i010")
FILTER_BILINEAR, FILTER_TRIANGLE = 0, 1
FILTER_DIM_MAX = 8192
IMPORT_MATRICES = {"bt601": 0, "bt709": 1}
IMPORT_RANGES = {"limited": 0, "full": 1}


def import_planes(planes, fmt):
    """The checks on the source planes that ``import_frames`` and ``drivers.import_frames_torch`` share: ``planes`` -- a tensor or a
    sequence of them -- as uint8 tensors of the format's shapes -> (list of planes, F, h, w).  The 16-bit formats "p010" and "i010"
    take uint16 planes, or int16 planes holding the same bits, and come back as int16 views.  ValueError otherwise."""
    if fmt not in IMPORT_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(IMPORT_FORMATS)}, not {fmt!r}")
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    want = {"nv12": 2, "i420": 3, "p010": 2, "i010": 3}.get(fmt, 1)
    if len(planes) != want or not all(torch.is_tensor(p) for p in planes):
        raise ValueError(f"{fmt} takes {want} plane tensor(s), not {len(planes)}")
    for p in planes:
        if fmt in IMPORT_16BIT:
            if p.dtype not in (torch.uint16, torch.int16):
                raise ValueError(f"{fmt} planes must be uint16 (or int16 holding the same bits), not {p.dtype}")
        elif p.dtype != torch.uint8:
            raise ValueError(f"{fmt} planes must be uint8, not {p.dtype}")
        if p.device != planes[0].device:
            raise ValueError("the planes must live on one device")
    if fmt in IMPORT_16BIT:
        planes = [p.view(torch.int16) for p in planes]
    first = planes[0]
    if want == 1:
        bpp = 4 if fmt in ("rgba32", "bgra32") else 3
        if first.dim() != 4 or first.shape[3] != bpp:
            raise ValueError(f"{fmt} frames must be (F,h,w,{bpp}), not {tuple(first.shape)}")
        F, h, w = first.shape[:3]
    else:
        if first.dim() != 3:
            raise ValueError(f"the Y plane must be (F,h,w), not {tuple(first.shape)}")
        F, h, w = first.shape
        ch, cw = (h + 1) // 2, (w + 1) // 2
        shapes = [(F, ch, cw, 2)] if fmt in ("nv12", "p010") else [(F, ch, cw)] * 2
        for p, s in zip(planes[1:], shapes):
            if tuple(p.shape) != s:
                raise ValueError(f"a {fmt} chroma plane of (F,h,w) = {(F, h, w)} must be {s}, not {tuple(p.shape)}")
    if h < 1 or w < 1:
        raise ValueError(f"frames of {h} x {w}: need at least 1 x 1")
    return planes, int(F), int(h), int(w)


def import_size(size, h, w, antialias):
    """``size`` of ``import_frames`` / ``drivers.import_frames_torch`` -> (H, W), held to PIPS_FILTER_TRIANGLE's limits when
    ``antialias`` asks for it and the size changes.  ValueError otherwise."""
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if H < 1 or W < 1:
        raise ValueError(f"size must be at least 1 x 1, not {H} x {W}")
    if antialias and (H, W) != (h, w):
        if max(h, w, H, W) > FILTER_DIM_MAX:
            raise ValueError(f"antialias=True takes sizes up to {FILTER_DIM_MAX}, not {h} x {w} -> {H} x {W}")
        if h > 16 * H or w > 16 * W:
            raise ValueError(f"antialias=True scales down by at most 16 per axis, not {h} x {w} -> {H} x {W}")
    return H, W


def _pitched(p, inner):
    """plane (F, rows, ...) whose trailing dimensions must have the element strides ``inner`` -> (plane, pitch, step) in bytes, the
    plane itself where its strides describe rows ``pitch`` >= a row's bytes apart and frames ``step`` >= pitch * rows apart (a view
    of a pitched surface imports as it is), one contiguous copy otherwise"""
    F, rows = p.shape[0], p.shape[1]
    row_bytes = p[0, 0].numel() if F else 0
    ok = all(p.stride(-1 - i) == s or p.shape[-1 - i] == 1 for i, s in enumerate(reversed(inner)))
    pitch, step = p.stride(1), p.stride(0)
    if rows == 1:
        pitch = max(pitch, row_bytes)                  # (the stride of a dimension of one element carries no meaning)
    if F == 1:
        step = pitch * rows
    if not ok or pitch < row_bytes or step < pitch * rows:
        p = p.contiguous()
        pitch, step = row_bytes, row_bytes * rows
    return p, pitch, step


def import_frames(planes, fmt, size=None, matrix="bt709", range="limited", dtype=torch.uint8, antialias=False):
    """pips_frames_import_ex on device planes in a decoder's layout -> planar frames (F,3,H,W), ``dtype`` uint8 or float32 (0..255):
    what ``encoder_fwd``, ``corner_table``, ``cut_table`` and ``Pips.encode`` read.  ``fmt``: "rgb24" / "bgr24" (planes (F,h,w,3)),
    "rgba32" / "bgra32" ((F,h,w,4), alpha not read), "nv12" ((y (F,h,w), uv (F,ceil(h/2),ceil(w/2),2))) or "i420" ((y, u, v)), all
    uint8; "p010" and "i010" are the 10-bit forms of nv12 and i420 in uint16 (or int16) planes of the same shapes, the value in the
    high ten bits of a p010 word and the low ten of an i010 word.  ``size`` = (H, W) resizes in the same launch: pips_resize_frames'
    two-tap bilinear arithmetic on the converted frames, or with ``antialias=True`` the triangle filter (torch's
    ``antialias=True``; sizes up to 8192, at most 16 x down per axis).  ``matrix`` "bt601" / "bt709" and ``range`` "limited" /
    "full" are read for the YCbCr formats only.  Row and frame strides go through as pitch
    and step: a ``surface[:, :h, :w]`` view of a pitched allocation is imported without a copy; a plane whose inner strides are not
    the format's is copied once (include/pips_hip.h has the whole rule)."""
    planes, F, h, w = import_planes(planes, fmt)
    if matrix not in IMPORT_MATRICES or range not in IMPORT_RANGES:
        raise ValueError(f"matrix must be one of {sorted(IMPORT_MATRICES)} and range one of {sorted(IMPORT_RANGES)}, "
                         f"not {matrix!r}, {range!r}")
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"dtype must be torch.uint8 or torch.float32, not {dtype}")
    H, W = import_size(size, h, w, antialias)
    if F * H * W > 2 ** 30:
        raise ValueError(f"{F} frames of {H} x {W} are more than 2^30 output pixels: split the chunk")
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    out = torch.empty(F, 3, H, W, dtype=dtype, device=dev)
    if F == 0:                                                                    # (an empty tensor has no pointer to pass)
        return out
    # the element strides the format asks of each plane's trailing dimensions
    inner = {"nv12": [(1,), (2, 1)], "i420": [(1,)] * 3, "p010": [(1,), (2, 1)], "i010": [(1,)] * 3}.get(fmt) or [(planes[0].shape[3], 1)]
    args, keep = [], []
    for p, tail in zip(planes, inner):
        p, pitch, step = _pitched(p, tail)
        keep.append(p)
        args += [_lib.ptr(p), pitch * p.element_size(), step * p.element_size()]
    args += [None, 0, 0] * (3 - len(planes))
    with torch.cuda.device(dev):
        _call("pips_frames_import_ex", IMPORT_FORMATS[fmt], IMPORT_MATRICES[matrix], IMPORT_RANGES[range],
              FILTER_TRIANGLE if antialias else FILTER_BILINEAR, F, h, w, *args, _lib.ptr(out), 1 if dtype == torch.uint8 else 0, H, W,
              _stream())
    return out


# include/pips_hip.h: the formats pips_tracks_draw takes, PIPS_DRAW_*
DRAW_FORMATS = {"rgb24": 0, "bgr24": 1, "rgba32": 2, "bgra32": 3, "nv12": 4, "i420": 5, "planar8": 8}
DRAW_FORMATS_EX = dict(DRAW_FORMATS, p010=6, i010=7)                  # pips_tracks_draw_ex takes the two 16-bit formats too
DRAW_DIM_MAX, DRAW_TRAIL_MAX, DRAW_RADIUS8_MAX, DRAW_JUMP8_MAX = 8192, 32, 128, 2047


def draw_planes(planes, fmt):
    """The checks on the surfaces that ``draw_tracks`` and ``drivers.draw_tracks_torch`` share: ``import_planes``' for the eight
    decoder formats ("p010" and "i010" as uint16 or int16 planes, which come back as int16 views), and for "planar8" one uint8
    tensor (F,3,h,w) -- the frames ``import_frames`` returns -> (list of planes, F, h, w).  ValueError otherwise."""
    if fmt not in DRAW_FORMATS_EX:
        raise ValueError(f"fmt must be one of {sorted(DRAW_FORMATS_EX)}, not {fmt!r}")
    if fmt != "planar8":
        return import_planes(planes, fmt)
    planes = [planes] if torch.is_tensor(planes) else list(planes)
    if len(planes) != 1 or not torch.is_tensor(planes[0]):
        raise ValueError(f"planar8 takes 1 plane tensor, not {len(planes)}")
    p = planes[0]
    if p.dtype != torch.uint8 or p.dim() != 4 or p.shape[1] != 3:
        raise ValueError(f"planar8 frames must be uint8 (F,3,h,w), not {p.dtype} {tuple(p.shape)}")
    F, _, h, w = p.shape
    if h < 1 or w < 1:
        raise ValueError(f"frames of {h} x {w}: need at least 1 x 1")
    return planes, int(F), int(h), int(w)


def draw_fade(fade, trail):
    """``fade`` of ``draw_tracks``: None, or a sequence of ``trail`` whole numbers in 0..256 -> None or the list of ints.  ValueError
    otherwise."""
    if fade is None:
        return None
    fade = fade.tolist() if torch.is_tensor(fade) else list(fade)
    if len(fade) != trail:
        raise ValueError(f"fade must have trail = {trail} entries, not {len(fade)}")
    for v in fade:
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 256:
            raise ValueError(f"a fade entry must be a whole number in 0..256, not {v!r}")
    return [int(v) for v in fade]


def draw_check(planes, fmt, trajs, vis, colors, first, src_size, trail, line8, dot8, alpha_vis, alpha_occ, matrix, range):
    """pips_tracks_draw_ex's limits on the values (but for the fade table: ``draw_fade``), shared by ``draw_tracks`` and the twin ->
    (planes, F, h, w, G, n, src_h, src_w)"""
    planes, F, h, w = draw_planes(planes, fmt)
    if matrix not in IMPORT_MATRICES or range not in IMPORT_RANGES:
        raise ValueError(f"matrix must be one of {sorted(IMPORT_MATRICES)} and range one of {sorted(IMPORT_RANGES)}, "
                         f"not {matrix!r}, {range!r}")
    if trajs.dim() != 3 or trajs.shape[2] != 2 or trajs.dtype != torch.float32:
        raise ValueError(f"trajs must be float32 (G,n,2), not {trajs.dtype} {tuple(trajs.shape)}")
    G, n = int(trajs.shape[0]), int(trajs.shape[1])
    if vis is not None and (tuple(vis.shape) != (G, n) or vis.dtype != torch.float32):
        raise ValueError(f"vis must be float32 (G,n) = {(G, n)} or None, not {vis.dtype} {tuple(vis.shape)}")
    if tuple(colors.shape) != (n, 3) or colors.dtype != torch.uint8:
        raise ValueError(f"colors must be uint8 (n,3) = {(n, 3)}, not {colors.dtype} {tuple(colors.shape)}")
    src_h, src_w = (h, w) if src_size is None else (int(src_size[0]), int(src_size[1]))
    if src_h < 1 or src_w < 1:
        raise ValueError(f"size must be at least 1 x 1, not {src_h} x {src_w}")
    if max(h, w) > DRAW_DIM_MAX:
        raise ValueError(f"surfaces up to {DRAW_DIM_MAX} a side, not {h} x {w}")
    if not 0 <= trail <= DRAW_TRAIL_MAX:
        raise ValueError(f"trail must lie in 0..{DRAW_TRAIL_MAX}, not {trail}")
    if max(line8, dot8) > DRAW_RADIUS8_MAX:
        raise ValueError(f"a radius of at most {DRAW_RADIUS8_MAX} eighths of a pixel, not line8 = {line8}, dot8 = {dot8}")
    if not (0 <= alpha_vis <= 256 and 0 <= alpha_occ <= 256):
        raise ValueError(f"alphas must lie in 0..256, not {alpha_vis}, {alpha_occ}")
    if first < 0 or first + F > G:
        raise ValueError(f"rows [{first}, {first} + {F}) of trajs with {G} rows")
    return planes, F, h, w, G, n, src_h, src_w


def _surface(p, inner):
    """plane (F, rows, ...) that is drawn on in place -> (pitch, step) in elements; ValueError where its strides do not describe
    rows ``pitch`` >= a row apart and frames ``step`` >= pitch * rows apart with the format's element strides ``inner`` inside a row
    (``_pitched`` copies such a plane; a copy cannot be drawn on)"""
    F, rows = p.shape[0], p.shape[1]
    row_bytes = p[0, 0].numel() if F else 0
    ok = all(p.stride(-1 - i) == s or p.shape[-1 - i] == 1 for i, s in enumerate(reversed(inner)))
    pitch, step = p.stride(1), p.stride(0)
    if rows == 1:
        pitch = max(pitch, row_bytes)
    if F == 1:
        step = pitch * rows
    if not ok or pitch < row_bytes or step < pitch * rows:
        raise ValueError(f"a surface of shape {tuple(p.shape)} and strides {tuple(p.stride())} cannot be drawn on in place")
    return pitch, step


def draw_workspace_bytes(F, n, trail):
    return int(_lib.load().pips_draw_workspace_bytes(int(F), int(n), int(trail)))


def draw_surfaces(planes, fmt):
    """the planes of ``draw_planes`` as the nine surface arguments of pips_tracks_draw: (pointer, pitch, step) per plane, in bytes.
    ValueError for a plane whose strides cannot be pitch and step (the planes may live on any device: nothing is read)"""
    size = planes[0].element_size()
    if fmt == "planar8":
        p = planes[0]
        pitch, step = _surface(p[:, 0], (1,))                                     # the three planes share pitch and step
        if p.stride(1) < pitch * p.shape[2]:
            raise ValueError(f"a surface of shape {tuple(p.shape)} and strides {tuple(p.stride())} cannot be drawn on in place")
        args = []
        for k in (0, 1, 2):
            args += [C.c_void_p(p.data_ptr() + k * p.stride(1)), pitch, step]
        return args
    semi = [(1,), (2, 1)]
    inner = {"nv12": semi, "p010": semi, "i420": [(1,)] * 3, "i010": [(1,)] * 3}.get(fmt) or [(planes[0].shape[3], 1)]
    args = []
    for p, tail in zip(planes, inner):
        pitch, step = _surface(p, tail)
        args += [_lib.ptr(p), pitch * size, step * size]
    return args + [None, 0, 0] * (3 - len(planes))


def draw_tracks(planes, fmt, trajs, vis, colors, first=0, src_size=None, trail=16, line8=8, dot8=24, alpha_vis=256, alpha_occ=90,
                vis_logit=0.0, matrix="bt709", range="limited", workspace=None, fade=None):
    """pips_tracks_draw: the trails of trajs (G,n,2) float32 (pixels of a ``src_size`` = (src_h, src_w) image, default the
    surfaces' own size) drawn IN PLACE into the device surfaces ``planes`` of format ``fmt`` -- ``import_frames``' formats and
    shapes ("p010" and "i010" as uint16 or int16 planes), or "planar8": one (F,3,h,w) uint8 tensor.  Frame k takes row
    ``first + k``; ``vis`` (G,n) logits or None, ``colors`` (n,3) uint8 RGB; radii in eighths of a pixel, alphas 0..256
    (include/pips_hip.h has the whole rule).  ``fade``: None, or ``trail`` ints 0..256, the factor on the opacity of the segment of
    each age (0: the one that ends on the head).  A 16-bit format or a fade goes to pips_tracks_draw_ex, every other call to
    pips_tracks_draw.  Row and frame strides go through as pitch and step: a ``surface[:, :h, :w]`` view of a pitched allocation is
    drawn on as it is; a plane whose strides cannot be expressed so is a ValueError.  ``workspace``: a device tensor of at least
    ``draw_workspace_bytes(F, n, trail)`` bytes to use instead of a fresh one."""
    trail, line8, dot8, alpha_vis, alpha_occ, first = (int(v) for v in (trail, line8, dot8, alpha_vis, alpha_occ, first))
    planes, F, h, w, G, n, src_h, src_w = draw_check(planes, fmt, trajs, vis, colors, first, src_size, trail, line8, dot8, alpha_vis,
                                                     alpha_occ, matrix, range)
    fade = draw_fade(fade, trail)
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    for t in (trajs, vis, colors, workspace):
        if t is not None and t.device != dev:
            raise ValueError("trajs, vis, colors and the workspace must live on the surfaces' device")
    if F == 0 or n == 0:
        return
    args = draw_surfaces(planes, fmt)
    trajs, colors = trajs.contiguous(), colors.contiguous()
    vis = None if vis is None else vis.contiguous()
    need = draw_workspace_bytes(F, n, trail)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    nbytes = workspace.numel() * workspace.element_size()
    head = (DRAW_FORMATS_EX[fmt], IMPORT_MATRICES[matrix], IMPORT_RANGES[range], F, h, w, *args, _lib.ptr(trajs), _lib.ptr(vis), G, n,
            first, src_h, src_w, _lib.ptr(colors), trail, line8, dot8, alpha_vis, alpha_occ, float(vis_logit))
    with torch.cuda.device(dev):
        if fmt in IMPORT_16BIT or fade is not None:
            table = None if fade is None else (C.c_int * max(trail, 1))(*fade)      # a host array: read before the launch
            _call("pips_tracks_draw_ex", *head, table, _lib.ptr(workspace), nbytes, _stream())
        else:
            _call("pips_tracks_draw", *head, _lib.ptr(workspace), nbytes, _stream())


# include/pips_hip.h: PIPS_MASK_*
MASK_NONE, MASK_RADIUS8_MAX, MASK_VOTE_MAX, MASK_N_MAX, MASK_LABELS_MAX = 255, 2048, 5, 65536, 255
MASK_TILE = 32                                                         # pips_amd/csrc/masks.hip: the pixels a side a raster block owns


def object_masks_check(trajs, labels, size, src_size, radius8, vote, first):
    """pips_object_masks' limits on the values, shared by ``object_masks`` and ``drivers.object_masks_torch`` -> (G, n, F, h, w,
    src_h, src_w); the call makes the F = G - first frames of the rows ``first`` .. G - 1"""
    if trajs.dim() != 3 or trajs.shape[2] != 2 or trajs.dtype != torch.float32:
        raise ValueError(f"trajs must be float32 (G,n,2), not {trajs.dtype} {tuple(trajs.shape)}")
    G, n = int(trajs.shape[0]), int(trajs.shape[1])
    if tuple(labels.shape) != (G, n) or labels.dtype != torch.uint8:
        raise ValueError(f"labels must be uint8 (G,n) = {(G, n)}, not {labels.dtype} {tuple(labels.shape)}")
    if n > MASK_N_MAX:
        raise ValueError(f"at most {MASK_N_MAX} columns, not {n}")
    h, w = int(size[0]), int(size[1])
    src_h, src_w = (h, w) if src_size is None else (int(src_size[0]), int(src_size[1]))
    if min(h, w, src_h, src_w) < 1:
        raise ValueError(f"sizes must be at least 1 x 1, not {h} x {w} from {src_h} x {src_w}")
    if max(h, w) > DRAW_DIM_MAX:
        raise ValueError(f"masks up to {DRAW_DIM_MAX} a side, not {h} x {w}")
    if not 0 <= radius8 <= MASK_RADIUS8_MAX:
        raise ValueError(f"radius8 must lie in 0..{MASK_RADIUS8_MAX} eighths of a pixel, not {radius8}")
    if not 1 <= vote <= MASK_VOTE_MAX:
        raise ValueError(f"vote must lie in 1..{MASK_VOTE_MAX}, not {vote}")
    if not 0 <= first <= G:
        raise ValueError(f"first = {first} of trajs with {G} rows")
    return G, n, G - first, h, w, src_h, src_w


def object_masks_workspace_bytes(F, n):
    return int(_lib.load().pips_object_masks_workspace_bytes(int(F), int(n)))


def object_masks(trajs, labels, size, src_size=None, radius8=384, vote=1, first=0, out=None, workspace=None):
    """pips_object_masks: a label per pixel from a label per track.  trajs (G,n,2) float32 are pixels of a ``src_size`` = (src_h,
    src_w) image (default ``size``), labels (G,n) uint8 with 255 for a column that takes no part; frame k of the result takes row
    ``first + k`` -> (G - first, h, w) uint8, ``size`` = (h, w): every pixel the label that its ``vote`` nearest participating
    tracks within ``radius8`` eighths of a pixel vote for, 255 where there is none (include/pips_hip.h has the whole rule).
    ``out``: a uint8 (F,h,w) device tensor to write instead of a fresh one -- row and frame strides go through as pitch and step, so
    a ``buffer[:, :h, :w]`` view of a pitched allocation is written as it is.  ``workspace``: a device tensor of at least
    ``object_masks_workspace_bytes(F, n)`` bytes to use instead of a fresh one."""
    radius8, vote, first = int(radius8), int(vote), int(first)
    G, n, F, h, w, src_h, src_w = object_masks_check(trajs, labels, size, src_size, radius8, vote, first)
    assert trajs.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = trajs.device
    if out is None:
        out = torch.empty(F, h, w, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, h, w):
        raise ValueError(f"out must be uint8 (F,h,w) = {(F, h, w)}, not {out.dtype} {tuple(out.shape)}")
    for t in (labels, out, workspace):
        if t is not None and t.device != dev:
            raise ValueError("trajs, labels, out and the workspace must live on one device")
    if F == 0:
        return out
    pitch, step = _surface(out, (1,))
    trajs, labels = trajs.contiguous(), labels.contiguous()
    need = object_masks_workspace_bytes(F, n)
    if workspace is None:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
    nbytes = workspace.numel() * workspace.element_size()
    with torch.cuda.device(dev):
        _call("pips_object_masks", _lib.ptr(trajs), _lib.ptr(labels), G, n, first, F, src_h, src_w, h, w, radius8, vote, _lib.ptr(out),
              pitch, step, _lib.ptr(workspace), nbytes, _stream())
    return out


def tint_check(planes, fmt, masks, colors, alpha, matrix, range):
    """pips_masks_tint's limits on the values, shared by ``masks_tint`` and ``drivers.tint_masks_torch`` -> (planes, F, h, w, C,
    alpha (F,C) int64 on the host)"""
    if fmt not in DRAW_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(DRAW_FORMATS)}, not {fmt!r}")
    planes, F, h, w = draw_planes(planes, fmt)
    if matrix not in IMPORT_MATRICES or range not in IMPORT_RANGES:
        raise ValueError(f"matrix must be one of {sorted(IMPORT_MATRICES)} and range one of {sorted(IMPORT_RANGES)}, "
                         f"not {matrix!r}, {range!r}")
    if max(h, w) > DRAW_DIM_MAX:
        raise ValueError(f"surfaces up to {DRAW_DIM_MAX} a side, not {h} x {w}")
    if not torch.is_tensor(masks) or masks.dtype != torch.uint8 or tuple(masks.shape) != (F, h, w):
        raise ValueError(f"masks must be uint8 (F,h,w) = {(F, h, w)}, not {getattr(masks, 'dtype', None)} {tuple(getattr(masks, 'shape', ()))}")
    if not torch.is_tensor(colors) or colors.dtype != torch.uint8 or colors.dim() != 3 or colors.shape[0] != F or colors.shape[2] != 3:
        raise ValueError(f"colors must be uint8 (F,C,3) with F = {F}, not {getattr(colors, 'dtype', None)} "
                         f"{tuple(getattr(colors, 'shape', ()))}")
    C = int(colors.shape[1])
    if not 1 <= C <= MASK_LABELS_MAX:
        raise ValueError(f"C must lie in 1..{MASK_LABELS_MAX}, not {C}")
    alpha = torch.as_tensor(alpha)
    if tuple(alpha.shape) != (F, C) or alpha.dtype.is_floating_point or alpha.dtype == torch.bool:
        raise ValueError(f"alpha must be integers (F,C) = {(F, C)}, not {alpha.dtype} {tuple(alpha.shape)}")
    alpha = alpha.to("cpu", torch.int64)
    if alpha.numel() and (int(alpha.min()) < 0 or int(alpha.max()) > 256):
        raise ValueError("an alpha must lie in 0..256")
    return planes, F, h, w, C, alpha


def masks_tint(planes, fmt, masks, colors, alpha, matrix="bt709", range="limited"):
    """pips_masks_tint: the label planes ``masks`` (F,h,w) uint8 shown IN PLACE on the device surfaces ``planes`` of format ``fmt``
    -- ``draw_tracks``' seven 8-bit formats and shapes.  A pixel of frame f with label l < C is blended towards ``colors[f][l]``
    ((F,C,3) uint8 R G B on the device) with the opacity ``alpha[f][l]`` ((F,C) whole numbers 0..256; they are read on the host: a
    device tensor is copied there first); a label >= C, 255 among them, leaves its pixel (include/pips_hip.h has the whole rule).
    Row and frame strides of the surfaces and of the masks go through as pitch and step; a plane whose strides cannot be expressed
    so is a ValueError."""
    planes, F, h, w, nlab, alpha = tint_check(planes, fmt, masks, colors, alpha, matrix, range)
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    if masks.device != dev or colors.device != dev:
        raise ValueError("masks and colors must live on the surfaces' device")
    if F == 0:
        return
    args = draw_surfaces(planes, fmt)
    mpitch, mstep = _surface(masks, (1,))
    colors = colors.contiguous()
    table = (C.c_int * (F * nlab))(*alpha.reshape(-1).tolist())                     # a host array: read before the launch
    with torch.cuda.device(dev):
        _call("pips_masks_tint", DRAW_FORMATS[fmt], IMPORT_MATRICES[matrix], IMPORT_RANGES[range], F, h, w, *args, _lib.ptr(masks), mpitch,
              mstep, _lib.ptr(colors), table, nlab, _stream())


# include/pips_hip.h: PIPS_MASK_EDGE_MAX, PIPS_MASK_REACH_MAX; pips_amd/csrc/masks_guided.hip: the tile a block stores and the halo
# around it, the steps one launch is good for
MASK_EDGE_MAX, MASK_REACH_MAX = 64, 32767
GUIDED_TILE, GUIDED_HALO = 64, 16
GUIDE_FORMATS = ("rgb24", "bgr24", "rgba32", "bgra32", "planar8")     # pips_guide_plane's; the Y plane of nv12 / i420 is a guide as it is


def guided_launches(reach):
    """the relaxation launches of one pips_object_masks_guided call with n > 0: ceil(floor(reach / 5) / GUIDED_HALO), at least one"""
    return max(1, -(-(int(reach) // 5) // GUIDED_HALO))


def object_masks_guided_check(trajs, labels, guide, size, src_size, edge, reach, first):
    """pips_object_masks_guided's limits on the values, shared by ``object_masks_guided`` and
    ``drivers.object_masks_guided_torch`` -> (G, n, F, h, w, src_h, src_w); ``guide`` may be None when n = 0"""
    G, n, F, h, w, src_h, src_w = object_masks_check(trajs, labels, size, src_size, 0, 1, first)
    if not 0 <= edge <= MASK_EDGE_MAX:
        raise ValueError(f"edge must lie in 0..{MASK_EDGE_MAX}, not {edge}")
    if not 0 <= reach <= MASK_REACH_MAX:
        raise ValueError(f"reach must lie in 0..{MASK_REACH_MAX}, not {reach}")
    if guide is None:
        if n > 0 and F > 0:
            raise ValueError("a call with columns needs a guide")
    elif not torch.is_tensor(guide) or guide.dtype != torch.uint8 or tuple(guide.shape) != (F, h, w):
        raise ValueError(f"guide must be uint8 (F,h,w) = {(F, h, w)}, not {getattr(guide, 'dtype', None)} {tuple(getattr(guide, 'shape', ()))}")
    return G, n, F, h, w, src_h, src_w


def object_masks_guided_workspace_bytes(F, n, h, w):
    return int(_lib.load().pips_object_masks_guided_workspace_bytes(int(F), int(n), int(h), int(w)))


def object_masks_guided(trajs, labels, guide, size, src_size=None, edge=4, reach=240, first=0, out=None, workspace=None):
    """pips_object_masks_guided: a label per pixel from a label per track along paths that avoid luma edges.  trajs, labels,
    ``size``, ``src_size`` and ``first`` as in ``object_masks``; ``guide`` (G - first, h, w) uint8 on the device is the 8-bit plane
    whose differences make a step expensive (``guide_plane``, or the Y plane of an NV12 / I420 surface) -- its row and frame
    strides go through as pitch and step, so a view of a pitched surface is read as it is.  Every pixel gets the label of the
    column whose seed pixel is nearest by the cost 5 / 7 per axial / diagonal step + ``edge`` x the step's guide difference,
    within ``reach``; 255 where there is none (include/pips_hip.h has the whole rule).  ``out`` and ``workspace`` as in
    ``object_masks``, the workspace of ``object_masks_guided_workspace_bytes(F, n, h, w)`` bytes."""
    edge, reach, first = int(edge), int(reach), int(first)
    G, n, F, h, w, src_h, src_w = object_masks_guided_check(trajs, labels, guide, size, src_size, edge, reach, first)
    assert trajs.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = trajs.device
    if out is None:
        out = torch.empty(F, h, w, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, h, w):
        raise ValueError(f"out must be uint8 (F,h,w) = {(F, h, w)}, not {out.dtype} {tuple(out.shape)}")
    for t in (labels, guide, out, workspace):
        if t is not None and t.device != dev:
            raise ValueError("trajs, labels, guide, out and the workspace must live on one device")
    if F == 0:
        return out
    pitch, step = _surface(out, (1,))
    gpitch, gstep = (0, 0) if guide is None else _surface(guide, (1,))
    trajs, labels = trajs.contiguous(), labels.contiguous()
    need = object_masks_guided_workspace_bytes(F, n, h, w)
    if workspace is None:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
    nbytes = workspace.numel() * workspace.element_size()
    with torch.cuda.device(dev):
        _call("pips_object_masks_guided", _lib.ptr(trajs), _lib.ptr(labels), G, n, first, F, src_h, src_w, h, w, edge, reach, _lib.ptr(guide),
              gpitch, gstep, _lib.ptr(out), pitch, step, _lib.ptr(workspace), nbytes, _stream())
    return out


def guide_check(planes, fmt):
    """pips_guide_plane's limits on the values, shared by ``guide_plane`` and ``drivers.guide_plane_torch`` -> (planes, F, h, w)"""
    if fmt not in GUIDE_FORMATS:
        raise ValueError(f"fmt must be one of {GUIDE_FORMATS}, not {fmt!r}")
    planes, F, h, w = draw_planes(planes, fmt)
    if max(h, w) > DRAW_DIM_MAX:
        raise ValueError(f"surfaces up to {DRAW_DIM_MAX} a side, not {h} x {w}")
    return planes, F, h, w


def guide_plane(planes, fmt, out=None):
    """pips_guide_plane: the 8-bit luma (77 R + 150 G + 29 B + 128) >> 8 of the device surfaces ``planes`` of format ``fmt`` --
    "rgb24", "bgr24", "rgba32", "bgra32" or "planar8" in ``draw_tracks``' shapes, pitched views included -> (F,h,w) uint8, the
    guide of ``object_masks_guided``.  ``out``: a uint8 (F,h,w) device tensor to write instead of a fresh one, row and frame strides
    as pitch and step."""
    planes, F, h, w = guide_check(planes, fmt)
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    if out is None:
        out = torch.empty(F, h, w, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, h, w) or out.device != dev:
        raise ValueError(f"out must be uint8 (F,h,w) = {(F, h, w)} on the surfaces' device, not {out.dtype} {tuple(out.shape)}")
    if F == 0:
        return out
    args = draw_surfaces(planes, fmt)
    gpitch, gstep = _surface(out, (1,))
    with torch.cuda.device(dev):
        _call("pips_guide_plane", DRAW_FORMATS[fmt], F, h, w, *args, _lib.ptr(out), gpitch, gstep, _stream())
    return out


# include/pips_hip.h: PIPS_WARP_BORDER_*, PIPS_WARP_DIM_MAX; pips_amd/csrc/common.h: the tile and the staging budget of warp.hip
WARP_BORDERS = {"constant": 0, "replicate": 1}
WARP_DIM_MAX, WARP_TILE_W, WARP_TILE_H, WARP_LDS_BYTES = 8192, 64, 16, 12288
_INT32 = (-2 ** 31, 2 ** 31 - 1)


def _warp_values(h, w, border, fill, matrix, range):
    """the limits on the values that pips_frames_warp and pips_frames_warp_fill share -> fill_rgb"""
    if matrix not in IMPORT_MATRICES or range not in IMPORT_RANGES:
        raise ValueError(f"matrix must be one of {sorted(IMPORT_MATRICES)} and range one of {sorted(IMPORT_RANGES)}, "
                         f"not {matrix!r}, {range!r}")
    if border not in WARP_BORDERS:
        raise ValueError(f"border must be one of {sorted(WARP_BORDERS)}, not {border!r}")
    if max(h, w) > WARP_DIM_MAX:
        raise ValueError(f"surfaces up to {WARP_DIM_MAX} a side, not {h} x {w}")
    fill = list(fill)
    if len(fill) != 3 or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255 for v in fill):
        raise ValueError(f"fill must be three whole numbers R, G, B in 0..255, not {fill!r}")
    return int(fill[0]) << 16 | int(fill[1]) << 8 | int(fill[2])


def _warp_rows(coef, shape, name):
    """integer rows of the given shape that fit int32 -> int32, on their own device"""
    coef = torch.as_tensor(coef)
    if tuple(coef.shape) != shape or coef.dtype.is_floating_point or coef.dtype == torch.bool:
        raise ValueError(f"coef must be integers {name} = {shape}, not {coef.dtype} {tuple(coef.shape)}")
    if coef.numel() and (int(coef.min()) < _INT32[0] or int(coef.max()) > _INT32[1]):
        raise ValueError("a coefficient does not fit int32")
    return coef.to(torch.int32)


def warp_check(planes, fmt, coef, border, fill, matrix, range):
    """pips_frames_warp's limits on the values, shared by ``warp_frames`` and ``drivers.warp_frames_torch`` -> (planes, F, h, w,
    coef (F,6) int32 on its own device, fill_rgb)"""
    planes, F, h, w = draw_planes(planes, fmt)
    fill_rgb = _warp_values(h, w, border, fill, matrix, range)
    return planes, F, h, w, _warp_rows(coef, (F, 6), "(F,6)"), fill_rgb


def warp_staged(row, fmt, x0=0, y0=0):
    """Which tap path warp.hip's block takes for the WARP_TILE_W x WARP_TILE_H tile of output luma at (x0, y0) under the six
    coefficients ``row``: True when the source box of every plane of ``fmt`` fits WARP_LDS_BYTES and is staged in LDS, False when the
    taps are read from global memory.  The box is the tap range of the tile's four corners, the +1 tap added, not held to the image;
    a row of it takes round_up(width x bytes of a pixel + 3, 4) bytes.  Python integers: the criterion, restated."""
    if fmt not in DRAW_FORMATS_EX:
        raise ValueError(f"fmt must be one of {sorted(DRAW_FORMATS_EX)}, not {fmt!r}")
    m = [int(v) for v in row]
    sb = 2 if fmt in IMPORT_16BIT else 1
    luma = {"rgb24": 3, "bgr24": 3, "rgba32": 4, "bgra32": 4}.get(fmt, sb)

    def fits(chroma, tx, ty, tw, th, pxb):
        us, vs = [], []
        for x, y in ((tx, ty), (tx + tw - 1, ty), (tx, ty + th - 1), (tx + tw - 1, ty + th - 1)):
            if chroma:
                us.append((m[0] * (4 * x + 1) + m[1] * (4 * y + 1) + 512 * m[2] - 2 ** 24 + 2 ** 17) >> 26)
                vs.append((m[3] * (4 * x + 1) + m[4] * (4 * y + 1) + 512 * m[5] - 2 ** 24 + 2 ** 17) >> 26)
            else:
                us.append((m[0] * x + m[1] * y + 256 * m[2] + 32768) >> 24)
                vs.append((m[3] * x + m[4] * y + 256 * m[5] + 32768) >> 24)
        bw, bh = max(us) + 1 - min(us) + 1, max(vs) + 1 - min(vs) + 1
        return bh * ((bw * pxb + 6) & ~3) <= WARP_LDS_BYTES
    ok = fits(False, x0, y0, WARP_TILE_W, WARP_TILE_H, luma)
    if fmt in ("nv12", "i420", "p010", "i010"):
        ok = ok and fits(True, x0 // 2, y0 // 2, WARP_TILE_W // 2, WARP_TILE_H // 2, 2 * sb if fmt in ("nv12", "p010") else sb)
    return ok


def warp_frames(planes, fmt, coef, border="constant", fill=(0, 0, 0), matrix="bt709", range="limited", out=None):
    """pips_frames_warp: the device surfaces ``planes`` of format ``fmt`` -- ``draw_tracks``' formats and shapes -- resampled into
    ``out`` (surfaces of the same format and shapes; allocated like the source when None) and returned as a list of planes.  ``coef``
    (F,6) int32, from the host or the device: row f = (m0, m1, m2, m3, m4, m5) maps the OUTPUT pixel (x, y) of frame f to the source
    position (m0 x + m1 y) / 2^24 + m2 / 2^16, (m3 x + m4 y) / 2^24 + m5 / 2^16 (include/pips_hip.h has the whole rule;
    ``drivers.warp_coefficients`` makes the rows).  ``border`` "constant" (a tap outside the image is ``fill`` = (R, G, B)) or
    "replicate"; ``matrix`` / ``range`` convert the fill for the YCbCr formats.  Row and frame strides go through as pitch and step,
    on both sides: ``surface[:, :h, :w]`` views of pitched allocations are read and written as they are; a plane whose strides
    cannot be expressed so is a ValueError, and so is an ``out`` that is not of the source's shapes.  ``out`` may not overlap
    ``planes``."""
    planes, F, h, w, coef, fill_rgb = warp_check(planes, fmt, coef, border, fill, matrix, range)
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    if out is None:
        out = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in planes]
    else:
        out, Fo, ho, wo = draw_planes(out, fmt)
        if (Fo, ho, wo) != (F, h, w) or any(o.device != dev for o in out):
            raise ValueError(f"out must be {F} surfaces of {h} x {w} on the source's device, not {Fo} of {ho} x {wo}")
    if F == 0:
        return out
    coef = coef.to(dev).contiguous()
    args = draw_surfaces(planes, fmt) + draw_surfaces(out, fmt)
    with torch.cuda.device(dev):
        _call("pips_frames_warp", DRAW_FORMATS_EX[fmt], IMPORT_MATRICES[matrix], IMPORT_RANGES[range], WARP_BORDERS[border], fill_rgb,
              F, h, w, *args, _lib.ptr(coef), _stream())
    return out


WARP_FILL_MAX = 16                                                    # include/pips_hip.h: PIPS_WARP_FILL_MAX
WARP_FILL_NONE = 255                                                  # the source map where no candidate covered


def warp_fill_check(planes, fmt, cand, coef, border, fill, matrix, range):
    """pips_frames_warp_fill's limits on the values, shared by ``warp_frames_fill`` and ``drivers.warp_frames_fill_torch`` -> (planes,
    Fs, Fd, K, h, w, cand (Fd,K) int32 and coef (Fd,K,6) int32 on their own devices, fill_rgb)"""
    planes, Fs, h, w = draw_planes(planes, fmt)
    cand = torch.as_tensor(cand)
    if cand.dim() != 2 or cand.dtype.is_floating_point or cand.dtype == torch.bool:
        raise ValueError(f"cand must be integers (Fd,K), not {cand.dtype} {tuple(cand.shape)}")
    Fd, K = cand.shape
    if not 1 <= K <= WARP_FILL_MAX:
        raise ValueError(f"1 to {WARP_FILL_MAX} candidates a frame, not {K}")
    if cand.numel() and (int(cand.min()) < _INT32[0] or int(cand.max()) > _INT32[1]):
        raise ValueError("a candidate index does not fit int32")
    fill_rgb = _warp_values(h, w, border, fill, matrix, range)
    return planes, Fs, Fd, K, h, w, cand.to(torch.int32), _warp_rows(coef, (Fd, K, 6), "(Fd,K,6)"), fill_rgb


def warp_frames_fill(planes, fmt, cand, coef, border="constant", fill=(0, 0, 0), matrix="bt709", range="limited", out=None,
                     source=None):
    """pips_frames_warp_fill: ``warp_frames`` with a list of candidates per output frame -- the border of a stabilised frame filled
    from its neighbours.  ``planes`` are Fs device surfaces of ``fmt``; ``cand`` (Fd,K) integers, ``cand[j][k]`` the source frame of
    candidate k of output frame j (outside 0..Fs-1, conventionally -1: none), and ``coef`` (Fd,K,6) its row in ``warp_frames``'
    meaning; both from the host or the device.  Every sample comes from the first candidate in list order whose taps with weight
    all lie inside the plane, and from candidate 0 under ``border`` / ``fill`` when none does (include/pips_hip.h has the whole
    rule).  ``out``: Fd surfaces of the source's format and size, allocated when None.  ``source``: True allocates the (Fd,h,w)
    uint8 map of the list position that supplied each sample of plane 0 (255: none), a tensor is used as given (row and frame
    strides as pitch and step), None asks for no map.  Returns the list of planes, or ``(planes, source)`` when a map was asked
    for.  ``out`` and ``source`` may not overlap ``planes`` or each other."""
    planes, Fs, Fd, K, h, w, cand, coef, fill_rgb = warp_fill_check(planes, fmt, cand, coef, border, fill, matrix, range)
    assert planes[0].is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    dev = planes[0].device
    if out is None:
        out = [torch.empty((Fd,) + tuple(p.shape[1:]), dtype=p.dtype, device=dev) for p in planes]
    else:
        out, Fo, ho, wo = draw_planes(out, fmt)
        if (Fo, ho, wo) != (Fd, h, w) or any(o.device != dev for o in out):
            raise ValueError(f"out must be {Fd} surfaces of {h} x {w} on the source's device, not {Fo} of {ho} x {wo}")
    if source is True:
        source = torch.empty(Fd, h, w, dtype=torch.uint8, device=dev)
    elif source is False:
        source = None
    elif source is not None and (source.dtype != torch.uint8 or tuple(source.shape) != (Fd, h, w) or source.device != dev):
        raise ValueError(f"source must be uint8 (Fd,h,w) = {(Fd, h, w)} on the surfaces' device, not {source.dtype} {tuple(source.shape)}")
    if Fd > 0:
        cand, coef = cand.to(dev).contiguous(), coef.to(dev).contiguous()
        mpitch, mstep = (0, 0) if source is None else _surface(source, (1,))
        # (no source frame: every candidate is invalid and no plane of src is read)
        src_args = draw_surfaces(planes, fmt) if Fs else draw_surfaces(out, fmt)
        with torch.cuda.device(dev):
            _call("pips_frames_warp_fill", DRAW_FORMATS_EX[fmt], IMPORT_MATRICES[matrix], IMPORT_RANGES[range], WARP_BORDERS[border],
                  fill_rgb, Fs, Fd, K, h, w, *src_args, *draw_surfaces(out, fmt), _lib.ptr(cand), _lib.ptr(coef), _lib.ptr(source), mpitch,
                  mstep, _stream())
    return out if source is None else (out, source)


def point_sample(level0, B, xy):
    """level0 (B*S,H8,W8,128), xy (B,N,2) map pixels -> (B,N,128)."""
    xy = _f32(xy)
    F, H8, W8, _ = level0.shape
    N = xy.shape[1]
    out = torch.empty(B, N, LATENT, dtype=torch.float32, device=xy.device)
    with torch.cuda.device(xy.device):
        _call("pips_point_sample", _lib.ptr(level0), B, F // B, H8, W8, _lib.ptr(xy), N, _lib.ptr(out), _stream())
    return out


def mixer_input_build(pyr, B, H8, W8, ffeats, coords, bf16_maps=False):
    """ffeats (B*N*S,128), coords (B*N*S,2) particle-major -> X (B*N*S, 544).  bf16_maps: the gather reads the bf16 mirror
    behind the fp32 levels of ``pyr`` (PIPS_FLAG_BF16_MAPS; pyramid_mirror() writes it)."""
    ffeats, coords = _f32(ffeats), _f32(coords)
    M = ffeats.shape[0]
    N = M // (B * S)
    X = torch.empty(M, KIN_PAD, dtype=torch.float32, device=ffeats.device)
    tt = times_table(ffeats.device)
    with torch.cuda.device(ffeats.device):
        _call("pips_mixer_input_build_ex", _lib.ptr(pyr), B, S, H8, W8, _lib.ptr(ffeats), _lib.ptr(coords), _lib.ptr(tt), N, None,
              FLAG_BF16_MAPS if bf16_maps else 0, _lib.ptr(X), _stream())
    return X


def mixer_input_build_clips(pyr, T, H8, W8, ffeats, coords, win_start, win_dir, win_clip, clip_first, clip_frames,
                            bf16_maps=False, S=8):
    """pips_mixer_input_build_clips on a linear cache of T frames (B = 1): ffeats (N*S,128), coords (N*S,2) particle-major,
    win_start / win_dir / win_clip (N) int32 (the last two may be None) and the clip table -> X (N*S, 544).  win_clip = None is
    pips_mixer_input_build_win."""
    ffeats, coords = _f32(ffeats), _f32(coords)
    M = ffeats.shape[0]
    X = torch.empty(M, KIN_PAD, dtype=torch.float32, device=ffeats.device)
    tt = times_table(ffeats.device, S)
    with torch.cuda.device(ffeats.device):
        _call("pips_mixer_input_build_clips", _lib.ptr(pyr), 1, int(T), int(T), int(H8), int(W8), _lib.ptr(ffeats), _lib.ptr(coords),
              _lib.ptr(tt), M // S, _i32(win_start), _i32(win_dir), _i32(win_clip), _i32(clip_first), _i32(clip_frames),
              0 if clip_frames is None else clip_frames.numel(), FLAG_BF16_MAPS if bf16_maps else 0, int(S), _lib.ptr(X), _stream())
    return X


def mixer_input_build_rings(pyr, F, R, H8, W8, ffeats, coords, win_start, win_dir, win_clip, clip_first, clip_frames,
                            bf16_maps=False, S=8):
    """pips_mixer_input_build_rings on a flat cache of F slots holding V rings of R slots (B = 1): the arguments of
    ``mixer_input_build_clips``, clip_frames the logical frames appended to each ring so far -> X (N*S, 544)."""
    ffeats, coords = _f32(ffeats), _f32(coords)
    M = ffeats.shape[0]
    X = torch.empty(M, KIN_PAD, dtype=torch.float32, device=ffeats.device)
    tt = times_table(ffeats.device, S)
    with torch.cuda.device(ffeats.device):
        _call("pips_mixer_input_build_rings", _lib.ptr(pyr), 1, int(F), int(R), int(H8), int(W8), _lib.ptr(ffeats), _lib.ptr(coords),
              _lib.ptr(tt), M // S, _i32(win_start), _i32(win_dir), _i32(win_clip), _i32(clip_first), _i32(clip_frames),
              0 if clip_frames is None else clip_frames.numel(), FLAG_BF16_MAPS if bf16_maps else 0, int(S), _lib.ptr(X), _stream())
    return X


def pyramid_append_at(src, F_src, src_first, k, dst, F, ring_first, R, T0, H, W, stride):
    """pips_pyramid_append_at: frames [src_first, src_first + k) of the encoder pyramid ``src`` of F_src frames -> slots ring_first +
    (T0 + i) % R of the pyramid ``dst`` laid out for F slots, fp32 levels and bf16 mirror."""
    with torch.cuda.device(dst.device):
        _call("pips_pyramid_append_at", _lib.ptr(src), int(F_src), int(src_first), int(k), _lib.ptr(dst), int(F), int(ring_first),
              int(R), int(T0), int(H), int(W), int(stride), _stream())
    return dst


def pyramid_mirror(pyr, F, H, W, stride):
    """(re)write the bf16 mirror of a packed pyramid buffer from its fp32 levels (pips_pyramid_mirror)"""
    with torch.cuda.device(pyr.device):
        _call("pips_pyramid_mirror", _lib.ptr(pyr), F, H, W, stride, _stream())
    return pyr


def _gather_tiled(pyr, B, H8, W8, ffeats, coords, out, bf16_maps, ms):
    lib = _lib.load()
    ffeats, coords = _f32(ffeats), _f32(coords)
    M = ffeats.shape[0]
    N = M // (B * S)
    X = out if out is not None else torch.empty(M, KIN_PAD, dtype=torch.float32, device=ffeats.device)
    tt = times_table(ffeats.device)
    nb = lib.pips_gather_scratch_bytes(B, N, H8, W8)
    scratch = torch.empty(nb, dtype=torch.uint8, device=ffeats.device)
    with torch.cuda.device(ffeats.device):
        _call("pips_mixer_input_build_tiled_ex", _lib.ptr(pyr), B, S, H8, W8, _lib.ptr(ffeats), _lib.ptr(coords), _lib.ptr(tt), N,
              FLAG_BF16_MAPS if bf16_maps else 0, _lib.ptr(X), _lib.ptr(scratch), nb, _stream(), ms)
    return X


def mixer_input_build_tiled(pyr, B, H8, W8, ffeats, coords, out=None, bf16_maps=False):
    """Same as mixer_input_build through the tiled kernels for dense query sets.  bf16_maps: the bf16 mode's matrix-core kernel on
    the bf16 mirror behind the fp32 levels of ``pyr`` (PIPS_FLAG_BF16_MAPS; features rounded to bf16 as well, like the
    reference under autocast)."""
    return _gather_tiled(pyr, B, H8, W8, ffeats, coords, out, bf16_maps, None)


def mixer_input_build_tiled_timed(pyr, B, H8, W8, ffeats, coords, bf16_maps=False):
    """(X, {"bin": ms, "embed": ms, "gather": ms}): HIP-event durations of the three launches of the tiled path."""
    ms = (C.c_float * 3)()
    X = _gather_tiled(pyr, B, H8, W8, ffeats, coords, None, bf16_maps, ms)
    return X, {"bin": ms[0], "embed": ms[1], "gather": ms[2]}


def score_map_terms(pyr, B, H8, W8, ffeats, tgt):
    """Per mixer row {loss at the target pixel, sum of the losses of the other pixels} of the dense score map
    (nets/pips.py:501-511 + score_map_loss :58-92).  ffeats (B*N*S,128), tgt (B*N*S,3) = {x, y, use}."""
    return score_map_terms_u(score_map_prepare(pyr, B, S, H8, W8), B, S, H8, W8, ffeats, tgt)


def score_map_prepare(pyr, B, S, H8, W8):
    """pips_score_map_prepare alone: the four levels of a packed pyramid of B*S frames upsampled (align_corners=True) to the
    level-0 size and summed -> U (B*S, H8, W8, 128)."""
    U = torch.empty(B * S, H8, W8, LATENT, dtype=torch.float32, device=pyr.device)
    with torch.cuda.device(pyr.device):
        _call("pips_score_map_prepare", _lib.ptr(pyr), int(B), int(S), int(H8), int(W8), _lib.ptr(U), _stream())
    return U


def score_map_terms_u(U, B, S, H8, W8, ffeats, tgt):
    """pips_score_map_terms alone on a given U (B*S, H8, W8, 128), any window length S: ffeats (B*N*S,128), tgt (B*N*S,3) =
    {x, y, use} -> (B*N*S, 2) {loss at the target pixel, sum of the losses of the other pixels}."""
    ffeats, tgt = _f32(ffeats), _f32(tgt)
    assert U.is_cuda and U.is_contiguous() and U.dtype == torch.float32 and U.numel() == B * S * H8 * W8 * LATENT
    M = ffeats.shape[0]
    out = torch.empty(M, 2, dtype=torch.float32, device=ffeats.device)
    with torch.cuda.device(ffeats.device):
        _call("pips_score_map_terms", _lib.ptr(U), int(B), int(S), int(H8), int(W8), _lib.ptr(ffeats), M // (B * S), _lib.ptr(tgt),
              _lib.ptr(out), _stream())
    return out


def track_ce(arena, pyr, B, H8, W8, xys, stride, iters, flags=0, ce_tgt=None):
    """pips_track_ce on a cached pyramid of B clips of 8 frames: xys (B,N,2) px -> (trajs (iters+1,B,8,N,2), vis (B,8,N),
    ffeat0 (B,N,128), ce_terms (iters,B*N*8,2) or None).  ce_tgt (B*N*8,3): the score-map targets; None = pips_track."""
    lib = _lib.load()
    xys = _f32(xys)
    N = xys.shape[1]
    dev = xys.device
    trajs = torch.empty(iters + 1, B, S, N, 2, dtype=torch.float32, device=dev)
    vis = torch.empty(B, S, N, dtype=torch.float32, device=dev)
    ffeat0 = torch.empty(B, N, LATENT, dtype=torch.float32, device=dev)
    nb = lib.pips_track_workspace_bytes(B, N)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
    tt = times_table(dev)
    ce_terms = ce_ws = None
    if ce_tgt is not None:
        ce_tgt = _f32(ce_tgt)
        ce_terms = torch.empty(iters, B * N * S, 2, dtype=torch.float32, device=dev)
        ce_ws = torch.empty(lib.pips_score_map_workspace_bytes(B, S, H8, W8) // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("pips_track_ce", _lib.ptr(arena), _lib.ptr(pyr), int(B), S, int(H8), int(W8), _lib.ptr(xys), None, None, None, _lib.ptr(tt),
              N, int(stride), int(iters), int(flags), _lib.ptr(ws), nb, _lib.ptr(trajs), _lib.ptr(vis), _lib.ptr(ffeat0), _lib.ptr(ce_tgt),
              _lib.ptr(ce_terms), _lib.ptr(ce_ws), 0 if ce_ws is None else ce_ws.numel() * 4, _stream())
    return trajs, vis, ffeat0, ce_terms


def _mixer_buffers(X, S):
    """(delta (M/S, pips_delta_stride(S)), workspace, its bytes) of a mixer pass on X (M,544)"""
    lib = _lib.load()
    M = X.shape[0]
    delta = torch.empty(M // S, lib.pips_delta_stride(int(S)), dtype=torch.float32, device=X.device)
    nb = lib.pips_mixer_workspace_bytes_s(M, int(S))
    return delta, torch.empty(nb // 4, dtype=torch.float32, device=X.device), nb


def mixer_fwd(arena, X, bf16=False, split=False, S=8, stream_bf16=False):
    """X (M,544) -> delta (M/S, S*130).  bf16: bf16 MFMA operands in the channel-mix/head GEMMs;
    split: every GEMM on the fp32-grade split-bf16 path.  S != 8 (arena packed for that S):
    rows of the library's output are pips_delta_stride(S) apart (cut back to S*130 here).
    stream_bf16 (with bf16, S = 8): the residual stream is a bf16 tensor (PIPS_FLAG_BF16_STREAM)."""
    X = _f32(X)
    if stream_bf16:
        assert bf16 and S == 8 and not split
    flags = FLAG_SPLIT_BF16 if split else (FLAG_BF16_MIXER if bf16 else 0)
    if stream_bf16:
        flags |= FLAG_BF16_STREAM
    delta, ws, nb = _mixer_buffers(X, S)
    with torch.cuda.device(X.device):
        _call("pips_mixer_fwd_s", _lib.ptr(arena), _lib.ptr(X), X.shape[0], int(S), flags, _lib.ptr(delta), _lib.ptr(ws), nb,
              _stream())
    return delta if delta.shape[1] == S * 130 else delta[:, :S * 130]


def mixer_fwd_timed(arena, X, flags=0):
    """Profiling: one mixer pass with HIP events around every GEMM launch.
    flags: 0 exact fp32, FLAG_BF16_MIXER bf16 operands, FLAG_SPLIT_BF16 split-bf16 (PIPS_FLAG_*).
    Returns (delta, {in_proj, up_proj, down_proj, head} milliseconds per launch)."""
    X = _f32(X)
    delta, ws, nb = _mixer_buffers(X, S)
    ms = (C.c_float * 5)()
    with torch.cuda.device(X.device):
        _call("pips_mixer_fwd_timed_ex", _lib.ptr(arena), _lib.ptr(X), X.shape[0], flags, _lib.ptr(delta), _lib.ptr(ws), nb,
              _stream(), ms)
    return delta, {"in_proj": ms[0], "up_proj": ms[1], "down_proj": ms[2], "head": ms[3], "event_overhead": ms[4]}


def mixer_gemm_train(arena, X, flags=0, reps=4):
    """Profiling: a mixer pass on X, then the 12 up-projections / 12 down-projections of the pass as back-to-back launch
    trains between ONE event pair each (pips_mixer_gemm_train).  Returns {up_proj, down_proj} milliseconds per launch,
    start to start -- durations that tile the forward's timeline (no per-launch markers, nothing subtracted)."""
    X = _f32(X)
    M = X.shape[0]
    delta, ws, nb = _mixer_buffers(X, S)
    ms = (C.c_float * 2)()
    with torch.cuda.device(X.device):
        _call("pips_mixer_fwd_s", _lib.ptr(arena), _lib.ptr(X), M, S, flags, _lib.ptr(delta), _lib.ptr(ws), nb, _stream())
        _call("pips_mixer_gemm_train", _lib.ptr(arena), M, flags, _lib.ptr(ws), nb, _stream(), reps, ms)
    return {"up_proj": ms[0], "down_proj": ms[1]}


def state_update(arena, delta, ffeats, coords, coords0, B, N, stride, want_vis=False, S=8):
    """In-place update of ffeats/coords (particle-major); returns (traj (B,S,N,2) px, vis or None).  S != 8 (arena packed
    for that S): delta rows are pips_delta_stride(S) floats apart (pips_state_update_s)."""
    traj = torch.empty(B, S, N, 2, dtype=torch.float32, device=delta.device)
    vis = torch.empty(B, S, N, dtype=torch.float32, device=delta.device) if want_vis else None
    with torch.cuda.device(delta.device):
        if S == 8:
            _call("pips_state_update", _lib.ptr(arena), _lib.ptr(delta), _lib.ptr(ffeats), _lib.ptr(coords), _lib.ptr(coords0), B, N,
                  float(stride), _lib.ptr(traj), _lib.ptr(vis), _stream())
        else:
            _call("pips_state_update_s", _lib.ptr(arena), _lib.ptr(delta), _lib.ptr(ffeats), _lib.ptr(coords), _lib.ptr(coords0), B,
                  N, int(S), float(stride), _lib.ptr(traj), _lib.ptr(vis), _stream())
    return traj, vis


def _stage_flags(bf16, stream_bf16, S):
    if stream_bf16:
        assert bf16 and S == 8
    return (FLAG_BF16_MIXER if bf16 else 0) | (FLAG_BF16_STREAM if stream_bf16 else 0)


def token_mix(arena, layer, x, bf16=False, stream_bf16=False):
    """One launch of the token-mixing kernel of mixer layer ``layer`` (pips_token_mix; exposed for unit tests): x
    (particles, S, 512), fp32 or (stream_bf16) bfloat16, is updated IN PLACE; returns xn = LayerNorm-2 of the new x, fp32 or
    (bf16) bfloat16.  The arena must have been packed for S = x.shape[1]."""
    assert x.is_cuda and x.is_contiguous() and x.dtype == (torch.bfloat16 if stream_bf16 else torch.float32)
    P, Sw, D = x.shape
    assert D == 512
    xn = torch.empty(P, Sw, D, dtype=torch.bfloat16 if bf16 else torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call("pips_token_mix", _lib.ptr(arena), int(layer), _lib.ptr(x), _lib.ptr(xn), P, Sw, _stage_flags(bf16, stream_bf16, Sw),
              _stream())
    return xn


def ln_mean(arena, x, bf16=False, stream_bf16=False):
    """The final LayerNorm and the mean over tokens (pips_ln_mean; exposed for unit tests): x (particles, S, 512) fp32 or
    (stream_bf16) bfloat16 -> (particles, 512) fp32."""
    assert x.is_cuda and x.is_contiguous() and x.dtype == (torch.bfloat16 if stream_bf16 else torch.float32)
    P, Sw, D = x.shape
    assert D == 512
    out = torch.empty(P, D, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call("pips_ln_mean", _lib.ptr(arena), _lib.ptr(x), _lib.ptr(out), P, Sw, _stage_flags(bf16, stream_bf16, Sw), _stream())
    return out


def vis_head(arena, ffeats, B, N):
    """vis_predictor alone (pips_vis_head; exposed for unit tests): ffeats (B*N, S, 128) fp32 -> (B, S, N) logits."""
    assert ffeats.is_cuda and ffeats.is_contiguous() and ffeats.dtype == torch.float32 and ffeats.shape[0] == B * N
    Sw = ffeats.shape[1]
    vis = torch.empty(B, Sw, N, dtype=torch.float32, device=ffeats.device)
    with torch.cuda.device(ffeats.device):
        _call("pips_vis_head", _lib.ptr(arena), _lib.ptr(ffeats), B, N, Sw, _lib.ptr(vis), _stream())
    return vis


def chain_thresholds() -> torch.Tensor:
    """The 64 thresholds of the library's skip scan (pips_chain_threshold; host function) as a float32 CPU tensor."""
    lib = _lib.load()
    return torch.tensor([lib.pips_chain_threshold(k) for k in range(64)], dtype=torch.float32)


def _i32(t):
    assert t is None or (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()), "chaining state is contiguous int32 on the GPU"
    return _lib.ptr(t)


def _chain_f32(t):
    assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()), "chaining state is contiguous float32 on the GPU"
    return _lib.ptr(t)


def chain_gather(trajs, base, cur, dirs, feat, active, n_act, sample_feat=False, clip=None):
    """pips_chain_gather_clips: the staging arrays of one hop for ``active[:n_act]`` -> (xy (n_act,2), ws, wd (n_act) int32,
    fi (n_act,128); fi is left unwritten with ``sample_feat``).  trajs (L,n,2); cur / dirs / active int32, dirs may be None.
    ``clip`` (n) int32 -> (xy, ws, wd, wc, fi), wc (n_act) the staged video indices; None: a NULL table, the one-video form."""
    L, n = trajs.shape[0], trajs.shape[1]
    dev = trajs.device
    xy = torch.empty(n_act, 2, dtype=torch.float32, device=dev)
    ws = torch.empty(n_act, dtype=torch.int32, device=dev)
    wd = torch.empty(n_act, dtype=torch.int32, device=dev)
    wc = None if clip is None else torch.empty(n_act, dtype=torch.int32, device=dev)
    fi = torch.empty(n_act, LATENT, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("pips_chain_gather_clips", _chain_f32(trajs), L, int(base), n, _i32(cur), _i32(dirs), _i32(clip), _chain_f32(feat),
              _i32(active), int(n_act), int(bool(sample_feat)), _lib.ptr(xy), _lib.ptr(ws), _lib.ptr(wd), _lib.ptr(wc), _lib.ptr(fi),
              _stream())
    return (xy, ws, wd, fi) if clip is None else (xy, ws, wd, wc, fi)


def chain_step(win_trajs, win_vis, win_ffeat0, T, active, n_act, trajs, vis, base, cur, dirs, feat, next_active, next_count,
               steps=None, sample_feat=False, clips=None):
    """pips_chain_step_clips, in place on the caller's state: write-back of the windows win_trajs (8,n_act,2) / win_vis (8,n_act),
    skip scan, ``cur`` (and, with ``sample_feat``, ``feat`` from win_ffeat0 (n_act,128)) update, and the live members of
    ``active[:n_act]`` in their order in ``next_active`` with their number in ``next_count`` (device int32, not read back here).
    ``clips`` = (clip (n), clip_frames (V)) int32: live = inside the particle's own video; None: a NULL table, inside the T frames."""
    L, n = trajs.shape[0], trajs.shape[1]
    clip, frames = (None, None) if clips is None else clips
    with torch.cuda.device(trajs.device):
        _call("pips_chain_step_clips", _chain_f32(win_trajs), _chain_f32(win_vis), _chain_f32(win_ffeat0), int(T), n, _i32(active),
              int(n_act), int(bool(sample_feat)), _chain_f32(trajs), _chain_f32(vis), L, int(base), _i32(cur), _i32(dirs), _i32(clip),
              _i32(frames), 0 if frames is None else frames.numel(), _chain_f32(feat), _i32(next_active), _i32(next_count),
              _i32(steps), _stream())


def chain_hop(arena, pyr, T, R, H8, W8, times, stride, iters, flags, active, n_act, trajs, vis, base, cur, dirs, feat,
              next_active, next_count, steps, workspace, sample_feat=False, clips=None):
    """pips_chain_hop_clips: one hop of chain_demo.py:40-83 for ``active[:n_act]``, in place on the caller's state (see
    chain_step), on the packed pyramid ``pyr`` of R frame slots holding T logical frames.  No host synchronisation.
    ``clips`` = (clip (n), clip_first (V), clip_frames (V)) int32: a flat cache of V videos; None: a NULL table, one video."""
    L, n = trajs.shape[0], trajs.shape[1]
    clip, first, frames = (None, None, None) if clips is None else clips
    with torch.cuda.device(trajs.device):
        _call("pips_chain_hop_clips", _lib.ptr(arena), _lib.ptr(pyr), int(T), int(R), int(H8), int(W8), _lib.ptr(times), int(stride),
              int(iters), int(flags), n, _i32(active), int(n_act), int(bool(sample_feat)), _chain_f32(trajs), _chain_f32(vis), L,
              int(base), _i32(cur), _i32(dirs), _i32(clip), _i32(first), _i32(frames), 0 if frames is None else frames.numel(),
              _chain_f32(feat), _i32(next_active), _i32(next_count), _i32(steps), _lib.ptr(workspace), workspace.numel() * 4,
              _stream())


def stream_workspace_bytes(n, iters):
    """pips_stream_workspace_bytes: the workspace of one round over a state of ``n`` queries (host function)."""
    return _lib.load().pips_stream_workspace_bytes(int(n), int(iters))


def stream_select(T, final, tq, xy, cur, status, trajs, active, new_list, counts):
    """pips_stream_select, in place on the caller's stream state (include/pips_hip.h): tq / cur / status (n) int32, xy (n,2), trajs
    (L,n,2); ``active`` / ``new_list`` (n) int32 receive the ready queries and the ones that join, ``counts`` (4) int32 their
    numbers and the lowest pending window start (device: the caller reads it back)."""
    L, n = trajs.shape[0], trajs.shape[1]
    with torch.cuda.device(trajs.device):
        _call("pips_stream_select", int(T), int(bool(final)), n, _i32(tq), _chain_f32(xy), _i32(cur), _i32(status), _chain_f32(trajs), L,
              _i32(active), _i32(new_list), _i32(counts), _stream())


def stream_round(arena, pyr, T, R, H8, W8, times, stride, iters, flags, final, n_act, n_new, tq, xy, cur, status, feat, trajs, vis,
                 active, new_list, counts, steps, workspace):
    """pips_stream_round: the join of ``new_list[:n_new]``, one hop of ``active[:n_act]`` and the selection of the next round, in
    place on the caller's stream state, on the packed ring pyramid ``pyr`` of R frame slots holding T logical frames.  No host
    synchronisation."""
    L, n = trajs.shape[0], trajs.shape[1]
    with torch.cuda.device(trajs.device):
        _call("pips_stream_round", _lib.ptr(arena), _lib.ptr(pyr), int(T), int(R), int(H8), int(W8), _lib.ptr(times), int(stride),
              int(iters), int(flags), int(bool(final)), n, int(n_act), int(n_new), _i32(tq), _chain_f32(xy), _i32(cur), _i32(status),
              _chain_f32(feat), _chain_f32(trajs), _chain_f32(vis), L, _i32(active), _i32(new_list), _i32(counts), _i32(steps),
              _lib.ptr(workspace), workspace.numel() * 4, _stream())


def stream_emit(trajs, vis, f0, f1):
    """pips_stream_emit: frames [f0, f1) of the row ring trajs (L,n,2) / vis (L,n) -> dense (f1-f0,n,2) and (f1-f0,n); their ring
    rows are reset to NaN."""
    L, n = trajs.shape[0], trajs.shape[1]
    m = max(int(f1) - int(f0), 0)
    out_t = torch.empty(m, n, 2, dtype=torch.float32, device=trajs.device)
    out_v = torch.empty(m, n, dtype=torch.float32, device=trajs.device)
    with torch.cuda.device(trajs.device):
        _call("pips_stream_emit", _chain_f32(trajs), _chain_f32(vis), L, n, int(f0), int(f1), _lib.ptr(out_t), _lib.ptr(out_v), _stream())
    return out_t, out_v


def stream_workspace_bytes_clips(n, iters, V):
    """pips_stream_workspace_bytes_clips: the workspace of one round over a state of ``n`` queries of V streams (host function)."""
    return _lib.load().pips_stream_workspace_bytes_clips(int(n), int(iters), int(V))


def stream_select_clips(tq, xy, cur, status, clip, clip_frames, clip_final, trajs, active, new_list, counts):
    """pips_stream_select_clips, in place on a state over V streams (include/pips_hip.h): ``stream_select`` with the stream of each
    query ``clip`` (n) and the tables ``clip_frames`` / ``clip_final`` (V) int32 in the place of T / final; ``counts`` is (4 + V)."""
    L, n = trajs.shape[0], trajs.shape[1]
    with torch.cuda.device(trajs.device):
        _call("pips_stream_select_clips", n, _i32(tq), _chain_f32(xy), _i32(cur), _i32(status), _i32(clip), _i32(clip_frames),
              _i32(clip_final), clip_frames.numel(), _chain_f32(trajs), L, _i32(active), _i32(new_list), _i32(counts), _stream())


def stream_round_clips(arena, pyr, F, R, H8, W8, times, stride, iters, flags, n_act, n_new, tq, xy, cur, status, clip, feat, trajs, vis,
                       clip_first, clip_frames, clip_final, active, new_list, counts, steps, workspace):
    """pips_stream_round_clips: ``stream_round`` on a state over V streams, on the packed pyramid ``pyr`` of F slots holding V rings
    of R slots.  No host synchronisation."""
    L, n = trajs.shape[0], trajs.shape[1]
    with torch.cuda.device(trajs.device):
        _call("pips_stream_round_clips", _lib.ptr(arena), _lib.ptr(pyr), int(F), int(R), int(H8), int(W8), _lib.ptr(times), int(stride),
              int(iters), int(flags), n, int(n_act), int(n_new), _i32(tq), _chain_f32(xy), _i32(cur), _i32(status), _i32(clip),
              _chain_f32(feat), _chain_f32(trajs), _chain_f32(vis), L, _i32(clip_first), _i32(clip_frames), _i32(clip_final),
              clip_frames.numel(), _i32(active), _i32(new_list), _i32(counts), _i32(steps), _lib.ptr(workspace),
              workspace.numel() * 4, _stream())


def stream_emit_cols(trajs, vis, f0, f1, cols):
    """pips_stream_emit_cols: frames [f0, f1) of the columns ``cols`` (m) int32 of the row ring trajs (L,n,2) / vis (L,n) -> dense
    (f1-f0,m,2) and (f1-f0,m); exactly those elements are reset to NaN."""
    L, n = trajs.shape[0], trajs.shape[1]
    nf, m = max(int(f1) - int(f0), 0), cols.numel()
    out_t = torch.empty(nf, m, 2, dtype=torch.float32, device=trajs.device)
    out_v = torch.empty(nf, m, dtype=torch.float32, device=trajs.device)
    with torch.cuda.device(trajs.device):
        _call("pips_stream_emit_cols", _chain_f32(trajs), _chain_f32(vis), L, n, int(f0), int(f1), _i32(cols), m, _lib.ptr(out_t),
              _lib.ptr(out_v), _stream())
    return out_t, out_v


def stream_keep(keep, tq, xy, cur, status, feat, trajs, vis, clip=None, V=0):
    """pips_stream_keep: the columns ``keep`` (m) int32, ascending, of the stream state tq / cur / status (n) int32, xy (n,2), feat
    (n,128), trajs (L,n,2), vis (L,n) -- and ``clip`` (n) int32 of a state over ``V`` streams -- in new arrays for m queries; the
    inputs are left as they were.  -> (tq, xy, cur, status, feat, trajs, vis[, clip], counts): ``counts`` (4, or 4 + V with
    ``clip``) int32 on the device holds {0, 0, low, 0[, low_0 .. low_{V-1}]} of the kept set (the caller reads it back)."""
    L, n = trajs.shape[0], trajs.shape[1]
    m, dev, i32, f32 = keep.numel(), trajs.device, torch.int32, torch.float32
    o_tq, o_cur, o_status = (torch.empty(m, dtype=i32, device=dev) for _ in range(3))
    o_clip = None if clip is None else torch.empty(m, dtype=i32, device=dev)
    o_xy, o_feat = torch.empty(m, 2, dtype=f32, device=dev), torch.empty(m, LATENT, dtype=f32, device=dev)
    o_trajs, o_vis = torch.empty(L, m, 2, dtype=f32, device=dev), torch.empty(L, m, dtype=f32, device=dev)
    counts = torch.empty(4 if clip is None else 4 + int(V), dtype=i32, device=dev)
    with torch.cuda.device(dev):
        _call("pips_stream_keep", n, _i32(keep), m, _i32(tq), _chain_f32(xy), _i32(cur), _i32(status), _i32(clip), _chain_f32(feat),
              _chain_f32(trajs), _chain_f32(vis), L, _lib.ptr(o_tq), _lib.ptr(o_xy), _lib.ptr(o_cur), _lib.ptr(o_status),
              _lib.ptr(o_clip), _lib.ptr(o_feat), _lib.ptr(o_trajs), _lib.ptr(o_vis), int(V), _lib.ptr(counts), _stream())
    return (o_tq, o_xy, o_cur, o_status, o_feat, o_trajs, o_vis) + (() if clip is None else (o_clip,)) + (counts,)


def cover_step(trajs, vis, f1, tq, xy, lost, H, W, cell, vis_logit, lost_after, max_queries):
    """pips_cover_step on the rows trajs (m,n,2) / vis (m,n) of frames [f1 - m, f1) and the per-query tq / lost (n) int32 and xy
    (n,2): which queries are kept and where new ones are seeded (include/pips_hip.h).  -> (keep (n) int32, lost_out (n) int32,
    seeds (min(cells, max_queries),3), counts (4) int32) on ``xy``'s device: counts = {n_keep, n_seed, n_outside, n_lost} says how
    much of each list was written (the caller reads it back); the inputs are left as they were."""
    m, n, dev = vis.shape[0], tq.numel(), xy.device
    gh, gw = (int(H) - 1) // int(cell) + 1, (int(W) - 1) // int(cell) + 1
    keep, lost_out = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    seeds = torch.empty(max(min(gh * gw, int(max_queries)), 1), 3, dtype=torch.float32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.load().pips_cover_workspace_bytes(n, gh, gw) // 4, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _call("pips_cover_step", n, m, int(f1), _chain_f32(trajs), _chain_f32(vis), _i32(tq), _chain_f32(xy), _i32(lost), int(H), int(W),
              int(cell), float(vis_logit), int(lost_after), int(max_queries), _lib.ptr(keep), _lib.ptr(lost_out), _lib.ptr(seeds),
              _lib.ptr(counts), _lib.ptr(ws), ws.numel() * 4, _stream())
    return keep, lost_out, seeds, counts


def cover_step_thin(trajs, vis, f1, tq, xy, lost, crowd, H, W, cell, vis_logit, lost_after, max_queries, per_cell, crowd_after):
    """pips_cover_step_thin: ``cover_step`` with at most ``per_cell`` tracks in a cell -- ``crowd`` (n) int32 is the second run of each
    query, and a query that was surplus in its cell for ``crowd_after`` returned frames in a row is retired (include/pips_hip.h).
    -> (keep (n), lost_out (n), crowd_out (n) int32, seeds (min(cells, max_queries),3), gone (n), reason (n) int32, counts (5)
    int32) on ``xy``'s device: counts = {n_keep, n_seed, n_outside, n_lost, n_crowded}; keep / lost_out / crowd_out are written up to
    n_keep, gone / reason (1 outside, 2 lost, 3 crowded) up to n - n_keep; the inputs are left as they were."""
    m, n, dev = vis.shape[0], tq.numel(), xy.device
    gh, gw = (int(H) - 1) // int(cell) + 1, (int(W) - 1) // int(cell) + 1
    keep, lost_out, crowd_out, gone, reason = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(5))
    seeds = torch.empty(max(min(gh * gw, int(max_queries)), 1), 3, dtype=torch.float32, device=dev)
    counts = torch.empty(5, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.load().pips_cover_thin_workspace_bytes(n, m, gh, gw) // 4, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _call("pips_cover_step_thin", n, m, int(f1), _chain_f32(trajs), _chain_f32(vis), _i32(tq), _chain_f32(xy), _i32(lost), _i32(crowd),
              int(H), int(W), int(cell), float(vis_logit), int(lost_after), int(max_queries), int(per_cell), int(crowd_after),
              _lib.ptr(keep), _lib.ptr(lost_out), _lib.ptr(crowd_out), _lib.ptr(seeds), _lib.ptr(gone), _lib.ptr(reason), _lib.ptr(counts),
              _lib.ptr(ws), ws.numel() * 4, _stream())
    return keep, lost_out, crowd_out, seeds, gone, reason, counts


def corner_table(frames, cell):
    """pips_corner_table on device frames (F,3,h,w), uint8 or float 0..255 -> table (F,gh,gw,3) float32 = (x, y, S): the best
    corner of each cover cell of each frame and its score; a cell without a candidate holds its centre and -1 (include/pips_hip.h)."""
    assert frames.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames must be (F,3,h,w), not {tuple(frames.shape)}")
    src = frames.contiguous() if frames.dtype == torch.uint8 else _f32(frames)
    F, _, h, w = src.shape
    gh, gw = (h - 1) // int(cell) + 1, (w - 1) // int(cell) + 1
    table = torch.empty(F, gh, gw, 3, dtype=torch.float32, device=src.device)
    if F == 0:                                                                    # (an empty tensor has no pointer to pass)
        return table
    with torch.cuda.device(src.device):
        _call("pips_corner_table", _lib.ptr(src), 1 if src.dtype == torch.uint8 else 0, F, h, w, int(cell), _lib.ptr(table), _stream())
    return table


def cut_table(frames, prev_hist=None):
    """pips_cut_table on device frames (F,3,h,w), uint8 or float 0..255 -> (hist (F,16,32) int32, dist (F,) int32): the regional
    luma histogram of each frame and its distance to the frame before -- frame 0 against ``prev_hist`` (16,32) int32, the last
    histogram of the call before, or 0 without it (include/pips_hip.h).  Outputs and workspace are allocated here: one call."""
    assert frames.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames must be (F,3,h,w), not {tuple(frames.shape)}")
    src = frames.contiguous() if frames.dtype == torch.uint8 else _f32(frames)
    F, _, h, w = src.shape
    if h < 1 or w < 1 or h * w > 2 ** 30:
        raise ValueError(f"frames of {h} x {w}: need at least 1 x 1 and at most 2^30 pixels")
    if prev_hist is not None:
        if tuple(prev_hist.shape) != (16, 32) or prev_hist.is_floating_point():
            raise ValueError(f"prev_hist must be a (16,32) integer tensor, not {tuple(prev_hist.shape)} {prev_hist.dtype}")
        prev_hist = prev_hist.to(src.device, torch.int32).contiguous()
    hist = torch.empty(F, 16, 32, dtype=torch.int32, device=src.device)
    dist = torch.empty(F, dtype=torch.int32, device=src.device)
    if F == 0:                                                                    # (an empty tensor has no pointer to pass)
        return hist, dist
    lib = _lib.load()
    nbytes = lib.pips_cut_workspace_bytes(F, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        _call("pips_cut_table", _lib.ptr(src), 1 if src.dtype == torch.uint8 else 0, F, h, w, _lib.ptr(prev_hist), _lib.ptr(hist),
              _lib.ptr(dist), _lib.ptr(ws), nbytes, _stream())
    return hist, dist


# include/pips_hip.h: PIPS_MOTION_*; MOTION_TILE is csrc/common.h's (the points a scoring block holds in LDS at a time: n may be larger)
MOTION_QUARTER_MAX, MOTION_HYPS_MAX, MOTION_THR4_MAX, MOTION_N_MAX = 8191, 1024, 1024, 65536
MOTION_HYPS, MOTION_TILE = 64, 2048


def motion_workspace_bytes(F, n, K):
    return int(_lib.load().pips_motion_workspace_bytes(int(F), int(n), int(K)))


def motion_fit(trajs, vis, frame0, vis_logit, K, thr4, seed):
    """pips_motion_fit on device rows trajs (F,n,2) float32 and vis (F,n) logits or None -> (head (P,4) int32, sums (P,8) int64,
    model (P,4) float64, flags (P,n) uint8) for the P = max(F - 1, 0) pairs of consecutive rows: the consensus similarity of each
    pair (include/pips_hip.h has the rule).  Outputs and workspace are allocated here: one call."""
    assert trajs.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    if trajs.dim() != 3 or trajs.shape[2] != 2:
        raise ValueError(f"trajs must be (F,n,2), not {tuple(trajs.shape)}")
    src = _f32(trajs)
    F, n = src.shape[:2]
    if vis is not None:
        if tuple(vis.shape) != (F, n):
            raise ValueError(f"vis must be (F,n) = {(F, n)}, not {tuple(vis.shape)}")
        vis = _f32(vis.to(src.device))
    K, thr4, frame0, seed = int(K), int(thr4), int(frame0), int(seed)
    if n > MOTION_N_MAX:
        raise ValueError(f"{n} columns: the sums are exact up to {MOTION_N_MAX}")
    if not 1 <= K <= MOTION_HYPS_MAX or not 1 <= thr4 <= MOTION_THR4_MAX:
        raise ValueError(f"need 1 <= K <= {MOTION_HYPS_MAX} and 1 <= thr4 <= {MOTION_THR4_MAX} (K={K}, thr4={thr4})")
    if frame0 < 0 or frame0 + F > 2 ** 31 - 1 or not 0 <= seed < 2 ** 32:
        raise ValueError(f"frame0 + F must fit an int32 and seed a uint32 (frame0={frame0}, seed={seed})")
    P, dev = max(F - 1, 0), src.device
    head = torch.empty(P, 4, dtype=torch.int32, device=dev)
    sums = torch.empty(P, 8, dtype=torch.int64, device=dev)
    model = torch.empty(P, 4, dtype=torch.float64, device=dev)
    flags = torch.empty(P, n, dtype=torch.uint8, device=dev)
    if P == 0:                                                                    # (nothing is launched, nothing to write)
        return head, sums, model, flags
    nbytes = motion_workspace_bytes(F, n, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _call("pips_motion_fit", _lib.ptr(src) if n else None, _lib.ptr(vis) if n else None, F, n, frame0, float(vis_logit), K, thr4,
              seed - (1 << 32) if seed >= 1 << 31 else seed, _lib.ptr(head), _lib.ptr(sums), _lib.ptr(model), _lib.ptr(flags) if n else None, _lib.ptr(ws), nbytes, _stream())
    return head, sums, model, flags


MOTION_LAYERS_MAX = 8                                                              # PIPS_MOTION_LAYERS_MAX


def motion_layers_workspace_bytes(F, n, K, L):
    return int(_lib.load().pips_motion_layers_workspace_bytes(int(F), int(n), int(K), int(L)))


def motion_layers(trajs, vis, frame0, vis_logit, K, thr4, seed, L, min_in, prev_layer=None):
    """pips_motion_layers on device rows trajs (F,n,2) float32, vis (F,n) logits or None and prev_layer (n,) uint8 or None -> (head
    (P,L,4) int32, sums (P,L,8) int64, model (P,L,4) float64, box (P,L,4) int32, layer (P,n) uint8, overlap (P,L,L) int32) for the
    P = max(F - 1, 0) pairs of consecutive rows: the consensus of ``motion_fit`` peeled into L layers a pair (include/pips_hip.h has
    the rule).  Outputs and workspace are allocated here: one call."""
    assert trajs.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    if trajs.dim() != 3 or trajs.shape[2] != 2:
        raise ValueError(f"trajs must be (F,n,2), not {tuple(trajs.shape)}")
    src = _f32(trajs)
    F, n = src.shape[:2]
    if vis is not None:
        if tuple(vis.shape) != (F, n):
            raise ValueError(f"vis must be (F,n) = {(F, n)}, not {tuple(vis.shape)}")
        vis = _f32(vis.to(src.device))
    if prev_layer is not None:
        if tuple(prev_layer.shape) != (n,) or prev_layer.dtype != torch.uint8:
            raise ValueError(f"prev_layer must be uint8 (n,) = {(n,)}, not {prev_layer.dtype} {tuple(prev_layer.shape)}")
        prev_layer = prev_layer.to(src.device).contiguous()
    K, thr4, frame0, seed, L, min_in = int(K), int(thr4), int(frame0), int(seed), int(L), int(min_in)
    if n > MOTION_N_MAX:
        raise ValueError(f"{n} columns: the sums are exact up to {MOTION_N_MAX}")
    if not 1 <= K <= MOTION_HYPS_MAX or not 1 <= thr4 <= MOTION_THR4_MAX:
        raise ValueError(f"need 1 <= K <= {MOTION_HYPS_MAX} and 1 <= thr4 <= {MOTION_THR4_MAX} (K={K}, thr4={thr4})")
    if frame0 < 0 or frame0 + F > 2 ** 31 - 1 or not 0 <= seed < 2 ** 32:
        raise ValueError(f"frame0 + F must fit an int32 and seed a uint32 (frame0={frame0}, seed={seed})")
    if not 1 <= L <= MOTION_LAYERS_MAX or not 2 <= min_in <= MOTION_N_MAX:
        raise ValueError(f"need 1 <= L <= {MOTION_LAYERS_MAX} and 2 <= min_in <= {MOTION_N_MAX} (L={L}, min_in={min_in})")
    P, dev = max(F - 1, 0), src.device
    head = torch.empty(P, L, 4, dtype=torch.int32, device=dev)
    sums = torch.empty(P, L, 8, dtype=torch.int64, device=dev)
    model = torch.empty(P, L, 4, dtype=torch.float64, device=dev)
    box = torch.empty(P, L, 4, dtype=torch.int32, device=dev)
    layer = torch.empty(P, n, dtype=torch.uint8, device=dev)
    overlap = torch.empty(P, L, L, dtype=torch.int32, device=dev)
    if P == 0:                                                                    # (nothing is launched, nothing to write)
        return head, sums, model, box, layer, overlap
    nbytes = motion_layers_workspace_bytes(F, n, K, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _call("pips_motion_layers", _lib.ptr(src) if n else None, _lib.ptr(vis) if n else None, _lib.ptr(prev_layer) if n else None, F, n,
              frame0, float(vis_logit), K, thr4, seed - (1 << 32) if seed >= 1 << 31 else seed, L, min_in, _lib.ptr(head),
              _lib.ptr(sums), _lib.ptr(model), _lib.ptr(box), _lib.ptr(layer) if n else None, _lib.ptr(overlap), _lib.ptr(ws), nbytes,
              _stream())
    return head, sums, model, box, layer, overlap


def cover_place(seeds, table, h, w, cell, min_corner):
    """pips_cover_place: the seeds (k,3) = (t, x, y) of a cover step, float32 and contiguous, are moved IN PLACE onto the corners
    of ``table`` (gh,gw,3), the table of the seeds' frame, where the cell's score is above ``min_corner`` -> seeds"""
    assert seeds.is_cuda and table.is_cuda, "pips_amd runs on the GPU only (no CPU fallback)"
    gh, gw = (int(h) - 1) // int(cell) + 1, (int(w) - 1) // int(cell) + 1
    if seeds.dtype != torch.float32 or not seeds.is_contiguous() or seeds.dim() != 2 or seeds.shape[1] != 3:
        raise ValueError("seeds must be a contiguous float32 (k,3) tensor")
    if table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape) != (gh, gw, 3):
        raise ValueError(f"table must be a contiguous float32 ({gh},{gw},3) tensor, not {tuple(table.shape)}")
    if seeds.shape[0] == 0:
        return seeds
    with torch.cuda.device(seeds.device):
        _call("pips_cover_place", _lib.ptr(seeds), seeds.shape[0], _lib.ptr(table), int(h), int(w), int(cell), int(min_corner), _stream())
    return seeds


def gemm(A, W, bias=None, epi=0, R=None):
    """C = epi(A @ W.T + bias).  epi: 0 none, 1 GELU, 2 + R."""
    A, W = _f32(A), _f32(W)
    M, K = A.shape
    N = W.shape[0]
    Cm = torch.empty(M, N, dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        _call("pips_gemm_f32", _lib.ptr(A), K, _lib.ptr(W), _lib.ptr(bias), _lib.ptr(Cm), N, M, N, K, epi, _lib.ptr(R),
              N if R is not None else 0, _stream())
    return Cm


def split_bf16x3(w):
    """fp32 tensor -> its three bf16 planes, int16 tensor of shape (3, *w.shape) (exact split: each plane is the round-to-nearest-even bf16 of the
    remainder, so the three sum to w and the dropped cross terms are zero-mean; gemm_x3.hip)."""
    w = _f32(w)
    out = torch.empty((3,) + tuple(w.shape), dtype=torch.int16, device=w.device)
    with torch.cuda.device(w.device):
        _call("pips_split_bf16x3", _lib.ptr(w), w.numel(), _lib.ptr(out), _stream())
    return out


def gemm_x3(A, W3, bias=None, epi=0, R=None):
    """gemm() on the split-bf16 path; W3 = split_bf16x3(W) with W of shape (N, K)."""
    A = _f32(A)
    M, K = A.shape
    N = W3.shape[1]
    Cm = torch.empty(M, N, dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        _call("pips_gemm_f32x3", _lib.ptr(A), K, _lib.ptr(W3), _lib.ptr(bias), _lib.ptr(Cm), N, M, N, K, epi, _lib.ptr(R),
              N if R is not None else 0, _stream())
    return Cm


def gemm_bf16(A, W, bias=None, epi=0, R=None, out_bf16=False):
    """gemm() with bf16 MFMA operands: A fp32 or bfloat16 (M,K), W bfloat16 (N,K); returns fp32 or bfloat16 (M,N)."""
    assert W.dtype == torch.bfloat16 and A.dtype in (torch.float32, torch.bfloat16)
    A, W = A.contiguous(), W.contiguous()
    M, K = A.shape
    N = W.shape[0]
    Cm = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=A.device)
    if R is not None and R.dtype == torch.bfloat16:      # a bf16 residual (with a bf16 output): the mixer's bf16 residual stream
        assert out_bf16 and epi == EPI_RESIDUAL
        epi = epi | EPI_RES_BF16
        R = R.contiguous()
    with torch.cuda.device(A.device):
        _call("pips_gemm_bf16", _lib.ptr(A), int(A.dtype == torch.bfloat16), K, _lib.ptr(W), _lib.ptr(bias), _lib.ptr(Cm),
              int(out_bf16), N, M, N, K, epi, _lib.ptr(R), N if R is not None else 0, _stream())
    return Cm


def partial_sums(stats):
    """Pivoted InstanceNorm partials (F, parts, C, 4) = {sum(x-p), sum((x-p)^2), p, n} -> fp64 (sum x, sum x^2) per (F, C)."""
    st = stats.double()
    s, q, p, n = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
    p = torch.where(n > 0, p, torch.zeros_like(p))
    return (n * p + s).sum(dim=1), (q + 2 * p * s + n * p * p).sum(dim=1)


def inorm_finalize(stats):
    """Pivoted InstanceNorm partials (F, parts, C, 4) -> (F, C, 2) = {mean, rstd}: the encoder's own finalize kernel."""
    st = _f32(stats)
    F, parts, Cc, _ = st.shape
    out = torch.empty(F, Cc, 2, dtype=torch.float32, device=st.device)
    with torch.cuda.device(st.device):
        _call("pips_inorm_finalize_pivot", _lib.ptr(st), F, parts, Cc, _lib.ptr(out), _stream())
    return out


def _map(t):
    """an NHWC activation map as the stage entry points take it: contiguous fp32 or bfloat16 on the device"""
    assert t.is_cuda and t.dtype in (torch.float32, torch.bfloat16), "a map is a float32 or bfloat16 device tensor"
    return t.contiguous()


def encoder_stem(arena, rgbs, bf16=False):
    """pips_encoder_stem: rgbs (F,3,H,W) 0..255, float or uint8 -> the raw conv1 map (F,Ho,Wo,64), fp32 or (bf16) bfloat16, and
    its pivoted partial statistics (F, parts, 64, 4) -- feed those to inorm_finalize()."""
    lib = _lib.load()
    u8 = rgbs.dtype == torch.uint8
    rgbs = rgbs.contiguous() if u8 else _f32(rgbs)
    F, _, H, W = rgbs.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    parts = lib.pips_encoder_stem_parts(H, W)
    out = torch.empty(F, Ho, Wo, 64, dtype=torch.bfloat16 if bf16 else torch.float32, device=rgbs.device)
    stats = torch.zeros(F, parts, 64, 4, dtype=torch.float32, device=rgbs.device)
    told = C.c_int(0)
    with torch.cuda.device(rgbs.device):
        _call("pips_encoder_stem", _lib.ptr(arena), _lib.ptr(rgbs), F, H, W, (FLAG_BF16_ENCODER if bf16 else 0) | (FLAG_RGB_U8 if u8 else 0),
              _lib.ptr(out), _lib.ptr(stats), C.byref(told), _stream())
    assert told.value == parts
    return out, stats


def inorm_apply(x, stats, res=None, res_stats=None, mode=0):
    """pips_inorm_apply (fp32 maps in mode 3: pips_inorm_apply_f32) on NHWC maps x (F,...,C), fp32 or bfloat16, with stats (F,C,2) = {mean, rstd}: mode 0 relu(n(x)), 1
    relu(res + relu(n(x))), 2 relu(n2(res) + relu(n(x))), 3 relu(relu(n2(res)) + relu(n(x)))."""
    x, stats = _map(x), _f32(stats)
    res = None if res is None else _map(res)
    res_stats = None if res_stats is None else _f32(res_stats)
    assert res is None or (res.dtype == x.dtype and res.shape == x.shape)
    F, Cc = x.shape[0], x.shape[-1]
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        if int(mode) == 3 and x.dtype == torch.float32:       # fp32 maps: mode 3 lives on the fp32 entry point
            _call("pips_inorm_apply_f32", _lib.ptr(x), _lib.ptr(stats), _lib.ptr(res), _lib.ptr(res_stats), 3, _lib.ptr(y), F,
                  x.numel() // (F * Cc), Cc, _stream())
        else:
            _call("pips_inorm_apply", _lib.ptr(x), _lib.ptr(stats), _lib.ptr(res), _lib.ptr(res_stats), int(mode), _lib.ptr(y), F,
                  x.numel() // (F * Cc), Cc, int(x.dtype == torch.bfloat16), _stream())
    return y


def resize_into(src, dst, coff):
    """pips_resize_into: the align_corners bilinear resize of src (F,Hs,Ws,C) written IN PLACE into channels [coff, coff + C) of
    dst (F,Hd,Wd,Cdst), a contiguous map of the same type (fp32 or bfloat16) -> dst"""
    src = _map(src)
    assert dst.is_cuda and dst.is_contiguous() and dst.dtype == src.dtype and dst.shape[0] == src.shape[0]
    F, Hs, Ws, Cc = src.shape
    _, Hd, Wd, Cdst = dst.shape
    with torch.cuda.device(src.device):
        _call("pips_resize_into", _lib.ptr(src), F, Hs, Ws, Cc, _lib.ptr(dst), Hd, Wd, Cdst, int(coff),
              int(src.dtype == torch.bfloat16), _stream())
    return dst


def avgpool2(src):
    """pips_avgpool2: fp32 NHWC map (F,H,W,C) -> its 2x2 means (F,H//2,W//2,C)"""
    src = _f32(src)
    F, H, W, Cc = src.shape
    dst = torch.empty(F, H // 2, W // 2, Cc, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _call("pips_avgpool2", _lib.ptr(src), F, H, W, Cc, _lib.ptr(dst), _stream())
    return dst


def _conv(name, x, w, bias, ksize, stride, pad, want_stats, in_norm=None, out_dtype=torch.float32, route=None, out=None):
    """One NHWC convolution entry point: x (F,H,W,Cin), w with Cout = ``w.shape[-4]`` -> (F,Ho,Wo,Cout) [+ its pivoted partial
    statistics (F, parts, Cout, 4), cut to the parts the kernel reports].  ``pips_conv_nhwc_bf16_maps`` also takes in_norm,
    the output type and the room for partials (the larger bound of the LDS-resident 64 -> 64 kernel)."""
    maps = name == "pips_conv_nhwc_bf16_maps"
    F, H, W, Cin = x.shape
    Cout = w.shape[-4]
    Ho = (H + 2 * pad - ksize) // stride + 1
    Wo = (W + 2 * pad - ksize) // stride + 1
    if out is None:
        out = torch.empty(F, Ho, Wo, Cout, dtype=out_dtype, device=x.device)
    assert out.shape == (F, Ho, Wo, Cout) and out.dtype == out_dtype and out.is_contiguous() and out.device == x.device
    cap = 2 * ((Ho * Wo + 63) // 64) + 4
    if maps:
        cap = max(cap, ((Wo + 31) // 32) * ((Ho + 3) // 4) * 4)
    stats = torch.zeros(F, cap, Cout, 4, dtype=torch.float32, device=x.device) if want_stats else None
    tiles = C.c_int(0)
    geom = (F, H, W, Cin, _lib.ptr(w), _lib.ptr(bias), Cout, ksize, stride, pad, _lib.ptr(out))
    with torch.cuda.device(x.device):
        if maps:
            _call(name, _lib.ptr(x), _lib.ptr(in_norm), *geom, 1 if out_dtype == torch.bfloat16 else 0, _lib.ptr(stats), cap,
                  C.byref(tiles), _stream())
        elif route is not None:
            _call(name, _lib.ptr(x), *geom, _lib.ptr(stats), C.byref(tiles), route, _stream())
        else:
            _call(name, _lib.ptr(x), *geom, _lib.ptr(stats), C.byref(tiles), _stream())
    if want_stats:
        return out, stats.view(-1)[: F * tiles.value * Cout * 4].view(F, tiles.value, Cout, 4)
    return out


def conv_nhwc(x, w_packed, bias, ksize, stride, pad, want_stats=False, route=None, out=None):
    """x (F,H,W,Cin) NHWC, w_packed (Cout, k, k, Cin) -> (F,Ho,Wo,Cout) [+ pivoted partial stats (F, parts, Cout, 4),
    parts = m tiles x wave rows: see partial_sums()].  route: None = the kernel the shape selects, "igemm" = igemm_f32_kernel,
    "e" = the 64 x 64 LDS-DMA body of conv_f32_e.hip (pips_conv_nhwc_f32_route).  out: a contiguous (F,Ho,Wo,Cout) fp32 tensor to
    write into (it may be a view of a larger buffer)."""
    if route is None:
        return _conv("pips_conv_nhwc_f32", _f32(x), _f32(w_packed), bias, ksize, stride, pad, want_stats, out=out)
    return _conv("pips_conv_nhwc_f32_route", _f32(x), _f32(w_packed), bias, ksize, stride, pad, want_stats,
                 route={"igemm": 1, "e": 2}[route], out=out)


def conv_nhwc_f32_r(x, w_packed, bias, in_norm=None, ksize=3, stride=1, pad=1, out=None, stats=None):
    """pips_conv_nhwc_f32_r: the LDS-resident 64 -> 64 3x3 convolution of the fp32 encoder's layer 1 at any map size.  x (F,H,W,64)
    fp32, ``in_norm`` (F,64,2) = {mean, rstd} of the producing layer (relu((x - mean) * rstd) while the map is staged) -> the raw
    map (F,H,W,64) and its partials (F, parts, 64, 4), parts = 4 * ceil(H/4) * ceil(W/32).  out / stats: contiguous fp32 tensors to
    write into (views of larger buffers in the containment tests); stats holds (F, cap, 64, 4), its cap is handed to the library."""
    x, w = _f32(x), _f32(w_packed)
    F, H, W, Cin = x.shape
    Cout = w.shape[-4]
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    if out is None:
        out = torch.empty(F, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    if stats is None:
        stats = torch.zeros(F, 4 * ((Ho + 3) // 4) * ((Wo + 31) // 32), Cout, 4, dtype=torch.float32, device=x.device)
    assert out.shape == (F, Ho, Wo, Cout) and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
    assert stats.dim() == 4 and stats.shape[0] == F and stats.shape[2:] == (Cout, 4) and stats.is_contiguous()
    parts = C.c_int(0)
    with torch.cuda.device(x.device):
        _call("pips_conv_nhwc_f32_r", _lib.ptr(x), _lib.ptr(None if in_norm is None else _f32(in_norm)), F, H, W, Cin, _lib.ptr(w),
              _lib.ptr(bias), Cout, ksize, stride, pad, _lib.ptr(out), _lib.ptr(stats), stats.shape[1], C.byref(parts), _stream())
    return out, stats.view(-1)[: F * parts.value * Cout * 4].view(F, parts.value, Cout, 4)


def encoder_l1_fused(F, H, W):
    """pips_encoder_l1_fused: does the exact-fp32 encoder run layer 1 of F frames of H x W pixels on that kernel (current device)?"""
    return bool(_lib.load().pips_encoder_l1_fused(int(F), int(H), int(W)))


def conv_nhwc_bf16(x, w_bf16, bias, ksize, stride, pad, want_stats=False):
    """conv_nhwc() with bf16 MFMA operands; w_bf16 = w_packed.bfloat16() of shape (Cout, k, k, Cin)."""
    assert w_bf16.dtype == torch.bfloat16
    return _conv("pips_conv_nhwc_bf16", _f32(x), w_bf16.contiguous(), bias, ksize, stride, pad, want_stats)


def conv_nhwc_bf16_maps(x_bf16, w_bf16, bias, ksize, stride, pad, in_norm=None, out_bf16=True, want_stats=False):
    """The same convolution on a bf16 NHWC map (the bf16 encoder's form): ``in_norm`` (F, Cin, 2) = {mean, rstd} of the
    producing layer applies relu((x - mean) * rstd) while the map is staged (64 -> 64 3x3 layers the LDS-resident kernel
    takes); the output map is bf16 or fp32."""
    assert x_bf16.dtype == torch.bfloat16 and w_bf16.dtype == torch.bfloat16 and x_bf16.is_cuda
    return _conv("pips_conv_nhwc_bf16_maps", x_bf16.contiguous(), w_bf16.contiguous(), bias, ksize, stride, pad, want_stats,
                 in_norm=None if in_norm is None else _f32(in_norm), out_dtype=torch.bfloat16 if out_bf16 else torch.float32)


def conv_nhwc_x3(x, w3, bias, ksize, stride, pad, want_stats=False):
    """conv_nhwc() on the split-bf16 path; w3 = split_bf16x3(w_packed)."""
    return _conv("pips_conv_nhwc_f32x3", _f32(x), w3, bias, ksize, stride, pad, want_stats)
