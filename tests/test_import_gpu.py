"""GPU: decoder frames in.  pips_frames_import is held, bit for bit, to drivers.import_frames_torch run on the CPU: every format,
matrix, range and output type; rows that are tight, one byte and 64 bytes wider; planes that start 0, 1 and 4 bytes off the 16-byte
grid; frames with a gap between them; sizes with odd width and height, a head and a tail around the 16-byte groups, and outputs
whose planes do not share their alignment -- into poisoned buffers with guard bands on both sides.  The fused resize is held to the
twin and to the two-step library path (import at source size, then pips_resize_frames).  Then the return codes, and the imported
frames in use: corner and cut tables, Pips.encode and a streamed tracker fed imported chunks."""
import ctypes as C
import math

import pytest
import torch

from test_import import FORMATS, MATRICES, PACKED, RANGES, source
from test_stream_rounds_gpu import H_, W_, _bits, _model, _queries, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                                     # elements on either side of dst
E_ARG = -1
COMBOS = [(m, r) for m in MATRICES for r in RANGES]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poison(dtype):
    return 171 if dtype == torch.uint8 else -77.0


def _surface(plane, pad, off, gap, seed):
    """the host plane (F, rows, ...) on the device as a view of a random byte buffer: rows ``pad`` bytes wider than their bytes,
    frames ``gap`` bytes further apart than their rows, the first byte ``off`` bytes behind a 16-byte address"""
    F, rows = plane.shape[:2]
    row_bytes = math.prod(plane.shape[2:])
    pitch = row_bytes + pad
    step = pitch * rows + gap
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, 256, (F * step + 48,), generator=g, dtype=torch.uint8).to(DEV)
    lead = (-buf.data_ptr()) % 16 + off
    inner = [math.prod(plane.shape[k + 1:]) for k in range(2, plane.dim())]        # the format's own element strides
    view = torch.as_strided(buf, tuple(plane.shape), (step, pitch, *inner), lead)
    view.copy_(plane)
    assert F == 0 or view.data_ptr() % 16 == off
    return view


def _raw_import(lib, planes, fmt, matrix, range_, dtype, size=None, dst_off=0):
    """pips_frames_import itself on device planes (pitch and step from their strides) into a poisoned buffer with guard bands;
    ``dst_off``: elements between dst and a 16-byte address -> dst on the host; the bands are checked"""
    from pips_amd import ops
    F, h, w = planes[0].shape[:3]
    H, W = (h, w) if size is None else size
    n = F * 3 * H * W
    es = 1 if dtype == torch.uint8 else 4
    out = torch.full((n + 2 * GUARD + 16,), _poison(dtype), dtype=dtype, device=DEV)
    lead = ((-out.data_ptr()) % 16) // es + GUARD - GUARD % (16 // es) + dst_off
    args = []
    for p in planes:
        args += [C.c_void_p(p.data_ptr()), p.stride(1), p.stride(0)]
    args += [None, 0, 0] * (3 - len(planes))
    before = [p.clone() for p in planes]
    rc = lib.pips_frames_import(ops.IMPORT_FORMATS[fmt], ops.IMPORT_MATRICES[matrix], ops.IMPORT_RANGES[range_], F, h, w, *args,
                                C.c_void_p(out.data_ptr() + lead * es), int(dtype == torch.uint8), H, W, _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    assert bool((out[:lead] == _poison(dtype)).all()) and bool((out[lead + n:] == _poison(dtype)).all()), "written outside dst"
    assert all(torch.equal(a, b) for a, b in zip(planes, before))
    return out[lead:lead + n].view(F, 3, H, W).cpu()


def _same(a, b):
    flat = lambda t: t.contiguous().reshape(-1).view(torch.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(flat(a), flat(b))


# (pad, off, gap): tight rows on the grid; rows a byte wider from a base 1 byte off; rows 64 bytes wider from a base 4 bytes off,
# frames 7 bytes further apart
LAYOUTS = [(0, 0, 0), (1, 1, 0), (64, 4, 7), (0, 4, 0), (64, 1, 16)]


# 1x1, 2x2; 3x5: odd x odd; 16x53 and 37x53: a head, groups and a tail in rows that start at every alignment, planes that do (16x53
# uint8) and do not share their alignment; 64x96: whole groups only
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (16, 53), (37, 53), (64, 96)])
def test_import_is_the_torch_form(fmt, h, w):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    combos = COMBOS if fmt not in PACKED else COMBOS[:1]
    for F in (0, 1, 3):
        host = [p.contiguous() for p in source(fmt, F, h, w, 31 * h + w + F)]
        want = {(c, dt): drivers.import_frames_torch(host, fmt, None, *c, dt) for c in combos for dt in (torch.uint8, torch.float32)}
        for i, (pad, off, gap) in enumerate(LAYOUTS if F else LAYOUTS[:1]):
            planes = [_surface(p, pad, off, gap, i) for p in host]
            for j, c in enumerate(combos):
                if i > 0 and j != i % len(combos):                          # every matrix and range on the first layout, one on the others
                    continue
                for dt in (torch.uint8, torch.float32):
                    for dst_off in ((0, 1, 4) if dt == torch.uint8 and i < 2 else (0,)):
                        got = _raw_import(lib, planes, fmt, *c, dt, dst_off=dst_off)
                        assert _same(got, want[(c, dt)]), (fmt, h, w, F, pad, off, gap, c, dt, dst_off)
                    assert _same(ops.import_frames(planes, fmt, None, *c, dt).cpu(), want[(c, dt)])       # strides passed through


@pytest.mark.parametrize("fmt,h,w,F", [("nv12", 360, 640, 1), ("bgr24", 360, 640, 1), ("i420", 360, 640, 1), ("rgba32", 360, 640, 1),
                                       ("nv12", 1080, 1920, 2)])
def test_import_at_video_sizes(fmt, h, w, F):
    """several blocks a row and a frame index behind the first; a decoder's pitch (rows padded to 256 bytes) and the tight one"""
    from pips_amd import _lib, drivers
    lib = _lib.load()
    host = [p.contiguous() for p in source(fmt, F, h, w, h + F)]
    for pad, off, gap, dt in ((0, 0, 0, torch.uint8), ((-host[0][0, 0].numel()) % 256, 0, 512, torch.float32)):
        want = drivers.import_frames_torch(host, fmt, None, "bt709", "limited", dt)
        got = _raw_import(lib, [_surface(p, pad, off, gap, 1) for p in host], fmt, "bt709", "limited", dt)
        assert _same(got, want), (fmt, pad, dt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("src,dst", [((3, 5), (8, 8)), ((37, 53), (16, 20)), ((64, 96), (64, 96))])
def test_fused_resize_is_the_twin_and_the_two_step_path(fmt, src, dst):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    host = [p.contiguous() for p in source(fmt, 2, src[0], src[1], 5 * src[0])]
    for i, (pad, off, gap) in enumerate(LAYOUTS[:3]):
        planes = [_surface(p, pad, off, gap, i) for p in host]
        c = COMBOS[i]
        want = drivers.import_frames_torch(host, fmt, dst, *c, torch.float32)
        got = _raw_import(lib, planes, fmt, *c, torch.float32, size=dst)
        assert _same(got, want), (fmt, src, dst, c)
        two_step = ops.resize_frames(ops.import_frames(planes, fmt, None, *c, torch.uint8), dst)
        assert _same(got, two_step.cpu())
        as_u8 = _raw_import(lib, planes, fmt, *c, torch.uint8, size=dst, dst_off=i)
        assert _same(as_u8, (got + 0.5).floor().to(torch.uint8)) and _same(as_u8, drivers.import_frames_torch(host, fmt, dst, *c))
        assert _same(ops.import_frames(planes, fmt, dst, *c, torch.float32).cpu(), want)


@pytest.mark.parametrize("fmt", ["nv12", "bgr24"])
def test_fused_resize_1080p_to_the_models_size(fmt):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    host = [p.contiguous() for p in source(fmt, 1, 1080, 1920, 9)]
    planes = [_surface(p, (-p[0, 0].numel()) % 256, 0, 0, 2) for p in host]
    want = drivers.import_frames_torch(host, fmt, (360, 640), "bt709", "limited", torch.float32)
    got = _raw_import(lib, planes, fmt, "bt709", "limited", torch.float32, size=(360, 640))
    assert _same(got, want)
    assert _same(got, ops.resize_frames(ops.import_frames(planes, fmt), (360, 640)).cpu())
    as_u8 = _raw_import(lib, planes, fmt, "bt709", "limited", torch.uint8, size=(360, 640))
    assert _same(as_u8, (got + 0.5).floor().to(torch.uint8))


def test_bad_arguments_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    F, h, w = 2, 6, 9
    y, uv, v = (_surface(p, 3, 0, 0, k) for k, p in enumerate(source("nv12", F, h, w, 1) + source("i420", F, h, w, 2)[2:]))
    rgba = _surface(source("rgba32", F, h, w, 3)[0], 3, 0, 0, 4)
    out = torch.full((F * 3 * 12 * 12,), 171, dtype=torch.uint8, device=DEV)
    ptr = lambda t: t.data_ptr()

    def call(fmt=4, matrix=1, range_=0, F=F, h=h, w=w, p=(ptr(y), ptr(uv), 0), pitch=(12, 13, 0), step=(72, 39, 0), dst=ptr(out), u8=1,
             H=h, W=w):
        rc = lib.pips_frames_import(fmt, matrix, range_, F, h, w, p[0] or None, pitch[0], step[0], p[1] or None, pitch[1], step[1],
                                    p[2] or None, pitch[2], step[2], dst or None, u8, H, W, _stream())
        torch.cuda.synchronize()
        assert bool((out == 171).all())
        return rc

    assert (y.stride(1), uv.stride(1), y.stride(0), uv.stride(0)) == (12, 13, 72, 39)
    i420 = dict(fmt=5, p=(ptr(y), ptr(uv), ptr(v)), pitch=(12, 8, 8), step=(72, 24, 24))     # (uv's bytes as a U plane, v's as V)
    assert v.stride(1) == 8 and v.stride(0) == 24
    packed = dict(fmt=2, p=(ptr(rgba), 0, 0), pitch=(39, 0, 0), step=(234, 0, 0))
    assert rgba.stride(1) == 39 and rgba.stride(0) == 234
    for over in (dict(fmt=-1), dict(fmt=6), dict(matrix=2), dict(matrix=-1), dict(range_=2), dict(range_=-1), dict(F=-1), dict(h=0),
                 dict(w=0), dict(h=-6), dict(H=0), dict(W=0), dict(W=-9), dict(dst=0), dict(p=(0, ptr(uv), 0)), dict(p=(ptr(y), 0, 0)),
                 dict(pitch=(8, 13, 0)), dict(pitch=(12, 9, 0)), dict(step=(71, 39, 0)), dict(step=(72, 38, 0)), dict(step=(0, 0, 0)),
                 dict(F=1 << 10, H=1 << 10, W=(1 << 10) + 1),
                 dict(i420, p=(ptr(y), ptr(uv), 0)), dict(i420, pitch=(12, 8, 4)), dict(i420, step=(72, 24, 23)), dict(i420, matrix=5),
                 dict(packed, pitch=(35, 0, 0)), dict(packed, p=(0, 0, 0)), dict(packed, step=(233, 0, 0)), dict(packed, fmt=7)):
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error()
    assert call(F=0) == 0 and call(F=0, p=(0, 0, 0), dst=0) == 0 and call(F=0, H=12, W=12) == 0       # nothing is launched
    assert call(**dict(packed, F=0, matrix=9, range_=9)) == 0                    # matrix and range are not read for a packed format
    assert lib.pips_abi_version() == 3


def test_tables_agree_on_the_uint8_and_the_float_output():
    """pips_corner_table and pips_cut_table quantise a float frame the way the import quantises its uint8 output"""
    from pips_amd import ops
    planes = [p.to(DEV) for p in source("nv12", 3, 100, 150, 6, 2, 1)]
    for size in ((64, 96), None):
        as_u8, as_f32 = (ops.import_frames(planes, "nv12", size, "bt601", "full", dt) for dt in (torch.uint8, torch.float32))
        assert size is None or not torch.equal(as_f32, as_f32.round())              # the float output is not on the 8-bit grid
        assert torch.equal(_bits(ops.corner_table(as_u8, 16)), _bits(ops.corner_table(as_f32, 16)))
        for a, b in zip(ops.cut_table(as_u8), ops.cut_table(as_f32)):
            assert torch.equal(a, b)


def _yuv_of(video):
    """an NV12 form of a planar uint8 video (T,3,h,w), even h and w: any plausible Y and 2 x 2 averaged chroma"""
    r, g, b = (video[:, k].float() for k in range(3))
    y = (0.2126 * r + 0.7152 * g + 0.0722 * b) * (219.0 / 255.0) + 16.0
    cb, cr = ((b - y) * 0.5 + 128.0, (r - y) * 0.6 + 128.0)
    pool = lambda c: torch.nn.functional.avg_pool2d(c.unsqueeze(1), 2).squeeze(1)
    to8 = lambda c: c.round().clamp(0, 255).to(torch.uint8)
    return to8(y), torch.stack([to8(pool(cb)), to8(pool(cr))], dim=-1)


def test_encode_and_a_streamed_tracker_take_imported_frames(weights_tamed):
    """Pips.encode of an imported chunk is Pips.encode of the twin's frames; a stream fed drivers.import_frames chunks -- the BGR24
    and the NV12 form of one video, from the host and from a pitched device surface -- is the stream fed the twin's planar frames,
    in bits and hop lists"""
    from pips_amd import drivers, ops
    m = _model(weights_tamed)
    T = 12
    video = _video(T, H_, W_, seed=91)[0].to(torch.uint8)                         # (T,3,H,W)
    q = _queries([0, 0, 2, 5], 92).to(DEV)
    forms = {"bgr24": [video.permute(0, 2, 3, 1).flip(-1).contiguous()], "nv12": list(_yuv_of(video))}
    for fmt, host in forms.items():
        twin = drivers.import_frames_torch(host, fmt).unsqueeze(0)
        assert fmt != "bgr24" or torch.equal(twin[0], video)
        device = [_surface(p, (-p[0, 0].numel()) % 64 + 64, 0, 0, 3) for p in host]
        got = drivers.import_frames(device, fmt)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, T, 3, H_, W_) and torch.equal(got.cpu(), twin)
        levels = [ops.pyramid_levels(m.encode(x).pyr, 8, H_, W_, 8) for x in (got[:, :8], twin[:, :8].to(DEV))]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*levels))       # (behind the levels the buffer is not written)
        chunks = [slice(0, 5), slice(5, 8), slice(8, 12)]
        ref = drivers.track_stream(m, [twin[:, s].to(DEV) for s in chunks], q, iters=6, slots=9, return_hops=True)
        for planes in (host, device):                                              # host planes cross in their source format
            fed = [drivers.import_frames([p[s] for p in planes], fmt, device=DEV) for s in chunks]
            out = drivers.track_stream(m, fed, q, iters=6, slots=9, return_hops=True)
            assert torch.equal(_bits(out[0]), _bits(ref[0])) and torch.equal(_bits(out[1]), _bits(ref[1])) and out[2] == ref[2], fmt
        assert bool(torch.isfinite(ref[0][:, 5:]).all())
