"""GPU: pips_frames_import_ex -- the triangle (antialiasing) filter and the 10-bit formats P010 and I010 -- held, bit for bit, to
drivers.import_frames_torch run on the CPU: every format and both output types on pitched surfaces whose planes start off the
16-byte grid, into poisoned buffers with guard bands; shapes of one pixel, of a footprint that is most of the image, of several
ragged tiles, of one axis scaled up and one down, and one where the tile is shortened to fit its LDS.  The 10-bit formats without a
resize and with the bilinear one (the twin and the two-step library path); then the return codes, and the antialiased frames in
use: corner and cut tables, Pips.encode and a streamed tracker."""
import ctypes as C

import pytest
import torch

from test_import import FORMATS, source
from test_import_aa import FORMATS16, source16
from test_import_gpu import COMBOS, DEV, E_ARG, GUARD, _poison, _same, _stream, _surface
from test_stream_rounds_gpu import H_, W_, _bits, _model, _queries, _video

pytestmark = pytest.mark.gpu
ALL_FORMATS = FORMATS + FORMATS16
BILINEAR, TRIANGLE = 0, 1


def _host(fmt, F, h, w, seed):
    return [p.contiguous() for p in (source16 if fmt in FORMATS16 else source)(fmt, F, h, w, seed)]


def _surface16(plane, pad, off, gap, seed):
    """``_surface`` for a plane of 16-bit words: the words' bytes on a pitched surface (``pad``, ``off`` and ``gap`` even), seen as
    int16 again"""
    assert pad % 2 == 0 and off % 2 == 0 and gap % 2 == 0
    as_bytes = plane.contiguous().view(torch.uint8)                               # the last dimension doubles
    return _surface(as_bytes, pad, off, gap, seed).view(torch.int16)


def _surfaces(fmt, host, i):
    """the planes on the device: tight on the grid (i = 0); rows a sample wider from an odd base -- 1 byte off, or 2 for 16-bit
    words -- (1); rows 64 bytes wider from a base 4 bytes off and frames further apart (2)"""
    if fmt in FORMATS16:
        pad, off, gap = [(0, 0, 0), (2, 2, 0), (64, 4, 6)][i]
        return [_surface16(p, pad, off, gap, i) for p in host]
    pad, off, gap = [(0, 0, 0), (1, 1, 0), (64, 4, 7)][i]
    return [_surface(p, pad, off, gap, i) for p in host]


def _raw_import_ex(lib, planes, fmt, matrix, range_, dtype, size=None, dst_off=0, filt=BILINEAR):
    """pips_frames_import_ex itself on device planes (pitch and step in bytes from their strides) into a poisoned buffer with guard
    bands; ``dst_off``: elements between dst and a 16-byte address -> dst on the host; the bands and the planes are checked"""
    from pips_amd import ops
    F, h, w = planes[0].shape[:3]
    H, W = (h, w) if size is None else size
    n = F * 3 * H * W
    es = 1 if dtype == torch.uint8 else 4
    out = torch.full((n + 2 * GUARD + 16,), _poison(dtype), dtype=dtype, device=DEV)
    lead = ((-out.data_ptr()) % 16) // es + GUARD - GUARD % (16 // es) + dst_off
    args = []
    for p in planes:
        args += [C.c_void_p(p.data_ptr()), p.stride(1) * p.element_size(), p.stride(0) * p.element_size()]
    args += [None, 0, 0] * (3 - len(planes))
    before = [p.clone() for p in planes]
    rc = lib.pips_frames_import_ex(ops.IMPORT_FORMATS[fmt], ops.IMPORT_MATRICES[matrix], ops.IMPORT_RANGES[range_], filt, F, h, w, *args,
                                   C.c_void_p(out.data_ptr() + lead * es), int(dtype == torch.uint8), H, W, _stream())
    assert rc == 0, lib.pips_last_error()
    torch.cuda.synchronize()
    assert bool((out[:lead] == _poison(dtype)).all()) and bool((out[lead + n:] == _poison(dtype)).all()), "written outside dst"
    assert all(torch.equal(a, b) for a, b in zip(planes, before))
    return out[lead:lead + n].view(F, 3, H, W).cpu()


# 1x1; (3,5)->(2,2): every output reads most of the image; (37,53)->(8,12): one ragged tile; (30,40)->(45,16): up on one axis,
# down on the other; (32,47)->(2,3): next to the 16 x limit; (130,300)->(40,70): 3 x 5 tiles, the last ragged on both axes, a
# footprint walked in several batches of eight rows; (64,96)->(64,96): equal sizes, the plain conversion
@pytest.mark.parametrize("fmt", ALL_FORMATS)
@pytest.mark.parametrize("src,dst,F", [((1, 1), (1, 1), 2), ((3, 5), (2, 2), 2), ((37, 53), (8, 12), 2), ((30, 40), (45, 16), 2),
                                       ((32, 47), (2, 3), 2), ((130, 300), (40, 70), 2), ((64, 96), (64, 96), 3)])
def test_triangle_filter_is_the_twin(fmt, src, dst, F):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    host = _host(fmt, F, src[0], src[1], 7 * src[0] + src[1])
    for i in (1, 2):
        planes = _surfaces(fmt, host, i)
        c = COMBOS[(i + len(fmt)) % 4]
        want = drivers.import_frames_torch(host, fmt, dst, *c, torch.float32, antialias=True)
        got = _raw_import_ex(lib, planes, fmt, *c, torch.float32, size=dst, filt=TRIANGLE)
        assert _same(got, want), (fmt, src, dst, c)
        as_u8 = _raw_import_ex(lib, planes, fmt, *c, torch.uint8, size=dst, dst_off=i, filt=TRIANGLE)
        assert _same(as_u8, drivers.import_frames_torch(host, fmt, dst, *c, antialias=True))
        assert _same(as_u8, (got + 0.5).floor().to(torch.uint8))
        assert _same(ops.import_frames(planes, fmt, dst, *c, torch.float32, antialias=True).cpu(), want)
        if src == dst:
            assert _same(got, drivers.import_frames_torch(host, fmt, None, *c, torch.float32))


@pytest.mark.parametrize("fmt", ["rgb24", "p010"])
def test_triangle_filter_at_the_ratio_that_shortens_the_tile(fmt):
    """16 x 15 down: a tile of 8 rows would need more than 64 KiB of LDS, so the launch takes shorter tiles, with the
    widest footprint a tile can have"""
    from pips_amd import _lib, drivers
    lib = _lib.load()
    host = _host(fmt, 1, 512, 600, 77)
    planes = _surfaces(fmt, host, 2)
    for dt in (torch.float32, torch.uint8):
        want = drivers.import_frames_torch(host, fmt, (32, 40), "bt601", "limited", dt, antialias=True)
        assert _same(_raw_import_ex(lib, planes, fmt, "bt601", "limited", dt, size=(32, 40), filt=TRIANGLE), want)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_triangle_filter_1080p_to_the_models_size(fmt):
    from pips_amd import _lib, drivers
    lib = _lib.load()
    host = _host(fmt, 1, 1080, 1920, 9)
    pad = (-host[0][0, 0].numel() * host[0].element_size()) % 256                  # a decoder's pitch
    planes = [(_surface16 if fmt in FORMATS16 else _surface)(p, pad, 0, 0, 2) for p in host]
    want = drivers.import_frames_torch(host, fmt, (368, 496), "bt709", "limited", torch.float32, antialias=True)
    got = _raw_import_ex(lib, planes, fmt, "bt709", "limited", torch.float32, size=(368, 496), filt=TRIANGLE)
    assert _same(got, want)
    as_u8 = _raw_import_ex(lib, planes, fmt, "bt709", "limited", torch.uint8, size=(368, 496), filt=TRIANGLE)
    assert _same(as_u8, (got + 0.5).floor().to(torch.uint8))


# the shapes of test_import_is_the_torch_form: a head, groups and a tail in rows that start at every (even) alignment
@pytest.mark.parametrize("fmt", FORMATS16)
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (16, 53), (37, 53), (64, 96)])
def test_ten_bit_import_is_the_torch_form(fmt, h, w):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    for F in (0, 1, 3):
        host = _host(fmt, F, h, w, 31 * h + w + F)
        want = {(c, dt): drivers.import_frames_torch(host, fmt, None, *c, dt) for c in COMBOS for dt in (torch.uint8, torch.float32)}
        for i in (0, 1, 2) if F else (0,):
            planes = _surfaces(fmt, host, i)
            for j, c in enumerate(COMBOS):
                if i > 0 and j != i:                                             # every matrix and range on the first layout, one on the others
                    continue
                for dt in (torch.uint8, torch.float32):
                    for dst_off in ((0, 1, 4) if dt == torch.uint8 and i < 2 else (0,)):
                        for filt in (BILINEAR, TRIANGLE):                        # (equal sizes: no filter runs)
                            got = _raw_import_ex(lib, planes, fmt, *c, dt, dst_off=dst_off, filt=filt)
                            assert _same(got, want[(c, dt)]), (fmt, h, w, F, i, c, dt, dst_off, filt)
                    assert _same(ops.import_frames(planes, fmt, None, *c, dt).cpu(), want[(c, dt)])       # strides passed through


@pytest.mark.parametrize("fmt", FORMATS16)
@pytest.mark.parametrize("src,dst", [((37, 53), (16, 20)), ((3, 5), (8, 8))])
def test_ten_bit_bilinear_resize_is_the_twin_and_the_two_step_path(fmt, src, dst):
    from pips_amd import _lib, drivers, ops
    lib = _lib.load()
    host = _host(fmt, 2, src[0], src[1], 5 * src[0])
    for i in (0, 1, 2):
        planes = _surfaces(fmt, host, i)
        c = COMBOS[i]
        want = drivers.import_frames_torch(host, fmt, dst, *c, torch.float32)
        got = _raw_import_ex(lib, planes, fmt, *c, torch.float32, size=dst)
        assert _same(got, want), (fmt, src, dst, c)
        assert _same(got, ops.resize_frames(ops.import_frames(planes, fmt, None, *c, torch.uint8), dst).cpu())
        as_u8 = _raw_import_ex(lib, planes, fmt, *c, torch.uint8, size=dst, dst_off=i)
        assert _same(as_u8, (got + 0.5).floor().to(torch.uint8)) and _same(as_u8, drivers.import_frames_torch(host, fmt, dst, *c))
        assert _same(ops.import_frames(planes, fmt, dst, *c, torch.float32).cpu(), want)


def test_bad_arguments_of_the_new_entry_are_rejected_and_nothing_is_written():
    from pips_amd import _lib
    lib = _lib.load()
    F, h, w = 2, 6, 9
    y, uv = (_surface(p, 3, 0, 0, k) for k, p in enumerate(source("nv12", F, h, w, 1)))
    y16, uv16 = (_surface16(p, 2, 0, 0, k) for k, p in enumerate(source16("p010", F, h, w, 2)))
    u16, v16 = (_surface16(p, 2, 0, 0, k) for k, p in enumerate(source16("i010", F, h, w, 3)[1:]))
    out = torch.full((F * 3 * 12 * 12,), 171, dtype=torch.uint8, device=DEV)
    ptr = lambda t: t.data_ptr()

    def call(fmt=4, matrix=1, range_=0, filt=BILINEAR, F=F, h=h, w=w, p=(ptr(y), ptr(uv), 0), pitch=(12, 13, 0), step=(72, 39, 0),
             dst=ptr(out), u8=1, H=h, W=w, written=False):
        rc = lib.pips_frames_import_ex(fmt, matrix, range_, filt, F, h, w, p[0] or None, pitch[0], step[0], p[1] or None, pitch[1],
                                       step[1], p[2] or None, pitch[2], step[2], dst or None, u8, H, W, _stream())
        torch.cuda.synchronize()
        assert written or bool((out == 171).all())
        return rc

    assert (y.stride(1), uv.stride(1), y.stride(0), uv.stride(0)) == (12, 13, 72, 39)
    assert (y16.stride(1), uv16.stride(1), y16.stride(0), uv16.stride(0)) == (10, 11, 60, 33)       # in words: 20, 22, 120, 66 bytes
    assert (u16.stride(1), u16.stride(0), v16.stride(1), v16.stride(0)) == (6, 18, 6, 18)
    p010 = dict(fmt=6, p=(ptr(y16), ptr(uv16), 0), pitch=(20, 22, 0), step=(120, 66, 0))
    i010 = dict(fmt=7, p=(ptr(y16), ptr(u16), ptr(v16)), pitch=(20, 12, 12), step=(120, 36, 36))
    for over in (dict(fmt=-1), dict(fmt=8), dict(filt=2), dict(filt=-1), dict(matrix=2), dict(range_=-1), dict(F=-1), dict(h=0), dict(W=0),
                 dict(dst=0), dict(p=(0, ptr(uv), 0)), dict(pitch=(8, 13, 0)), dict(step=(72, 38, 0)),
                 dict(F=1 << 10, H=1 << 10, W=(1 << 10) + 1),
                 dict(filt=TRIANGLE, H=6, W=8193), dict(filt=TRIANGLE, h=8193, pitch=(12, 13, 0), F=1, H=4096),
                 dict(filt=TRIANGLE, w=9, W=0), dict(filt=TRIANGLE, F=1, h=33, H=2),
                 dict(p010, matrix=2), dict(p010, pitch=(16, 22, 0)), dict(p010, pitch=(20, 18, 0)), dict(p010, pitch=(21, 22, 0)),
                 dict(p010, pitch=(20, 23, 0)), dict(p010, step=(121, 66, 0)), dict(p010, step=(120, 67, 0)),
                 dict(p010, p=(ptr(y16) + 1, ptr(uv16), 0)), dict(p010, p=(ptr(y16), ptr(uv16) + 1, 0)), dict(p010, p=(ptr(y16), 0, 0)),
                 dict(p010, step=(118, 66, 0)), dict(p010, filt=3),
                 dict(i010, p=(ptr(y16), ptr(u16), 0)), dict(i010, pitch=(20, 12, 8)), dict(i010, pitch=(20, 12, 13)),
                 dict(i010, p=(ptr(y16), ptr(u16), ptr(v16) + 1)), dict(i010, step=(120, 36, 37)), dict(i010, step=(120, 36, 34))):
        assert call(**over) == E_ARG, over
        assert lib.pips_last_error()
    assert call(F=0) == 0 and call(F=0, filt=TRIANGLE, H=12, W=12) == 0 and call(**dict(p010, F=0)) == 0           # nothing is launched
    assert lib.pips_abi_version() == 3
    # the same surfaces as they are, are taken: dst is written
    for ok in (dict(), dict(filt=TRIANGLE, H=4, W=5), p010, dict(i010, filt=TRIANGLE, H=12, W=12)):
        out.fill_(171)
        assert call(**dict(ok, written=True)) == 0, lib.pips_last_error()
        assert not bool((out == 171).all())


def test_tables_agree_on_the_uint8_and_the_float_output_of_an_antialiased_import():
    from pips_amd import ops
    planes = [p.to(DEV) for p in source16("p010", 3, 200, 310, 6)]
    as_u8, as_f32 = (ops.import_frames(planes, "p010", (64, 96), "bt601", "full", dt, antialias=True) for dt in (torch.uint8, torch.float32))
    assert not torch.equal(as_f32, as_f32.round())                                   # the float output is not on the 8-bit grid
    assert torch.equal(_bits(ops.corner_table(as_u8, 16)), _bits(ops.corner_table(as_f32, 16)))
    for a, b in zip(ops.cut_table(as_u8), ops.cut_table(as_f32)):
        assert torch.equal(a, b)


def _p010_of(video):
    """a P010 form of a planar uint8 video (T,3,h,w), even h and w: any plausible 10-bit Y and 2 x 2 averaged chroma, in the high
    ten bits of the words, the low six filled with a pattern"""
    r, g, b = (video[:, k].float() for k in range(3))
    y = (0.2126 * r + 0.7152 * g + 0.0722 * b) * (876.0 / 255.0) + 64.0
    cb, cr = ((b * 4 - y) * 0.5 + 512.0, (r * 4 - y) * 0.6 + 512.0)
    pool = lambda c: torch.nn.functional.avg_pool2d(c.unsqueeze(1), 2).squeeze(1)
    word = lambda c: ((c.round().clamp(0, 1023).to(torch.int32) << 6) | 37).to(torch.uint16)
    return word(y), torch.stack([word(pool(cb)), word(pool(cr))], dim=-1)


def test_encode_and_a_streamed_tracker_take_antialiased_p010_frames(weights_tamed):
    """drivers.import_frames(p010 planes, "p010", size=(H_, W_), antialias=True) of a video twice the model's size, fed to
    Pips.encode and to a streamed tracker, gives the bits that the twin's frames give"""
    from pips_amd import drivers, ops
    m = _model(weights_tamed)
    T = 12
    big = torch.nn.functional.interpolate(_video(T, H_, W_, seed=93)[0], (2 * H_ + 6, 2 * W_ + 10), mode="bilinear").round().to(torch.uint8)
    host = list(_p010_of(big))
    q = _queries([0, 0, 2, 5], 94).to(DEV)
    for dt in (torch.uint8, torch.float32):
        twin = drivers.import_frames_torch(host, "p010", (H_, W_), dtype=dt, antialias=True).unsqueeze(0)
        device = [_surface16(p, 64, 2, 0, 3) for p in host]
        got = drivers.import_frames(device, "p010", (H_, W_), dtype=dt, antialias=True)
        assert got.dtype == dt and got.is_cuda and tuple(got.shape) == (1, T, 3, H_, W_) and _same(got.cpu(), twin)
        levels = [ops.pyramid_levels(m.encode(x).pyr, 8, H_, W_, 8) for x in (got[:, :8], twin[:, :8].to(DEV))]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*levels))
        if dt != torch.uint8:                                                      # (the stream: on the uint8 frames)
            continue
        chunks = [slice(0, 5), slice(5, 8), slice(8, 12)]
        ref = drivers.track_stream(m, [twin[:, s].to(DEV) for s in chunks], q, iters=6, slots=9, return_hops=True)
        for planes in (host, device):                                              # host planes cross in their source format
            fed = [drivers.import_frames([p[s] for p in planes], "p010", (H_, W_), dtype=dt, device=DEV, antialias=True) for s in chunks]
            out = drivers.track_stream(m, fed, q, iters=6, slots=9, return_hops=True)
            assert torch.equal(_bits(out[0]), _bits(ref[0])) and torch.equal(_bits(out[1]), _bits(ref[1])) and out[2] == ref[2], dt
        assert bool(torch.isfinite(ref[0][:, 5:]).all())
