"""CPU: the seams of the launchers -- the sizes at which a call is cut into several launches with a base index (``f_base +
blockIdx.y``), a grid is held to a cap and the kernel walks the rest in a stride loop, or one block walks a list in chunks.  The
table of them is DESIGN.md's "Launch seams".  Here: each constant read out of the source text it is defined in, the cases of
tests/test_seams_gpu.py made and shown to lie on the far side of their constant with at least one exactly at it (whoever changes
a constant finds this test failing, not the GPU test quietly on one side), the inputs shown not to be vacuous, the periodic
expectation of the 65535-frame cases held to the twin run over every frame at a small count, and the torch-indexing references
of pips_stream_keep / pips_stream_emit / pips_stream_emit_cols held to plain loops.  (The twins of masks, tint, draw and warp
against their rules by plain loops: tests/test_masks.py, test_draw.py, test_draw_ex.py, test_warp.py.)"""
import math
import os
import re

import pytest
import torch

from pips_amd import drivers
from test_clips_gpu import LENGTHS_C, P_SET, _expected_step as chain_step_reference, _nan_filled
from test_draw import SENTINEL, buffers, views
from test_draw_ex import WIDE, any_buffers
from test_stream_keep_gpu import V_, _expected_keep as keep_reference, _state as keep_state
from test_warp import coefficient_sets, make_surfaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pips_amd", "csrc")
I32 = torch.int32
QUIET_NAN = 0x7FC00000
NONE = 255


# ------------------------------------------------------------------------------------------------- the constants, as written
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(file, name):
    """the value of the one ``constexpr int NAME = <number>;`` of csrc/<file>"""
    found = re.findall(r"^\s*constexpr int %s = (\d+);" % name, _text(file), flags=re.M)
    assert len(found) == 1, (file, name, found)
    return int(found[0])


def grid_caps(file, what):
    """the caps of the ``min(<blocks>, cap)`` forms of csrc/<file>: what = "bx" for ``const int bx = min(..., cap);``, "blocks" for
    ``const int blocks = (int)(n < cap ? n : cap);`` (both sides must name the same number)"""
    if what == "bx":
        return [int(v) for v in re.findall(r"const int bx = min\(.*, (\d+)\);", _text(file))]
    pairs = re.findall(r"const int blocks = \(int\)\(\(total\d \+ 255\) / 256 < (\d+) \? \(total\d \+ 255\) / 256 : (\d+)\);", _text(file))
    assert all(a == b for a, b in pairs), (file, pairs)
    return [int(a) for a, _ in pairs]


TINT_ALPHAS = constant("common.h", "TINT_ALPHAS")
FRAMES_A_LAUNCH = {f: constant(f, "FRAMES_A_LAUNCH") for f in ("draw.hip", "masks.hip", "warp.hip")}
KEEP_ROWS_Y, KEEP_FEAT_Y = constant("stream.hip", "KEEP_ROWS_Y"), constant("stream.hip", "KEEP_FEAT_Y")
SEL_THREADS = constant("stream.hip", "SEL_THREADS")
COV_ROWS_MAX = constant("cover.hip", "COV_ROWS_MAX")
BX_CAPS = grid_caps("stream.hip", "bx")                              # pips_stream_emit's and pips_stream_keep's blocks along x
BLOCK_CAPS = {f: grid_caps(f, "blocks") for f in ("encoder.hip", "encoder_bf16.hip", "scoremap.hip")}
PIPS_C = 128                                                         # floats of a feature row (include/pips_hip.h)
GRID_Y_MAX = 65535                                                   # the y and z of a HIP grid


def test_the_constants_are_the_ones_the_cases_were_made_for():
    """a changed constant fails here: the cases below are sized to these values"""
    print(f"TINT_ALPHAS={TINT_ALPHAS} FRAMES_A_LAUNCH={FRAMES_A_LAUNCH} KEEP_ROWS_Y={KEEP_ROWS_Y} KEEP_FEAT_Y={KEEP_FEAT_Y} "
          f"SEL_THREADS={SEL_THREADS} COV_ROWS_MAX={COV_ROWS_MAX} bx caps={BX_CAPS} block caps={BLOCK_CAPS}")
    assert TINT_ALPHAS == 1024 and set(FRAMES_A_LAUNCH.values()) == {65535} and (KEEP_ROWS_Y, KEEP_FEAT_Y, SEL_THREADS) == (4096, 4, 256)
    assert COV_ROWS_MAX == GRID_Y_MAX and BX_CAPS == [64, 64]
    assert BLOCK_CAPS == {"encoder.hip": [4096, 4096, 4096], "encoder_bf16.hip": [4096], "scoremap.hip": [8192]}
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    assert re.search(r"#define\s+PIPS_C\s+%d\b" % PIPS_C, hdr) or re.search(r"PIPS_C\s*=\s*%d\b" % PIPS_C, _text("common.h"))
    assert re.search(r"#define\s+PIPS_STREAM_EMIT_FRAMES_MAX\s+%d\b" % GRID_Y_MAX, hdr)


def test_every_launch_site_is_in_the_table_of_seams():
    """the kernel of every hipLaunchKernelGGL of csrc is named in DESIGN.md's "Launch seams": a new launch gets its row"""
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    doc = doc[doc.index("## 8. Launch seams"):]
    sites = 0
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip") or name == "gemm_launch.h":
            for kernel in re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_0-9]+)", _text(name)):
                sites += 1
                assert kernel in ("kern", "Kern") or kernel in doc, (name, kernel)
    assert sites > 100 and "mixer_input_kernel" in doc and "launch_tiles" in doc          # (the two launched through a parameter)
    for test in re.findall(r"`(?:S|tests/test_[a-z0-9_]+\.py)::(test_[a-z0-9_]+)", doc):
        assert any(("def %s(" % test) in open(os.path.join(ROOT, "tests", f)).read() for f in os.listdir(os.path.join(ROOT, "tests"))
                   if f.endswith(".py")), test


def side(value, limit):
    """where ``value`` lies against ``limit``: the far side is "beyond" """
    return "beyond" if value > limit else "at" if value == limit else "below"


# ------------------------------------------------------------------------------------------------- tint across launches
TINT_SIZE = (17, 15)


def tint_seam_cases():
    """(fmt, C, F): every kernel layout once at C = 255, F = 5 (packed3 in RGB order, packed4 in BGR order), the rest on NV12 and
    planar8"""
    out = [(fmt, 255, 5) for fmt in ("rgb24", "bgra32", "i420")]
    for fmt in ("nv12", "planar8"):
        out += [(fmt, 255, 4), (fmt, 255, 5), (fmt, 255, 9), (fmt, 4, 257), (fmt, 1, 1025)]
    return out


def tint_seam_id(c):
    return f"{c[0]}-C{c[1]}-F{c[2]}"


def tint_seam_inputs(case):
    """-> (surface buffers, the mask's buffer, colors (F,C,3), alpha ints (F,C)) like test_masks.tint_inputs, for F frames: colours
    and opacities drawn independently per (frame, label), a quarter of the opacities 0, one 256; label f % C has a non-zero opacity
    on frame f and stands on its first pixel, so every frame is tinted"""
    fmt, C, F = case
    h, w = TINT_SIZE
    seed = 9000 + 7 * C + F + 31 * len(fmt)
    g = torch.Generator().manual_seed(seed)
    mbuf = torch.full((F, h + 3, w + 5), SENTINEL, dtype=torch.uint8)
    lab = torch.randint(0, min(C + 2, 256), (F, h, w), generator=g)
    lab[torch.rand(F, h, w, generator=g) < 0.1] = NONE
    own = torch.arange(F) % C
    lab[:, 0, 0] = own
    mbuf[:, :h, :w] = lab.to(torch.uint8)
    colors = torch.randint(0, 256, (F, C, 3), generator=g, dtype=torch.uint8)
    alpha = torch.randint(1, 256, (F, C), generator=g)
    alpha[torch.rand(F, C, generator=g) < 0.25] = 0
    alpha[torch.arange(F), own] = torch.randint(64, 256, (F,), generator=g)
    alpha[0, 0] = 256
    return buffers(fmt, F, h, w, seed + 1), mbuf, colors, alpha


def tint_reference(case):
    fmt, C, F = case
    h, w = TINT_SIZE
    bufs, mbuf, colors, alpha = tint_seam_inputs(case)
    want = drivers.tint_masks_torch(views(bufs, fmt, h, w), fmt, mbuf[:, :h, :w], colors, alpha / 256.0)
    return bufs, mbuf, colors, alpha, ([want] if torch.is_tensor(want) else list(want))


def test_tint_cases_cross_the_table_of_a_launch():
    """F against TINT_ALPHAS / C frames a launch: 4 of 4 at C = 255 exactly fills one launch, 5 and 9 take two and three, 257 at
    C = 4 and 1025 at C = 1 take two.  Every frame of the reference differs from its source, and two frames that stand at the same
    place of different launches carry different tables, so that a table slice or a colour row from the wrong launch changes bytes."""
    seen, layouts = set(), set()
    for case in tint_seam_cases():
        fmt, C, F = case
        per = TINT_ALPHAS // C
        where = side(F, per)
        print(f"{tint_seam_id(case)}: TINT_ALPHAS / C = {per} frames a launch, F = {F} lies {where} ({-(-F // per)} launches)")
        seen.add((C, where))
        layouts.add(fmt)
        if fmt in ("nv12", "rgb24") or F <= 9:                       # (the inputs do not depend on the layout but for the surfaces)
            bufs, mbuf, colors, alpha, want = tint_reference(case)
            before = views(bufs, fmt, *TINT_SIZE)
            for f in range(F):
                assert any(not torch.equal(a[f], b[f]) for a, b in zip(want, before)), (case, f)
                for g in range(f % per, f, per):
                    assert not torch.equal(alpha[f], alpha[g]) and not torch.equal(colors[f], colors[g]), (case, f, g)
    assert seen == {(255, "at"), (255, "beyond"), (4, "beyond"), (1, "beyond")}
    assert layouts == {"rgb24", "bgra32", "nv12", "i420", "planar8"}
    assert {(c[1], c[2]) for c in tint_seam_cases() if c[0] in ("nv12", "planar8")} == {(255, 4), (255, 5), (255, 9), (4, 257), (1, 1025)}


# ------------------------------------------------------------------------------------------------- 65535 frames a launch
PERIOD = 7                                                           # a prime that does not divide 65535 = 3 * 5 * 17 * 257
FRAME_COUNTS = (65535, 65537)
FRAME_SIZE = (3, 5)
DRAW_TRAIL = 2
DRAW_STYLE = dict(width=1.0, dot=1.0, alpha=0.9, alpha_occ=0.4, vis_thr=0.5)     # line8 = 4, dot8 = 8, alphas 230 and 102
DRAW_INTS = (4, 8, 230, 102)
DRAW_FADE = (1.0, 0.5)                                               # the factors by age; in the rule's integers:
DRAW_FADE_INTS = (256, 128)
MASK_RADIUS8 = 12
MASK_VOTES = (1, 3)


def periodic(t, F):
    """``t`` (PERIOD, ...) repeated to F entries: entry f is t[f % PERIOD]"""
    return t[torch.arange(F) % PERIOD]


def periodic_index(F, head=0):
    """entry f of a result whose first ``head`` entries stand alone and which repeats with PERIOD from there on, as an index into the
    ``head + PERIOD`` entries of the reference"""
    f = torch.arange(F)
    return torch.where(f < head, f, head + (f - head) % PERIOD)


def mask_seam_inputs():
    """one period: rows (PERIOD,3,2) float32 inside the 3 x 5 frame and labels (PERIOD,3) in 0..3 with one 255"""
    h, w = FRAME_SIZE
    g = torch.Generator().manual_seed(77)
    rows = torch.rand(PERIOD, 3, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    lab = torch.randint(0, 4, (PERIOD, 3), generator=g)
    lab[3, 1] = NONE
    return rows.float(), lab


def mask_reference(vote):
    rows, lab = mask_seam_inputs()
    return drivers.object_masks_torch(rows[None], lab, FRAME_SIZE, out_size=FRAME_SIZE, radius=MASK_RADIUS8 / 8.0, vote=vote)


def draw_seam_inputs(fmt):
    """one period: rows (PERIOD,2,2) inside the frame, logits (PERIOD,2) on both sides of 0, two colours, and PERIOD surfaces of
    ``fmt`` in test_draw's pitched buffers"""
    h, w = FRAME_SIZE
    g = torch.Generator().manual_seed(78)
    rows = torch.rand(PERIOD, 2, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    vis = torch.randn(PERIOD, 2, generator=g) * 2.0
    colors = torch.tensor([[250, 30, 60], [20, 200, 240]], dtype=torch.uint8)
    return rows.float(), vis.float(), colors, any_buffers(fmt, PERIOD, h, w, 79 + len(fmt))


def draw_frames(fmt, F):
    """the inputs of F frames: rows and logits repeat with PERIOD, frame f lies on a copy of surface f % PERIOD -> (buffers, trajs
    (1,F,2,2), vis (1,F,2), colors)"""
    rows, vis, colors, bufs = draw_seam_inputs(fmt)
    return [periodic(b, F) for b in bufs], periodic(rows, F)[None], periodic(vis, F)[None], colors


def _list(out):
    return [out] if torch.is_tensor(out) else list(out)


def draw_reference(fmt, faded):
    """the twin on the first DRAW_TRAIL + PERIOD frames -- the first DRAW_TRAIL, whose trails are cut at row 0, in a run of their
    own -- as planes of DRAW_TRAIL + PERIOD frames: frame f of any longer call is entry periodic_index(F, DRAW_TRAIL)[f]"""
    h, w = FRAME_SIZE
    n = DRAW_TRAIL + PERIOD
    bufs, trajs, vis, colors = draw_frames(fmt, n)
    kw = dict(colors=colors, trail=DRAW_TRAIL, fade=list(DRAW_FADE) if faded else None, **DRAW_STYLE)
    planes = views(bufs, fmt, h, w)
    head = _list(drivers.draw_tracks_torch([p[:DRAW_TRAIL] for p in planes], fmt, trajs[:, :DRAW_TRAIL], vis[:, :DRAW_TRAIL], first=0, **kw))
    rest = _list(drivers.draw_tracks_torch([p[DRAW_TRAIL:] for p in planes], fmt, trajs, vis, first=DRAW_TRAIL, **kw))
    return [torch.cat([a, b]) for a, b in zip(head, rest)], planes


def warp_seam_inputs(fmt):
    """one period: seven of test_warp's coefficient sets for a 3 x 5 image and PERIOD random source surfaces (views of guarded
    allocations)"""
    h, w = FRAME_SIZE
    sets = coefficient_sets(h, w)
    coef = torch.tensor([sets[k] for k in ("identity", "shift", "rot2", "quarter", "scale_quarter", "shear", "scale4")], dtype=torch.int64)
    assert coef.shape[0] == PERIOD
    return coef, make_surfaces(fmt, PERIOD, h, w, seed=80 + len(fmt), off=1, pad=3, gap=6)


WARP_BORDER = {"planar8": "constant", "nv12": "replicate", "p010": "constant"}
WARP_FILL = (200, 40, 90)


def warp_reference(fmt):
    coef, (_, planes) = warp_seam_inputs(fmt)
    return _list(drivers.warp_frames_torch(planes, fmt, coef, WARP_BORDER[fmt], fill=WARP_FILL))


def _pairwise_different(planes):
    n = planes[0].shape[0]
    return all(any(not torch.equal(p[a], p[b]) for p in planes) for a in range(n) for b in range(a))


def test_frame_counts_lie_at_and_beyond_every_frames_a_launch():
    for file, value in FRAMES_A_LAUNCH.items():
        for F in FRAME_COUNTS:
            print(f"{file}: FRAMES_A_LAUNCH = {value}, F = {F} lies {side(F, value)}; frame {value} shows entry {value % PERIOD} of the period")
        assert {side(F, value) for F in FRAME_COUNTS} == {"at", "beyond"}
        assert value % PERIOD != 0 and max(FRAME_COUNTS) - value >= 2            # a dropped f_base shows entry 0 in the place of another


def test_the_periodic_references_are_not_vacuous():
    """the PERIOD reference frames of every entry are pairwise different; no mask is all PIPS_MASK_NONE and vote 3 differs from vote
    1; every drawn frame changes at least one byte of every format; the fade changes the result"""
    m1, m3 = mask_reference(1), mask_reference(3)
    for m in (m1, m3):
        assert _pairwise_different([m]) and all(bool((m[f] != NONE).any()) for f in range(PERIOD))
        assert bool((m == NONE).any())
    assert not torch.equal(m1, m3)
    for fmt in ("planar8", "nv12", "p010"):
        for faded in (False, True):
            if fmt == "p010" and not faded:
                continue
            want, before = draw_reference(fmt, faded)
            assert _pairwise_different([p[DRAW_TRAIL:] for p in want]), (fmt, faded)
            for f in range(DRAW_TRAIL + PERIOD):
                assert any(not torch.equal(a[f], b[f]) for a, b in zip(want, before)), (fmt, faded, f)
        if fmt != "p010":
            assert any(not torch.equal(a, b) for a, b in zip(draw_reference(fmt, True)[0], draw_reference(fmt, False)[0]))
        assert _pairwise_different(warp_reference(fmt)), fmt
    assert drivers._draw_fade(list(DRAW_FADE), DRAW_TRAIL) == list(DRAW_FADE_INTS)
    assert DRAW_INTS == (math.floor(4 * DRAW_STYLE["width"] + 0.5), math.floor(8 * DRAW_STYLE["dot"] + 0.5), math.floor(256 * 0.9 + 0.5),
                         math.floor(256 * 0.4 + 0.5))


def test_the_periodic_expectation_is_the_twin_over_every_frame():
    """F = 2 * PERIOD + 3 frames, every one through the twin, against PERIOD (+ DRAW_TRAIL) reference frames picked by
    periodic_index: what the GPU test relies on at 65537 frames"""
    F = 2 * PERIOD + 3
    h, w = FRAME_SIZE
    rows, lab = mask_seam_inputs()
    for vote in MASK_VOTES:
        whole = drivers.object_masks_torch(periodic(rows, F)[None], periodic(lab, F), FRAME_SIZE, out_size=FRAME_SIZE, radius=MASK_RADIUS8 / 8.0,
                                           vote=vote)
        assert torch.equal(whole, mask_reference(vote)[periodic_index(F)])
    for fmt, faded in (("planar8", False), ("nv12", False), ("nv12", True), ("p010", True)):
        bufs, trajs, vis, colors = draw_frames(fmt, F)
        whole = _list(drivers.draw_tracks_torch(views(bufs, fmt, h, w), fmt, trajs, vis, colors=colors, trail=DRAW_TRAIL,
                                                fade=list(DRAW_FADE) if faded else None, **DRAW_STYLE))
        want, _ = draw_reference(fmt, faded)
        at = periodic_index(F, DRAW_TRAIL)
        assert all(torch.equal(a, b[at]) for a, b in zip(whole, want)), (fmt, faded)
        assert not all(torch.equal(a, b[periodic_index(F)]) for a, b in zip(whole, want))       # (the first frames do stand alone)
    for fmt in WARP_BORDER:
        coef, (_, planes) = warp_seam_inputs(fmt)
        whole = _list(drivers.warp_frames_torch([periodic(p, F) for p in planes], fmt, periodic(coef, F), WARP_BORDER[fmt], fill=WARP_FILL))
        assert all(torch.equal(a, b[periodic_index(F)]) for a, b in zip(whole, warp_reference(fmt))), fmt
    assert set(WARP_BORDER) & set(WIDE) == {"p010"}


# ------------------------------------------------------------------------------------------------- pips_stream_keep
KEEP_CASES = [(4096, 5, 3), (4097, 5, 3), (8193, 6, 4), (16, 16390, 16385), (16, 16390, 16384), (17, 33000, 32771)]      # (L, n, m)


def keep_list(n, m):
    """m ascending members with -1 in front and n at the end"""
    assert 3 <= m <= n
    g = torch.Generator().manual_seed(n + m)
    inner = torch.sort(torch.randperm(n, generator=g)[:m - 2]).values.tolist()
    return [-1] + inner + [n]


def test_keep_cases_cross_the_three_stride_paths():
    rows, cols, feat = set(), set(), set()
    for L, n, m in KEEP_CASES:
        bx = min(-(-m // SEL_THREADS), BX_CAPS[1])
        a, b = side(L, KEEP_ROWS_Y), side(m, BX_CAPS[1] * SEL_THREADS)
        c = side(m * (PIPS_C // 4), bx * SEL_THREADS * KEEP_FEAT_Y), side(m * PIPS_C, bx * SEL_THREADS * KEEP_FEAT_Y)
        print(f"L={L} n={n} m={m}: rows {a} KEEP_ROWS_Y={KEEP_ROWS_Y}; columns {b} {BX_CAPS[1]} x {SEL_THREADS}; feature pieces "
              f"(16-byte / words) {c[0]} / {c[1]} {bx} x {SEL_THREADS} x KEEP_FEAT_Y={KEEP_FEAT_Y}")
        rows.add(a), cols.add(b), feat.update(c)
        keep = keep_list(n, m)
        assert len(keep) == m and keep[0] == -1 and keep[-1] == n and keep == sorted(keep) and len(set(keep)) == m
    assert rows == {"below", "at", "beyond"} and cols == {"below", "at", "beyond"} and "beyond" in feat
    assert any(m % 2 for _, _, m in KEEP_CASES) and any(n % 2 == 0 and m % 4 == 0 for _, n, m in KEEP_CASES)


def test_keep_reference_is_the_rule_by_plain_loops():
    n, L, keep = 9, 16, [-1, 1, 4, 5, 8, 9]
    s = keep_state(n, L, 3)
    for clips in (False, True):
        out, counts = keep_reference(s, keep, n, clips)
        low, lows = 2 ** 31 - 1, [2 ** 31 - 1] * V_
        for j, c in enumerate(keep):
            ok = 0 <= c < n
            assert int(out["status"][j]) == (int(s["status"][c]) if ok else 2) and int(out["tq"][j]) == (int(s["tq"][c]) if ok else 0)
            assert int(out["cur"][j]) == (int(s["cur"][c]) if ok else 0) and int(out["clip"][j]) == (int(s["clip"][c]) if ok else 0)
            assert out["xy"][j].tolist() == (s["xy"][c].tolist() if ok else [0, 0])
            assert out["feat"][j].tolist() == (s["feat"][c].tolist() if ok else [0] * PIPS_C)
            for y in range(L):
                assert out["trajs"][y, j].tolist() == (s["trajs"][y, c].tolist() if ok else [QUIET_NAN] * 2)
                assert int(out["vis"][y, j]) == (int(s["vis"][y, c]) if ok else QUIET_NAN)
            if ok and int(s["status"][c]) != 2:
                low = min(low, int(s["cur"][c]))
                v = min(max(int(s["clip"][c]), 0), V_ - 1)
                lows[v] = min(lows[v], int(s["cur"][c]))
        assert counts == [0, 0, low, 0] + (lows if clips else [])


# ------------------------------------------------------------------------------------------------- pips_stream_emit / _emit_cols
EMIT_L = 17
EMIT_N = (300, 8193, 32772, 32768)
EMIT_COLS_N, EMIT_COLS_M = 700, (256, 257, 600)
JOIN_N_NEW = (256, 257)


def emit_frames(L):
    """test_stream_rounds_gpu's wrapping range: rows L-3, L-2, L-1, 0, 1, 2, 3"""
    f0 = 3 * L + L - 3
    return f0, f0 + 7


def emit_reference(trajs, vis, f0, f1):
    """pips_stream_emit by torch indexing on int32 bit patterns -> (out_trajs, out_vis, trajs after, vis after)"""
    rows = torch.arange(f0, f1) % trajs.shape[0]
    after_t, after_v = trajs.clone(), vis.clone()
    after_t[rows], after_v[rows] = QUIET_NAN, QUIET_NAN
    return trajs[rows], vis[rows], after_t, after_v


def emit_cols_list(n, m):
    """m ascending columns, -1 in front and n at the end"""
    g = torch.Generator().manual_seed(n + m)
    return [-1] + torch.sort(torch.randperm(n, generator=g)[:m - 2]).values.tolist() + [n]


def emit_cols_reference(trajs, vis, f0, f1, cols):
    n = trajs.shape[1]
    rows = torch.arange(f0, f1) % trajs.shape[0]
    c = torch.tensor(cols, dtype=torch.int64)
    ok = (c >= 0) & (c < n)
    safe = torch.where(ok, c, torch.zeros_like(c))
    out_t, out_v = trajs[rows][:, safe].clone(), vis[rows][:, safe].clone()
    out_t[:, ~ok], out_v[:, ~ok] = QUIET_NAN, QUIET_NAN
    after_t, after_v = trajs.clone(), vis.clone()
    at = torch.zeros(trajs.shape[0], n, dtype=torch.bool)
    at[rows.view(-1, 1), safe[ok].view(1, -1)] = True
    after_t[at], after_v[at] = QUIET_NAN, QUIET_NAN
    return out_t, out_v, after_t, after_v


def ring(L, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-2 ** 31, 2 ** 31, (L, n, 2), generator=g).to(I32), torch.randint(-2 ** 31, 2 ** 31, (L, n), generator=g).to(I32))


def test_emit_cases_cross_the_blocks_along_x():
    cap = BX_CAPS[0] * SEL_THREADS
    where = {}
    for n in EMIT_N:
        pieces = 2 * n // 4 if (2 * n) % 4 == 0 else 2 * n              # 16-byte pieces of a trajs row on aligned buffers, words otherwise
        where[n] = side(pieces, cap)
        print(f"emit n={n}: {pieces} {'16-byte pieces' if (2 * n) % 4 == 0 else 'words'} a row against {BX_CAPS[0]} x {SEL_THREADS} "
              f"threads: {where[n]}; {min(-(-pieces // SEL_THREADS), BX_CAPS[0])} blocks along x")
    assert where == {300: "below", 8193: "beyond", 32772: "beyond", 32768: "at"} and 2 * 300 // 4 <= SEL_THREADS < 2 * 300
    assert (2 * 8193) % 4 != 0 and (2 * 32772) % 4 == 0 and 2 * 8193 - cap == 2 and 32772 // 2 - cap == 2
    for m in EMIT_COLS_M:
        print(f"emit_cols m={m}: {-(-m // SEL_THREADS)} blocks of SEL_THREADS={SEL_THREADS} along x")
    assert [side(m, SEL_THREADS) for m in EMIT_COLS_M] == ["at", "beyond", "beyond"] and max(EMIT_COLS_M) > 2 * SEL_THREADS
    assert [side(k, SEL_THREADS) for k in JOIN_N_NEW] == ["at", "beyond"]
    f0, f1 = emit_frames(EMIT_L)
    assert (torch.arange(f0, f1) % EMIT_L).tolist() == [14, 15, 16, 0, 1, 2, 3]


def test_emit_references_are_the_rule_by_plain_loops():
    L, n = 16, 6
    trajs, vis = ring(L, n, 5)
    f0, f1 = 2 * L + L - 2, 2 * L + L + 3
    out_t, out_v, after_t, after_v = emit_reference(trajs, vis, f0, f1)
    cols = [4, -1, 0, n, 5]
    col_t, col_v, cafter_t, cafter_v = emit_cols_reference(trajs, vis, f0, f1, cols)
    want_t, want_v, cwant_t, cwant_v = trajs.clone(), vis.clone(), trajs.clone(), vis.clone()
    for i, f in enumerate(range(f0, f1)):
        r = f % L
        for c in range(n):
            assert out_t[i, c].tolist() == trajs[r, c].tolist() and int(out_v[i, c]) == int(vis[r, c])
            want_t[r, c], want_v[r, c] = QUIET_NAN, QUIET_NAN
        for j, c in enumerate(cols):
            if 0 <= c < n:
                assert col_t[i, j].tolist() == trajs[r, c].tolist() and int(col_v[i, j]) == int(vis[r, c])
                cwant_t[r, c], cwant_v[r, c] = QUIET_NAN, QUIET_NAN
            else:
                assert col_t[i, j].tolist() == [QUIET_NAN] * 2 and int(col_v[i, j]) == QUIET_NAN
    assert torch.equal(after_t, want_t) and torch.equal(after_v, want_v) and torch.equal(cafter_t, cwant_t) and torch.equal(cafter_v, cwant_v)
    assert int((cafter_t != trajs).sum()) == 2 * 3 * (f1 - f0)
    for m in EMIT_COLS_M:
        cols = emit_cols_list(EMIT_COLS_N, m)
        assert len(set(cols)) == m and cols == sorted(cols) and cols[0] == -1 and cols[-1] == EMIT_COLS_N


# ------------------------------------------------------------------------------------------------- single-block list kernels
LIST_COUNTS = (255, 256, 257, 513)
STEP_THREADS = constant("chain.hip", "STEP_THREADS")


def chain_seam_state(n_act):
    """test_clips_gpu's synthetic hop at n_act active particles of n = 2 n_act - 3 in three videos (T = 9, 21, 13; L = 35, base 7): the
    state that its _expected_step (the torch lines of a hop) reads; video indices outside the table among them"""
    g = torch.Generator().manual_seed(700 + n_act)
    n = 2 * n_act - 3
    active = torch.sort(torch.randperm(n, generator=g)[:n_act]).values.to(I32)
    clip = torch.randint(0, 3, (n,), generator=g).to(I32)
    clip[int(active[1])], clip[int(active[n_act - 2])] = -4, 9
    pick = torch.tensor(P_SET)[torch.randint(0, len(P_SET), (8, n_act), generator=g)]
    L = max(LENGTHS_C) + 14
    return dict(L=L, base=7, n=n, n_act=n_act, active=active, cur=torch.randint(0, 9, (n,), generator=g).to(I32),
                dirs=torch.where(torch.rand(n, generator=g) < 0.5, -1, 1).to(I32), clip=clip,
                win_vis=torch.log(pick.double() / (1.0 - pick.double())).float(), win_trajs=torch.randn(8, n_act, 2, generator=g) * 50,
                win_ffeat0=torch.randn(n_act, PIPS_C, generator=g), feat=torch.randn(n, PIPS_C, generator=g), trajs=_nan_filled(L, n, 2),
                vis=_nan_filled(L, n))


def test_list_counts_lie_around_the_chunk_of_the_one_block_walks():
    """chain_step_kernel walks n_act in chunks of STEP_THREADS with the carried offset of next_active and, under sample_feat, the
    chunk's own window of win_ffeat0; the other one-block list kernels (stream_select, stream_keep_state, cover_list) are crossed by
    tests that DESIGN.md's table names.  The reference of the hop, _expected_step, against plain loops at five particles"""
    assert STEP_THREADS == SEL_THREADS == constant("cover.hip", "COV_THREADS") == 256
    for k in LIST_COUNTS:
        print(f"chain_step n_act={k}: {-(-k // STEP_THREADS)} chunks of STEP_THREADS={STEP_THREADS}; {side(k, STEP_THREADS)}")
        s = chain_seam_state(k)
        nxt = chain_step_reference(s, True, True)["next_active"].tolist()
        assert 0.2 * k < len(nxt) < 0.9 * k and all(any(a <= j < a + 256 for j in range(k) if int(s["active"][j]) in nxt)
                                                     for a in range(0, k, 256) if k - a > 8)
    assert [side(k, STEP_THREADS) for k in LIST_COUNTS] == ["below", "at", "beyond", "beyond"] and LIST_COUNTS[-1] > 2 * STEP_THREADS
    s = chain_seam_state(5)
    exp = chain_step_reference(s, True, True)
    si = drivers.skip_scan(torch.sigmoid(s["win_vis"])).tolist()
    trajs, vis, feat, cur, nxt = s["trajs"].clone(), s["vis"].clone(), s["feat"].clone(), s["cur"].clone(), []
    for j, q in enumerate(s["active"].tolist()):
        d = -1 if int(s["dirs"][q]) < 0 else 1
        for k in range(8):
            r = (int(s["cur"][q]) + d * k + s["base"]) % s["L"]
            trajs[r, q], vis[r, q] = s["win_trajs"][k, j], s["win_vis"][k, j]
        cur[q] = int(s["cur"][q]) + d * si[j]
        feat[q] = s["win_ffeat0"][j]
        if 0 <= int(cur[q]) < LENGTHS_C[min(max(int(s["clip"][q]), 0), 2)]:
            nxt.append(q)
    same = lambda a, b: torch.equal(a.view(I32), b.view(I32))
    assert same(exp["trajs"], trajs) and same(exp["vis"], vis) and same(exp["feat"], feat) and torch.equal(exp["cur"], cur)
    assert exp["next_active"].tolist() == nxt and exp["steps"].tolist() == si


# ------------------------------------------------------------------------------------------------- capped element-wise grids
RESIZE_BF16_STRIDE = (24, (23, 31), (46, 62), 128, 160)              # frames, source and target size, channels, first channel


def test_the_bf16_resize_case_crosses_its_cap():
    """resize_into_bf16_kernel moves 8 channels a thread: test_encoder_stages_gpu's grid-stride case (12 frames) passes the fp32
    kernel's 4096 x 256 float4 and stays below the bf16 kernel's 4096 x 256 groups of eight; 24 frames pass it"""
    Fr, _, (hd, wd), Cc, _ = RESIZE_BF16_STRIDE
    cap = BLOCK_CAPS["encoder_bf16.hip"][0] * 256
    print(f"resize_into bf16: {Fr * hd * wd * Cc // 8} groups of 8 channels against {cap}: {side(Fr * hd * wd * Cc // 8, cap)}")
    assert 12 * hd * wd * Cc // 8 < cap < Fr * hd * wd * Cc // 8 and 12 * hd * wd * Cc // 4 > BLOCK_CAPS["encoder.hip"][1] * 256


# ------------------------------------------------------------------------------------------------- grid y from a caller's count
EMIT_GOOD = dict(trajs=0x1000, vis=0x2000, L=70000, n=3, f0=5, f1=5 + GRID_Y_MAX, out_trajs=0x3000, out_vis=0x4000, stream=None)
EMIT_COLS_GOOD = dict(trajs=0x1000, vis=0x2000, L=70000, n=3, f0=5, f1=5 + GRID_Y_MAX, cols=0x5000, m=2, out_trajs=0x3000, out_vis=0x4000,
                      stream=None)


def test_emit_rejects_more_frames_than_a_grid_has_rows_ahead_of_any_launch():
    """pips_stream_emit and pips_stream_emit_cols put a frame on each row of blocks: more than PIPS_STREAM_EMIT_FRAMES_MAX = 65535
    frames in one call (a ring that long is legal) is PIPS_E_ARG with a message.  The pointers are never followed -- nothing is
    launched -- so this runs without a device; the largest legal count is only shown to pass the check on an empty call"""
    from pips_amd import _lib
    lib = _lib.load()
    for name, good in (("pips_stream_emit", EMIT_GOOD), ("pips_stream_emit_cols", EMIT_COLS_GOOD)):
        call = lambda **change: getattr(lib, name)(*[dict(good, **change)[k] for k in good])
        for change in (dict(f1=good["f0"] + GRID_Y_MAX + 1), dict(f1=good["f0"] + 70000), dict(L=2 ** 31 - 1, f0=0, f1=2 ** 31 - 1)):
            assert call(**change) == -1, (name, change)
            msg = lib.pips_last_error().decode()
            assert msg.startswith(name[5:] + ":") and str(GRID_Y_MAX) in msg, msg
        assert call(f1=good["f0"]) == 0                                # no frame: PIPS_OK, nothing launched
    assert lib.pips_stream_emit_cols(*[dict(EMIT_COLS_GOOD, m=0)[k] for k in EMIT_COLS_GOOD]) == 0          # 65535 frames of no column
