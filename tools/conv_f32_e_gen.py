#!/usr/bin/env python
"""Emit pips_amd/csrc/conv_f32_e_asm.inc: the bodies of conv_f32_e_kernel (conv_f32_e.hip), each ONE assembly statement -- the
encoder's exact-fp32 convolutions that the 128-pixel pipeline of tools/gen_conv_f32_t4.py does not cover (1x1 and 3x3, stride 1 or
2, 64 / 96 / 128 / 256 input channels) on shape E of tools/gen_gemm_f32_t4.py with the addressing of an implicit GEMM.

Taken over unchanged from shape E: the 64 x 64 tile, every wave the whole tile on ONE quarter of each 32-wide K stage, operands
staged by LDS-DMA with per-lane global offsets (wave w fills LDS rows 32 w .. 32 w + 31: waves 0, 1 the tile's pixels, waves 2, 3
its output channels; four DMA instructions of 8 rows per stage), four buffers of 128 dense 128-byte rows, chunk slot j of row r
holding global chunk j ^ ((r >> 1) & 7), a stage requested three stages ahead and waited for by its own wave before the barrier at
the end of the stage two before its use, the four partial tiles summed through LDS in the order ((0 + 1) + 2) + 3, every wave
finishing ONE 32 x 32 block.

What is the convolution's: rows are output pixels of one frame, K runs tap-major, then input channels in stages of 32 (a stage
never crosses a tap).  A DMA instruction's address is  per-lane row base (one VGPR per instruction: pixel (ho s - pad, wo s - pad)
of the input map, or the weight row) + TAP[tap] + 128 (channel block), formed in a vector register: the frame's buffer descriptor
range-checks it, which supplies the zero rows above and below the image; for the kw = 0 / 2 taps of a 3x3 kernel the lanes whose
input column falls outside the image are sent out of range through a lane mask computed once in the prologue.  The weight waves
run the same instructions on their own TAP table (tap * Cin * 4) and empty masks.  The stage count is small (2 .. 36), so the K
loop is unrolled whole: every displacement is static and the loop carries one v_add_u32 (and one v_cndmask_b32 on a border tap)
per DMA instruction, nothing else on the vector ALU.

Accumulators are C (the pixel fragment is the MFMA's row operand), as in tools/gen_conv_f32_t4.py: a lane holds channel l & 31 of
a 32-channel block and 16 pixels (rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)) -- per-channel sums stay in the lane.  Epilogue of the
wave that finishes a block: + bias, 4-byte stores (rows behind the frame's last pixel are dropped by the output descriptor),
InstanceNorm partials {sum(x - p), sum((x - p)^2), p, n} about the block's first pixel: one float4 per (32-pixel block, channel),
the partition of igemm_f32_kernel's 64-row tiles.

Registers (all clobbered; v[216:255] stay with the compiler):
    a[0:63]      accumulators: MFMA block (i, j) = pixels 32 i.., channels 32 j.. -> a[16 (i + 2 j) : +15]
    v[0:31]      two fragment sets: A0 A1 W0 W1 (4 registers each)
    v[36:39]     the addresses of the four DMA instructions of a stage;  v40 the out-of-range offset;  v[41:43] bias
    v[44:46]     temporaries;  v[48:79] the four partials of two quads;  v[80:95] the block's values;  v[96:111] their offsets
    v[112:115]   {s1, s2, p, n}
    s[40:55] buffer descriptors X (this wave's operand), C, bias, statistics;  s[56:64] TAP;  s[65:67] temporaries;
    s[68:83] lane masks: instruction k, left column at 68 + 4 k, right column at 70 + 4 k
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asm_guards as G  # noqa: E402  (wait-state guards: the numbers live in tools/asm_hazard_lint.py)
from asm_emit import Emit, descriptor, out_path, write_inc  # noqa: E402  (the issue model, shared by every generator)
from gen_gemm_f32_t4 import EBUF, FA, FRAG_ORDER, FW  # noqa: E402  (shape E's LDS image and fragment sets)

OUT = out_path("conv_f32_e_asm.inc")
NV = 216
RS_X, RS_C, RS_B, RS_S = 40, 44, 48, 52
S_TAP = 56
S_T, S_T2, S_T3 = 65, 66, 67
S_MASK = 68
V_OFF, V_OOB, V_BIAS, V_T, V_D = 36, 40, 41, 44, 45
V_P, V_O, V_OFFC, V_S = 48, 80, 96, 112
BLOCKS = [(i, j) for j in range(2) for i in range(2)]
# (input channels, kernel size) of the bodies: the 128-channel layers of the encoder, their stride-2 entries and 1x1 shortcuts
CONFIGS = [(64, 3), (96, 3), (128, 3), (64, 1), (96, 1), (128, 1), (256, 1)]


def acc(i, j):
    return 16 * (i + 2 * j)


def mfma(e, fset, c, i, j, zero):
    e.need_lds({("fw", fset, j), ("fa", fset, i)})
    a = acc(i, j)
    e.raw("v_mfma_f32_32x32x2_f32 a[%d:%d], v%d, v%d, %s" %
          (a, a + 15, FA[fset] + 4 * i + c, FW[fset] + 4 * j + c, "0" if zero else "a[%d:%d]" % (a, a + 15)))


def fread(e, buf, fset, which, idx):
    reg = (FA if which == "a" else FW)[fset] + 4 * idx
    e.lds("ds_read_b128 v[%d:%d], %%[r%s0] offset:%d" % (reg, reg + 3, "A" if which == "a" else "W", buf * EBUF + idx * 32 * 128),
          ("f" + which, fset, idx))


def stage_offset(e, cin, t):
    """scalar register holding TAP[tap] + 128 (channel block) of stage t"""
    tap, cb = divmod(t, cin // 32)
    if cb == 0:
        return S_TAP + tap
    e.raw("s_add_u32 s%d, s%d, %d" % (S_T, S_TAP + tap, 128 * cb))
    return S_T


def dma(e, cin, ks, t, k, sreg):
    """DMA instruction k (8 rows) of stage t -> buffer t % 4"""
    kw = (t // (cin // 32)) % ks
    e.raw("s_add_u32 m0, %%[ldsw], %d" % ((t % 4) * EBUF + 8 * k * 128))
    e.raw("v_add_u32 v%d, s%d, %%[vo%d]" % (V_OFF + k, sreg, k))
    if ks == 3 and kw != 1:
        m = S_MASK + 4 * k + (0 if kw == 0 else 2)
        e.raw("v_cndmask_b32_e64 v%d, v%d, v%d, s[%d:%d]" % (V_OFF + k, V_OFF + k, V_OOB, m, m + 1))
    G.emit_m0_guard(e.raw, already=1)                         # SALU writes M0 -> the LDS-DMA load reads it; the v_add_u32 sits in between
    e.vmem("buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (V_OFF + k, RS_X, RS_X + 3), ("st", t, k))


def stage(e, cin, ks, kt, t):
    """Stage t: 16 MFMAs on buffer t % 4; the fragments of stage t + 1 are read at once, stage t + 3 is requested, stage t + 2 is
    waited for (by its own wave) in front of the barrier at the stage's end"""
    sreg = stage_offset(e, cin, t + 3) if t + 3 < kt else None
    slots = {}

    def put(n, fn):
        slots.setdefault(n, []).append(fn)

    if t + 1 < kt:
        for r, (which, idx) in enumerate(FRAG_ORDER):
            put(1 + r, lambda which=which, idx=idx: fread(e, (t + 1) % 4, (t + 1) & 1, which, idx))
    if t + 3 < kt:
        for k in range(4):
            put(5 + 2 * k, lambda k=k: dma(e, cin, ks, t + 3, k, sreg))
    if t + 2 < kt:
        put(15, lambda: (e.need_vm({("st", t + 2, k) for k in range(4)}), e.barrier()))
    n = 0
    for c in range(4):
        for (i, j) in BLOCKS:
            mfma(e, t & 1, c, i, j, t == 0 and c == 0)
            for fn in slots.get(n, []):
                fn()
            n += 1


def epilogue(e):
    """the four partial tiles -> LDS -> every wave sums ONE 32 x 32 block in the order ((0 + 1) + 2) + 3, + bias, stores, partials"""
    e.need_loads()
    e.barrier()                                              # every wave is done with the stage buffers
    G.emit_mfma_result_guard(e.raw, "v_mfma_f32_32x32x2_f32")
    for b in range(4):
        for q in range(4):
            a = 16 * b + 4 * q
            e.lds("ds_write_b128 %%[redW], a[%d:%d] offset:%d" % (a, a + 3, (4 * b + q) * 1024), ("rw", b, q))
    e.barrier()
    e.raw("v_mov_b32 v%d, v%d" % (V_BIAS + 1, V_BIAS))
    e.raw("v_mov_b32 v%d, v%d" % (V_BIAS + 2, V_BIAS))
    for half in range(2):
        for ksp in range(4):
            for q2 in range(2):
                r = V_P + 4 * (2 * ksp + q2)
                e.lds("ds_read_b128 v[%d:%d], %%[redR] offset:%d" % (r, r + 3, ksp * 16384 + (2 * half + q2) * 1024), ("rr", ksp, q2))
        for q2 in range(2):
            X, O = V_P + 4 * q2, V_O + 4 * (2 * half + q2)
            for ksp in range(1, 4):
                e.need_lds({("rr", 0, q2), ("rr", ksp, q2)})
                r = V_P + 4 * (2 * ksp + q2)
                for p in range(2):
                    e.raw("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (X + 2 * p, X + 2 * p + 1, X + 2 * p, X + 2 * p + 1, r + 2 * p, r + 2 * p + 1))
            for p in range(2):
                e.raw("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (O + 2 * p, O + 2 * p + 1, X + 2 * p, X + 2 * p + 1, V_BIAS + 1, V_BIAS + 2))
    # the pivot: the block's first pixel (row 0: lane half 0, register 0) per channel, to both lane halves
    S = V_S
    e.lds("ds_bpermute_b32 v%d, %%[vl31x4], v%d" % (S + 2, V_O), ("piv",))
    e.raw("v_mov_b32 v%d, 0" % S)
    e.raw("v_mov_b32 v%d, 0" % (S + 1))
    e.need_lds({("piv",)})
    for r in range(16):
        rho = (r & 3) + 8 * (r >> 2)
        e.raw("s_sub_i32 s%d, %%[nv], %d" % (S_T2, rho))
        e.raw("s_mul_i32 s%d, %%[ldcb], %d" % (S_T3, rho))
        e.raw("v_cmp_gt_i32 vcc, s%d, %%[vrow]" % S_T2)                   # this row lies inside the frame
        e.raw("v_add_u32 v%d, s%d, %%[voC]" % (V_OFFC + r, S_T3))         # (vector offset: range-checked -- the ragged last tile)
        e.raw("v_sub_f32 v%d, v%d, v%d" % (V_D, V_O + r, S + 2))
        G.emit_sgpr_to_valu_guard(e.raw, already=2)                      # VCC written by a VALU compare -> v_cndmask reads it
        e.raw("v_cndmask_b32 v%d, 0, v%d, vcc" % (V_D, V_D))
        e.raw("v_add_f32 v%d, v%d, v%d" % (S, S, V_D))
        e.raw("v_fmac_f32 v%d, v%d, v%d" % (S + 1, V_D, V_D))
        e.vmem("buffer_store_dword v%d, v%d, s[%d:%d], 0 offen" % (V_O + r, V_OFFC + r, RS_C, RS_C + 3), ("out", r))
    # the lane halves' sums meet (ds_bpermute with lane ^ 32), the lower half stores {s1, s2, p, n}
    e.lds("ds_bpermute_b32 v%d, %%[vswap], v%d" % (V_D, S), ("sw", 0))
    e.lds("ds_bpermute_b32 v%d, %%[vswap], v%d" % (V_D + 1, S + 1), ("sw", 1))
    e.raw("v_mov_b32 v%d, %%[nvf]" % (S + 3))
    e.need_lds({("sw", 0), ("sw", 1)})
    e.raw("v_add_f32 v%d, v%d, v%d" % (S, S, V_D))
    e.raw("v_add_f32 v%d, v%d, v%d" % (S + 1, S + 1, V_D + 1))
    e.vmem("buffer_store_dwordx4 v[%d:%d], %%[voS], s[%d:%d], 0 offen" % (S, S + 3, RS_S, RS_S + 3), ("out", "s"))


def body(cin, ks):
    kt = ks * ks * cin // 32
    e = Emit()
    descriptor(e, RS_X, "%[xlo]", "%[xhi]", "%[nrecX]")      # this wave's operand (the frame's map for waves 0, 1; W for waves 2, 3)
    descriptor(e, RS_C, "%[clo]", "%[chi]", "%[nrecC]")
    descriptor(e, RS_B, "%[blo]", "%[bhi]", "%[nrecB]")
    descriptor(e, RS_S, "%[slo]", "%[shi]", "%[nrecS]")
    e.raw("v_mov_b32 v%d, 0x80000000" % V_OOB)
    for kh in range(ks):                                     # TAP[kh ks + kw] = kh tapH + kw tapW (wrapping unsigned numbers)
        for kw in range(ks):
            t = ks * kh + kw
            if t == 0:
                e.raw("s_mov_b32 s%d, 0" % S_TAP)
            elif kw == 0:
                e.raw("s_add_u32 s%d, s%d, %%[tapH]" % (S_TAP + t, S_TAP + t - ks))
            else:
                e.raw("s_add_u32 s%d, s%d, %%[tapW]" % (S_TAP + t, S_TAP + t - 1))
    if ks == 3:                                              # lane masks of the border columns: bits 2 k (left), 2 k + 1 (right) of vflag
        for k in range(4):
            for side in range(2):
                m = S_MASK + 4 * k + 2 * side
                e.raw("v_and_b32 v%d, %d, %%[vflag]" % (V_T, 1 << (2 * k + side)))
                e.raw("v_cmp_ne_u32_e64 s[%d:%d], 0, v%d" % (m, m + 1, V_T))
    e.vmem("buffer_load_dword v%d, %%[voB], s[%d:%d], 0 offen" % (V_BIAS, RS_B, RS_B + 3), ("bias",))
    for t in range(min(3, kt)):                              # stages 0, 1, 2 requested
        sreg = stage_offset(e, cin, t)
        for k in range(4):
            dma(e, cin, ks, t, k, sreg)
    e.need_vm({("st", min(1, kt - 1), k) for k in range(4)})  # stages 0 and 1 of this wave have landed
    e.barrier()
    for which, idx in FRAG_ORDER:
        fread(e, 0, 0, which, idx)
    for t in range(kt):
        stage(e, cin, ks, kt, t)
    epilogue(e)
    e.drain()
    return e.lines


def main():
    bodies = [("PIPS_CF32E_C%d_K%d_TEXT" % (cin, ks), body(cin, ks)) for cin, ks in CONFIGS]
    write_inc(OUT, "conv_f32_e_gen.py", bodies, "PIPS_CF32E_CLOBBER", 64, NV, range(40, 84),
              notes=[", %d stages" % (ks * ks * cin // 32) for cin, ks in CONFIGS])


if __name__ == "__main__":
    main()
