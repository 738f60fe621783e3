"""GPU: the mixer's and the update's stage kernels, each alone through its own entry point (pips_token_mix, pips_ln_mean,
pips_state_update_s, pips_vis_head) against the operation in fp64, with the per-element bounds of
tests/golden/mixer_stages.py (proven on the CPU by tests/test_mixer_stages.py).  Token rows differ in kind, so a statistic
handed to the wrong token misses a bound by four orders of magnitude; every case runs on trained-like weights (an identity
affine pair hides a dropped or swapped scale / shift) and the layer index moves over 0, 5, 11 (an off-by-one in mix[d]).
The kernels are reached otherwise only through twelve layers and 26 GEMMs, gated at 1e-4 (fp32) and 3e-2 (bf16) of the output.
"""
import pytest
import torch

import cases as G
import mixer_stages as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16_P = (1, 3, 4, 9)          # four particles per block: a partly filled block, a full one, one wave into a third
_cache = {}


def _tl(S=8):
    """S -> (trained-like state dict, its packed arena); built once per window length"""
    if S not in _cache:
        from pips_amd import ops
        sd = G.trained_like_state_dict(0, S=S)
        _cache[S] = (sd, ops.pack_weights(sd, torch.device(DEV), S=S))
    return _cache[S]


def _family_rows(P, S, fam, r):
    return M.token_rows(P, S, "shifted" if fam == "shifted" else fam, r)


def _name(fam, r):
    return f"shifted({r:g})" if fam == "shifted" else fam


FAMILIES = (("centred", 0.0), ("hot", 0.0)) + tuple(("shifted", r) for r in M.SHIFTS[1:] + (M.SHIFT_PROBE,))


def _excess(got, ref):
    """what of |got - ref| a bf16 rounding of the exact value cannot explain, as a fraction of the half-ulp of the row's largest
    value: a lower bound of the pre-rounding error (and, over thousands of elements near a tie, close to it)"""
    e = ((got.double() - ref).abs() - M.bf16_half_ulp(ref)).clamp_min(0)
    return float((e / M.row_half_ulp(ref)).max())


# ------------------------------------------------------------------ token mixing, S = 8
@pytest.mark.parametrize("P", [1, 5])
def test_token_mix_fp32(P):
    """token_mix_kernel<false>, one block per particle.  x' and LayerNorm 2 (of the stored x') against their bounds.
    Measured worst error / bound (x', xn) at P = 1 / P = 5: centred 0.01, 0.12 / 0.01, 0.11; hot 0.01, 0.11 / 0.01, 0.12;
    shifted(1.43) 0.01, 0.10 / 0.01, 0.10; shifted(5.72) 0.01, 0.09 / 0.01, 0.08; shifted(64) 0.02, 0.09 / 0.01, 0.05."""
    from pips_amd import ops
    sd, arena = _tl()
    for i, (fam, r) in enumerate(FAMILIES):
        layer = M.LAYERS[(i + P) % 3]
        w = M.mix_weights(sd, layer)
        x0 = _family_rows(P, 8, fam, r)
        y, by = M.token_mix_ref(x0, w)
        x = x0.to(DEV)
        xn = ops.token_mix(arena, layer, x).cpu()
        x = x.cpu()
        ref, gate = M.ln_ref(x, w["g2"], w["b2"])
        ry, rn = M.worst((x.double() - y).abs(), by), M.worst((xn.double() - ref).abs(), gate)
        print(f"token_mix fp32 P={P} layer {layer} {_name(fam, r)}: x' {ry:.2f} of its bound, xn {rn:.2f}")
        assert ry <= 1.0 and rn <= 1.0


@pytest.mark.parametrize("P", BF16_P)
def test_token_mix_bf16_operands(P):
    """token_mix_mfma_kernel<false>: bf16 operands on the matrix cores, fp32 stream, bf16 LayerNorm-2 output.  x' against the
    bound of the bf16 contract (token_mix_ref: the allowance of gelu_bf16out2 through sum |w3|, one bf16 ulp for each operand
    within its own gate of a rounding tie); xn against half a bf16 ulp + the yardstick gate of LayerNorm 2 on the stored x'.
    At shifted(64) both pre-rounding gates are the bf16 half-ulp of the row's largest value: no worse than one more rounding.
    Measured, x' / bound, xn / bound, and the part of xn's error that no rounding of the exact value explains as a fraction
    of that half-ulp (a lower bound of the one-pass statistics' pre-rounding error; the yardstick gate in the same unit):
      P = 9: centred 0.97, 0.999, 0 (7.7e-4); hot 0.94, 0.997, 0 (8.8e-4); shifted(1.43) 0.97, 0.998, 6.6e-7 (1.4e-3);
             shifted(5.72) 0.96, 0.999, 1.5e-4 (2.8e-3); shifted(64) 0.05, 0.579, 0.16 (1.6e-2)
      P = 1 / 3 / 4: x' 0.92-0.97 (0.05-0.06 at 64), xn 0.993-0.999 (0.475-0.539 at 64), excess <= 2.7e-6 at 1.43,
             8.1e-5 .. 1.2e-4 at 5.72, 0.027 / 0.078 / 0.078 at 64.
    x' sits near 1 wherever a hidden unit did land on the other side of a tie: the allowance is the size of that step.  At 64
    stds the one-pass statistics are ten times the yardstick gate and a sixth of the half-ulp; the kernel is left as it is."""
    from pips_amd import ops
    sd, arena = _tl()
    for i, (fam, r) in enumerate(FAMILIES):
        layer = M.LAYERS[(i + P) % 3]
        w = M.mix_weights(sd, layer)
        x0 = _family_rows(P, 8, fam, r)
        probe = fam == "shifted" and r == M.SHIFT_PROBE
        n1, _ = M.ln_ref(x0, w["g1"], w["b1"])
        y, by = M.token_mix_ref(x0, w, bf16=True, dn=M.row_half_ulp(n1) if probe else None)
        x = x0.to(DEV)
        xn = ops.token_mix(arena, layer, x, bf16=True).cpu()
        x = x.cpu()
        assert xn.dtype == torch.bfloat16
        ref, gate = M.ln_ref(x, w["g2"], w["b2"])
        pre = M.row_half_ulp(ref) if probe else gate
        ry = M.worst((x.double() - y).abs(), by)
        rn = M.worst((xn.double() - ref).abs(), M.stored_bf16_bound(ref, pre))
        print(f"token_mix bf16 operands P={P} layer {layer} {_name(fam, r)}: x' {ry:.2f} of its bound, xn {rn:.3f}, pre-rounding "
              f"excess of xn {_excess(xn, ref):.1e} of a bf16 half-ulp (yardstick gate {float((gate / M.row_half_ulp(ref)).max()):.1e})")
        assert ry <= 1.0 and rn <= 1.0


@pytest.mark.parametrize("P", BF16_P)
def test_token_mix_bf16_stream(P):
    """token_mix_mfma_kernel<true>: the stream is bf16 in memory.  x' as bf16 against the reference rounded once; LayerNorm 2
    on the stored (rounded) stream, which is what the kernel normalises.
    Measured (x', xn) / bound: 0.992-0.997, 0.999 on both families at every P; excess of xn <= 8.3e-7 of a bf16 half-ulp."""
    from pips_amd import ops
    sd, arena = _tl()
    for i, (fam, r) in enumerate((("centred", 0.0), ("shifted", M.R))):
        layer = M.LAYERS[(i + P) % 3]
        w = M.mix_weights(sd, layer)
        x0 = _family_rows(P, 8, fam, r).bfloat16()
        y, by = M.token_mix_ref(x0.float(), w, bf16=True)
        x = x0.to(DEV)
        xn = ops.token_mix(arena, layer, x, bf16=True, stream_bf16=True).cpu()
        x = x.cpu()
        assert x.dtype == torch.bfloat16 and xn.dtype == torch.bfloat16
        ref, gate = M.ln_ref(x.float(), w["g2"], w["b2"])
        ry = M.worst((x.double() - y).abs(), M.stored_bf16_bound(y, by))
        rn = M.worst((xn.double() - ref).abs(), M.stored_bf16_bound(ref, gate))
        print(f"token_mix bf16 stream P={P} layer {layer} {_name(fam, r)}: x' {ry:.3f} of its bound, xn {rn:.3f}, pre-rounding excess "
              f"of xn {_excess(xn, ref):.1e} of a bf16 half-ulp")
        assert ry <= 1.0 and rn <= 1.0


# ------------------------------------------------------------------ token mixing, any window
@pytest.mark.parametrize("S,P", M.WINDOWS)
def test_token_mix_any_window(S, P):
    """token_mix_any_kernel<16 | 32, false | true>: fp32 arithmetic on S tokens, xn fp32 or bf16.
    Measured: x' 0.00-0.03 of the bound, xn 0.09-0.13 (fp32) and 0.994-1.000 (bf16: the store's half ulp) over the six windows."""
    from pips_amd import ops
    sd, arena = _tl(S)
    for i, (fam, r) in enumerate((("centred", 0.0), ("shifted", M.R))):
        layer = M.LAYERS[(i + S) % 3]
        w = M.mix_weights(sd, layer)
        x0 = _family_rows(P, S, fam, r)
        y, by = M.token_mix_ref(x0, w)
        for bf16 in (False, True):
            x = x0.to(DEV)
            xn = ops.token_mix(arena, layer, x, bf16=bf16).cpu()
            x = x.cpu()
            ref, gate = M.ln_ref(x, w["g2"], w["b2"])
            ry = M.worst((x.double() - y).abs(), by)
            rn = M.worst((xn.double() - ref).abs(), M.stored_bf16_bound(ref, gate) if bf16 else gate)
            print(f"token_mix S={S} P={P} layer {layer} {_name(fam, r)} xn {'bf16' if bf16 else 'fp32'}: x' {ry:.2f}, xn {rn:.3f} of the bound")
            assert xn.dtype == (torch.bfloat16 if bf16 else torch.float32)
            assert ry <= 1.0 and rn <= 1.0


# ------------------------------------------------------------------ final LayerNorm + mean
def _ln_mean_case(S, P, stream_bf16):
    from pips_amd import ops
    sd, arena = _tl(S)
    g, b = M.final_ln(sd)
    out = []
    for fam, r in (("centred", 0.0), ("shifted", M.R), ("shifted", 4 * M.R), ("hot", 0.0)):
        x = _family_rows(P, S, fam, r)
        if stream_bf16:
            x = x.bfloat16()
        ref, gate = M.ln_mean_ref(x.float(), g, b)
        got = ops.ln_mean(arena, x.to(DEV), bf16=stream_bf16, stream_bf16=stream_bf16).cpu()
        out.append(M.worst((got.double() - ref).abs(), gate))
        print(f"ln_mean S={S} P={P} {'bf16' if stream_bf16 else 'fp32'} stream {_name(fam, r)}: {out[-1]:.2f} of the gate")
    assert max(out) <= 1.0


@pytest.mark.parametrize("P", [1, 5])
def test_ln_mean_fp32(P):
    """ln_mean_kernel<false>: the mean over tokens of each token's own LayerNorm.  Measured 0.02-0.15 of the gate (hot rows highest)."""
    _ln_mean_case(8, P, False)


@pytest.mark.parametrize("P", BF16_P)
def test_ln_mean_wave(P):
    """ln_mean_wave_kernel on a bf16 stream, four particles per block.  Measured 0.02-0.13 of the gate."""
    _ln_mean_case(8, P, True)


@pytest.mark.parametrize("S,P", M.WINDOWS)
def test_ln_mean_any_window(S, P):
    """ln_mean_any_kernel<16 | 32>.  Measured 0.02-0.17 of the gate over the six windows."""
    _ln_mean_case(S, P, False)


# ------------------------------------------------------------------ state update
@pytest.mark.parametrize("B,N", [(2, 3), (1, 1)])
@pytest.mark.parametrize("S", [1, 5, 8, 12, 24, 32])
def test_state_update_s(S, B, N):
    """state_update_kernel (S = 8) / state_update_any_kernel: groups of 8 rows with a partly live last group, delta rows
    pips_delta_stride(S) apart, with and without the visibility head.
    Measured over the twelve cases: features 0.009-0.018 of the bound, coordinates 0.37-0.49 (one rounding of two allowed; 0 at
    S = 1, where only the locked frame exists), out_vis 0.001-0.005 of the bound of a dot product on the stored features."""
    from pips_amd import ops
    sd, arena = _tl(S)
    stride = 4.0
    delta, ff0, co0_, c0 = M.update_inputs(B, N, S)
    ref = M.update_ref(sd, delta, ff0, co0_, c0, S, stride)
    runs = {}
    for want_vis in (True, False):
        for pad in ((1.0e3, -7.5e8) if delta.shape[1] != S * 130 else (1.0e3,)):
            d = M.update_inputs(B, N, S, pad=pad)[0]
            assert torch.equal(d[:, :S * 130], delta[:, :S * 130])
            ff, co = ff0.to(DEV), co0_.to(DEV)
            other = torch.full((3, S, 128), 3.25, device=DEV)          # rows of another particle behind ffeats: views of one buffer
            buf = torch.cat([ff, other])
            ff = buf[:B * N]
            traj, vis = ops.state_update(arena, d.to(DEV), ff, co, c0.to(DEV), B, N, stride, want_vis=want_vis, S=S)
            assert bool((buf[B * N:] == 3.25).all())
            runs[(want_vis, pad)] = (ff.cpu(), co.cpu(), traj.cpu(), None if vis is None else vis.cpu())
    first = runs[(True, 1.0e3)]
    for key, r in runs.items():                                       # same bits whatever the padding holds, with or without vis
        assert torch.equal(r[0], first[0]) and torch.equal(r[1], first[1]) and torch.equal(r[2], first[2]), key
        assert (r[3] is None) == (not key[0]) and (r[3] is None or torch.equal(r[3], first[3]))
    ff, co, traj, vis = first
    r_ff = M.worst((ff.double() - ref["ffeats"][0]).abs(), ref["ffeats"][1])
    r_co = M.worst((co.double() - ref["coords"][0]).abs(), ref["coords"][1])
    r_vis = M.worst((M.to_bsn(ref["vis"][0], B, N) - vis.double()).abs(), M.to_bsn(ref["vis"][1], B, N))
    own, own_b = M.vis_ref(sd, ff)                                     # the head on the kernel's own new features
    r_own = M.worst((M.to_bsn(own, B, N) - vis.double()).abs(), M.to_bsn(own_b, B, N))
    print(f"state_update S={S} B={B} N={N}: ffeats {r_ff:.3f}, coords {r_co:.2f}, vis {r_vis:.3f} of the bound; vis against the head of "
          f"the stored features {r_own:.4f}")
    assert r_ff <= 1.0 and r_co <= 1.0 and r_vis <= 1.0 and r_own <= 1.0
    assert tuple(traj.shape) == (B, S, N, 2) and torch.equal(traj, M.to_bsn(co, B, N) * stride)      # (B, S, N, 2) order, one product
    assert torch.equal(co[:, 0], c0[:, 0])                                                            # frame 0 is the query


# ------------------------------------------------------------------ visibility head
@pytest.mark.parametrize("B,N,S", [(2, 3, 5), (1, 1, 8), (1, 7, 12)])
def test_vis_head(B, N, S):
    """vis_head_kernel, one wave per row, M % 4 != 0 in two of the cases; equal to the out_vis of the state update on the same
    new features, to the bound of two correct dot products.  Measured 0.002-0.004 of the bound, 0.001-0.003 against the update's."""
    from pips_amd import ops
    sd, arena = _tl(S)
    delta, ff, co, c0 = M.update_inputs(B, N, S, seed=23)
    ff = ff.to(DEV)
    _, vis_upd = ops.state_update(arena, delta.to(DEV), ff, co.to(DEV), c0.to(DEV), B, N, 8.0, want_vis=True, S=S)
    got = ops.vis_head(arena, ff, B, N).cpu()
    ref, bound = M.vis_ref(sd, ff.cpu())
    ref, bound = M.to_bsn(ref, B, N), M.to_bsn(bound, B, N)
    r = M.worst((got.double() - ref).abs(), bound)
    r2 = M.worst((got.double() - vis_upd.cpu().double()).abs(), 2 * bound)
    print(f"vis_head B={B} N={N} S={S}: {r:.4f} of the bound; against the update's out_vis {r2:.4f}")
    assert tuple(got.shape) == (B, S, N) and r <= 1.0 and r2 <= 1.0


# ------------------------------------------------------------------ the stages chained = the product's mixer
def _arena_offsets(S=8):
    """Offsets of the mixer's GEMM operands in a packed arena (csrc/api.hip: build_layout): fp32 tensors in floats from the
    arena base, their bf16 copies in bf16 elements from the end of the fp32 section.  Only a wrong offset here can fail
    the bit comparison below, never pass it."""
    off = 0

    def take(n, unit=64):
        nonlocal off
        o = off
        off += (n + unit - 1) // unit * unit
        return o
    convs = [(64, 3, 7)]
    ci = 64
    for dim, st in zip((64, 96, 128, 128), (1, 2, 2, 2)):
        for blk in range(2):
            s = st if blk == 0 else 1
            convs += [(dim, ci, 3), (dim, dim, 3)] + ([(dim, ci, 1)] if s != 1 else [])
            ci = dim
    convs += [(256, 416, 3), (128, 256, 1)]
    for co, cin, k in convs:
        take(co * cin * k * k), take(co)
    A = {"w_in": take(512 * 544), "b_in": take(512), "w1": [], "b1": [], "w2": [], "b2": [], "h_w1": [], "h_w2": []}
    for _ in range(12):
        take(512), take(512)
        A["w1"].append(take(2048 * 512)), A["b1"].append(take(2048)), A["w2"].append(take(2048 * 512)), A["b2"].append(take(512))
        take(512), take(512)
    for n in (512, 512, 128, 128, 128 * 128, 128, 128, 1):
        take(n)
    total, off = off, 0
    for _ in range(12):
        A["h_w1"].append(take(2048 * 512, 128)), A["h_w2"].append(take(2048 * 512, 128))
    for co, cin, k in convs[1:]:
        take(co * cin * k * k, 128)
    A["h_in"] = take(512 * 544, 128)
    total_h, off = off, 0
    for n in [512 * 544] + [2048 * 512] * 24 + [co * cin * k * k for co, cin, k in convs[1:]]:
        take(3 * n, 128)
    total_t = off
    off = (total + (total_h + total_t + 1) // 2 + 63) // 64 * 64
    for _ in range(12):
        take(4 * S * S), take(4 * S), take(4 * S * S), take(S)
    nout = M.delta_stride(S)
    A["w_head"], A["b_head"] = take(nout * 512), take(nout)
    A["h_head"] = 2 * (take((nout * 512 + 1) // 2) - total)
    take((3 * nout * 512 + 1) // 2)
    A["total"], A["total_all"] = total, off
    return A


@pytest.mark.parametrize("bf16", [False, True])
def test_stages_chain_to_the_mixer(bf16):
    """in-projection, 12 x (token_mix, up, down), ln_mean, head through the stage entry points and ops.gemm* on the arena's own
    weights reproduce ops.mixer_fwd bit for bit (P = 5, S = 8; fp32, and bf16 operands with the fp32 stream): the stage tests
    above judge the launches the product makes"""
    from pips_amd import ops
    sd, arena = _tl()
    A = _arena_offsets()
    P = 5
    X = torch.zeros(P * 8, 544)
    X[:, :519] = G.mixer_rows(P).reshape(P * 8, 519)
    X = X.to(DEV)
    want = ops.mixer_fwd(arena, X, bf16=bf16)
    hw = arena.view(torch.bfloat16)[2 * A["total"]:]

    def f32(o, n, k=None):
        return arena[o:o + n * (k or 1)].view(*((n, k) if k else (n,)))

    def lin(inp, w, hk, b, n, k, epi=0, R=None, out_bf16=False):
        if bf16:
            return ops.gemm_bf16(inp, hw[hk:hk + n * k].view(n, k), f32(b, n), epi=epi, R=R, out_bf16=out_bf16)
        return ops.gemm(inp, f32(w, n, k), f32(b, n), epi=epi, R=R)
    # the packed weights are the state dict's: a wrong offset cannot go unnoticed
    assert A["total_all"] == arena.numel()
    assert torch.equal(f32(A["w1"][11], 2048, 512).cpu(), sd[f"{M.MD}.12.1.fn.0.weight"])
    assert torch.equal(f32(A["b_head"], 1040).cpu(), sd[f"{M.MD}.15.bias"])
    x = lin(X, A["w_in"], A["h_in"], A["b_in"], 512, 544)
    for d in range(12):
        x = x.view(P, 8, 512)
        xn = ops.token_mix(arena, d, x, bf16=bf16)
        h = lin(xn.view(P * 8, 512), A["w1"][d], A["h_w1"][d], A["b1"][d], 2048, 512, epi=ops.EPI_GELU, out_bf16=bf16)
        x = lin(h, A["w2"][d], A["h_w2"][d], A["b2"][d], 512, 2048, epi=ops.EPI_RESIDUAL, R=x.view(P * 8, 512))
    pooled = ops.ln_mean(arena, x.view(P, 8, 512), bf16=bf16)
    got = lin(pooled, A["w_head"], A["h_head"], A["b_head"], 1040, 512)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(got, want)
