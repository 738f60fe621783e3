"""CPU: the drop-in boundary -- state-dict compatibility, the C ABI surface, loud failure
without a GPU.  No compute calls."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_matches_reference_keys():
    from pips_amd import Pips
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        ref = json.load(f)
    sd = Pips(S=8, stride=8).state_dict()
    assert list(sd.keys()) == list(ref.keys())                 # same names, same order
    assert {k: list(v.shape) for k, v in sd.items()} == ref
    assert sum(v.numel() for v in sd.values()) == 28677713


def test_load_reference_format_checkpoint(tmp_path, weights_tamed):
    """saverloader.py:58-59 style: torch.load(...)['model_state_dict'] -> load_state_dict(strict=False)."""
    from pips_amd import Pips
    path = tmp_path / "model-000000001.pth"
    torch.save({"model_state_dict": weights_tamed, "optimizer_state_dict": {}}, path)
    ck = torch.load(path)
    m = Pips(stride=4)
    res = m.load_state_dict(ck["model_state_dict"], strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    k = "delta_block.to_delta.15.weight"
    assert torch.equal(m.state_dict()[k], weights_tamed[k])


def test_library_exports_every_declared_symbol():
    import ctypes
    from pips_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pips_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 15
    assert declared == set(_lib.SIGNATURES)                    # binding table mirrors the header
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.pips_abi_version() == 3        # 3: slack behind the bf16 mirror, larger tiled-gather scratch, PIPS_EPI_RES_BF16 public (2: bf16 mirror in the pyramid buffer)
    assert lib.pips_weight_arena_bytes() > 28677713 * 4
    # sizing queries are pure host functions
    assert lib.pips_workspace_bytes(1, 8, 368, 496, 256, 8) > 0
    assert lib.pips_workspace_bytes(1, 7, 368, 496, 256, 8) > 0           # any window length 1..PIPS_S_MAX
    assert lib.pips_workspace_bytes(1, 33, 368, 496, 256, 8) == 0 and lib.pips_weight_arena_bytes_s(33) == 0
    assert lib.pips_weight_arena_bytes_s(8) == lib.pips_weight_arena_bytes()
    assert lib.pips_weight_arena_bytes_s(5) < lib.pips_weight_arena_bytes() < lib.pips_weight_arena_bytes_s(12)
    assert lib.pips_delta_stride(8) == 1040 and lib.pips_delta_stride(5) == 652 and lib.pips_delta_stride(0) == 0
    assert lib.pips_track_workspace_bytes_s(2, 64, 8) == lib.pips_track_workspace_bytes(2, 64)
    assert lib.pips_mixer_workspace_bytes_s(1024, 8) == lib.pips_mixer_workspace_bytes(1024)
    assert lib.pips_pyramid_offset(8, 368, 496, 8, 1) == 8 * 46 * 62 * 128
    assert lib.pips_pyramid_floats(8, 368, 496, 8) >= 8 * 128 * (46 * 62 + 23 * 31 + 11 * 15 + 5 * 7)


def test_binding_table_matches_every_prototype():
    """Each SIGNATURES row against its prototype in include/pips_hip.h: the number of arguments, the kind of each one
    (pointer / int / size_t / float) and the kind of the return value.  The names alone (the test above) would let a row
    that dropped or swapped an argument through, and ctypes would then marshal a corrupted call."""
    import ctypes as C
    from pips_amd import _lib

    def c_kind(decl):
        if "*" in decl:
            return "pointer"
        kinds = [t for t in decl.split() if t in ("int", "size_t", "float")]
        assert len(kinds) == 1, f"cannot classify {decl!r}"
        return kinds[0]

    def ctypes_kind(t):
        if t in (C.c_void_p, C.c_char_p) or isinstance(t, type(C.POINTER(C.c_int))):
            return "pointer"
        return {C.c_int: "int", C.c_size_t: "size_t", C.c_float: "float"}[t]

    hdr = open(os.path.join(ROOT, "include", "pips_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = "\n".join(l for l in hdr.splitlines() if not l.lstrip().startswith("#"))
    protos = re.findall(r"([\w\s\*]+?)\b(pips_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert {name for _, name, _ in protos} == set(_lib.SIGNATURES) and len(protos) == len(_lib.SIGNATURES)
    for ret, name, params in protos:
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        res, args = _lib.SIGNATURES[name]
        assert ctypes_kind(res) == c_kind(ret), f"{name}: returns {ret.strip()!r}"
        assert len(args) == len(params), f"{name}: {len(params)} parameters declared, {len(args)} bound"
        for i, (a, p) in enumerate(zip(args, params)):
            assert ctypes_kind(a) == c_kind(p), f"{name}: argument {i} is {p!r}"
    # the check has teeth: a 24-argument row with one c_int dropped, or an int bound as a pointer, is caught
    assert ctypes_kind(C.POINTER(C.c_float)) == "pointer" and c_kind("const void* const* params_host") == "pointer"
    assert c_kind("size_t workspace_bytes") == "size_t" != ctypes_kind(C.c_int)


def test_no_cpu_fallback():
    from pips_amd import Pips, PipsHipError
    m = Pips()
    with pytest.raises(PipsHipError):
        m(torch.zeros(1, 4, 2), torch.zeros(1, 8, 3, 128, 160), iters=1)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pips_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} references the oracle"


def test_reference_import_path_resolves_to_the_hip_model():
    """Every reference caller does `from nets.pips import Pips` (demo.py:9, chain_demo.py:9, test_on_flt.py:6, ...)."""
    import nets.pips
    import pips_amd
    assert nets.pips.Pips is pips_amd.Pips


def test_nets_is_a_namespace_package_merged_with_the_reference(tmp_path):
    """``nets`` ships no __init__.py: with this repository ahead of the reference checkout on sys.path the reference's
    sibling modules stay importable (``from nets.raftnet import Raftnet`` is line 5 of test_on_flt.py / test_on_crohd.py
    / test_on_badja.py, ahead of ``from nets.pips import Pips``) while nets.pips resolves to the HIP model.  The checkout
    is stood in for by a tree of the same shape: ``nets/`` without __init__.py, a sibling ``raftnet.py`` and a
    ``pips.py`` of its own that must lose to this repository's."""
    import subprocess, sys
    assert not os.path.exists(os.path.join(ROOT, "nets", "__init__.py"))
    ref_root = str(tmp_path / "checkout")
    os.makedirs(os.path.join(ref_root, "nets"))
    with open(os.path.join(ref_root, "nets", "raftnet.py"), "w") as f:
        f.write("class Raftnet:\n    pass\n")
    with open(os.path.join(ref_root, "nets", "pips.py"), "w") as f:
        f.write("raise ImportError('the checkout nets.pips shadowed the HIP model')\n")
    code = ("import sys, importlib.util\n"
            f"sys.path[:0] = [{ROOT!r}, {ref_root!r}]\n"
            "import nets.pips, pips_amd\n"
            "assert nets.pips.Pips is pips_amd.Pips\n"
            "assert nets.pips.__file__.startswith(%r)\n" % ROOT +
            f"spec = importlib.util.find_spec('nets.raftnet')\nassert spec is not None and spec.origin.startswith({ref_root!r}), spec\n"
            "from nets.raftnet import Raftnet\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_reference_saverloader_round_trip(tmp_path, weights_tamed):
    """Checkpoints of pips_amd.Pips in the layout the reference's saverloader.save / saverloader.load (saverloader.py:5-69)
    use, recorded from those functions on this model in tests/golden/saverloader_layout.json (make_saverloader_golden.py):
    ``<ckpt_dir>/model-%09d.pth`` per global step, a dict of optimizer_state_dict + model_state_dict; load takes the
    highest step and does ``load_state_dict(ckpt['model_state_dict'], strict=False)``."""
    with open(os.path.join(ROOT, "tests", "golden", "saverloader_layout.json")) as f:
        layout = json.load(f)
    from nets.pips import Pips
    src = Pips(stride=8)
    src.load_state_dict(weights_tamed)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    ckpt_dir = tmp_path / "ckpt"
    ckpt_dir.mkdir()
    for step in layout["saved_steps"]:
        parts = {"optimizer_state_dict": opt.state_dict(), "model_state_dict": src.state_dict()}
        torch.save({k: parts[k] for k in layout["checkpoint_keys"]}, ckpt_dir / ("model-%09d.pth" % step))
    names = sorted(os.listdir(ckpt_dir))
    assert names == layout["files"]
    step = max(int(n.split("-")[1].split(".")[0]) for n in names)
    assert step == layout["load_returned_step"] == 7
    ck = torch.load(ckpt_dir / ("model-%09d.pth" % step))
    assert list(ck.keys()) == layout["checkpoint_keys"]
    assert type(ck["model_state_dict"]).__name__ == layout["model_state_dict_type"]
    assert layout["model_state_dict_keys_match"] and list(ck["model_state_dict"].keys()) == list(src.state_dict().keys())
    dst = Pips(stride=8)                                        # seeded init != tamed weights
    res = dst.load_state_dict(ck["model_state_dict"], strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    for (ka, a), (kb, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert ka == kb and torch.equal(a, b)


def test_packed_weights_follow_parameter_changes():
    """The kernel-side arena is rebuilt when storage or version of a parameter changes; .data writes need invalidate."""
    from pips_amd import Pips
    m = Pips()
    assert m._plist is None and m._arena is None
    m.invalidate_weights()
    m2 = m.float()                                             # _apply path
    assert m2 is m and m._arena is None
    # a REPLACED parameter (load_state_dict(assign=True), node.weight = nn.Parameter(...)) changes the cache key too:
    # the key is built from the live objects, not from a list captured at the first forward
    import pips_amd.ops as ops
    packed = []
    orig = ops.pack_weights
    ops.pack_weights = lambda sd, dev, sections=7, S=8: packed.append({k: v for k, v in sd.items()}) or object()
    try:
        m._packed("cpu")
        m._packed("cpu")
        assert len(packed) == 1
        node = m.delta_block.to_delta._modules["15"]
        node.weight = torch.nn.Parameter(node.weight.detach().clone() * 2, requires_grad=False)
        m._packed("cpu")
        assert len(packed) == 2 and packed[1]["delta_block.to_delta.15.weight"] is node.weight
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd, assign=True)
        m._packed("cpu")
        assert len(packed) == 3
    finally:
        ops.pack_weights = orig


GENERATED_ASM = (("gen_gather_asm.py", "gather_item_asm.inc"), ("gen_gemm_bf16_t4.py", "gemm_bf16_t4_asm.inc"),
                 ("gen_gemm_bf16_t4up.py", "gemm_bf16_t4up_asm.inc"), ("gen_conv_bf16_t4c.py", "conv_bf16_t4c_asm.inc"),
                 ("gen_gemm_f32_t4.py", "gemm_f32_t4_asm.inc"), ("gen_conv_f32_t4.py", "conv_f32_t4_asm.inc"))


def test_build_script_dependencies_exist_and_asm_is_current(tmp_path):
    """The build script's dependency list names real files (a stale name makes every rebuild fail), and every committed generated
    assembly file is what its generator in tools/ emits today (in the default environment: the generators' tuning switches are
    taken out of the child's)."""
    import subprocess, sys
    from pips_amd import _build
    for h in _build.headers():
        assert os.path.exists(h), h
    env = dict(os.environ)
    for k in ("PIPS_GEN_ABLATE", "PIPS_GEN_TRACE", "PIPS_GEN_STORE_POLICY", "PIPS_GEN_D4"):
        env.pop(k, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for gen, inc in GENERATED_ASM:
        out = tmp_path / inc
        env["PIPS_GEN_OUT"] = str(out)
        subprocess.check_call([sys.executable, os.path.join(root, "tools", gen)], env=env, stdout=subprocess.DEVNULL)
        assert out.read_text() == open(os.path.join(root, "pips_amd", "csrc", inc)).read(), inc


def _lint():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("asm_hazard_lint", os.path.join(root, "tools", "asm_hazard_lint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, root


def test_asm_hazard_lint_passes_head_and_flags_the_round5_scatter():
    """Every instruction stream of the shipped library -- hipcc's code and the 37 k lines of generated / hand-written assembly that
    its hazard recognizer never sees -- holds the software wait states of tools/asm_hazard_lint.py's table (MFMA result -> any
    reader or writer, VALU-written SGPR / VCC -> VALU / vector memory / lane select, M0 -> LDS-DMA, ...): the disassembly of
    libpips_hip.so has no finding.  The negative fixture is the scatter of gather_mfma_kernel as commit a4e2782~1 built it -- the MFMA ->
    DS-read hazard round 5 met by accident: the lint must flag its four ds_write_b32."""
    L, root = _lint()
    from pips_amd import _build
    findings, st = L.lint_path(_build.build_library(verbose=False))
    assert st["kernels"] > 100 and st["mfma"] > 10000, st          # the whole library was read
    assert findings == [], findings[:5]
    neg, _ = L.lint_path(os.path.join(root, "tests", "golden", "hazard_negative_gather_mfma_pre_a4e2782.s"))
    assert len(neg) == 4 and all("v_mfma_f32_32x32x16_bf16 result -> read by ds_write_b32" in f["rule"] for f in neg), neg
    assert sorted(f["have"] for f in neg) == [4, 6, 8, 10] and all(f["need"] == 12 for f in neg)


def test_product_library_ships_only_reachable_gemm_tiles():
    """A kernel that only a tuning hook can select exists only in a tuning build (common.h): the product library holds exactly the
    igemm_f32_kernel / gemm_x3_kernel instantiations that launch_gemm / launch_conv / launch_gemm_x3 / launch_conv_x3 can reach
    without a hook -- template arguments (BM, BN, WGM, WGN, KS, CONV[, BKE]) -- and the register-staged bf16 family keeps its 51."""
    L, _ = _lint()
    from pips_amd import _build
    names = {n for text in L.disassemble(_build.build_library(verbose=False)) for n in L.parse_objdump(text)}

    def instantiations(kernel):
        out = set()
        for n in names:
            m = re.match(r"_ZN4pips\d+%sI((?:L[ib]\d+E)+)E" % kernel, n)
            if m:
                out.add(tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))))
        return out

    assert instantiations("igemm_f32_kernel") == {
        (128, 128, 2, 2, 1, 0), (64, 64, 2, 2, 1, 0), (64, 64, 2, 2, 2, 0),
        (128, 128, 2, 2, 1, 1), (64, 128, 2, 2, 1, 1), (128, 96, 4, 1, 1, 1), (64, 96, 2, 1, 1, 1), (128, 64, 2, 2, 1, 1), (64, 64, 2, 2, 1, 1)}
    assert instantiations("gemm_x3_kernel") == {
        (256, 128, 4, 2, 1, 0, 32), (128, 128, 2, 2, 2, 0, 16), (128, 128, 2, 2, 1, 0, 32), (64, 64, 2, 2, 2, 0, 32), (64, 64, 2, 2, 1, 0, 32),
        (256, 128, 4, 2, 1, 1, 32), (128, 128, 2, 2, 1, 1, 32), (128, 64, 2, 2, 1, 1, 32), (64, 128, 2, 2, 1, 1, 32), (64, 64, 2, 2, 1, 1, 32)}
    assert len(instantiations("gemm_bf16_kernel")) == 51


def test_hazard_table_matches_the_compilers_recognizer():
    """gfx950's wait-state table is not in this image; the lint's numbers are pinned against hipcc's own hazard recognizer: one probe
    kernel per producer / consumer pair (tools/asm_hazard_probe.hip, builtins + sched_barriers), the s_nops hipcc inserts are the
    requirement."""
    L, _ = _lint()
    rows = L.measure_probes()
    assert len(rows) >= 28
    bad = [r for r in rows if r[1] != r[2]]
    assert not bad, bad


def test_generators_take_their_wait_states_from_one_place():
    """The five pasted `s_nop 15; s_nop 15` pairs of rounds 4-5 are gone: every generator takes its guards from tools/asm_guards.py,
    whose numbers are the lint's table.  The same for what counts the s_waitcnt: the issue model, the buffer descriptor, the GELU and
    the float literal live in tools/asm_emit.py alone -- no generator, the parked ones of tools/experiments included, has a copy."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gens = sorted(glob.glob(os.path.join(root, "tools", "gen_*.py")))
    assert len(gens) == 6
    assert [os.path.basename(g) for g in gens] == sorted(gen for gen, _ in GENERATED_ASM)
    for g in gens:
        src = open(g).read()
        assert "import asm_guards" in src and "s_nop 15" not in src, g
    parked = sorted(glob.glob(os.path.join(root, "tools", "experiments", "gen_*.py")))
    assert parked
    for g in gens + parked:
        src = open(g).read()
        assert re.search(r"^(from asm_emit import|import asm_emit)\b", src, re.M), g
        for copy in ("class Emit", "def descriptor", "def f32(", "def gelu4("):
            assert copy not in src, (g, copy)
    shared = open(os.path.join(root, "tools", "asm_emit.py")).read()
    for one in ("class Emit", "def descriptor(", "def f32(", "def gelu4(", "def write_inc(", "def out_path("):
        assert shared.count(one) == 1, one


def test_profiles_readme_is_generated_from_the_files():
    """The current round's table of profiles/README.md is what tools/profiles_readme.py generates from the committed evidence files
    (rounds 3-5 copied their numbers by hand and the prose drifted from the files three times)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "profiles_readme.py"), "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_gather_mfma2_variant_builds_and_passes_the_lint(tmp_path):
    """gather_mfma2_kernel (round 6's re-cut of the bf16 dense gather: LDS-DMA requests as assembly statements with counted waits) is not in
    the product library -- it is 3-4 % slower than gather_mfma_kernel -- but stays buildable for A/B runs (-DPIPS_GM_V_DEFAULT=2): the variant
    object compiles for gfx950 and its hand-written request statements hold their wait states (M0 -> LDS-DMA, fresh SGPR -> vector memory)."""
    import subprocess
    L, root = _lint()
    from pips_amd import _build
    obj = tmp_path / "gather_gm2.o"
    cmd = [_build._hipcc(), *_build.FLAGS, "-DPIPS_GM_V_DEFAULT=2", "-c", os.path.join(_build.CSRC, "gather_tiled.hip"), "-o", str(obj)]
    subprocess.check_call(cmd)
    findings, st = L.lint_path(str(obj))
    assert st["kernels"] >= 6 and findings == [], findings[:5]
    dis = "\n".join(L.disassemble(str(obj)))
    assert "gather_mfma2_kernel" in dis and dis.count("offen lds") >= 16        # the requests are there (two blocks of eight pieces + records)
