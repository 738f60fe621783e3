"""pips_amd/csrc/conv_f32_e_asm.inc is what tools/conv_f32_e_gen.py writes."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_inc_is_the_generators_output(tmp_path):
    out = tmp_path / "conv_f32_e_asm.inc"
    env = dict(os.environ, PIPS_GEN_OUT=str(out))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "conv_f32_e_gen.py")], env=env, stdout=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "pips_amd", "csrc", "conv_f32_e_asm.inc")) as f:
        assert out.read_text() == f.read(), "regenerate: python tools/conv_f32_e_gen.py"


def test_generator_takes_guards_and_issue_model_from_the_shared_modules():
    """tests/test_boundary.py pins the set of tools/gen_*.py, so this generator carries another name and is held to the same
    rules here: wait states from tools/asm_guards.py, issue model / descriptor / writer from tools/asm_emit.py, no copy of either."""
    import re
    src = open(os.path.join(ROOT, "tools", "conv_f32_e_gen.py")).read()
    assert "import asm_guards" in src and "s_nop" not in src
    assert re.search(r"^(from asm_emit import|import asm_emit)\b", src, re.M)
    for copy in ("class Emit", "def descriptor", "def f32(", "def gelu4(", "def write_inc(", "def out_path("):
        assert copy not in src, copy
