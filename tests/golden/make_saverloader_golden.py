"""Record the reference's checkpoint layout (build container only).

    python tests/golden/make_saverloader_golden.py

Runs the reference's own saverloader.save twice (global steps 3 and 7) on pips_amd.Pips with the tamed weights, then
its saverloader.load into a fresh Pips, and writes what that left on disk to tests/golden/saverloader_layout.json:
the checkpoint file names, the top-level keys of a checkpoint (in order), the type of its model_state_dict and the
step load() returned.  tests/test_boundary.py::test_reference_saverloader_round_trip writes and reads checkpoints in
exactly that layout, so the round trip is held to the reference without the reference being present.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import reference_shim as R            # noqa: E402
from pips_amd.weights import init_state_dict      # noqa: E402

STEPS = [3, 7]


def main():
    assert R.available(), "reference not mounted"
    sys.dont_write_bytecode = True                 # the mount is read-only by contract
    spec = importlib.util.spec_from_file_location("_reference_saverloader", os.path.join(R.REFERENCE_ROOT, "saverloader.py"))
    saverloader = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(saverloader)
    from pips_amd import Pips
    src = Pips(stride=8)
    src.load_state_dict(init_state_dict(0, tamed=True))
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with tempfile.TemporaryDirectory() as d:
        ckpt_dir = os.path.join(d, "ckpt")
        for step in STEPS:
            saverloader.save(ckpt_dir, opt, src, global_step=step)
        files = sorted(os.listdir(ckpt_dir))
        ck = torch.load(os.path.join(ckpt_dir, files[-1]))
        dst = Pips(stride=8)
        step = saverloader.load(ckpt_dir, dst)
        for (ka, a), (kb, b) in zip(src.state_dict().items(), dst.state_dict().items()):
            assert ka == kb and torch.equal(a, b)
    out = {"saved_steps": STEPS, "files": files, "checkpoint_keys": list(ck.keys()),
           "model_state_dict_type": type(ck["model_state_dict"]).__name__,
           "model_state_dict_keys_match": list(ck["model_state_dict"].keys()) == list(src.state_dict().keys()),
           "load_returned_step": step}
    with open(os.path.join(HERE, "saverloader_layout.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
