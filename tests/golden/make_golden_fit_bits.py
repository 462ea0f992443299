"""Every output bit of the object-pose fit family's Python side (contact_pair, silhouette, pose, mesh_sdf, contact_icp, fit) on the cases
of tests/_fit_bits.py, pinned as data: tests/golden/fit_bits.json.  Needs the GPU.

    python tests/golden/make_golden_fit_bits.py COMMIT

THE COMMITTED FILE WAS NOT PRODUCED BY THE PACKAGE OF THIS TREE.  It was recorded from the package at commit 25cdd93, BEFORE the six
Python modules were rewritten around shared argument checks, one saved-gradient Function, ``fit.FitScene`` and ``fit.TERMS``.
tests/test_fit_bits_gpu.py replays the same cases through this tree and requires equality, output for output.  Regenerating the file
from the current tree only makes the test vacuous: do that for an INTENDED change of a result, and say so in the change.

A record is one output: its shape and the hex of its int32 / uint8 view (``_fit_bits.encode``).  COMMIT is written into the file as
given: the tree cannot tell where it was copied from.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fit_bits.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import torch

    import _fit_bits

    dev = torch.device("cuda:0")
    with torch.enable_grad():
        cases = {name: _fit_bits.record(name, dev) for name in _fit_bits.CASES}
    out = {"commit": sys.argv[1], "torch": torch.__version__, "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{OUT}: " + ", ".join(f"{len(v)} {k}" for k, v in cases.items()))


if __name__ == "__main__":
    main()
