"""Every output bit of the dense, data-movement and decode-attention wrappers of interactvlm_amd/ops.py on the cases of
tests/_dense_bits.py, pinned as data: tests/golden/dense_bits.json.  Needs the GPU.

    python tests/golden/make_golden_dense_bits.py COMMIT [FILE]     (FILE: write there instead of tests/golden/dense_bits.json)

THE COMMITTED FILE WAS NOT PRODUCED BY THE PACKAGE OF THIS TREE.  It was recorded on an MI355X from the package at commit 37130e4,
BEFORE those wrappers were folded onto one launch frame, one epilogue filler, one kind table and one set of decode-attention checks
(this file and tests/_dense_bits.py copied into a checkout of that commit: they use public signatures only).  The fold claims to hand
every C call the arguments it got before, and tests/test_dense_bits_gpu.py holds it, and whatever later touches a wrapper, to that by
replaying the same cases through this tree and requiring equality, output for output.  Recorded twice at that commit, in two
processes: the two files were identical.  Regenerating the file from the current tree only makes the test vacuous: do that for an
INTENDED change of a result, and say so in the change.

A record is one output: its shape, its dtype and the hex of its bytes, or their sha256 when they are more than 64
(``_dense_bits.encode``).  COMMIT is written into the file as given: the tree cannot tell where it was copied from.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dense_bits.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import torch

    import _dense_bits

    dev = torch.device("cuda:0")
    cases = {name: _dense_bits.record(name, dev) for name in _dense_bits.CASES}
    out = {"commit": sys.argv[1], "torch": torch.__version__, "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": cases}
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{path}: " + ", ".join(f"{len(v)} {k}" for k, v in cases.items()))


if __name__ == "__main__":
    main()
