"""Every deterministic output bit of the mask-to-vertex lift family (plan build, plan gather, fused low-res gather, mask band census)
on the cases of tests/_lift_bits.py, pinned as data: tests/golden/lift_bits.json.  Needs the GPU.

    python tests/golden/make_golden_lift_bits.py COMMIT [FILE]     (FILE: write there instead of tests/golden/lift_bits.json)

THE COMMITTED FILE WAS NOT PRODUCED BY THE PACKAGE OF THIS TREE.  It was recorded on an MI355X from the package at commit 0c4d1fe,
BEFORE the host side of csrc/lift.hip was rewritten around one plan builder, one vote-slab frame, one streaming launcher and one mode
dispatch, and before the lift wrappers of ops.py and the predictors' plan caches were folded.  Those changes claim to move no result
bit - the summation order of the gather in particular: per lane k = 0..3 within a stride, strides in index order, the wave
butterfly, views in view order - and tests/test_lift_bits_gpu.py holds them, and whatever later touches the gather or the census
walk, to it by replaying the same cases through this tree and requiring equality, output for output.  Regenerating the file from the current tree only makes the test vacuous: do that
for an INTENDED change of a result, and say so in the change.

A record is one output: its shape and the hex of its int32 view, or the sha256 of that view's bytes when they are more than 64
(``_lift_bits.encode``).  COMMIT is written into the file as given: the tree cannot tell where it was copied from.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lift_bits.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import torch

    import _lift_bits

    dev = torch.device("cuda:0")
    cases = {name: _lift_bits.record(name, dev) for name in _lift_bits.CASES}
    out = {"commit": sys.argv[1], "torch": torch.__version__, "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": cases}
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{path}: "+ ", ".join(f"{len(v)} {k}" for k, v in cases.items()))


if __name__ == "__main__":
    main()
