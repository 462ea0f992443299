"""Every output bit of the screen-space face walks - soft silhouette, its image terms, z-buffer, depth-order term and the two fit
callers - on the cases of tests/_screen_bits.py, pinned as data: tests/golden/screen_bits.json.  Needs the GPU.

    python tests/golden/make_golden_screen_bits.py COMMIT [FILE]     (FILE: write there instead of tests/golden/screen_bits.json)

THE COMMITTED FILE WAS NOT PRODUCED BY THE LIBRARY OF THIS TREE.  It was recorded on an MI355X from the library built of commit
bc24efb's csrc/ (loaded through IVLM_LIB_PATH; the Python side is the same), BEFORE csrc/silhouette.hip and csrc/depth_order.hip
were rewritten around the shared walk of csrc/screen_common.h: one projection, one face test, one union fold, one tile walk, one box
walk, one gather.  That change claims to move no result bit - the compaction order of a tile's faces, the length of the fp32 chains,
the fp64 fold across the lanes, the order of a vertex's incident faces, and each file's own -ffp-contract setting - and
tests/test_screen_bits_gpu.py holds it, and whatever later touches the walk, to it by replaying the same cases through this tree and
requiring equality, output for output.  Regenerating the file from the current tree only makes the test vacuous: do that for an
INTENDED change of a result, and say so in the change.

A record is one output: its shape and the hex of its int32 view, or the sha256 of that view's bytes when they are more than 64
(``_lift_bits.encode``).  COMMIT is written into the file as given: the tree cannot tell where its library was built from.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "screen_bits.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import torch

    import _screen_bits

    dev = torch.device("cuda:0")
    cases = {name: _screen_bits.record(name, dev) for name in _screen_bits.CASES}
    out = {"commit": sys.argv[1], "torch": torch.__version__, "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": cases}
    path = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{path}: " + ", ".join(f"{len(v)} {k}" for k, v in cases.items()))


if __name__ == "__main__":
    main()
