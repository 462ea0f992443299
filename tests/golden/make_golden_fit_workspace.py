"""Workspace and plan sizes of the object-pose fit family (contact_pair, contact_icp, soft_silhouette, pose_transform, mesh_sdf,
fit_step), pinned as data: tests/golden/fit_workspace.json.

    python tests/golden/make_golden_fit_workspace.py [path/to/libivlm_hip.so]

THE COMMITTED FILE WAS NOT PRODUCED BY THE LIBRARY OF THIS TREE.  It was recorded from the library built at the commit BEFORE the
six layout functions were rewritten around one carve helper (csrc/fit_common.h).  tests/test_fit_workspace_cpu.py replays the same
grid through this tree's size queries and requires equality, record for record.  A caller sizes its buffer by these numbers and the
launchers carve it by the same layout, so a layout that moves shows here.  Regenerating the file from the current library only
makes the test vacuous: do that for an INTENDED layout change, and say so in the change.

A record is the arguments of one query followed by the bytes it answers (0: the sizes are refused).  The queries are host-only: no
GPU is needed.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fit_workspace.json")

# 1, the 256-byte alignment edges, the block edges of the fold (256), stationary (256), tile (512) and chunk (1024) sizes
SIZES = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
BATCHES = (1, 2, 24, 65535, 65536)  # 65535: the grid limit, 65536: refused
MAX_POINTS, MAX_FACES, MAX_SIDE = 1 << 20, 1 << 22, 16384


def upto(limit):
    return SIZES + (limit, limit + 1)


# name -> the values of each argument, in the order of the C prototype
GRIDS = {
    "ivlm_contact_pair_workspace_bytes": (BATCHES, upto(MAX_POINTS), upto(MAX_POINTS)),                  # B, N_o, N_h
    "ivlm_contact_icp_workspace_bytes": (BATCHES, upto(MAX_POINTS)),                                     # B, N_o
    "ivlm_soft_silhouette_workspace_bytes": (BATCHES, upto(MAX_FACES), upto(MAX_FACES), upto(MAX_SIDE), upto(MAX_SIDE)),  # B, N, F, H, W
    "ivlm_pose_transform_workspace_bytes": (BATCHES, upto(MAX_FACES)),                                   # B, N
    "ivlm_mesh_sdf_plan_bytes": (upto(MAX_FACES), upto(MAX_FACES)),                                      # N_h, F
    "ivlm_mesh_sdf_workspace_bytes": (BATCHES, upto(MAX_POINTS), upto(MAX_FACES)),                       # B, N, F
    # B, N, F, H, W, N_h (N is bounded by the contact term's limit, the smallest of its members')
    "ivlm_fit_step_workspace_bytes": (BATCHES, upto(MAX_POINTS), upto(MAX_FACES), upto(MAX_SIDE), upto(MAX_SIDE), upto(MAX_POINTS)),
}


def cases(axes):
    """Up to three arguments: the full product.  More: every argument swept over all its values around two base points (the second
    and the fourth value of each axis: 255 and 257, B = 2 and 65535), the product of the two smallest values of every axis, and the
    product of {limit, limit + 1} of every axis - each limit alone and together with every other."""
    if len(axes) <= 3:
        return list(itertools.product(*axes))
    seen = {}
    for base in ([a[1] for a in axes], [a[3] for a in axes]):
        for k, axis in enumerate(axes):
            for v in axis:
                seen[tuple(base[:k] + [v] + base[k + 1:])] = None
    for corner in (itertools.product(*(a[:2] for a in axes)), itertools.product(*(a[-2:] for a in axes))):
        for c in corner:
            seen[tuple(c)] = None
    return list(seen)


def load(path=None):
    lib = C.CDLL(path or os.path.join(os.path.dirname(os.path.dirname(HERE)), "interactvlm_amd", "libivlm_hip.so"))
    for name, axes in GRIDS.items():
        fn = getattr(lib, name)
        fn.argtypes = [C.c_int] * len(axes)
        fn.restype = C.c_size_t
    return lib


def records(lib, name):
    fn = getattr(lib, name)
    return [[*c, fn(*c)] for c in cases(GRIDS[name])]


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    out = {name: records(lib, name) for name in GRIDS}
    with open(OUT, "w") as f:  # (one function per block, eight records per line: readable diffs)
        row = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
        blocks = []
        for name, recs in out.items():
            lines = [",".join(row(r) for r in recs[i:i + 8]) for i in range(0, len(recs), 8)]
            blocks.append('%s:[\n%s\n]' % (row(name), ",\n".join(lines)))
        f.write("{\n%s\n}\n" % ",\n".join(blocks))
    print(f"{OUT}: " + ", ".join(f"{len(v)} {k[5:-6]}" for k, v in out.items()))


if __name__ == "__main__":
    main()
