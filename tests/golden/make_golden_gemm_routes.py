"""Routes of the tile GEMM (csrc/gemm.hip: kernel family, tile, operand / output kind, activation, grid, LDS) and the split-K rule,
pinned as data: tests/golden/gemm_routes.json.

    python tests/golden/make_golden_gemm_routes.py [path/to/libivlm_hip.so]

THE COMMITTED FILE WAS NOT PRODUCED BY THE LIBRARY OF THIS TREE.  It was recorded from the commit BEFORE the GEMM host side was
rewritten around one gemm_route(): that commit's launchers (launch_cfg / launch256 / launch320 / the split-K reduce launch) were
instrumented to record their kernel instantiation, grid and LDS bytes under a dry-run flag instead of launching, behind the same
ivlm_gemm_route_query signature, and this script ran against that library.  tests/test_gemm_routes_cpu.py replays the same sweep
through this tree's ivlm_gemm_route_query and requires equality, record for record.  Regenerating the file from the current library
only makes the test vacuous: do that for an INTENDED routing change, and say so in the change.

A record is 9 ints: (family, BM, BN, operand kind, OUT_F32, activation, grid.x, grid.z, dynamic LDS bytes); family 0 = tile kernels of
gemm.hip, 1 = 8-phase 256 x 256, 2 = 256 x 320, 3 = split-K reduce launch, 4 = "reduction fused into the launch before", -1 = the
call is rejected with return code BM.  No GPU is needed: nothing is launched.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gemm_routes.json")

ACTS = ("none", "gelu", "quick_gelu", "relu", "silu", "swiglu", "sigmoid")  # = activation codes 0..6
OPKS = ("bf16", "fp16", "fp8")
TILES = (0, 64, 96, 128, 176, 256, 320, 512)
# every decision boundary of the routing code (tile counts of 128 / 176 / 256 / 320 tiles against the 256 CUs, M <= 352, N >= 8192,
# N % 320, N % 256, K >= 2048, K % 64, K % 8)
MS = (17, 128, 129, 257, 330, 352, 353, 700, 1024, 1025, 2047, 2048, 4096, 16384, 65536)
NS = (64, 256, 900, 1024, 1280, 2560, 3840, 4096, 5120, 8192, 12288, 22016)
KS = (64, 200, 1096, 1280, 2048, 4096, 5120, 11008)
A_SPLIT, OUT_SPLIT, F16, OUT_F16, W_PANEL, RES_F32 = 4, 8, 16, 32, 64, 2
ENTRY_GEMM, ENTRY_PANEL, ENTRY_FP8, ENTRY_SPLITK, ENTRY_SPLITK_FUSED = range(5)
MAX_REC = 8

# the split-K rule: grid of the former test_splitk_rule_is_the_same_in_python_and_c plus M = 128, 129, 352, 353 and N = 8192
SK_MS = (1, 9, 16, 17, 128, 129, 257, 330, 352, 353, 1000, 1025, 16384)
SK_NS = (256, 1024, 4096, 8192, 12288, 22016)
SK_KS = (512, 1024, 4096, 11008)
SK_MODES = ((0, 0), (5, 0), (0, 1))  # (activation code, has_rms)


def splitk_grid():
    return [(M, N, K, act, rms) for M in SK_MS for N in SK_NS for K in SK_KS for act, rms in SK_MODES]


def load(path=None):
    lib = C.CDLL(path or os.path.join(os.path.dirname(os.path.dirname(HERE)), "interactvlm_amd", "libivlm_hip.so"))
    i, q, p = C.c_int, C.c_int64, C.c_void_p
    lib.ivlm_gemm_route_query.argtypes = [i, i, i, i, q, q, q, q, q, q, q, i, i, i, i, i, i, i, i, i, i, p, i]
    lib.ivlm_gemm_splitk_choice.argtypes = [i] * 5
    for h in ("ivlm_gemm_tile_override", "ivlm_gemm_nsplit", "ivlm_gemm_tile320"):
        getattr(lib, h).argtypes = [i]
    return lib


def case(opk, M, N, K, act, out="16", res=None, a_split=False, batch=1, out_rows=0, a_rows=0, panel="", entry=None, splits=0):
    """One call as the 21 leading arguments of ivlm_gemm_route_query.  out: 16 | f32 | split | f16 | fp8; res: None | bf16 | f32;
    panel: any of the letters W A C (the K-panel entry point), or 'w' = IVLM_GEMM_W_PANEL through ivlm_gemm_bf16."""
    n_out = N // 2 if act == 5 else N
    flags = RES_F32 if res == "f32" else 0
    if opk == "fp8":  # byte matrices; out_kind 0 fp32, 1 bf16, 2 e4m3
        return (ENTRY_FP8, M, N, K, K, K, n_out, N, 0, 0, 0, act, {"16": 1, "f32": 0, "fp8": 2}[out], 1, int(res is not None), 0, 1, flags,
                out_rows, a_rows, 0)
    if opk == "fp16":
        flags |= F16
    if a_split:
        flags |= A_SPLIT
    if out == "split":
        flags |= OUT_SPLIT
    if out == "f16":
        flags |= OUT_F16
    lda, ldc = (2 * K if a_split else K), (2 * n_out if out == "split" else n_out)
    if panel and panel != "w":
        return (ENTRY_PANEL, M, N, K, lda, K, ldc, N, 64 * M if "A" in panel else 0, 64 * N if "W" in panel else 0,
                64 * M if "C" in panel else 0, act, int(out == "f32"), 1, int(res is not None), 0, 1, flags, out_rows, a_rows, 0)
    if panel == "w":
        flags |= W_PANEL
    return (ENTRY_GEMM if entry is None else entry, M, N, K, lda, K, ldc, N, 0, 0, 0, act, int(out == "f32"), 1, int(res is not None), 0,
            batch, flags, out_rows, a_rows, splits)


_buf = (C.c_int32 * (9 * MAX_REC))()


def query(lib, c):
    n = lib.ivlm_gemm_route_query(*c, _buf, MAX_REC)
    assert 1 <= n <= MAX_REC, (c, n)
    return [list(_buf[9 * r:9 * r + 9]) for r in range(n)]


def variants(opk, M, N, K, act):
    """the calls of one shape besides the plain one: output kinds, residuals, split A, batches, row maps, panels"""
    if opk == "fp8":
        for out, res in (("f32", None), ("fp8", None), ("16", "bf16"), ("f32", "f32")):
            yield case(opk, M, N, K, act, out=out, res=res)
        yield case(opk, M, N, K, act, out_rows=1)
        yield case(opk, M, N, K, act, a_rows=1)
        return
    for out, res in (("f32", None), ("split", None), ("f16", None), ("16", "bf16"), ("f32", "f32")):
        yield case(opk, M, N, K, act, out=out, res=res)
    yield case(opk, M, N, K, act, a_split=True)
    yield case(opk, M, N, K, act, batch=2)
    yield case(opk, M, N, K, act, batch=16)
    yield case(opk, M, N, K, act, out_rows=1)
    yield case(opk, M, N, K, act, a_rows=1, out="f32")
    if opk == "bf16":
        for panel in ("W", "A", "C", "WAC", "w"):
            yield case(opk, M, N, K, act, panel=panel)


def splitk_cases(lib, opk, M, N, K, act):
    if opk == "fp8" or M > 2047:
        return
    auto = lib.ivlm_gemm_splitk_choice(M, N, K, act, 0)
    for entry in (ENTRY_SPLITK, ENTRY_SPLITK_FUSED):
        for sp in sorted({auto, 2} - {1}):
            yield case(opk, M, N, K, act, out="f32", res="f32", entry=entry, splits=sp)
        yield case(opk, M, N, K, act, entry=entry, splits=2)


def slice_cases(lib, opk, act, tile):
    """every call of one (operand kind, activation, forced tile) slice, hooks as (nsplit, tile320) in front"""
    full = tile == 0
    for M in MS:
        for N in NS:
            for K in (KS if full else (1280, 4096)):
                yield (1, 1), case(opk, M, N, K, act)
    ms, ns, ks = (MS, NS, (1280, 4096)) if full else ((17, 330, 700, 4096), (900, 1280, 8192), (1280,))
    for M in ms:
        for N in ns:
            for K in ks:
                for c in variants(opk, M, N, K, act):
                    yield (1, 1), c
                yield (0, 1), case(opk, M, N, K, act, out="f32", res="f32")
                yield (1, 0), case(opk, M, N, K, act, out="f32", res="f32")
                yield (0, 0), case(opk, M, N, K, act)
    for M in (MS if full else (17, 330, 700)):
        for N in (NS if full else (900, 4096, 8192)):
            for K in ((1280, 2048, 4096, 11008) if full else (4096,)):
                for c in splitk_cases(lib, opk, M, N, K, act):
                    yield (1, 1), c


def run(lib, hooks_cases, tile):
    """-> the records of every case; the three hooks are restored to their defaults"""
    lib.ivlm_gemm_tile_override(tile)
    try:
        for (nsplit, t320), c in hooks_cases:
            lib.ivlm_gemm_nsplit(nsplit)
            lib.ivlm_gemm_tile320(t320)
            yield c, query(lib, c)
    finally:
        lib.ivlm_gemm_tile_override(0)
        lib.ivlm_gemm_nsplit(1)
        lib.ivlm_gemm_tile320(1)


def slice_digest(lib, opk, act, tile):
    h = hashlib.sha256()
    n = 0
    for c, recs in run(lib, slice_cases(lib, opk, act, tile), tile):
        h.update(repr((c, recs)).encode())
        n += 1
    return n, h.hexdigest()


def explicit_cases():
    """(tile, hooks, case): the GEMMs of the three towers and the benchmark (LLaMA-7B prefill of 330 rows, CLIP ViT-L/14 of 257 rows
    for 1 and 4 images, SAM ViT-H over 4 and 16 views, windowed and global rows), then every forced tile x operand kind x activation at
    one ragged shape"""
    towers = [(330, 12288, 4096, 0), (330, 4096, 4096, 0), (330, 22016, 4096, 5), (330, 4096, 11008, 0),
              (257, 3072, 1024, 0), (257, 1024, 1024, 0), (257, 4096, 1024, 2), (257, 1024, 4096, 0),
              (1028, 3072, 1024, 0), (1028, 1024, 1024, 0), (1028, 4096, 1024, 2), (1028, 1024, 4096, 0),
              (16384, 3840, 1280, 0), (16384, 1280, 1280, 0), (16384, 5120, 1280, 1), (16384, 1280, 5120, 0),
              (19600, 3840, 1280, 0), (65536, 3840, 1280, 0), (65536, 1280, 1280, 0), (65536, 5120, 1280, 1), (65536, 1280, 5120, 0),
              (78400, 3840, 1280, 0), (16384, 256, 1280, 0), (16384, 256, 2304, 0)]
    for opk in OPKS:
        for M, N, K, act in towers:
            yield 0, (1, 1), case(opk, M, N, K, act)
            yield 0, (1, 1), case(opk, M, N, K, act, out="f32", res="f32")
            if opk != "fp8":
                yield 0, (1, 1), case(opk, M, N, K, act, out="split", a_split=True)
    for tile in TILES:
        for opk in OPKS:
            for act in range(7):
                yield tile, (1, 1), case(opk, 700, 900, 1096, act)
                if opk == "fp8":  # (1096 bytes are no whole 16-byte granules: rejected; 1104 are)
                    yield tile, (1, 1), case(opk, 700, 900, 1104, act)


def explicit_rows(lib):
    rows = []
    for tile, hooks, c in explicit_cases():
        (_, recs), = run(lib, [(hooks, c)], tile)
        rows.append({"tile": tile, "case": list(c), "records": recs})
    return rows


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    digests = {}
    total = 0
    for opk in OPKS:
        for act in range(7):
            for tile in TILES:
                n, d = slice_digest(lib, opk, act, tile)
                digests[f"{opk}/{ACTS[act]}/{tile}"] = [n, d]
                total += n
    out = {"record": ["family", "BM", "BN", "operand_kind", "out_f32", "act", "grid_x", "grid_z", "lds_bytes"],
           "explicit": explicit_rows(lib), "digests": digests,
           "splitk_rule": [lib.ivlm_gemm_splitk_choice(*a) for a in splitk_grid()]}
    with open(OUT, "w") as f:  # (one explicit row / digest per line: readable diffs)
        row = lambda v: json.dumps(v, separators=(",", ":"))
        f.write('{"record":%s,\n"explicit":[\n%s\n],\n"digests":{\n%s\n},\n"splitk_rule":%s}\n' % (
            row(out["record"]), ",\n".join(row(r) for r in out["explicit"]),
            ",\n".join(f"{row(k)}:{row(v)}" for k, v in digests.items()), row(out["splitk_rule"])))
    print(f"{OUT}: {len(out['explicit'])} explicit rows, {len(digests)} slice digests over {total} calls, "
          f"{len(out['splitk_rule'])} split-K choices")


if __name__ == "__main__":
    main()
