"""Argument check and routing of the decode-attention family (csrc/decode.hip, decode_prefix.hip, verify.hip, decode_fused.hip: return
code, kernel, template flags, grid, block, offset of the partials in the scratch), pinned as data: tests/golden/decode_attn_routes.json.

    python tests/golden/make_golden_decode_attn.py [path/to/libivlm_hip.so]

THE COMMITTED FILE WAS NOT PRODUCED BY THE LIBRARY OF THIS TREE.  It was recorded from the commit BEFORE the host side of the family was
rewritten around DecodeAttnArgs / decode_attn_check / decode_attn: that commit's launch sites (launch_decode_attn, the raw <<<>>> sites of
the split-KV, parts, verify and fused forms, the two ivlm_launch pairs of the prefix form) were made to record their kernel
instantiation, grid and block under a dry-run flag instead of launching, its fused form took the CU count from the query, and its
positional internal functions were called behind the same ivlm_llama_decode_attn_query signature; this script ran against that
library.  tests/test_decode_attn_args_cpu.py replays the same rows through this tree's query and requires equality, record for
record - but for the rows of LONE_TABLE below, the one intended change (every form now rejects a lone cos / sin table).  Regenerating
the file from the current library only makes the test vacuous: do that for an INTENDED change, and say so in the change.

The sweep slices hold one record per call of shape_cases(), in its order, without trailing zeros.  A record is 14 ints: the return
code, the number of launches, then (kernel, flags, grid.x, grid.y, block, partials offset) twice, see ivlm_hip.h.  No GPU is needed:
nothing is launched.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "decode_attn_routes.json")

FORMS = ("one_block", "batched", "split_kv", "parts", "prefix", "verify", "fused")
ONE, BATCHED, SPLIT_KV, PARTS, PREFIX, VERIFY, FUSED = range(7)
PTRS = ("qkv", "kcache", "vcache", "o", "pos_dev", "prefix_len", "kcache_lo", "vcache_lo", "cos", "sin", "scratch", "wo", "x", "x_out",
        "step", "counter", "status")  # bit i of `present`, in the order ivlm_hip.h documents
F32, BF16 = 0, 1  # IVLM_F32, IVLM_BF16
INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4

# the pointers a form requires besides the tables (pos_dev: optional for the forms that take a host position)
NEEDS = {
    ONE: ("qkv", "kcache", "vcache", "o"), BATCHED: ("qkv", "kcache", "vcache", "o", "pos_dev"),
    SPLIT_KV: ("qkv", "kcache", "vcache", "o", "scratch"), PARTS: ("qkv", "kcache", "vcache", "scratch"),
    PREFIX: ("qkv", "kcache", "vcache", "o", "pos_dev", "prefix_len", "scratch"), VERIFY: ("qkv", "kcache", "vcache", "o", "pos_dev"),
    FUSED: ("qkv", "kcache", "vcache", "pos_dev", "scratch", "wo", "x", "x_out", "step", "counter", "status"),
}
HOST_POS = (ONE, SPLIT_KV, PARTS)
STRIDED = (BATCHED, PREFIX)
# (io, cache) kinds the entry points of a form admit; "hilo" = hi + lo bf16 planes
KINDS = {
    ONE: (("bf16", "bf16"), ("f32", "bf16"), ("f32", "f16"), ("f32", "hilo")),
    BATCHED: (("bf16", "bf16"), ("f32", "bf16"), ("f32", "f16"), ("f32", "hilo")),
    SPLIT_KV: (("f32", "bf16"), ("f32", "f16")), PARTS: (("f32", "bf16"), ("f32", "f16")),
    PREFIX: (("bf16", "bf16"), ("f32", "bf16"), ("f32", "f16")), VERIFY: (("f32", "bf16"), ("f32", "f16")), FUSED: (("f32", "bf16"),),
}

HS = (1, 3, 32, 40, 256, 65536)
DS = (0, 8, 16, 24, 80, 128, 144)
BS = (0, 1, 16, 17, 65535, 65536)
TMAXS = (0, 1, 4096, 5000)
FUSED_HD = ((4, 128), (8, 128), (12, 128), (32, 128), (40, 128), (64, 128), (68, 128), (32, 16), (64, 16))  # hidden 512 .. 8704
CUS = (16, 160, 256)


def load(path=None):
    lib = C.CDLL(path or os.path.join(os.path.dirname(os.path.dirname(HERE)), "interactvlm_amd", "libivlm_hip.so"))
    i, q, p = C.c_int, C.c_int64, C.c_void_p
    lib.ivlm_llama_decode_attn_query.argtypes = [i, i, i, q, q, q, i, i, i, i, i, i, i, q, i, p]
    lib.ivlm_llama_decode_attn_splitkv_scratch_bytes.restype = C.c_size_t
    lib.ivlm_llama_decode_attn_splitkv_scratch_bytes.argtypes = [i, i]
    lib.ivlm_llama_decode_attn_batch_prefix_scratch_bytes.restype = C.c_size_t
    lib.ivlm_llama_decode_attn_batch_prefix_scratch_bytes.argtypes = [i, i, i]
    for h in ("ivlm_llama_decode_attn_splits", "ivlm_decode_parts_tuning"):
        getattr(lib, h).argtypes = [i]
    return lib


def spec(form, io="f32", cache="bf16", H=32, D=128, B=None, tmax=4096, pos=None, null=(), tables="both", ldq_d=0, ldo_d=0, cs_d=0,
         cs_rows=None, scratch_d=0, skew=0, cus=256):
    """One described call.  pos None = a device position; null: names of PTRS withheld; tables: both | none | cos | sin; ldq_d / ldo_d /
    cs_d: elements added to the natural strides 3*H*D / H*D / cs_rows*H*D (cs_rows None = tmax); scratch_d: bytes added to the size
    the form asks for."""
    if B is None:
        B = {BATCHED: 3, PREFIX: 3, VERIFY: 4}.get(form, 1)
    return dict(form=form, io=io, cache=cache, H=H, D=D, B=B, tmax=tmax, pos=pos, null=tuple(null), tables=tables, ldq_d=ldq_d,
                ldo_d=ldo_d, cs_d=cs_d, cs_rows=cs_rows, scratch_d=scratch_d, skew=skew, cus=cus)


def call(lib, s):
    """-> the 15 leading arguments of ivlm_llama_decode_attn_query"""
    form, H, D, B, tmax = s["form"], s["H"], s["D"], s["B"], s["tmax"]
    names = set(NEEDS[form])
    if s["pos"] is None:
        names.add("pos_dev")
    if s["cache"] == "hilo":
        names |= {"kcache_lo", "vcache_lo"}
    names |= {"both": {"cos", "sin"}, "none": set(), "cos": {"cos"}, "sin": {"sin"}}[s["tables"]]
    names -= set(s["null"])
    present = sum(1 << PTRS.index(n) for n in names)
    hd = H * D
    strided = form in STRIDED
    ldq, ldo = (3 * hd + s["ldq_d"], hd + s["ldo_d"]) if strided else (0, 0)
    cstride = (tmax if s["cs_rows"] is None else s["cs_rows"]) * hd + s["cs_d"] if strided else 0
    need = 0
    if form == SPLIT_KV:
        need = lib.ivlm_llama_decode_attn_splitkv_scratch_bytes(H, D)
    elif form == PREFIX:
        need = lib.ivlm_llama_decode_attn_batch_prefix_scratch_bytes(B, H, D)
    return (form, F32 if s["io"] == "f32" else BF16, int(s["cache"] == "f16"), ldq, ldo, cstride, tmax, B, H, D,
            0 if s["pos"] is None else s["pos"], present, s["skew"], max(0, need + s["scratch_d"]), s["cus"])


_rec = (C.c_int32 * 14)()


def query(lib, c):
    assert lib.ivlm_llama_decode_attn_query(*c, _rec) == 0, c
    return list(_rec)


def positions(tmax):
    return (None, -1, 0, tmax - 1, tmax, 4096)


def shape_cases(form, io, cache):
    """the cartesian sweep of one (form, io, cache): H x D x B / k x tmax x position, natural strides, the scratch the form asks for"""
    bs = BS if form in (BATCHED, PREFIX, VERIFY) else (1,)
    for H, D, B, tmax in itertools.product(HS, DS, bs, TMAXS):
        for pos in (positions(tmax) if form in HOST_POS else (None,)):
            yield spec(form, io, cache, H=H, D=D, B=B, tmax=tmax, pos=pos)


def trimmed(rec):
    """a record without its trailing zeros (a rejected call is [rc])"""
    n = len(rec)
    while n > 1 and rec[n - 1] == 0:
        n -= 1
    return rec[:n]


def shape_rows(lib, form, io, cache):
    """-> [(call, trimmed record)] of the sweep of one (form, io, cache)"""
    return [(c, trimmed(query(lib, c))) for c in (call(lib, s) for s in shape_cases(form, io, cache))]


# ---- the rules of each form as single violations: (return-code class, name, changes to a valid spec) ------------------------------------
def violations(form):
    v = [(INVALID, "null " + n, dict(null=(n,))) for n in NEEDS[form]]
    v += [(INVALID, "H=0", dict(H=0)), (INVALID, "D=0", dict(D=0))]
    if form in HOST_POS:
        v += [(INVALID, "pos=tmax", dict(pos=4096)), (INVALID, "pos=-1", dict(pos=-1))]
    if form in (BATCHED, PREFIX, VERIFY):
        v += [(INVALID, "B=0", dict(B=0))]
    if form == BATCHED:
        v += [(INVALID, "B=65536", dict(B=65536))]
    if form == VERIFY:
        v += [(INVALID, "k=17", dict(B=17))]
    if form in STRIDED:
        v += [(INVALID, "ldq short", dict(ldq_d=-8)), (INVALID, "ldo misaligned", dict(ldo_d=4)), (INVALID, "slab short", dict(cs_d=-8))]
    if form == PARTS:
        v += [(INVALID, "parts misaligned", dict(skew=8))]
    if form == PREFIX:
        v += [(INVALID, "H=65536", dict(H=65536)), (UNSUPPORTED, "io bf16", dict(io="bf16")), (UNSUPPORTED, "D=144", dict(D=144)),
              (UNSUPPORTED, "D=24", dict(D=24)), (UNSUPPORTED, "B=17", dict(B=17)), (INVALID, "lone cos", dict(tables="cos"))]
    elif form == FUSED:
        v += [(INVALID, "D=144", dict(D=144)), (UNSUPPORTED, "hidden=1536", dict(H=12)), (UNSUPPORTED, "hidden=8704", dict(H=68)),
              (UNSUPPORTED, "tmax=0", dict(tmax=0)), (UNSUPPORTED, "cus=16", dict(cus=16))]
    else:
        v += [(INVALID, "D=144", dict(D=144)), (INVALID, "D=24", dict(D=24)), (INVALID, "tmax=0", dict(tmax=0))]
    if form == VERIFY:
        v += [(INVALID, "lone sin", dict(tables="sin"))]
    if form in (SPLIT_KV, PREFIX):
        v += [(WORKSPACE, "scratch one byte short", dict(scratch_d=-1)), (WORKSPACE, "scratch misaligned", dict(skew=8))]
    return v


# the forms whose parent launched a kernel that read the missing table: now IVLM_ERR_INVALID_ARG (the prefix and verify forms always were)
LONE_TABLE = [spec(form, io, cache, tables=t) for form in range(7) for io, cache in KINDS[form] for t in ("cos", "sin")
              if (form, io) != (PREFIX, "bf16")]  # (otherwise valid calls only: the prefix form has no bf16 I/O)


def explicit_cases():
    """(splits hook, parts hook, spec)"""
    for form in range(7):
        for io, cache in KINDS[form]:
            yield 8, 4, spec(form, io, cache)                  # the valid call of every kind
            yield 8, 4, spec(form, io, cache, tables="none")   # ... computing cos / sin itself
            yield 8, 4, spec(form, io, cache, H=3, D=16, tmax=5000)
        # every single violation, then every pair of different return-code classes (changes of the same member do not combine)
        vs = violations(form)
        for _, _, ch in vs:
            yield 8, 4, spec(form, **ch)
        for (ca, _, a), (cb, _, b) in itertools.combinations(vs, 2):
            if ca != cb and not set(a) & set(b):
                yield 8, 4, spec(form, **a, **b)
    # cache kinds no entry point offers, through the one-block and batched forms that carry the flags
    for form in (ONE, BATCHED):
        yield 8, 4, spec(form, "bf16", "f16")
        yield 8, 4, spec(form, "bf16", "hilo")
        yield 8, 4, spec(form, "f32", "hilo", null=("kcache_lo",))
        yield 8, 4, spec(form, "f32", "hilo", null=("vcache_lo",))
    # strides at, below and 8-misaligned around H*D and 3*H*D; tmax*H*D at and one above the slab stride
    for form in STRIDED:
        for d in (0, -8, -4, 4, 8):
            yield 8, 4, spec(form, ldq_d=d)
            yield 8, 4, spec(form, ldo_d=d)
            yield 8, 4, spec(form, cs_d=d)
            yield 8, 4, spec(form, cs_rows=1, cs_d=d, tmax=1)
        yield 8, 4, spec(form, tmax=4096, cs_rows=4095, cs_d=128 * 32 - 8)  # tmax*H*D one row of 8 above the stride
        yield 8, 4, spec(form, tmax=4096, cs_rows=4097)
    # scratch: null, one byte short, exact, generous, 8-misaligned, 16-aligned
    for form in (SPLIT_KV, PARTS, PREFIX, FUSED):
        for H, D in ((32, 128), (40, 128), (3, 16), (256, 16)):
            if form == FUSED and H * D not in (512, 4096, 5120):
                continue
            yield 8, 4, spec(form, H=H, D=D, null=("scratch",))
            for d in (-1, 0, 1, 4096):
                yield 8, 4, spec(form, H=H, D=D, scratch_d=d)
            for skew in (8, 16, 4):
                yield 8, 4, spec(form, H=H, D=D, skew=skew, scratch_d=64)
    # the key ranges of the split-KV and parts forms
    for splits in (1, 3, 8, 16):
        for H, D in ((1, 16), (32, 128), (40, 128), (256, 80)):
            for cache in ("bf16", "f16"):
                yield splits, 4, spec(SPLIT_KV, cache=cache, H=H, D=D)
    for S in (2, 4):
        for H, D in ((1, 16), (32, 128), (40, 128), (256, 80)):
            for cache in ("bf16", "f16"):
                yield 8, S, spec(PARTS, cache=cache, H=H, D=D)
    # the shared-prefix form's key ranges follow H
    for H in (1, 3, 16, 17, 32, 40, 128, 256, 257, 65535):
        for B in (1, 16):
            yield 8, 4, spec(PREFIX, H=H, D=16, B=B, tmax=64)
    # the fused form over its hidden sizes and CU counts
    for H, D in FUSED_HD:
        for cus in CUS:
            yield 8, 4, spec(FUSED, H=H, D=D, cus=cus)
    for cus in (39, 40, 159, 160, 199, 200):  # the grids of hidden 512 / 1024 / 4096 / 5120 at and one below the CU count
        for H, D in ((4, 128), (8, 128), (32, 128), (40, 128), (32, 16)):
            yield 8, 4, spec(FUSED, H=H, D=D, cus=cus)
    for s in LONE_TABLE:
        yield 8, 4, s
    # a lone table next to an unsupported hidden size / CU count: the fused form reports UNSUPPORTED first
    yield 8, 4, spec(FUSED, H=12, tables="cos")
    yield 8, 4, spec(FUSED, cus=16, tables="sin")


def run(lib, hooks_specs):
    """-> (call, record) of every case; the two hooks are restored to their defaults"""
    try:
        for splits, parts, s in hooks_specs:
            assert lib.ivlm_llama_decode_attn_splits(splits) == 0 and lib.ivlm_decode_parts_tuning(parts) == 0
            c = call(lib, s)
            yield c, query(lib, c)
    finally:
        lib.ivlm_llama_decode_attn_splits(8)
        lib.ivlm_decode_parts_tuning(4)


def explicit_rows(lib):
    return [{"splits": sp, "parts": pt, "lone_table": s in LONE_TABLE, "case": list(c), "record": r}
            for (sp, pt, s), (c, r) in zip(explicit_cases(), run(lib, explicit_cases()))]


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    sweep = {f"{FORMS[form]}/{io}/{cache}": [r for _, r in shape_rows(lib, form, io, cache)] for form in range(7) for io, cache in KINDS[form]}
    total = sum(len(v) for v in sweep.values())
    rows = explicit_rows(lib)
    with open(OUT, "w") as f:  # (one explicit row / sweep slice per line)
        row = lambda v: json.dumps(v, separators=(",", ":"))
        f.write('{"record":%s,\n"explicit":[\n%s\n],\n"sweep":{\n%s\n}}\n' % (
            row(["rc", "launches", "kernel", "flags", "grid_x", "grid_y", "block", "part_off", "kernel2", "flags2", "grid_x2", "grid_y2",
                 "block2", "part_off2"]),
            ",\n".join(row(r) for r in rows), ",\n".join(f"{row(k)}:{row(v)}" for k, v in sweep.items())))
    print(f"{OUT}: {len(rows)} explicit rows, {len(sweep)} sweep slices of {total} calls")


if __name__ == "__main__":
    main()
