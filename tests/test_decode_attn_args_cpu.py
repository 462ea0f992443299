"""The argument check and the routing of the decode-attention family against tests/golden/decode_attn_routes.json, which was recorded
from the launch sites of the commit before the host side was rewritten around DecodeAttnArgs / decode_attn_check / decode_attn
(tests/golden/make_golden_decode_attn.py says how).  Nothing is launched and no pointer reaches a launching entry point:
ivlm_llama_decode_attn_query records what a described call would return and launch.  No GPU."""
import importlib.util
import json
import os

import pytest

INVALID_ARG = -1


@pytest.fixture(scope="module")
def sweep(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_decode_attn", os.path.join(golden_dir, "make_golden_decode_attn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from interactvlm_amd import _lib

    _lib.load()  # (the header's prototypes against the library: the query and ivlm_llama_attn_oproj_fits are declared there)
    return mod, mod.load(_lib.LIB_PATH), json.load(open(os.path.join(golden_dir, "decode_attn_routes.json")))


def test_explicit_rows_equal_the_recorded_ones(sweep):
    """Every form x I/O x cache kind, every single violated rule and every pair from different return-code classes, the strides, the
    scratch (null, short, misaligned), each pointer withheld in turn, the key-range hooks and the fused form over hidden x CUs: return
    code, kernel, template flags, grid, block and partials offset, record for record.  The one exception is listed, not inferred: a call
    with exactly one of cos_tab / sin_tab, which every form now rejects (the parent launched five of the seven forms on it)."""
    mod, lib, gold = sweep
    rows = mod.explicit_rows(lib)
    assert len(rows) == len(gold["explicit"]) > 600
    lone = [mod.call(lib, s) for s in mod.LONE_TABLE]
    assert len(lone) == 34
    n_lone = 0
    for got, want in zip(rows, gold["explicit"]):
        assert got["case"] == want["case"] and (got["splits"], got["parts"]) == (want["splits"], want["parts"])
        if tuple(got["case"]) in lone and got["splits"] == 8 and got["parts"] == 4:
            assert want["lone_table"] and want["record"][0] in (0, INVALID_ARG)  # (the parent: launched, or rejected it already)
            assert got["record"] == [INVALID_ARG] + [0] * 13, got
            n_lone += 1
        else:
            assert got["record"] == want["record"], (got, want)
    assert n_lone >= len(lone)


def test_shape_sweep_equals_the_recorded_one(sweep):
    """H x D x B / k x tmax x host and device positions of every (form, I/O, cache kind), natural strides and the scratch the form asks
    for: one recorded row per call, compared row by row (a difference names the call)."""
    mod, lib, gold = sweep
    assert len(gold["sweep"]) == sum(len(k) for k in mod.KINDS.values())
    total = 0
    for key, want in gold["sweep"].items():
        form, io, cache = key.split("/")
        rows = mod.shape_rows(lib, mod.FORMS.index(form), io, cache)
        assert len(rows) == len(want), key
        for (case, got), w in zip(rows, want):
            assert got == w, (key, case, got, w)
        total += len(rows)
    assert total > 17000


def test_attn_oproj_fits_agrees_with_the_recorded_fused_rows(sweep):
    """ivlm_llama_attn_oproj_fits - what decode_step and llava._graph_key ask - says "fits" exactly where the parent's fused entry point
    launched on an otherwise valid call, and the hidden sizes outside {512, 1024, 4096, 5120} never fit."""
    from interactvlm_amd import _lib

    mod, _, gold = sweep
    fits = _lib.load().ivlm_llama_attn_oproj_fits
    valid = sum(1 << mod.PTRS.index(n) for n in mod.NEEDS[mod.FUSED] + ("cos", "sin"))
    seen = set()
    for row in gold["explicit"]:
        c = row["case"]
        if c[0] == mod.FUSED and c[11] == valid and c[6] > 0 and c[9] in (16, 128):  # (all pointers, tmax > 0, a D the form takes)
            H, D, cus = c[8], c[9], c[14]
            assert bool(fits(H, D, cus)) == (row["record"][0] == 0), row
            seen.add((H * D, bool(fits(H, D, cus))))
    assert {(h, False) for h in (512, 1024, 1536, 4096, 5120, 8192, 8704)} | {(h, True) for h in (512, 1024, 4096, 5120)} <= seen
    assert not fits(0, 128, 256) and not fits(32, 0, 256) and not fits(32, 128, 159) and fits(32, 128, 160)
