"""The routing of the tile GEMM family and the split-K rule against tests/golden/gemm_routes.json, which was recorded from the
launchers of the commit before the host side was rewritten around gemm_route() (tests/golden/make_golden_gemm_routes.py says how).
Nothing is launched: ivlm_gemm_route_query records what a call would launch.  No GPU."""
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def sweep(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_gemm_routes", os.path.join(golden_dir, "make_golden_gemm_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from interactvlm_amd import _lib

    _lib.load()  # (the header's prototypes against the library: ivlm_gemm_route_query is declared there)
    return mod, mod.load(_lib.LIB_PATH), json.load(open(os.path.join(golden_dir, "gemm_routes.json")))


def test_explicit_routes_equal_the_recorded_ones(sweep):
    """The GEMMs of the three towers (bf16 / fp16 / fp8 operands; 16-bit, fp32 + residual and split forms) and every forced tile x
    operand kind x activation at 700 x 900 x 1096: kernel family, tile, operand / output kind, activation, grid and LDS bytes, or the
    return code of a rejected call, record for record."""
    mod, lib, gold = sweep
    rows = mod.explicit_rows(lib)
    assert len(rows) == len(gold["explicit"]) > 400
    for got, want in zip(rows, gold["explicit"]):
        assert got == want


def test_route_sweep_digests_equal_the_recorded_ones(sweep):
    """Every (operand kind, activation, forced tile) slice of the sweep over the decision boundaries (M, N, K, output kinds, residuals,
    split A, panels, batches, row maps, the nsplit / tile320 hooks, split-K through both entry points): one digest per slice."""
    mod, lib, gold = sweep
    assert len(gold["digests"]) == len(mod.OPKS) * len(mod.ACTS) * len(mod.TILES)
    bad = []
    for key, (n, digest) in gold["digests"].items():
        opk, act, tile = key.split("/")
        if mod.slice_digest(lib, opk, mod.ACTS.index(act), int(tile)) != (n, digest):
            bad.append(key)
    assert not bad, bad


def test_splitk_rule_equals_the_recorded_one(sweep):
    """ivlm_gemm_splitk_choice - which the C sequencers use and ops._splitk_choice asks - on the grid of the former Python-against-C
    comparison plus M = 128, 129, 352, 353 and N = 8192, against the values of the rule before it moved."""
    from interactvlm_amd import ops

    mod, lib, gold = sweep
    grid = mod.splitk_grid()
    assert len(grid) == len(gold["splitk_rule"])
    names = {code: name for name, code in ops.ACT.items()}
    for (M, N, K, act, rms), want in zip(grid, gold["splitk_rule"]):
        assert lib.ivlm_gemm_splitk_choice(M, N, K, act, rms) == want, (M, N, K, act, rms)
        assert ops._splitk_choice(M, N, K, names[act], (1, 1e-5) if rms else None) == want, (M, N, K, act, rms)
