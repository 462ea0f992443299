"""The case table of tests/test_gemm_exact_gpu.py is what it claims (tests/_gemm_exact.py): every case stays inside the exactness budget,
reaches the kernel it names (ivlm_gemm_route_query: nothing is launched), and together the cases cover every kernel of the build with
both stores.  No GPU."""
import ctypes

import pytest
import torch

import _gemm_exact as G


@pytest.fixture(scope="module")
def lib():
    from interactvlm_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def built():
    """every case, built once (the reference of the column-split shape is computed on the device, not here)"""
    return {c.id: G.make_case(c, with_ref=c.group != "F") for c in G.cases()}


def test_every_case_is_inside_the_exactness_budget(built):
    """make_case asserts the budget (< 2^24 granules), hi + lo == x for split operands and that bias and residual are multiples of the
    granule; here: every group is present, and the reference of every exact case is an fp32 number."""
    groups = {c.group for c in G.cases()}
    assert groups == set("ABCDEF")
    for b in built.values():
        assert 0 < b.budget < 2 ** 24, b.case.id
        if b.case.vals == "act":  # pre-activations inside about +-8: both signs, zero and the tails
            assert float(b.z.min()) <= -6.0 and float(b.z.max()) >= 6.0 and float(b.z.abs().max()) <= 12.0 and bool((b.z == 0).any()), b.case.id
        if b.ref is not None and b.case.vals == "int":
            assert torch.equal(b.ref.float().double(), b.ref), b.case.id
            assert torch.equal(torch.round(b.ref / b.granule) * b.granule, b.ref), b.case.id


def test_every_case_reaches_the_kernel_it_names(lib, built):
    """(family, BM, BN, operand kind, fp32 epilogue, activation) of every launch the case's call makes under the case's hooks, against
    what the table names: a forced tile that falls back to another kernel fails HERE."""
    bad = []
    for b in built.values():
        got = G.route_records(lib, b.case, b.args)
        if got != b.case.expected_routes():
            bad.append((b.case.id, got, b.case.expected_routes()))
    assert not bad, bad[:5]
    assert lib.ivlm_gemm_tile_override(0) == 0  # (the hooks are back at their defaults)


# every kernel of the build (gemm_instantiated of csrc/gemm_route.h, written out): (family, BM, BN, operand kind 0 bf16 / 1 e4m3 / 2 fp16)
ALL_KERNELS = {
    (0, 128, 64, 0), (0, 128, 64, 1), (0, 128, 64, 2), (0, 128, 128, 0), (0, 128, 128, 1), (0, 128, 128, 2),
    (0, 128, 96, 0), (0, 176, 128, 0), (0, 176, 128, 2), (0, 256, 256, 0),
    (1, 256, 256, 0), (1, 256, 256, 1), (1, 256, 256, 2),
    (2, 256, 320, 0), (2, 256, 320, 2),
}


def test_the_cases_cover_every_kernel_with_both_stores(lib, built):
    """each kernel appears with the fp32 store and with the 16-bit store under ACT_NONE, in the exact groups"""
    seen = set()
    for b in built.values():
        if b.case.vals != "int":
            continue
        for r in G.route_records(lib, b.case, b.args):
            if r[0] in (0, 1, 2) and r[5] == 0:
                seen.add(r[:5])
    want = {k + (f32,) for k in ALL_KERNELS for f32 in (0, 1)}
    assert want <= seen, sorted(want - seen)
    assert {r[:4] for r in seen} == ALL_KERNELS  # (and nothing the list does not know)


def _query(lib, M, N, K, act, f32res, nsplit):
    buf = (ctypes.c_int32 * 72)()
    lib.ivlm_gemm_nsplit(nsplit)
    try:
        n = lib.ivlm_gemm_route_query(0, M, N, K, K, K, N, N, 0, 0, 0, act, 1, 1, 1, 0, 1, G.RES_F32 if f32res else 0, 0, 0, 0,
                                      ctypes.cast(buf, ctypes.c_void_p), 8)
    finally:
        lib.ivlm_gemm_nsplit(1)
    return [tuple(buf[9 * r:9 * r + 6]) for r in range(n)]


def test_the_column_split_case_splits(lib, built):
    """8192 x 2304 x 2048: 2048 columns on the 8-phase 256 x 256 kernel + a 256-column strip on 128 x 64 tiles; one launch without"""
    for c in G.cases_of("F"):
        got = G.route_records(lib, c, built[c.id].args)
        assert len(got) == 2 and got[0][:3] == (1, 256, 256) and got[1][:3] == (0, 128, 64), (c.id, got)
    M, N, K = G.F_SHAPE
    assert _query(lib, M, N, K, 0, True, 0) == [(1, 256, 256, 0, 1, 0)]
    assert _query(lib, M, N, K, 1, False, 1) == [(1, 256, 256, 0, 1, 1), (0, 128, 64, 0, 1, 1)]


def test_the_former_column_split_shapes_do_not_split(lib):
    """What the four shapes test_gemm_column_split_matches_unsplit used to run alone really launch: ONE kernel each, hook on or off
    (K < 2048, or whole rounds of 256 x 320 tiles) - which is why that test now also runs shapes that do split."""
    want = {(16384, 1280, 1280, 0, True): [(2, 256, 320, 0, 1, 0)], (16384, 1280, 5120, 0, True): [(2, 256, 320, 0, 1, 0)],
            (8192, 768, 512, 1, False): [(0, 128, 64, 0, 1, 1)], (4096, 1536, 256, 0, False): [(0, 128, 64, 0, 1, 0)]}
    for key, recs in want.items():
        assert _query(lib, *key, 1) == recs and _query(lib, *key, 0) == recs, key


def test_rejected_calls_return_their_code(lib):
    """host checks of gemm.hip this suite relies on: an e4m3 output needs N % 4 == 0 (the scalar tail of gemm_epilogue4 has no e4m3
    store: such a call used to be accepted and wrote 16-bit values into the byte matrix) and ldc % 4 == 0, SwiGLU needs N % 4 == 0,
    rows of 16-byte granules"""
    def rc(entry, M, N, K, lda, ldw, ldc, act, out_kind):
        buf = (ctypes.c_int32 * 72)()
        n = lib.ivlm_gemm_route_query(entry, M, N, K, lda, ldw, ldc, N, 0, 0, 0, act, out_kind, 0, 0, 0, 1, 0, 0, 0, 0,
                                      ctypes.cast(buf, ctypes.c_void_p), 8)
        assert n == 1
        return buf[1] if buf[0] == -1 else 0
    assert rc(2, 300, 328, 272, 272, 272, 338, 0, 2) == G.ERR_INVALID_ARG
    assert rc(2, 300, 328, 272, 272, 272, 336, 0, 2) == G.OK
    for N in (329, 330, 331):
        assert rc(2, 300, N, 272, 272, 272, 340, 0, 2) == G.ERR_UNSUPPORTED  # (fp32 and bf16 outputs of the same call are fine)
        assert rc(2, 300, N, 272, 272, 272, 340, 0, 0) == G.OK and rc(2, 300, N, 272, 272, 272, 340, 0, 1) == G.OK
    assert rc(0, 300, 330, 136, 136, 136, 170, G.ACT["swiglu"], 1) == G.ERR_UNSUPPORTED
    assert rc(0, 300, 328, 136, 140, 136, 336, 0, 1) == G.ERR_UNSUPPORTED
    assert rc(0, 300, 328, 136, 136, 136, 334, 0, 1) == G.OK  # ldc = 2 (mod 4) is legal: the direct epilogue takes it


def test_16_bit_activation_cases_stay_clear_of_rounding_ties(built):
    """A 16-bit (or e4m3) store of an activation may differ from the rounded float64 reference only where an fp32 error of the
    activation's bound moves the value across a rounding tie.  For the inputs of the table such elements are at most 0.1 % of any
    output (so the GPU test can cap them there)."""
    n = 0
    for b in built.values():
        c = b.case
        if c.vals == "int" or c.out not in ("16", "e4m3"):
            continue
        lo, hi = G.rounded_window(c, b.ref, G.ACT_BOUND[c.act])
        frac = float((lo != hi).double().mean())
        assert frac <= 1e-3, (c.id, frac)
        n += 1
    assert n > 20
