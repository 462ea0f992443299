"""The three fp32 attention kernels (csrc/attention_f32.hip) against the fp64 reference of tests/_attn_ref.py.

``attention_f32()`` picks the kernel from (D, Sk) alone:

| route (``_route``) | taken when | kernel |
|---|---|---|
| few   | D in {16, 32}, Sk <= 64 | ``attn_f32_fewkeys_kernel<4/8>``: thread per query, 256 queries per block, K / V of the (batch, head) in LDS |
| many  | D in {16, 32}, Sk > 64  | ``attn_f32_manykeys_kernel<4/8>``: wave per query, 4 waves per block, lanes stride the keys, butterfly merge |
| wide  | every other D % 4 == 0 up to 256 | ``attn_f32_wide_kernel``: wave per query, lane l owns channels 4l .. 4l+3 (D / 4 live lanes) |

Which case takes which route:

* key-tail probes (R.F32_KEY_TAIL): D 16 / 32 with Sk 1, 2, 9, 63, 64 -> few; Sk 65, 127, 128, 129, 200, 4096 -> many (lanes with 1, 63, 0,
  1 keys more than their neighbours; 64 keys per lane at 4096); D 48, 64, 80, 128, 256 (12, 16, 20, 32, 64 live lanes) -> wide;
* query-edge probes (R.F32_QUERY_EDGES): Sk 9 at D 16 / 32 -> few, Sq around the 256-query block; Sk 70 at D 16 / 32 -> many and Sk 4 at
  D 128 -> wide, with 1, 2 and 3 live waves in the last block;
* K/V broadcast (R.F32_KV_ROUTES): (Sk 9, D 16) few, (Sk 70, D 16) many, (Sk 4, D 128) wide;
* widths no probe can be built for (D % 16 != 0): D 4, 8, 20, 36, 252 -> wide with 1, 2, 5, 9, 63 live lanes; D 16 / 32 at Sk 64 -> few and
  at Sk 65 -> many on the same random values;
* score range: (D 16, Sk 64) few, (D 32, Sk 65) and (D 16, Sk 200) many, (D 128, Sk 9) wide; all-equal scores: D 16 at Sk 64 few, at Sk 65
  and 4096 many, D 32 at Sk 4096 many, D 128 at Sk 65 wide;
* host refusals: no route - every one returns before a launch.

Probe tests read off the output WHICH keys a kernel saw (tests/_attn_ref.py, probe_f32); with random values a dropped key or a key of
the wrong batch moves the output by about 1 / Sk, far inside any bound.  Every tensor is a view into a larger buffer of finite poison
with different strides for K and V, the output goes into a sentinel-filled buffer that must be untouched outside the logical region
(tests/_attn_gpu.py, _attend_f32).  Every probe and score-range case is launched twice: the results must be bit-identical (the file
header of attention_f32.hip promises a fixed-order merge)."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from _attn_gpu import SENTINEL, _attend_f32, _bh, _id  # noqa: E402

F32 = torch.float32


def _route(D, Sk):
    """attention_f32()'s choice, restated"""
    return "wide" if D not in (16, 32) else ("few" if Sk <= 64 else "many")


def _twice(*args, **kw):
    got = _attend_f32(*args, **kw)
    assert torch.equal(got, _attend_f32(*args, **kw)), "two launches on the same inputs differ"
    return got


def _check_probe(got, vt, o, vis, what):
    """got [B,H,Sq,D] (cpu): every (b, h) against the verdict of _attn_ref; prints the largest figures of the run."""
    worst = [0.0, float("inf"), 0.0]
    for b in range(got.shape[0]):
        for h in range(got.shape[1]):
            e = R.probe_errors_f32(got[b, h], vt, o, vis)
            worst = [max(worst[0], e[0] or 0.0), min(worst[1], float("inf") if e[1] is None else e[1]), max(worst[2], e[2] or 0.0)]
            bad = R.probe_verdict_f32(got[b, h], vt, o, vis)
            assert not bad, f"{what} (b {b}, h {h}): {bad}"
    print(f"\n[{what}] visible |got - V[target]| {worst[0]:.3g} (bound {R.VISIBLE_TOL_F32:.3g}); hidden: separation {worst[1]:.3g} "
          f"(>= {R.SEPARATION:.3g}), |got - fp64| {worst[2]:.3g} (bound {R.F32_TOL:.3g})")


# ---- a. key tails ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk,D", R.F32_KEY_TAIL)
def test_key_tail_probe(hip_lib, cuda, Sk, D):
    """Every key is seen by the query that targets it ("spread"), the LAST key by all of them ("last"), and a key one row past the end
    (its code and value sit in the first slack row of K and of V) by none ("ghost")."""
    B, H = 2, 3
    for name in R.key_tail_targets(Sk):
        q, k, v, ghost, scale, vt, o, vis = R.f32_probe_case(R.KEY_TAIL_SQ, Sk, D, name)
        got = _twice(_bh(q, B, H), _bh(k, B, H), _bh(v, B, H), cuda, scale, ghost=ghost)
        _check_probe(got, vt, o, vis, f"key tail '{name}' Sk {Sk} D {D} ({_route(D, Sk)})")


# ---- b. query edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.F32_QUERY_EDGES, ids=_id)
def test_query_edge_probe(hip_lib, cuda, case):
    """Every query row finds its own key (targets spread over the keys); nothing is written past row Sq - 1 or outside the D columns
    (_attend_f32 checks the sentinel buffer).  few: Sq around the 256-query block; many / wide: 1, 2, 3 live waves in the last block."""
    B, H, Sq, Sk, D = case
    q, k, v, _, scale, vt, o, vis = R.f32_probe_case(Sq, Sk, D, "edges")
    got = _attend_f32(_bh(q, B, H), _bh(k, B, H), _bh(v, B, H), cuda, scale)
    _check_probe(got, vt, o, vis, f"query edge {case} ({_route(D, Sk)})")


# ---- c. K/V broadcast ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roll", ["v", "k"])
@pytest.mark.parametrize("div", R.KV_DIVS)
@pytest.mark.parametrize("Sk,D", R.F32_KV_ROUTES)
def test_kv_broadcast_probe(hip_lib, cuda, Sk, D, div, roll):
    """4 query batches on 4 / div K/V batches that hold DIFFERENT value rows under the same keys ("v") or different key rows under the
    same values ("k"): query batch b must return the row of K/V batch b // div; any other batch's row is at least 1/16 away."""
    B, H = R.F32_KV_B, 2
    q, ks, vs, scale, want = R.f32_kv_case(Sk, D, roll)
    got = _attend_f32(_bh(q, B, H), ks.expand(B, H, Sk, D), vs.expand(B, H, Sk, D), cuda, scale, kv_batches=B // div)
    worst = 0.0
    for b in range(B):
        e = float((got[b].double() - want[b // div]).abs().max())
        worst = max(worst, e)
        assert e <= R.VISIBLE_TOL_F32, f"query batch {b} did not get K/V batch {b // div} ({_route(D, Sk)}, rolled {roll}): off by {e:.3g}"
    print(f"\n[kv broadcast Sk {Sk} D {D} div {div} roll {roll}] |got - V[target]| {worst:.3g} (bound {R.VISIBLE_TOL_F32:.3g})")


# ---- d. widths the code cannot probe -----------------------------------------------------------------------------------------------------
def _assert_f32_tol(got, o, what, tol=R.F32_TOL):
    e = float((got.double() - o).abs().max())
    print(f"\n[{what}] |got - fp64| {e:.3g} (bound {tol:.3g})")
    assert e <= tol, f"{what}: |got - fp64| = {e:.3g} > {tol:.3g}"


@pytest.mark.parametrize("Sk", [1, 5, 70])
@pytest.mark.parametrize("D", [4, 8, 20, 36, 252])
def test_odd_widths_random(hip_lib, cuda, D, Sk):
    """D / 4 = 1, 2, 5, 9, 63 live lanes of the wide kernel; 42 waves: the last block has two dead ones."""
    B, H, Sq = 2, 3, 7
    g = torch.Generator().manual_seed(100 * D + Sk)
    q, k, v = torch.randn(B, H, Sq, D, generator=g), torch.randn(B, H, Sk, D, generator=g), torch.randn(B, H, Sk, D, generator=g)
    scale = D ** -0.5
    _assert_f32_tol(_attend_f32(q, k, v, cuda, scale), R.ref64(q, k, v, scale)[0], f"random D {D} Sk {Sk} ({_route(D, Sk)})")


@pytest.mark.parametrize("D", [16, 32])
def test_route_boundary_random(hip_lib, cuda, D):
    """Sk = 64 (thread per query) and Sk = 65 (wave per query) on the same values: the 64-key case is the first 64 keys of the other."""
    B, H, Sq = 2, 3, 33
    g = torch.Generator().manual_seed(D)
    q, k, v = torch.randn(B, H, Sq, D, generator=g), torch.randn(B, H, 65, D, generator=g), torch.randn(B, H, 65, D, generator=g)
    scale = D ** -0.5
    for Sk in (64, 65):
        ks, vs = k[:, :, :Sk], v[:, :, :Sk]
        _assert_f32_tol(_attend_f32(q, ks, vs, cuda, scale), R.ref64(q, ks, vs, scale)[0], f"random D {D} Sk {Sk} ({_route(D, Sk)})")


# ---- e. score range ------------------------------------------------------------------------------------------------------------------------
SMAX = 80.0
RANGE_CASES = [(16, 64), (32, 65), (16, 200), (128, 9)]  # D, Sk: few, many, many, wide
QUERY_FACTORS = (1.0, -1.0, 0.5, 0.3, -0.7)  # a: the largest score sits on the peak key for a > 0, on the key farthest from it for a < 0


def _peaks(D, Sk):
    p = [0, Sk - 1, Sk // 2]
    return p + [j for j in (63, 64, 65) if _route(D, Sk) == "many" and j < Sk and j not in p]  # around the lanes' second key


_RANGE = [(D, Sk, p) for D, Sk in RANGE_CASES for p in _peaks(D, Sk)]


@pytest.mark.parametrize("D,Sk,peak", _RANGE)
def test_score_range(hip_lib, cuda, D, Sk, peak):
    """One-hot q (q[..., 0] = a) and k[j, 0] = t_j: the score of key j is a * t_j * scale, a tent over the keys with +80 at ``peak`` and
    -80 at the key farthest from it; the other columns of k are random and meet zeros of q.  v is randn.

    Bound: F32_TOL + 2^-22 * smax * max|v| with smax the largest |score| of the fp64 reference.  A one-hot q gives one product rounding
    (a * t_j; the other products are exact zeros) and one rounding of the multiplication by the scale: at most 2^-23 * smax per score.
    A ratio of two weights sees the difference of two scores, so twice that: every weight is off by a factor within
    exp(+-2^-22 * smax).  The output is a weighted mean of v, so it moves by at most that times max|v|."""
    B, H = 2, 2
    g = torch.Generator().manual_seed(1000 * D + 10 * Sk + peak)
    scale = D ** -0.5
    j = torch.arange(Sk, dtype=torch.float64)
    tent = 1.0 - 2.0 * (j - peak).abs() / max(peak, Sk - 1 - peak, 1)
    q = torch.zeros(B, H, len(QUERY_FACTORS), D)
    q[..., 0] = torch.tensor(QUERY_FACTORS)
    k = torch.randn(B, H, Sk, D, generator=g)
    k[..., 0] = (tent * SMAX / scale).float()
    v = torch.randn(B, H, Sk, D, generator=g)
    o = R.ref64(q, k, v, scale)[0]
    smax = float((torch.einsum("bhqd,bhkd->bhqk", q.double(), k.double()) * scale).abs().max())
    assert 0.99 * SMAX <= smax <= 1.01 * SMAX
    tol = R.F32_TOL + 2.0 ** -22 * smax * float(v.abs().max())
    _assert_f32_tol(_twice(q, k, v, cuda, scale), o, f"score range D {D} Sk {Sk} peak {peak} ({_route(D, Sk)})", tol)


@pytest.mark.parametrize("D,Sk", [(16, 64), (16, 65), (16, 4096), (32, 4096), (128, 65)])
def test_equal_scores_give_the_mean(hip_lib, cuda, D, Sk):
    """q = 0: every score is 0 and the output is the mean of V."""
    B, H, Sq = 2, 2, 5
    g = torch.Generator().manual_seed(D + Sk)
    q, k, v = torch.zeros(B, H, Sq, D), torch.randn(B, H, Sk, D, generator=g), torch.randn(B, H, Sk, D, generator=g)
    mean = v.double().mean(dim=2, keepdim=True).expand(B, H, Sq, D)
    _assert_f32_tol(_twice(q, k, v, cuda, D ** -0.5), mean, f"equal scores D {D} Sk {Sk} ({_route(D, Sk)})")


# ---- g. host refusals --------------------------------------------------------------------------------------------------------------------
def _err(name):
    from interactvlm_amd import _lib

    return int(re.search(rf"^#define[ \t]+IVLM_ERR_{name}[ \t]+\((-?\d+)\)", open(_lib.HEADER_PATH).read(), flags=re.M).group(1))


_B, _H, _SQ, _SK, _D = 4, 2, 5, 7, 16
_REFUSALS = [  # name, changed arguments, error
    ("D=0", dict(D=0), "UNSUPPORTED"), ("D=6", dict(D=6), "UNSUPPORTED"), ("D=260", dict(D=260), "UNSUPPORTED"),
    ("q row stride 34", dict(stride=(2, 34)), "INVALID_ARG"), ("v head stride 18", dict(stride=(7, 18)), "INVALID_ARG"),
    ("o batch stride 161", dict(stride=(9, 161)), "INVALID_ARG"),
    ("B % kv_div", dict(kv_div=3), "INVALID_ARG"), ("kv_div=0", dict(kv_div=0), "INVALID_ARG"),
    ("q NULL", dict(null=0), "INVALID_ARG"), ("k NULL", dict(null=1), "INVALID_ARG"), ("v NULL", dict(null=2), "INVALID_ARG"),
    ("o NULL", dict(null=3), "INVALID_ARG"), ("strides NULL", dict(null=4), "INVALID_ARG"),
    # a pointer 4 bytes into its buffer: the rows stay inside the allocation, but every kernel moves float4
    ("q + 4 bytes", dict(shift=0), "INVALID_ARG"), ("k + 4 bytes", dict(shift=1), "INVALID_ARG"),
    ("v + 4 bytes", dict(shift=2), "INVALID_ARG"), ("o + 4 bytes", dict(shift=3), "INVALID_ARG"),
]


@pytest.mark.parametrize("name,change,err", _REFUSALS, ids=[r[0] for r in _REFUSALS])
def test_host_refusals(hip_lib, cuda, name, change, err):
    """Through the C entry point: the documented error code, before any launch - the sentinel output stays as it was."""
    from interactvlm_amd import ops

    rows = max(_SQ, _SK) + 1  # (one row more than any tensor has: a shifted pointer's rows end inside the buffer)
    q, k, v = (torch.zeros(_B, rows, _H, 264, dtype=F32, device=cuda) for _ in range(3))
    out = torch.full((_B, rows, _H, 264), SENTINEL, dtype=F32, device=cuda)
    strides = [rows * _H * 264, 264, _H * 264] * 4  # batch, head, row of q, k, v, o
    if "stride" in change:
        strides[change["stride"][0]] = change["stride"][1]
    ptrs = [t.data_ptr() for t in (q, k, v, out)] + [None]
    st = (ctypes.c_int64 * 12)(*strides)
    ptrs[4] = ctypes.cast(st, ctypes.c_void_p)
    if "null" in change:
        ptrs[change["null"]] = None
    if "shift" in change:
        ptrs[change["shift"]] += 4
    rc = hip_lib.ivlm_attention_f32(*ptrs, _B, _H, _SQ, _SK, change.get("D", _D), 0.25, change.get("kv_div", 1), ops._stream())
    torch.cuda.synchronize()
    assert rc == _err(err), f"{name}: returned {rc}, documented {err} ({_err(err)})"
    assert bool((out == SENTINEL).all()), f"{name}: the output was written"
