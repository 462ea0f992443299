"""One small case per row of the attention dispatch table (the comment above attn_route in csrc/attention.hip): every accepted route
computes its attention (against the fp64 reference of tests/_attn_ref.py, in units of the documented rounding, bounded by 2 x max /
1.5 x rms of the emulation like the edge tests), every refused one returns its status code before anything is launched.

B = 1, H = 2 unless the shape is the 64 x 64 grid (H = 1).  The rel-pos ARRAYS are random numbers (for bf16 operands: bf16 values,
the kernels carry them as bf16 operands), so the query count is free: 40 queries also against the 4096 keys of the 64 x 64 grid.
The arrays-64 form is tested on that grid and not on a 2 x 64 key grid: the kernel stages 64 rel_h values per query whatever
rel_kh is, and would read past the end of a [.., 2] array.

What this file shows, and what it does not.  Every accepted route computes attention to the bound of the single-operand kernels,
and every refused one is refused with its code.  It does NOT show which instantiation ran: the split cases are held to bf16
rounding units, about 100 x looser than the split kernels' own accuracy (the edge tests hold those to 3e-5 against fp64), and the
lo planes here are zeros - a split route that landed on a single-operand kernel, or an exact-q case at another QLV, would give the
same numbers.  Which kernel a route reaches is checked by comparing a kernel trace of this file between two builds, and by the
edge tests' probes.

The route's own lo-plane rules (bf16: all four planes or none; fp16: q_lo only) cannot be reached through the C ABI: no entry point
passes f16 together with k_lo, and ivlm_attention_bf16_split refuses a missing plane itself before the route is asked.  The
"split call that lacks a lo plane" case below therefore tests the entry point, not the route; "fp16 with k_lo" has no case."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attn_ref as R  # noqa: E402
from _attn_gpu import BF, F16, MODES, _assert_margin, _attend, _attend_split, _cat_table, _mid, _packed, block_shape  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID_ARG = -4, -1
B, H, S = 1, 2, 40


# ---- accepted: no rel-pos --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("D", [16, 32, 64, 80, 128])
def test_plain_routes(hip_lib, cuda, mode, causal, D):
    rt, pp = mode
    case = (B, H, S, S, D, causal, 0)
    q, k, v, scale, o, wabs, emu = R.random_case(case, rt)
    with block_shape(pp):
        got = _attend(q, k, v, rt, cuda, scale, causal=causal)
    _assert_margin(got, o, wabs, emu, rt, f"{_mid(mode)} {case}")


# ---- accepted: rel-pos terms as arrays ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _array_case(KH, KW, Sq, rt, exact_scale=False):
    """Random q [B,H,Sq,80], k / v [B,H,KH*KW,80], rel_h [B*H,Sq,KH], rel_w [B*H,Sq,KW] (fp32; bf16 values for bf16 operands), the
    fp64 reference with the bias rel_h[q, ky] + rel_w[q, kx] and the emulation's figures.  exact_scale: q * scale is not rounded
    (the split kernels scale hi + lo in fp32)."""
    g = torch.Generator().manual_seed(KH * 100 + KW + Sq)
    D, Sk = 80, KH * KW
    q = torch.randn(B, H, Sq, D, generator=g).to(rt)
    k = torch.randn(B, H, Sk, D, generator=g).to(rt)
    v = torch.randn(B, H, Sk, D, generator=g).to(rt)
    rel_h = torch.randn(B * H, Sq, KH, generator=g)
    rel_w = torch.randn(B * H, Sq, KW, generator=g)
    if rt == BF:
        rel_h, rel_w = rel_h.to(BF).float(), rel_w.to(BF).float()
    bias = (rel_h.double()[..., :, None] + rel_w.double()[..., None, :]).reshape(B, H, Sq, Sk)
    scale, pre = D ** -0.5, (None if exact_scale else rt)
    o, wabs = R.ref64(q, k, v, scale, bias=bias, prescale_rt=pre)
    emu = R.ratio_stats(R.emulate(q, k, v, scale, bias=bias, prescale_rt=pre, rt=rt), o, wabs, rt)
    return q, k, v, rel_h, rel_w, scale, o, wabs, emu


ARRAY_FORMS = [  # KH, KW, Sq
    pytest.param(9, 9, 81, id="small-9x9"),        # REL 1
    pytest.param(4, 4, 16, id="small-4x4"),        # REL 1
    pytest.param(14, 14, 196, id="small-14x14"),   # REL 1 (split: the whole-window kernel)
    pytest.param(20, 20, S, id="generic-20x20"),   # REL 3
    pytest.param(64, 64, S, id="arrays64-64x64"),  # REL 2
]


@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("KH,KW,Sq", ARRAY_FORMS)
def test_array_routes(hip_lib, cuda, mode, KH, KW, Sq):
    rt, pp = mode
    q, k, v, rel_h, rel_w, scale, o, wabs, emu = _array_case(KH, KW, Sq, rt)
    with block_shape(pp):
        got = _attend(q, k, v, rt, cuda, scale, rel=(rel_h.to(cuda), rel_w.to(cuda)))
    _assert_margin(got, o, wabs, emu, rt, f"{_mid(mode)} arrays {KH} x {KW}, {Sq} queries")


def test_f16_exact_q_arrays_routes(hip_lib, cuda):
    """A (zero) lo half of q with the terms as arrays: level 1 on any array form (the plain kernel), level 2 on arrays-64."""
    for KH, KW, level in ((9, 9, 1), (64, 64, 1), (64, 64, 2)):
        q, k, v, rel_h, rel_w, scale, o, wabs, emu = _array_case(KH, KW, 81 if KH == 9 else S, F16)
        got = _attend(q, k, v, F16, cuda, scale, rel=(rel_h.to(cuda), rel_w.to(cuda)), q_lo=True, q_lo_level=level)
        _assert_margin(got, o, wabs, emu, F16, f"f16 exact q level {level}, arrays {KH} x {KW}")


# ---- accepted: rel-pos terms from the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("side", [4, 14])
def test_window_table_routes(hip_lib, cuda, mode, side):
    """Side 14: the whole-window kernel; side 4: the flash kernel (ping-pong is dropped for it, not refused)."""
    rt, pp = mode
    q, k, v, tab_h, tab_w, scale, o, wabs, emu, _ = R.sam_random_case(side, B, H, rt)
    with block_shape(pp):
        got = _attend(q, k, v, rt, cuda, scale, rel_tab=(_cat_table(tab_h, tab_w, cuda), side))
    _assert_margin(got, o, wabs, emu, rt, f"{_mid(mode)} window {side} x {side}, table mode")


@pytest.mark.parametrize("rt,q_lo", [(BF, False), (F16, False), (F16, True)], ids=["bf16", "f16", "f16-exact-q-level-1"])
def test_grid_table_routes(hip_lib, cuda, rt, q_lo):
    q, k, v, tab_h, tab_w, scale, o, wabs, emu, _ = R.sam_random_case(64, 1, 1, rt)
    kw = dict(q_lo=True, q_lo_level=1) if q_lo else {}
    got = _attend(q, k, v, rt, cuda, scale, rel_tab=(_cat_table(tab_h, tab_w, cuda), 64), **kw)
    _assert_margin(got, o, wabs, emu, rt, "64 x 64 grid, table mode")


# ---- accepted: split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,causal", [(128, True), (64, False)], ids=["D128-causal", "D64-plain"])
def test_split_plain_routes(hip_lib, cuda, D, causal):
    q, k, v, scale, o, wabs, emu = R.random_case((B, H, S, S, D, causal, 0), BF)
    got = _attend_split(q, k, v, cuda, scale, causal=causal)
    _assert_margin(got, o, wabs, emu, BF, f"split D {D} causal {causal}")


@pytest.mark.parametrize("KH,KW,Sq", ARRAY_FORMS)
def test_split_array_routes(hip_lib, cuda, KH, KW, Sq):
    q, k, v, rel_h, rel_w, scale, o, wabs, emu = _array_case(KH, KW, Sq, BF, exact_scale=True)
    got = _attend_split(q, k, v, cuda, scale, rel=(rel_h.to(cuda), rel_w.to(cuda)))
    _assert_margin(got, o, wabs, emu, BF, f"split arrays {KH} x {KW}, {Sq} queries")


@pytest.mark.parametrize("side", [4, 14])
def test_split_window_table_routes(hip_lib, cuda, side):
    """Table mode of the split flash kernel (the whole-window split kernel takes arrays only).  bf16 tables, exact q * scale."""
    q, k, v, tab_h, tab_w, scale, _, _, _, _ = R.sam_random_case(side, B, H, BF)
    rel_h, rel_w = R.relpos_terms64(q, tab_h, tab_w, side)
    bias = (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, H, side * side, side * side)
    o, wabs = R.ref64(q, k, v, scale, bias=bias)
    emu = R.ratio_stats(R.emulate(q, k, v, scale, bias=bias, rt=BF), o, wabs, BF)
    t64 = torch.zeros(64, 80, dtype=BF)
    t64[: 2 * side - 1], t64[2 * side - 1: 4 * side - 2] = tab_h, tab_w
    got = _attend_split(q, k, v, cuda, scale, rel_tab=(t64.to(cuda), side))
    _assert_margin(got, o, wabs, emu, BF, f"split window {side} x {side}, table mode")


# ---- refused -----------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *args, **kw):
    from interactvlm_amd import ops

    with pytest.raises(ops.IvlmError) as e:
        fn(*args, **kw)
    assert f"({code})" in str(e.value), f"expected status {code}: {e.value}"


def _rand(Sq, Sk, D, rt, Hn=H):
    g = torch.Generator().manual_seed(Sq + Sk + D)
    return (torch.randn(B, Hn, n, D, generator=g).to(rt) for n in (Sq, Sk, Sk))


def _arrays(KH, KW, Sq, dev, Hn=H):
    return torch.zeros(B * Hn, Sq, KH, device=dev), torch.zeros(B * Hn, Sq, KW, device=dev)


def test_refused_single_operand_routes(hip_lib, cuda):
    q, k, v = _rand(81, 81, 80, BF)
    _refused(UNSUPPORTED, _attend, q, k, v, BF, cuda, 1.0, rel=_arrays(9, 9, 81, cuda), causal=True)  # causal with rel-pos
    q, k, v = _rand(81, 81, 64, BF)
    _refused(UNSUPPORTED, _attend, q, k, v, BF, cuda, 1.0, rel=_arrays(9, 9, 81, cuda))  # rel-pos at D = 64
    q, k, v = _rand(4096, 4096, 80, BF, 1)
    with block_shape(1):  # the grid table has no ping-pong kernel
        _refused(UNSUPPORTED, _attend, q, k, v, BF, cuda, 1.0, rel_tab=(torch.zeros(256, 80, dtype=BF, device=cuda), 64))
    q, k, v = _rand(4096, 4096, 80, F16, 1)  # fp16 exact q at level 2: arrays-64 only
    _refused(UNSUPPORTED, _attend, q, k, v, F16, cuda, 1.0, rel_tab=(torch.zeros(256, 80, dtype=F16, device=cuda), 64), q_lo=True, q_lo_level=2)
    q, k, v = _rand(S, S, 80, F16)  # fp16 exact q without rel-pos
    _refused(UNSUPPORTED, _attend, q, k, v, F16, cuda, 1.0, q_lo=True, q_lo_level=1)


def test_refused_split_routes(hip_lib, cuda):
    for D, causal in ((32, False), (64, True), (128, False)):
        q, k, v = _rand(S, S, D, BF)
        _refused(UNSUPPORTED, _attend_split, q, k, v, cuda, 1.0, causal=causal)
    q, k, v = _rand(4096, 4096, 80, BF, 1)  # the split kernels take the grid's terms as arrays
    _refused(UNSUPPORTED, _attend_split, q, k, v, cuda, 1.0, rel_tab=(torch.zeros(64, 80, dtype=BF, device=cuda), 64))


def test_refused_through_the_c_entry_points(hip_lib, cuda):
    """What ops cannot express: rel-pos without prescale_q (refused by the route), and a split call that lacks a lo plane (refused by
    the entry point's own check, before the route)."""
    from interactvlm_amd import _lib, ops

    lib = _lib.load()
    q, k, v = (_packed(t, BF, cuda) for t in _rand(81, 81, 80, BF))
    out = torch.empty_like(q)
    rel_h, rel_w = _arrays(9, 9, 81, cuda)
    st = (ctypes.c_int64 * 12)(*(t.stride(i) for t in (q, k, v, out) for i in range(3)))
    stp = ctypes.cast(st, ctypes.c_void_p)
    dims = (B, H, 81, 81, 80, 1.0, 0, 0)  # B, H, Sq, Sk, D, scale, causal, q_pos0
    rel = (rel_h.data_ptr(), rel_w.data_ptr(), 9, 9, 1)  # rel_h, rel_w, kh, kw, kv_batch_div
    assert lib.ivlm_attention_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), stp, *dims, *rel, 0, ops._stream()) == UNSUPPORTED
    lo = torch.zeros_like(q)
    assert lib.ivlm_attention_bf16_split(q.data_ptr(), lo.data_ptr(), k.data_ptr(), None, v.data_ptr(), lo.data_ptr(), out.data_ptr(),
                                         lo.data_ptr(), stp, *dims, None, None, 0, 0, 1, 0, ops._stream()) == INVALID_ARG
