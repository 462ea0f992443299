"""Edge tests of attn_kernel / win_attn_kernel (csrc/attention.hip) against the fp64 reference of tests/_attn_ref.py.

Probe tests: exact "one key per query" inputs - the output row of a query IS the value row of its target key when the kernel sees
that key, and is at least 1/32 away from it when it must not: key tails of every length class, query-block edges of both block
shapes, the causal diagonal to the exact key for every row, K/V broadcast, the split kernels, SAM's windows and grid.  Every tensor
is a view into a larger buffer of finite poison (a neighbouring "head" of poison directly behind each head's D columns, slack rows
behind the last row), the output goes into a sentinel-filled buffer that must be untouched outside the logical region.

Random-value tests: the error against fp64 in units of the rounding the kernel is documented to do (ratio of _attn_ref), bounded by
2 x (max) and 1.5 x (rms) what a plain emulation of those roundings gives on the same inputs; tests/test_attn_ref_cpu.py caps the
emulation's own figures."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from _attn_gpu import (BF, F16, MODES, _assert_margin, _attend, _attend_split, _bh, _cat_table, _id, _mid,  # noqa: E402
                       block_shape)


class Probe:
    """One probe run on the CPU side (B = H = 1 is computed, every (b, h) of the GPU run holds the same values): inputs in the
    operand type, fp64 reference, emulation statistics of the hidden rows."""

    def __init__(self, Sq, Sk, D, target, visible, rt, causal=False, q_pos0=0, prescale=False):
        n = max(Sk, int(target.max()) + 1)
        q, k, v = R.probe(Sq, n, D, target)
        self.q, self.k, self.v = q.to(rt), k[:Sk].to(rt), v[:Sk].to(rt)
        self.ghost = (k[Sk], v[Sk]) if n > Sk else (None, None)  # the target's own key and value row, one row past the end
        self.vt, self.visible, self.rt = v[target], visible, rt
        self.scale, self.kw = D ** -0.5, dict(causal=causal, q_pos0=q_pos0)
        pre = rt if prescale else None
        b = lambda t: t[None, None]
        self.o, self.wabs = (t[0, 0] for t in R.ref64(b(self.q), b(self.k), b(self.v), self.scale, causal, q_pos0, prescale_rt=pre))
        hid = ~visible
        self.emu = None
        if hid.any():
            emu = R.emulate(b(self.q), b(self.k), b(self.v), self.scale, causal, q_pos0, prescale_rt=pre, rt=rt)[0, 0]
            self.emu = R.ratio_stats(emu[hid], self.o[hid], self.wabs[hid], rt)

    def check(self, got, what):
        """got [B,H,Sq,D] (cpu)."""
        for b in range(got.shape[0]):
            for h in range(got.shape[1]):
                bad = R.probe_verdict(got[b, h], self.vt, self.o, self.wabs, self.visible, self.rt, self.emu)
                assert not bad, f"{what} (b {b}, h {h}): {bad}"

    def check_split(self, got, what):
        """hi + lo carries 2^-17 relative: a visible target to 2^-16 (its weight is within 2e-6 of 1), hidden rows to the split
        kernels' 3e-5 against fp64 and, as ever, not within 1/32 of the target's row."""
        for b in range(got.shape[0]):
            for h in range(got.shape[1]):
                d = (got[b, h] - self.vt).abs()
                if self.visible.any():
                    assert float(d[self.visible].max()) <= 2.0 ** -16, f"{what} (b {b}, h {h}): visible target missed"
                hid = ~self.visible
                if hid.any():
                    assert float(d[hid].amax(dim=-1).min()) >= R.SEPARATION, f"{what} (b {b}, h {h}): hidden target seen"
                    assert float((got[b, h][hid] - self.o[hid]).abs().max()) <= 3e-5, f"{what} (b {b}, h {h}): hidden rows off fp64"


# ---- probes: plain and causal attention ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("Sk,D", R.KEY_TAIL)
def test_key_tail_probe(hip_lib, cuda, mode, Sk, D):
    """Sk % 64 in every class (1, 15, 16, 17, 63, 0, 1 again past a tile, ...): every key is seen by the query that targets it, the
    LAST key by all of them, and a key one row past the end (its code and value sit in the slack row) by none."""
    rt, pp = mode
    B, H = 2, 3
    with block_shape(pp):
        for name, (target, vis) in R.key_tail_targets(Sk).items():
            p = Probe(R.KEY_TAIL_SQ, Sk, D, target, torch.full((R.KEY_TAIL_SQ,), vis), rt)
            got = _attend(_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), rt, cuda, p.scale, ghost=p.ghost)
            p.check(got, f"key tail '{name}' Sk {Sk} D {D}")


@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("Sq", R.QUERY_EDGES)
def test_query_edge_probe(hip_lib, cuda, mode, Sq):
    """Sq around the 128 / 256 query-block edges of both block shapes: every query row finds its own key (targets over all 70 keys),
    nothing is written past row Sq - 1."""
    rt, pp = mode
    with block_shape(pp):
        for D, B, H in ((64, 1, 2), (80, 2, 1)):
            target = R.spread_targets(Sq, R.QUERY_EDGES_SK)
            p = Probe(Sq, R.QUERY_EDGES_SK, D, target, torch.ones(Sq, dtype=torch.bool), rt)
            got = _attend(_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), rt, cuda, p.scale)
            p.check(got, f"query edge Sq {Sq} D {D}")


@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("shape,D", R.CAUSAL, ids=_id)
def test_causal_diagonal_probe(hip_lib, cuda, mode, shape, D):
    """Run A: every query targets its diagonal key i + q_pos0 (the last visible one: must be seen); run B: the key after it (the
    first hidden one: must not be seen).  Together they pin the mask to the exact key for every row and tile alignment."""
    rt, pp = mode
    Sq, Sk, q_pos0 = shape
    B, H = 1, 2
    with block_shape(pp):
        for name, (target, vis) in R.causal_targets(Sq, Sk, q_pos0).items():
            p = Probe(Sq, Sk, D, target, vis, rt, causal=True, q_pos0=q_pos0)
            got = _attend(_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), rt, cuda, p.scale, **p.kw)
            p.check(got, f"causal '{name}' {shape} D {D}")


@pytest.mark.parametrize("mode", MODES, ids=_mid)
@pytest.mark.parametrize("div", R.KV_DIVS)
def test_kv_broadcast_probe(hip_lib, cuda, mode, div):
    """B = 2 * div query batches on 2 K/V batches that hold DIFFERENT value rows: a wrong K/V batch index returns another row."""
    rt, pp = mode
    B, H, Sq, Sk, D = 2 * div, 2, 33, 70, 64
    target = R.spread_targets(Sq, Sk)
    q, k, v = R.probe(Sq, Sk, D, target)
    vs = R.kv_batches(v, 2).expand(2, H, Sk, D)
    with block_shape(pp):
        got = _attend(_bh(q, B, H), _bh(k, 2, H), vs, rt, cuda, D ** -0.5)
    for b in range(B):
        assert float((got[b].double() - vs[b // div][:, target]).abs().max()) <= R.VISIBLE_TOL[rt], f"query batch {b}: K/V batch {b // div}"


@pytest.mark.parametrize("Sk", [sk for sk, d in R.KEY_TAIL if d == 64])
def test_split_key_tail_probe(hip_lib, cuda, Sk):
    D, B, H = 64, 2, 2
    for name, (target, vis) in R.key_tail_targets(Sk).items():
        p = Probe(R.KEY_TAIL_SQ, Sk, D, target, torch.full((R.KEY_TAIL_SQ,), vis), BF)
        got = _attend_split(_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), cuda, p.scale, ghost=p.ghost)
        p.check_split(got, f"split key tail '{name}' Sk {Sk}")


@pytest.mark.parametrize("shape", R.CAUSAL_SHAPES, ids=_id)
def test_split_causal_probe(hip_lib, cuda, shape):
    Sq, Sk, q_pos0 = shape
    D, B, H = 128, 1, 2
    for name, (target, vis) in R.causal_targets(Sq, Sk, q_pos0).items():
        p = Probe(Sq, Sk, D, target, vis, BF, causal=True, q_pos0=q_pos0)
        got = _attend_split(_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), cuda, p.scale, **p.kw)
        p.check_split(got, f"split causal '{name}' {shape}")


# ---- probes: SAM shapes (D = 80, q * scale rounded to the operand type, zero rel-pos tables: the bias is exactly 0) -------------------
def _zero_table(rows, rt, dev):
    return torch.zeros(rows, 80, dtype=rt, device=dev)


@pytest.mark.parametrize("rt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("side", R.WINDOW_SIDES)
def test_sam_window_probe(hip_lib, cuda, rt, side):
    """Windows of side 14, 9 and 4 in table mode on the whole-window kernel and on the generic kernel; fp16 also with a zero lo half
    of q at levels 1 and 2 (whole-window kernel)."""
    from interactvlm_amd import _lib, ops

    lib = _lib.load()
    S, B, H = side * side, 3, 2
    p = Probe(S, S, 80, R.spread_targets(S, S), torch.ones(S, dtype=torch.bool), rt, prescale=True)
    args = (_bh(p.q, B, H), _bh(p.k, B, H), _bh(p.v, B, H), rt, cuda, p.scale)
    tab = (_zero_table(64, rt, cuda), side)
    try:
        for whole in (1, 0):
            lib.ivlm_attention_window_kernel(whole)
            p.check(_attend(*args, rel_tab=tab), f"SAM window side {side}, {'whole-window' if whole else 'generic'} kernel")
    finally:
        lib.ivlm_attention_window_kernel(1)
    if rt == F16:
        for level in (1, 2):
            if side == 14:
                p.check(_attend(*args, rel_tab=tab, q_lo=True, q_lo_level=level), f"SAM window side {side}, exact q level {level}")
            else:  # only the whole-window kernel takes a lo half of q in table mode, and it is built for 14 x 14: an error, not a result
                with pytest.raises(ops.IvlmError):
                    _attend(*args, rel_tab=tab, q_lo=True, q_lo_level=level)


@pytest.mark.parametrize("rt", [BF, F16], ids=["bf16", "f16"])
def test_sam_grid_probe(hip_lib, cuda, rt):
    """The 64 x 64 grid (B = H = 1): rel-pos terms as (zero) arrays and in table mode; table mode with the XCD-aware block map and
    without it is bit-identical."""
    from interactvlm_amd import _lib

    lib = _lib.load()
    S = 4096
    p = Probe(S, S, 80, R.spread_targets(S, S), torch.ones(S, dtype=torch.bool), rt, prescale=True)
    args = (_bh(p.q, 1, 1), _bh(p.k, 1, 1), _bh(p.v, 1, 1), rt, cuda, p.scale)
    zeros = torch.zeros(1, S, 64, dtype=torch.float32, device=cuda)
    p.check(_attend(*args, rel=(zeros, zeros.clone())), "SAM grid, array mode")
    tab = (_zero_table(256, rt, cuda), 64)
    outs = []
    try:
        for xcd in (1, 0):
            lib.ivlm_attention_xcd_map(xcd)
            outs.append(_attend(*args, rel_tab=tab))
            p.check(outs[-1], f"SAM grid, table mode, xcd map {xcd}")
    finally:
        lib.ivlm_attention_xcd_map(1)
    assert torch.equal(outs[0], outs[1])
    if rt == F16:
        p.check(_attend(*args, rel_tab=tab, q_lo=True, q_lo_level=1), "SAM grid, table mode, exact q level 1")


# ---- random values: the error in units of the documented rounding -----------------------------------------------------------------------
_RANDOM = [(m, c) for m in MODES for c in R.RANDOM_CASES[m[0]]]


@pytest.mark.parametrize("mode,case", _RANDOM, ids=[f"{_mid(m)}-{_id(c)}" for m, c in _RANDOM])
def test_random_values_track_the_rounding(hip_lib, cuda, mode, case):
    rt, pp = mode
    B, H, Sq, Sk, D, causal, q_pos0 = case
    with block_shape(pp):
        for pre in ((False, True) if D == 64 else (False,)):
            q, k, v, scale, o, wabs, emu = R.random_case(case, rt, pre)
            got = _attend(q, k, v, rt, cuda, scale, causal=causal, q_pos0=q_pos0, prescale_q=pre)
            _assert_margin(got, o, wabs, emu, rt, f"{_mid(mode)} {case} prescale_q {pre}")


@pytest.mark.parametrize("rt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("side,B,H", R.SAM_RANDOM)
def test_sam_random_values_track_the_rounding(hip_lib, cuda, rt, side, B, H):
    """SAM attention with random rel-pos tables (std 0.2) against fp64 with the bias in fp64: the 14 x 14 window (and sides 9 and 4)
    on the whole-window and the generic kernel, the 64 x 64 grid in table mode and with the terms as arrays."""
    from interactvlm_amd import _lib, ops

    lib = _lib.load()
    q, k, v, tab_h, tab_w, scale, o, wabs, emu, _ = R.sam_random_case(side, B, H, rt)
    cat = _cat_table(tab_h, tab_w, cuda)
    what = f"SAM {side} x {side} {'bf16' if rt == BF else 'f16'}"
    if side == 64:
        got = _attend(q, k, v, rt, cuda, scale, rel_tab=(cat, side))
        _assert_margin(got, o, wabs, emu, rt, what + " table mode")
        rel = ops.relpos_bias(q.to(cuda), tab_h.to(cuda), tab_w.to(cuda), side, side, cat=cat)  # (q: a view of contiguous [B,S,H,D] rows)
        got = _attend(q, k, v, rt, cuda, scale, rel=rel)
        _assert_margin(got, o, wabs, emu, rt, what + " array mode")
        return
    try:
        for whole in (1, 0):
            lib.ivlm_attention_window_kernel(whole)
            got = _attend(q, k, v, rt, cuda, scale, rel_tab=(cat, side))
            _assert_margin(got, o, wabs, emu, rt, what + (" whole-window kernel" if whole else " generic kernel"))
    finally:
        lib.ivlm_attention_window_kernel(1)
