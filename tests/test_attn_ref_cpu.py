"""The reference side of the attention edge tests, checked on its own (no GPU, no library):

* the probe inputs really are "one key per query": a visible target yields its value row to 1e-5 in fp64, a hidden one leaves the
  output at least 1/32 away in some column - for EVERY probe case the GPU test runs, so its two assertions cannot both hold;
* the emulation of the kernel's documented roundings stays under committed caps on every random-value case - the GPU thresholds are
  multiples of the emulation's ratio, so a changed seed or case cannot silently loosen them;
* mutants of the reference (last key dropped, causal mask shifted by one, K/V batch 0 for every query batch), rounded like a
  kernel's output, violate the GPU test's assertions;
* the fp32 probes of tests/test_attention_f32_gpu.py: every table entry stays inside half the visible bound and outside the separation
  in fp64, a plain fp32 softmax passes the verdict, and its mutants (last key dropped, ghost key seen, K/V batch b instead of
  b // div) do not."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attn_ref as R  # noqa: E402

RTS = [torch.bfloat16, torch.float16]
_id = lambda v: str(v).replace("torch.", "").replace(" ", "") if not isinstance(v, (int, str)) else str(v)


def _b(t, rt):
    return t.to(rt)[None, None]  # [S, D] -> [1, 1, S, D] in the operand type


def _probe_case(Sq, Sk, D, target, rt, causal=False, q_pos0=0, prescale=False):
    """fp64 output rows and value rows of the targets for one probe run: keys = the Sk real ones (a target >= Sk is absent)."""
    n = max(Sk, int(target.max()) + 1)
    q, k, v = R.probe(Sq, n, D, target)
    o, wabs = R.ref64(_b(q, rt), _b(k[:Sk], rt), _b(v[:Sk], rt), D ** -0.5, causal, q_pos0, prescale_rt=rt if prescale else None)
    return o[0, 0], wabs[0, 0], v[target]


def _assert_separable(o, vt, visible, what):
    d = (o - vt).abs()
    if visible.any():
        assert float(d[visible].max()) < 1e-5, what
    if (~visible).any():
        assert float(d[~visible].amax(dim=-1).min()) >= R.SEPARATION, what


def test_probe_construction():
    for D in (16, 32, 64, 80, 128):
        q, k, v = R.probe(5, 300, D, torch.tensor([0, 1, 77, 255, 299]))
        s = (q @ k.T) * D ** -0.5
        ham = torch.tensor([[bin(j ^ t).count("1") for j in range(300)] for t in (0, 1, 77, 255, 299)], dtype=torch.float64)
        assert torch.allclose(s, 128.0 - 16.0 * ham, atol=1e-9)
        for rt in RTS:
            assert torch.equal(k.to(rt).double(), k) and torch.equal(v.to(rt).double(), v)
            assert float(v.max()) <= 1.0 and float(v.min()) >= 0.0
        assert float(torch.cdist(v, v, p=float("inf")).fill_diagonal_(1.0).min()) >= 1.0 / 16


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("Sk,D", R.KEY_TAIL)
def test_key_tail_probes_separable(Sk, D, rt):
    for name, (target, vis) in R.key_tail_targets(Sk).items():
        o, _, vt = _probe_case(R.KEY_TAIL_SQ, Sk, D, target, rt)
        _assert_separable(o, vt, torch.full((R.KEY_TAIL_SQ,), vis), f"key tail {name} Sk={Sk} D={D}")


def test_key_tail_covers_every_head_dim():
    for D in (16, 32, 64, 80, 128):
        assert {17, 64, 65} <= {sk for sk, d in R.KEY_TAIL if d == D}
    assert {sk for sk, _ in R.KEY_TAIL} == {1, 15, 16, 17, 63, 64, 65, 127, 129, 200}


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("Sq", R.QUERY_EDGES)
def test_query_edge_probes_separable(Sq, rt):
    target = R.spread_targets(Sq, R.QUERY_EDGES_SK)
    if Sq >= R.QUERY_EDGES_SK:
        assert len(set(target.tolist())) == R.QUERY_EDGES_SK  # spread over ALL keys
    for D in (64, 80):
        o, _, vt = _probe_case(Sq, R.QUERY_EDGES_SK, D, target, rt)
        _assert_separable(o, vt, torch.ones(Sq, dtype=torch.bool), f"query edge Sq={Sq}")


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("shape,D", R.CAUSAL, ids=_id)
def test_causal_probes_separable(shape, D, rt):
    Sq, Sk, q_pos0 = shape
    for name, (target, vis) in R.causal_targets(Sq, Sk, q_pos0).items():
        o, _, vt = _probe_case(Sq, Sk, D, target, rt, causal=True, q_pos0=q_pos0)
        _assert_separable(o, vt, vis, f"causal {name} {shape} D={D}")
    hidden = ~R.causal_targets(Sq, Sk, q_pos0)["next"][1]
    assert hidden.any() or Sq == 1  # (1, 300, 299): the diagonal is the last key, nothing to hide


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("side", R.WINDOW_SIDES + [64])
def test_sam_probes_separable(side, rt):
    S = side * side
    target = R.spread_targets(S, S)
    o, _, vt = _probe_case(S, S, 80, target, rt, prescale=True)
    _assert_separable(o, vt, torch.ones(S, dtype=torch.bool), f"SAM side {side}")


# ---- the emulation's own error: what the GPU thresholds hang on ---------------------------------------------------------------------
@pytest.mark.parametrize("rt", RTS, ids=_id)
def test_emulation_under_caps(rt):
    for case in R.RANDOM_CASES[rt]:
        for pre in ((False, True) if case[4] == 64 else (False,)):
            emu = R.random_case(case, rt, pre)[-1]
            print(f"{_id(rt)} {case} prescale={pre}: emulation ratio max {emu[0]:.3f} rms {emu[1]:.3f}")
            assert emu[0] <= R.EMU_MAX_CAP and emu[1] <= R.EMU_RMS_CAP, (case, emu)
            assert emu[1] > 0.01, (case, emu)  # and it is not degenerate: 1.5 x rms is a real threshold


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("side,B,H", R.SAM_RANDOM)
def test_sam_emulation_under_caps(side, B, H, rt):
    *_, emu, caps = R.sam_random_case(side, B, H, rt)
    print(f"{_id(rt)} SAM {side} x {side}: emulation ratio max {emu[0]:.3f} rms {emu[1]:.3f} (caps {caps[0]:.2f} / {caps[1]:.2f})")
    assert emu[0] <= caps[0] and emu[1] <= caps[1] and emu[1] > 0.01, (emu, caps)


def test_rescale_case_under_caps():
    q, k, v, o, wabs, emu = rescale_case()
    print(f"rescale case: emulation ratio max {emu[0]:.3f} rms {emu[1]:.3f}")
    assert emu[0] <= R.EMU_MAX_CAP and emu[1] <= R.EMU_RMS_CAP


def rescale_case():
    """tests/test_attention_gpu.py::test_attention_rescale_branch_forced on the CPU."""
    g = torch.Generator().manual_seed(4)
    bf = torch.bfloat16
    q = torch.randn(1, 2, 70, 64, generator=g).to(bf)
    k = torch.randn(1, 2, 400, 64, generator=g).to(bf)
    v = torch.randn(1, 2, 400, 64, generator=g).to(bf)
    k[0, :, 333] = (q[0, :, 7] * 6).to(bf)
    o, wabs = R.ref64(q, k, v, 0.125)
    return q, k, v, o, wabs, R.ratio_stats(R.emulate(q, k, v, 0.125, rt=bf), o, wabs, bf)


# ---- mutants: a structurally wrong kernel, with the roundings of a right one, must violate the GPU assertions ------------------------
def _mutant_probe_fails(Sq, Sk, D, target, visible, rt, causal=False, q_pos0=0, mutate=None):
    """Section 3 on a mutated emulation.  mutate(k, v, q_pos0) -> (k, v, q_pos0)."""
    q, k, v = R.probe(Sq, max(Sk, int(target.max()) + 1), D, target)
    vt = v[target]
    qb, kb, vb = _b(q, rt), _b(k[:Sk], rt), _b(v[:Sk], rt)
    o, wabs = R.ref64(qb, kb, vb, D ** -0.5, causal, q_pos0)
    emu = R.emulate(qb, kb, vb, D ** -0.5, causal, q_pos0, rt=rt)
    hid = ~visible
    emu_stats = R.ratio_stats(emu[0, 0][hid], o[0, 0][hid], wabs[0, 0][hid], rt) if hid.any() else None
    assert R.probe_verdict(emu[0, 0], vt, o[0, 0], wabs[0, 0], visible, rt, emu_stats) == []  # the unmutated emulation passes
    km, vm, pm = mutate(kb, vb, q_pos0)
    got = R.emulate(qb, km, vm, D ** -0.5, causal, pm, rt=rt)
    return R.probe_verdict(got[0, 0], vt, o[0, 0], wabs[0, 0], visible, rt, emu_stats)


@pytest.mark.parametrize("rt", RTS, ids=_id)
def test_mutant_last_key_dropped(rt):
    drop = lambda k, v, p: (k[:, :, :-1], v[:, :, :-1], p)
    for Sk, D in [(17, 16), (64, 64), (65, 80), (129, 64), (200, 128)]:  # section 3: the "last" run of the key-tail cases
        target, vis = R.key_tail_targets(Sk)["last"]
        assert _mutant_probe_fails(R.KEY_TAIL_SQ, Sk, D, target, torch.full((R.KEY_TAIL_SQ,), vis), rt, mutate=drop)
    for case in R.RANDOM_CASES[rt]:  # section 4: every random-value case notices
        q, k, v, scale, o, wabs, emu = R.random_case(case, rt)
        if case[5] and case[3] - 1 > case[2] - 1 + case[6]:
            continue  # (causal and the last key is hidden from every query: nothing dropped)
        got = R.emulate(q, k[:, :, :-1], v[:, :, :-1], scale, case[5], case[6], rt=rt)
        gs = R.ratio_stats(got, o, wabs, rt)
        assert not R.within_margin(gs, emu), (case, gs, emu)


@pytest.mark.parametrize("rt", RTS, ids=_id)
def test_mutant_causal_mask_shifted(rt):
    for shape, D in R.CAUSAL:
        Sq, Sk, q_pos0 = shape
        t = R.causal_targets(Sq, Sk, q_pos0)
        # one key too few: run A (the diagonal key must be seen) fails; one key too many: run B (the next key must not be seen)
        assert _mutant_probe_fails(Sq, Sk, D, *t["diag"], rt, True, q_pos0, mutate=lambda k, v, p: (k, v, p - 1)), (shape, D)
        if (~t["next"][1]).any():
            assert _mutant_probe_fails(Sq, Sk, D, *t["next"], rt, True, q_pos0, mutate=lambda k, v, p: (k, v, p + 1)), (shape, D)
    for case in R.RANDOM_CASES[rt]:
        if not case[5]:
            continue
        q, k, v, scale, o, wabs, emu = R.random_case(case, rt)
        for shift in (-1, 1):
            if shift == 1 and case[2] - 1 + case[6] + 1 >= case[3] and case[2] == 1:
                continue  # (a single query that already sees every key)
            if case[6] + shift < 0:
                continue  # (query 0 would see no key at all)
            got = R.emulate(q, k, v, scale, True, case[6] + shift, rt=rt)
            gs = R.ratio_stats(got, o, wabs, rt)
            assert not R.within_margin(gs, emu), (case, shift, gs, emu)


@pytest.mark.parametrize("rt", RTS, ids=_id)
@pytest.mark.parametrize("div", R.KV_DIVS)
def test_mutant_kv_batch_zero(div, rt):
    """The K/V broadcast probe: every K/V batch holds a different V (rows rotated), so batch 0's row is another row."""
    B, Sq, Sk, D = 2 * div, 33, 70, 64
    target = R.spread_targets(Sq, Sk)
    q, k, v = R.probe(Sq, Sk, D, target)
    vs = R.kv_batches(v, B // div)
    qb = _b(q, rt).expand(B, 1, Sq, D)
    kb = _b(k, rt).expand(B // div, 1, Sk, D)
    o, wabs = R.ref64(qb, kb, vs.to(rt), D ** -0.5)
    good = R.emulate(qb, kb, vs.to(rt), D ** -0.5, rt=rt)
    bad = R.emulate(qb, kb[:1], vs[:1].to(rt), D ** -0.5, rt=rt)
    vis = torch.ones(Sq, dtype=torch.bool)
    for b in range(B):
        vt = vs[b // div, 0][target]
        assert R.probe_verdict(good[b, 0], vt, o[b, 0], wabs[b, 0], vis, rt) == []
        assert bool(R.probe_verdict(bad[b, 0], vt, o[b, 0], wabs[b, 0], vis, rt)) == (b // div != 0)



# ---- fp32 operands: the probes, tables and mutants of tests/test_attention_f32_gpu.py ---------------------------------------------------
F32_DS = (16, 32) + R.F32_WIDE_DS


def test_f32_probe_construction():
    tg = [0, 1, 77, 255, 299]
    ham = torch.tensor([[bin(j ^ t).count("1") for j in range(300)] for t in tg], dtype=torch.float64)
    for D in F32_DS:
        q, k, v, scale = R.probe_f32(5, 300, D, torch.tensor(tg))
        assert scale == float(np.float32(128.0 / D))
        for t in (q, k, v):
            assert torch.equal(t.float().double(), t)  # exact in fp32
        dot = q.float() @ k.float().T  # every partial sum is an integer of at most D: exact in any order
        assert torch.equal(dot.double(), q @ k.T) and float(dot.abs().max()) <= D
        s32 = (dot * torch.tensor(scale, dtype=torch.float32)).double()  # the kernel's score: ONE rounding
        want = 128.0 - 16.0 * ham
        assert float((s32 - (q @ k.T) * scale).abs().max()) <= 2.0 ** -24 * 128  # against ref64's score of the same fp32 scale
        assert float((s32 - want).abs().max()) <= 2.0 ** -24 * 128 * 2  # (and the rounding of the scale itself)
        if D & (D - 1) == 0:
            assert torch.equal(s32, want)


def test_f32_tables_cover_the_routes():
    for D in (16, 32):  # both sides of the few-keys / many-keys boundary, lane-count classes 1, 63, 0 and 1 past a 64-key stride
        assert {sk for sk, d in R.F32_KEY_TAIL if d == D} == set(R.F32_KEY_TAIL_SKS) and {64, 65, 63, 128, 129} <= set(R.F32_KEY_TAIL_SKS)
    for D in R.F32_WIDE_DS:
        assert {sk for sk, d in R.F32_KEY_TAIL if d == D} == {1, 4, 65, 200}
    few = {c[2] for c in R.F32_QUERY_EDGES if c[3] <= 64 and c[4] in (16, 32)}
    assert few == {1, 255, 256, 257, 300}
    for Sk, D in ((70, 16), (70, 32), (4, 128)):  # wave per query: every count of dead waves in the last block
        assert {c[0] * c[1] * c[2] % 4 for c in R.F32_QUERY_EDGES if c[3:] == (Sk, D)} == {1, 2, 3}


@pytest.mark.parametrize("Sk,D", R.F32_KEY_TAIL)
def test_f32_key_tail_probes_separable(Sk, D):
    """The reference alone stays inside HALF the visible bound and outside the separation, and a plain fp32 softmax passes the verdict."""
    for name in R.key_tail_targets(Sk):
        q, k, v, ghost, scale, vt, o, vis = R.f32_probe_case(R.KEY_TAIL_SQ, Sk, D, name)
        assert (ghost[0] is not None) == (name == "ghost")
        vis_err, sep, _ = R.probe_errors_f32(o, vt, o, vis)
        assert vis_err is None or vis_err <= R.VISIBLE_TOL_F32 / 2, (name, vis_err)
        assert sep is None or sep >= R.SEPARATION, (name, sep)
        got = R.attend32(q[None, None], k[None, None], v[None, None], scale)[0, 0]
        assert R.probe_verdict_f32(got, vt, o, vis) == [], name


@pytest.mark.parametrize("case", R.F32_QUERY_EDGES, ids=_id)
def test_f32_query_edge_probes_separable(case):
    B, H, Sq, Sk, D = case
    q, k, v, _, scale, vt, o, vis = R.f32_probe_case(Sq, Sk, D, "edges")
    if Sq >= Sk:
        assert len(set(R.spread_targets(Sq, Sk).tolist())) == Sk  # spread over ALL keys
    assert bool(vis.all()) and R.probe_errors_f32(o, vt, o, vis)[0] <= R.VISIBLE_TOL_F32 / 2
    assert R.probe_verdict_f32(R.attend32(q[None, None], k[None, None], v[None, None], scale)[0, 0], vt, o, vis) == []


@pytest.mark.parametrize("Sk,D", [c for c in R.F32_KEY_TAIL if c[0] > 1])
def test_f32_mutant_last_key_dropped(Sk, D):
    q, k, v, _, scale, vt, o, vis = R.f32_probe_case(R.KEY_TAIL_SQ, Sk, D, "last")
    got = R.attend32(q[None, None], k[None, None, :-1], v[None, None, :-1], scale)[0, 0]
    assert R.probe_verdict_f32(got, vt, o, vis)


@pytest.mark.parametrize("Sk,D", R.F32_KEY_TAIL)
def test_f32_mutant_ghost_key_seen(Sk, D):
    q, k, v, ghost, scale, vt, o, vis = R.f32_probe_case(R.KEY_TAIL_SQ, Sk, D, "ghost")
    kg, vg = torch.cat([k, ghost[0][None]]), torch.cat([v, ghost[1][None]])
    got = R.attend32(q[None, None], kg[None, None], vg[None, None], scale)[0, 0]
    assert R.probe_verdict_f32(got, vt, o, vis)


@pytest.mark.parametrize("roll", ["v", "k"])
@pytest.mark.parametrize("div", R.KV_DIVS)
@pytest.mark.parametrize("Sk,D", R.F32_KV_ROUTES)
def test_f32_mutant_kv_batch_not_divided(Sk, D, div, roll):
    """K/V batch b instead of b // div: every query batch but the first returns another batch's row, at least 1/16 away."""
    q, ks, vs, scale, want = R.f32_kv_case(Sk, D, roll)
    B, n = R.F32_KV_B, R.F32_KV_B // div
    for i in range(B):
        for j in range(i):
            assert float((want[i] - want[j]).abs().amax(dim=-1).min()) >= 1.0 / 16
    qb = q[None, None].expand(B, 1, *q.shape)
    o = R.ref64(qb, ks[:n], vs[:n], scale)[0]
    good, bad = R.attend32(qb, ks[:n], vs[:n], scale), R.attend32(qb, ks, vs, scale)
    vis = torch.ones(q.shape[0], dtype=torch.bool)
    for b in range(B):
        assert R.probe_verdict_f32(good[b, 0], want[b // div], o[b, 0], vis) == []
        assert bool(R.probe_verdict_f32(bad[b, 0], want[b // div], o[b, 0], vis)) == (b != b // div)
