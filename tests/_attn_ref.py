"""Reference side of the attention edge tests (pure torch, CPU, fp64).  Nothing here imports or calls the library.

* ``ref64``    plain softmax attention in fp64 on the given 16-bit values; returns ``o`` and ``wabs = softmax . |v|``.
* ``emulate``  the same with the kernel's DOCUMENTED rounding points and nothing else: the unnormalised ``p = exp(s - rowmax)`` rounded
               to the operand type, the denominator from the unrounded ``p``, the output rounded to the operand type.
* ``ratio``    ``|got - o| / (u * (wabs + |o|))`` with ``u`` = 2^-9 (bf16) / 2^-12 (fp16): the error in units of the first-order worst
               case of those two roundings (each at most ``u`` relative: ``u * wabs`` from p, ``u * |o|`` from the output).
* ``probe``    exact "one key per query" inputs: which keys a kernel saw can be read off its output.
* the case tables shared by ``test_attn_ref_cpu.py`` (separability, emulation caps, mutants) and ``test_attention_edges_gpu.py``.
* ``probe_f32``, ``probe_verdict_f32`` and the ``F32_*`` tables: the same for the fp32 kernels (``test_attention_f32_gpu.py``), whose
  bounds are absolute (no operand rounding to measure in units of).
"""
import functools
import math

import torch

U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
# a visible probe target: the output is V[target] (exact) times 1 / (1 + 2e-6), rounded once -> within one rounding step below 1
VISIBLE_TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SEPARATION = 1.0 / 32  # a hidden probe target leaves the output at least this far from V[target] in some column
MAX_MARGIN, RMS_MARGIN = 2.0, 1.5  # kernel against emulation: online-softmax rescaling, hardware exp2, fp32 summation order
# Caps on the emulation's own ratio (asserted on the CPU, so that a changed seed or case cannot silently loosen the GPU thresholds
# that hang on it).  To first order the ratio is <= 1 by construction; what exceeds it is second order (the rounded output is
# compared with the UNrounded o) and, for fp16, weights below 2^-14 that round on the subnormal grid.  Twice the first-order
# worst case for a maximum; for the rms, half of it (independent roundings of many weights average out: a uniform rounding error
# alone has rms 1 / sqrt(3) of its maximum, and the two terms never peak together).
EMU_MAX_CAP, EMU_RMS_CAP = 2.0, 0.5


def _expand_kv(t, B):
    return t if t.shape[0] == B else t.repeat_interleave(B // t.shape[0], dim=0)  # K/V of batch b // (B // Bk)


def _weights(q, k, scale, causal, q_pos0, bias, prescale_rt):
    """(unnormalised p = exp(s - rowmax), its row sum) in fp64; the rows always see key 0."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    kd = _expand_kv(k, B).double()
    if prescale_rt is not None:  # the kernels' prescale_q contract: q * scale in fp32, rounded to the operand type, then the dot product
        s = torch.einsum("bhqd,bhkd->bhqk", (q.float() * scale).to(prescale_rt).double(), kd)
    else:
        s = torch.einsum("bhqd,bhkd->bhqk", q.double(), kd) * scale
    if bias is not None:
        s = s + bias.double()
    if causal:
        hidden = torch.arange(Sk)[None, :] > torch.arange(Sq)[:, None] + q_pos0
        s = s.masked_fill(hidden, float("-inf"))
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return p, p.sum(dim=-1, keepdim=True)


def ref64(q, k, v, scale, causal=False, q_pos0=0, bias=None, prescale_rt=None):
    """q [B,H,Sq,D], k / v [Bk,H,Sk,D] (any float dtype; B % Bk == 0) -> (o, wabs) fp64 [B,H,Sq,D]."""
    p, den = _weights(q, k, scale, causal, q_pos0, bias, prescale_rt)
    vd = _expand_kv(v, q.shape[0]).double()
    w = p / den
    return torch.einsum("bhqk,bhkd->bhqd", w, vd), torch.einsum("bhqk,bhkd->bhqd", w, vd.abs())


def emulate(q, k, v, scale, causal=False, q_pos0=0, bias=None, prescale_rt=None, rt=torch.bfloat16):
    """ref64 with p rounded to ``rt`` for P.V, the denominator from the unrounded p, the output rounded to ``rt`` (returned as fp64)."""
    p, den = _weights(q, k, scale, causal, q_pos0, bias, prescale_rt)
    vd = _expand_kv(v, q.shape[0]).double()
    o = torch.einsum("bhqk,bhkd->bhqd", p.to(rt).double(), vd) / den
    return o.to(rt).double()


def ratio(got, o, wabs, rt):
    num = (got.double() - o).abs()
    return torch.where(num == 0, torch.zeros_like(num), num / (U[rt] * (wabs + o.abs())))  # (an exact 0 of an all-zero row: 0, not 0 / 0)


def ratio_stats(got, o, wabs, rt):
    r = ratio(got, o, wabs, rt)
    return float(r.max()), float(r.pow(2).mean().sqrt())


def within_margin(got_stats, emu_stats):
    return got_stats[0] <= MAX_MARGIN * emu_stats[0] and got_stats[1] <= RMS_MARGIN * emu_stats[1]


# ---- probe inputs ----------------------------------------------------------------------------------------------------------------
def _code(j, D):
    """+-1 code of the low 16 bits of j, repeated D / 16 times: [..., D]."""
    bits = (j[..., None] >> torch.arange(16)) & 1
    return (1.0 - 2.0 * bits.double()).repeat(*([1] * j.dim()), D // 16)


def probe_values(n, D):
    """V[j, d] = bit d of j (d < 16), ((j * (d + 1)) % 17) / 16 above: exact in bf16 / fp16, two keys differ by >= 1/16 somewhere."""
    j = torch.arange(n)
    d = torch.arange(D)
    hi = ((j[:, None] * (d[None, :] + 1)) % 17).double() / 16.0
    lo = ((j[:, None] >> d[None, :].clamp(max=15)) & 1).double()
    return torch.where(d[None, :] < 16, lo, hi)


def probe(Sq, Sk, D, target, scale=None):
    """q [Sq,D], k [Sk,D], v [Sk,D] (fp64, every k / v value exact in both 16-bit types; q = s * code with s = 128 / (D * scale), rounded
    by the caller's cast) with score(i, j) = 128 - 16 * hamming(j, target[i]): the target key carries a softmax weight of at least
    1 - 16 e^-16 whenever it is visible, and the output row IS its value row.  ``target`` may name keys >= Sk (hidden by absence)."""
    scale = D ** -0.5 if scale is None else scale
    target = torch.as_tensor(target, dtype=torch.int64).expand(Sq)
    k = _code(torch.arange(Sk), D)
    q = _code(target, D) * (128.0 / (D * scale))
    return q, k, probe_values(Sk, D)


# ---- the cases (shapes B, H are chosen by the GPU test; the CPU test uses B = H = 1 unless the case is about batches) --------------
KEY_TAIL = [  # (Sk, D): Sq = 33, non-causal; every D meets 17, 64 and 65
    (1, 64), (15, 16), (16, 128), (63, 32), (127, 80), (129, 64), (200, 128), (200, 16),
    (17, 16), (17, 32), (17, 64), (17, 80), (17, 128), (64, 16), (64, 32), (64, 64), (64, 80), (64, 128),
    (65, 16), (65, 32), (65, 64), (65, 80), (65, 128),
]
KEY_TAIL_SQ = 33
QUERY_EDGES = [1, 16, 127, 128, 129, 255, 256, 257, 300]  # Sq; Sk = 70
QUERY_EDGES_SK = 70
CAUSAL_SHAPES = [(130, 130, 0), (100, 333, 233), (1, 300, 299), (70, 200, 130), (257, 320, 63)]  # Sq, Sk, q_pos0
CAUSAL = [(s, D) for s in CAUSAL_SHAPES for D in (64, 128)] + [((70, 200, 130), 32)]
KV_DIVS = [2, 4]
WINDOW_SIDES = [14, 9, 4]


def key_tail_targets(Sk):
    """name -> (target per query, visible?)"""
    i = torch.arange(KEY_TAIL_SQ)
    return {"spread": (i % Sk, True), "last": (torch.full_like(i, Sk - 1), True), "ghost": (torch.full_like(i, Sk), False)}


def causal_targets(Sq, Sk, q_pos0):
    """Run A: the diagonal key (last visible); run B: the key after it (first hidden) where it exists, else the diagonal again."""
    diag = torch.arange(Sq) + q_pos0
    nxt = diag + 1
    has_next = nxt < Sk
    return {"diag": (diag, torch.ones(Sq, dtype=torch.bool)), "next": (torch.where(has_next, nxt, diag), ~has_next)}


def spread_targets(Sq, Sk):
    return (torch.arange(Sq) * 11 + 3) % Sk


def kv_batches(v, n):
    """[n, 1, Sk, D]: K/V batch i holds the value rows rotated by 5 i keys - any other batch's row differs by >= 1/16 somewhere."""
    return torch.stack([torch.roll(v, 5 * i, dims=0) for i in range(n)])[:, None]


def probe_verdict(got, vt, o, wabs, visible, rt, emu_stats=None, got_stats=None):
    """The section-3 assertions as one function (shared with the mutants of the CPU test).  got / vt / o / wabs [Sq, D] of one (b, h),
    visible [Sq] bool.  Returns a list of failure strings (empty = pass)."""
    bad = []
    d = (got.double() - vt).abs()
    if visible.any():
        e = float(d[visible].max())
        if not e <= VISIBLE_TOL[rt]:
            bad.append(f"visible target missed: |got - V[target]| = {e:.3g} > {VISIBLE_TOL[rt]:.3g}")
    hid = ~visible
    if hid.any():
        near = float(d[hid].amax(dim=-1).min())
        if not near >= SEPARATION:
            bad.append(f"hidden target seen: output within {near:.3g} of V[target]")
        if emu_stats is not None:
            gs = ratio_stats(got[hid], o[hid], wabs[hid], rt) if got_stats is None else got_stats
            if not within_margin(gs, emu_stats):
                bad.append(f"hidden-target rows off the reference: ratio max / rms {gs[0]:.3g} / {gs[1]:.3g} vs emulation {emu_stats[0]:.3g} / {emu_stats[1]:.3g}")
    return bad


# ---- fp32 operands (csrc/attention_f32.hip; tests/test_attention_f32_gpu.py) ------------------------------------------------------------
# A visible probe target: every other key has a score 16 * hamming lower, so the target's weight falls short of 1 by at most
# (1 + e^-16)^16 - 1 = 1.8e-6 (the sum over all 2^16 - 1 other codes, however many of them are keys).  All values lie in [0, 1], so
# the fp64 output is within 1.8e-6 of V[target]; 2^-18 = 3.8e-6 is twice that.  The fp32 kernel adds a few units of 2^-24: the
# scores are exact or one rounding off (probe_f32), the weights of the other keys sum to < 2e-6 and V[target] itself is exact.
VISIBLE_TOL_F32 = 2.0 ** -18
# the project's documented bound of this kernel against fp64 (DESIGN.md "attention_f32 ... torch fp64 | 2e-5"; the bound of
# tests/test_dense_gpu.py::test_attention_f32_vs_torch)
F32_TOL = 2e-5


def probe_f32(Sq, Sk, D, target):
    """``probe`` for fp32 operands, D % 16 == 0: -> (q, k, v, scale) with q the bare +-1 code (scale = 128 / D makes ``probe``'s q
    multiplier exactly 1) and scale = 128 / D rounded to fp32, as a python float: the number the test hands to the kernel AND to
    ref64.  Every dot product is then a small integer (|.| <= D, exact in fp32) and a score that integer times ONE fp32 constant:
    128 - 16 * hamming(j, target) up to a single rounding, exact when D (hence the scale) is a power of two."""
    assert D % 16 == 0
    q, k, v = probe(Sq, Sk, D, target, scale=128.0 / D)
    assert bool((q.abs() == 1.0).all())
    return q, k, v, float(torch.tensor(128.0 / D, dtype=torch.float32))


F32_KEY_TAIL_SKS = (1, 2, 9, 63, 64, 65, 127, 128, 129, 200, 4096)  # both sides of the 64 / 65 route boundary; Sk % 64 = 1, 63, 0, 1 past a stride
F32_WIDE_DS = (48, 64, 80, 128, 256)  # the wide kernel with 12 ... 64 live lanes
F32_KEY_TAIL = ([(Sk, D) for D in (16, 32) for Sk in F32_KEY_TAIL_SKS]  # (Sk, D): Sq = KEY_TAIL_SQ, targets of key_tail_targets
                + [(Sk, D) for D in F32_WIDE_DS for Sk in (1, 4, 65, 200)])
F32_QUERY_EDGES = (  # (B, H, Sq, Sk, D), targets of spread_targets
    # thread per query, 256 queries per block: the block edge from both sides, a second block with 1 and with 44 live threads
    [(1, 2, Sq, 9, 16) for Sq in (1, 255, 256, 257, 300)] + [(2, 1, Sq, 9, 32) for Sq in (1, 255, 256, 257, 300)]
    # wave per query, 4 waves per block: B * H * Sq % 4 = 1, 2, 3 - the last block has 3, 2, 1 dead waves
    + [(B, H, Sq, Sk, D) for Sk, D in ((70, 16), (70, 32), (4, 128)) for B, H, Sq in ((1, 1, 1), (1, 3, 2), (1, 1, 7))])
F32_KV_ROUTES = [(9, 16), (70, 16), (4, 128)]  # (Sk, D) of the K/V broadcast probe: once per route
F32_KV_B = 4


def attend32(q, k, v, scale):
    """plain fp32 torch softmax attention of fp32 operands (k / v of batch b // (B // Bk)): what a correct fp32 kernel computes up to
    the order of its sums - the stand-in for the kernel in the CPU mutants"""
    B = q.shape[0]
    s = torch.einsum("bhqd,bhkd->bhqk", q, _expand_kv(k, B)) * scale
    return torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), _expand_kv(v, B))


def probe_errors_f32(got, vt, o, visible):
    """(largest |got - V[target]| over the visible rows, smallest max-column distance from V[target] over the hidden rows, largest
    |got - o| over the hidden rows); None where there is no such row.  got / vt / o [Sq, D] of one (b, h), visible [Sq] bool."""
    d = (got.double() - vt).abs()
    hid = ~visible
    return (float(d[visible].max()) if visible.any() else None,
            float(d[hid].amax(dim=-1).min()) if hid.any() else None,
            float((got.double() - o)[hid].abs().max()) if hid.any() else None)


def probe_verdict_f32(got, vt, o, visible):
    """The probe assertions of test_attention_f32_gpu.py as one function (shared with the mutants of the CPU test): a list of failure
    strings (empty = pass)."""
    vis_err, sep, hid_err = probe_errors_f32(got, vt, o, visible)
    bad = []
    if vis_err is not None and not vis_err <= VISIBLE_TOL_F32:
        bad.append(f"visible target missed: |got - V[target]| = {vis_err:.3g} > {VISIBLE_TOL_F32:.3g}")
    if sep is not None and not sep >= SEPARATION:
        bad.append(f"hidden target seen: output within {sep:.3g} of V[target]")
    if hid_err is not None and not hid_err <= F32_TOL:
        bad.append(f"hidden-target rows off the reference: |got - fp64| = {hid_err:.3g} > {F32_TOL:.3g}")
    return bad


@functools.lru_cache(maxsize=None)
def f32_kv_case(Sk, D, roll):
    """The K/V broadcast probe, Sq = KEY_TAIL_SQ: (q [Sq,D], k, v [F32_KV_B,1,Sk,D], scale, expected rows [F32_KV_B,Sq,D] fp64 by K/V
    batch).  roll "v": every K/V batch holds the value rows rotated by another amount (kv_batches) under the same keys; roll "k":
    the key rows rotated under the same values (code t sits in row (t + 5 i) % Sk of batch i, so that row's value comes back).  A call
    with kv_div = div reads the first F32_KV_B // div batches; the others are there so that a wrong batch index is a wrong row."""
    target = spread_targets(KEY_TAIL_SQ, Sk)
    q, k, v, scale = probe_f32(KEY_TAIL_SQ, Sk, D, target)
    n = F32_KV_B
    if roll == "v":
        ks, vs = k.expand(n, 1, Sk, D), kv_batches(v, n)
        want = torch.stack([vs[i, 0][target] for i in range(n)])
    else:
        ks, vs = kv_batches(k, n), v.expand(n, 1, Sk, D)
        want = torch.stack([v[(target + 5 * i) % Sk] for i in range(n)])
    return q.float(), ks.float(), vs.float(), scale, want


@functools.lru_cache(maxsize=None)
def f32_probe_case(Sq, Sk, D, name):
    """One fp32 probe run, computed once per process: (q, k, v [Sk rows], ghost (k, v row Sk) or (None, None), scale, V[target], fp64
    output [Sq, D], visible [Sq]).  name: a key of key_tail_targets, or "edges" for spread_targets."""
    if name == "edges":
        target, vis = spread_targets(Sq, Sk), True
    else:
        assert Sq == KEY_TAIL_SQ
        target, vis = key_tail_targets(Sk)[name]
    n = max(Sk, int(target.max()) + 1)
    q, k, v, scale = probe_f32(Sq, n, D, target)
    q, k, v = q.float(), k.float(), v.float()
    ghost = (k[Sk], v[Sk]) if n > Sk else (None, None)
    o = ref64(q[None, None], k[None, None, :Sk], v[None, None, :Sk], scale)[0][0, 0]
    return q, k[:Sk], v[:Sk], ghost, scale, v[target].double(), o, torch.full((Sq,), vis)


# ---- random-value cases ------------------------------------------------------------------------------------------------------------
CASES = [  # B, H, Sq, Sk, D, causal, q_pos0 (tests/test_attention_gpu.py::CASES)
    (1, 8, 9, 9, 32, False, 0), (4, 8, 9, 4096, 16, False, 0), (4, 8, 4096, 9, 16, False, 0),
    (3, 16, 196, 196, 80, False, 0), (1, 16, 257, 257, 64, False, 0), (1, 32, 330, 330, 128, True, 0),
    (2, 32, 1, 300, 128, True, 299), (2, 4, 100, 333, 128, True, 233), (1, 2, 130, 70, 80, False, 0),
]
F16_CASES = [  # (tests/test_attention_gpu.py::F16_CASES)
    (1, 16, 257, 257, 64, False, 0), (2, 4, 70, 70, 64, False, 0), (1, 32, 330, 330, 128, True, 0), (2, 4, 100, 333, 128, True, 233),
]
CAUSAL_SMALL_D = [(2, 4, 100, 333, 32, True, 233), (2, 4, 100, 333, 80, True, 233), (1, 4, 130, 130, 16, True, 0)]
RANDOM_CASES = {
    torch.bfloat16: CASES + CAUSAL_SMALL_D,
    torch.float16: F16_CASES + [c for c in CASES if c[4] in (16, 32, 80)] + CAUSAL_SMALL_D,
}


@functools.lru_cache(maxsize=None)
def random_case(case, rt, prescale=False):
    """(q, k, v, scale, o, wabs, emulation's (max, rms) ratio) of a random-value case; computed once per process."""
    B, H, Sq, Sk, D, causal, q_pos0 = case
    g = torch.Generator().manual_seed(B * 1000 + Sq + Sk + D)
    q = torch.randn(B, H, Sq, D, generator=g).to(rt)
    k = torch.randn(B, H, Sk, D, generator=g).to(rt)
    v = torch.randn(B, H, Sk, D, generator=g).to(rt)
    scale = 1.0 / math.sqrt(D)
    pre = rt if prescale else None
    o, wabs = ref64(q, k, v, scale, causal, q_pos0, prescale_rt=pre)
    emu = ratio_stats(emulate(q, k, v, scale, causal, q_pos0, prescale_rt=pre, rt=rt), o, wabs, rt)
    return q, k, v, scale, o, wabs, emu


def relpos_terms64(q, tab_h, tab_w, side):
    """SAM's decomposed rel-pos terms in fp64 from the UNSCALED q [B,H,side*side,D] and the tables [2*side-1, D]:
    rel_h [B,H,qy,qx,ky], rel_w [B,H,qy,qx,kx]."""
    B, H, S, D = q.shape
    idx = torch.arange(side)[:, None] - torch.arange(side)[None, :] + (side - 1)
    rq = q.double().reshape(B, H, side, side, D)
    return (torch.einsum("bhyxd,ykd->bhyxk", rq, tab_h.double()[idx]), torch.einsum("bhyxd,xkd->bhyxk", rq, tab_w.double()[idx]))


def _bias_of(rel_h, rel_w):
    B, H, sy, sx, _ = rel_h.shape
    return (rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, H, sy * sx, sy * sx)


SAM_RANDOM = [(14, 3, 2), (64, 1, 1), (9, 2, 2), (4, 3, 2)]  # side, B, H: the window, the grid; two more window sides of the whole-window kernel


@functools.lru_cache(maxsize=None)
def sam_random_case(side, B, H, rt):
    """SAM attention (D = 80, q * scale rounded to the operand type, rel-pos tables of std 0.2) on random values: q, k, v as [B,H,S,D]
    views of [B,S,H,D] rows, the tables in ``rt`` (the kernels' table-mode operand), the fp64 bias of those values, o, wabs, emu."""
    g = torch.Generator().manual_seed(side + 7)
    D, S = 80, side * side
    q, k, v = (torch.randn(B, S, H, D, generator=g).to(rt).permute(0, 2, 1, 3) for _ in range(3))
    tab_h = (torch.randn(2 * side - 1, D, generator=g) * 0.2).to(rt)
    tab_w = (torch.randn(2 * side - 1, D, generator=g) * 0.2).to(rt)
    rel_h, rel_w = relpos_terms64(q, tab_h, tab_w, side)
    bias = _bias_of(rel_h, rel_w)  # the reference: fp64, unrounded
    scale = D ** -0.5
    o, wabs = ref64(q, k, v, scale, bias=bias, prescale_rt=rt)
    caps = (EMU_MAX_CAP, EMU_RMS_CAP)
    if rt == torch.bfloat16:
        # bf16 operands have one more documented rounding point: the two terms are rounded to bf16 (the bf16 model materialises
        # them).  It belongs to the emulation, not to the reference: where a term lies next to a rounding boundary, either
        # neighbour is equally far from the fp64 value, so the kernel's fp32 summation order cannot show up as an error.
        # A score then moves by d <= u (|rel_h| + |rel_w|) and the output by at most 2 d wabs: the cap grows by that.
        ebias = _bias_of(rel_h.to(rt).double(), rel_w.to(rt).double())
        grow = 2.0 * float(rel_h.abs().max() + rel_w.abs().max())
        caps = (EMU_MAX_CAP + grow, (EMU_MAX_CAP + grow) * EMU_RMS_CAP / EMU_MAX_CAP)
    else:
        ebias = bias  # fp16 operands: the terms stay fp32 (hi + lo fp16 operands)
    emu = ratio_stats(emulate(q, k, v, scale, bias=ebias, prescale_rt=rt, rt=rt), o, wabs, rt)
    return q, k, v, tab_h, tab_w, scale, o, wabs, emu, caps
