"""Exact-integer cases for the tile GEMM family (csrc/gemm.hip, gemm256.hip, gemm320.hip, gemm_common.h).  No GPU in this module.

Operands are small integers (times a power of two), so every product and every partial sum of a case is a multiple of one granule and
stays below 2^24 granules: fp32 accumulation is exact IN ANY ORDER, and the kernel's fp32 result, its 16-bit result (one
round-to-nearest-even of an exact value), its [hi | lo] planes and its e4m3 bytes must equal the reference BIT FOR BIT - whatever the
tile, the split-K order or the MFMA grouping.  Only the nonlinear activations keep a tolerance, which then covers the activation alone.

``cases()`` is the table of tests/test_gemm_exact_gpu.py; every case NAMES the kernel it is meant to reach (``Case.kernel``, from the
hand-written KERNEL table below) and tests/test_gemm_exact_cases_cpu.py checks that against ivlm_gemm_route_query.  ``make_case`` builds
the CPU tensors, asserts the exactness budget and gives the reference; ``run_case`` (used by the GPU tests) makes the launch through the
C entry point.  Every output buffer has spare rows and spare columns (ldc > N) filled with a sentinel, and the comparison is over the
WHOLE buffer: whatever the call must not touch has to keep its bits."""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math

import torch

ACT = {"none": 0, "gelu": 1, "quick_gelu": 2, "relu": 3, "silu": 4, "swiglu": 5, "sigmoid": 6}
OPK = {"bf16": 0, "e4m3": 1, "fp16": 2}
RES_F32, A_SPLIT, OUT_SPLIT, F16, OUT_F16, W_PANEL = 2, 4, 8, 16, 32, 64
ENTRY = {"gemm": 0, "panel": 1, "fp8": 2, "splitk": 3, "splitk_fused": 4}
GEMM_TILE, GEMM_256P, GEMM_320 = 0, 1, 2
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -4

# (tile code, operand kind) -> (family, BM, BN): every kernel of the build, written out by hand (NOT read from gemm_instantiated).
# A tile code that has no kernel of its own for an operand kind (96 / 256 for fp16, 96 / 176 / 256 / 320 for e4m3) is not in the table:
# such a call falls back to another entry's kernel and would test nothing new.
KERNEL = {
    (64, "bf16"): (GEMM_TILE, 128, 64), (64, "fp16"): (GEMM_TILE, 128, 64), (64, "e4m3"): (GEMM_TILE, 128, 64),
    (96, "bf16"): (GEMM_TILE, 128, 96),
    (128, "bf16"): (GEMM_TILE, 128, 128), (128, "fp16"): (GEMM_TILE, 128, 128), (128, "e4m3"): (GEMM_TILE, 128, 128),
    (176, "bf16"): (GEMM_TILE, 176, 128), (176, "fp16"): (GEMM_TILE, 176, 128),
    (256, "bf16"): (GEMM_TILE, 256, 256),
    (320, "bf16"): (GEMM_320, 256, 320), (320, "fp16"): (GEMM_320, 256, 320),
    (512, "bf16"): (GEMM_256P, 256, 256), (512, "fp16"): (GEMM_256P, 256, 256), (512, "e4m3"): (GEMM_256P, 256, 256),
}
# the activations a kernel is built with: all for bf16 operands, the towers' for fp16 / e4m3; 176 x 128 and 256 x 320 carry the
# epilogues of their one user only
ALL_ACTS = ("gelu", "quick_gelu", "silu", "sigmoid", "swiglu")
TOWER_ACTS = ("gelu", "quick_gelu", "swiglu")


def acts_of(tile, opk):
    if tile == 176:
        return ("swiglu",)
    if tile == 320:
        return ("gelu",)
    return ALL_ACTS if opk == "bf16" else TOWER_ACTS


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    M: int
    N: int
    K: int                    # (e4m3 operands: bytes = elements)
    tile: int = 0             # forced tile code (ivlm_gemm_tile_override); 0 = the automatic route
    opk: str = "bf16"
    out: str = "f32"          # f32 | 16 (bf16; fp16 for fp16 operands) | split ([hi | lo] 16-bit planes) | e4m3
    act: str = "none"
    entry: str = "gemm"       # gemm | panel | fp8 | splitk | splitk_fused
    bias: bool = False
    res: str = ""             # "" | bf16 | f32
    res_mod: int = 0
    scatter: bool = False     # out_rows: rows dropped (-1), the rest permuted into a taller C; fp32 out + fp32 residual: in place
    gather: bool = False      # a_rows from a taller source
    strided: int = 0          # 0: lda = K, ldw = K | 8: lda, ldw, ldc, ldr larger by multiples of 8 | 2: ldc, ldr = 2 (mod 4)
    batch: int = 1
    a_split: bool = False
    panel: str = ""           # letters of A W C (K-panel entry point) | "w" (IVLM_GEMM_W_PANEL)
    splits: int = 0
    probe: bool = False       # transposition probe: identity-like A against an asymmetric W
    vals: str = "int"         # int: integer operands | act: pre-activations on a 2^-4 grid inside about +-8 | pos: the same, z >= ~1.5
    nsplit: int = 1           # hooks
    kernel: tuple = ()        # the (family, BM, BN) this case NAMES; () = the automatic route, see ``routes``
    routes: tuple = ()        # explicit expected records (family, BM, BN, operand kind, fp32 epilogue, act) where kernel is ()

    @property
    def id(self):
        f = [self.group, f"t{self.tile}", self.opk, f"{self.M}x{self.N}x{self.K}", self.out, self.act, self.entry]
        f += [k for k in ("bias", "scatter", "gather", "a_split", "probe") if getattr(self, k)]
        f += [f"res{self.res}"] if self.res else []
        f += [f"mod{self.res_mod}"] if self.res_mod else []
        f += [f"ld{self.strided}"] if self.strided else []
        f += [f"b{self.batch}"] if self.batch > 1 else []
        f += [f"p{self.panel}"] if self.panel else []
        f += [f"s{self.splits}"] if self.splits else []
        return "-".join(f)

    @property
    def n_out(self):
        return self.N // 2 if self.act == "swiglu" else self.N

    @property
    def f32_epilogue(self):
        return int(self.out in ("f32", "split"))

    def expected_routes(self):
        """the records ivlm_gemm_route_query must give: (family, BM, BN, operand kind, fp32 epilogue, activation)"""
        if not self.kernel:
            return list(self.routes)
        k, a = OPK[self.opk], ACT[self.act]
        if self.entry in ("splitk", "splitk_fused"):  # fp32 partial tiles, then the reduce launch / "reduced in that launch"
            return [self.kernel + (k, 1, 0), ((3 if self.entry == "splitk" else 4), 0, 0, 0, self.f32_epilogue, a)]
        return [self.kernel + (k, self.f32_epilogue, a)]


# ---- the case table ----------------------------------------------------------------------------------------------------------------
MS, NS, KS = (300, 513), (328, 640), (64, 136, 456)
KS_FP8 = (128, 272, 912)  # the same K tiles in bytes; 272 and 912 are no multiples of 128


def _k(opk, K):
    return KS_FP8[KS.index(K)] if opk == "e4m3" else K


def _entry(opk):
    return "fp8" if opk == "e4m3" else "gemm"


def group_a():
    """plain product on every kernel x output kind x shape; ReLU for bf16 operands; the transposition probe"""
    for (tile, opk), kern in KERNEL.items():
        for out in (("f32", "16") if opk == "e4m3" else ("f32", "16", "split")):
            for M in MS:
                for K in KS:
                    for N in NS:
                        # (ReLU: bf16 operands; 176 x 128 and 256 x 320 are built for their users' activations only)
                        for act in (("none", "relu") if opk == "bf16" and tile not in (176, 320) else ("none",)):
                            yield Case("A", M, N, _k(opk, K), tile, opk, out, act, _entry(opk), kernel=kern)
            yield Case("A", 300, 328, _k(opk, 136), tile, opk, out, "none", _entry(opk), probe=True, kernel=kern)


def group_b():
    """epilogue and addressing features, each alone and one combination, per kernel (bf16 and fp16 operands)"""
    M, N, K = 300, 328, 136
    for (tile, opk), kern in KERNEL.items():
        if opk == "e4m3":
            continue
        mk = lambda **kw: Case("B", kw.pop("M", M), kw.pop("N", N), K, tile, opk, kernel=kern, **kw)
        # (a 16-bit output with a residual is outside the whole-line epilogue: fp32 output on the 256 x 320 kernel)
        if tile != 320:
            yield mk(bias=True, res="bf16", out="16")
        yield mk(bias=True, res="bf16", out="f32")
        yield mk(res="f32")
        yield mk(res="f32", out="split")
        yield mk(res="bf16", res_mod=11, out="f32")
        yield mk(scatter=True, res="f32")
        yield mk(scatter=True, res="f32", M=513)
        yield mk(scatter=True, out="16", bias=True)
        yield mk(gather=True, out="16")
        yield mk(strided=8, bias=True, res="f32")
        yield mk(strided=8, out="16")
        yield mk(a_split=True, out="f32")
        yield mk(a_split=True, out="split")
        yield mk(bias=True, res="f32", scatter=True, gather=True, strided=8)  # the combination
        if opk == "bf16" and tile not in (176, 320):  # an exact activation: the residual comes AFTER it (direct and whole-line epilogues)
            yield mk(act="relu", bias=True, res="bf16", out="16")
            yield mk(act="relu", bias=True, res="f32")
        if tile != 320:  # (the 256 x 320 kernel has the whole-line epilogue only: a forced 320 falls back to 128 x 128 for these)
            yield mk(strided=2, bias=True, res="f32")
            yield mk(strided=2, out="16", res="bf16")
            yield mk(strided=2, out="split")
            yield mk(batch=3, bias=True, res="bf16", out="16")
            yield mk(batch=3, res="f32", strided=8)
            for out in ("f32", "16", "split"):
                yield mk(N=330, out=out, bias=True, res="bf16" if out != "f32" else "f32")
    # e4m3 output (out_kind 2), power-of-two scale_out (N % 4 != 0 is rejected on the host: tests/test_gemm_exact_cases_cpu.py)
    for tile in (64, 128, 512):
        yield Case("B", 300, 328, 272, tile, "e4m3", "e4m3", "none", "fp8", bias=True, kernel=KERNEL[(tile, "e4m3")])
        yield Case("B", 513, 640, 912, tile, "e4m3", "e4m3", "none", "fp8", res="bf16", kernel=KERNEL[(tile, "e4m3")])
        yield Case("B", 300, 328, 272, tile, "e4m3", "f32", "none", "fp8", bias=True, res="f32", scatter=True, gather=True, strided=8,
                   kernel=KERNEL[(tile, "e4m3")])


def group_c():
    """activations on every kernel that has them; SwiGLU with fp32, 16-bit, split and e4m3-pair outputs"""
    for (tile, opk), kern in KERNEL.items():
        for act in acts_of(tile, opk):
            outs = ["f32"]
            if act == "swiglu":
                outs += ["e4m3"] if opk == "e4m3" else ["split"]
            for out in outs:
                yield Case("C", 300, 328, _k(opk, 136), tile, opk, out, act, _entry(opk), bias=True, vals="act", kernel=kern)
            if act != "swiglu":  # ... and the residual after it
                yield Case("C", 300, 328, _k(opk, 136), tile, opk, "f32", act, _entry(opk), bias=True, res="f32", vals="act", kernel=kern)
            # 16-bit store of an activation: inputs on the positive side, where an fp32 error of the bound rarely crosses a rounding tie
            if opk == "bf16" or act == "swiglu":
                yield Case("C", 300, 328, _k(opk, 136), tile, opk, "16", act, _entry(opk), bias=True, vals="pos", kernel=kern)


def group_d():
    """split-K through both entry points against the integer reference"""
    combos = (dict(out="f32", bias=True, res="f32"), dict(out="16", bias=True, res="bf16"),
              dict(out="split", res="f32", res_mod=11), dict(out="16", bias=True, panel="w"), dict(out="f32", panel="w", res="bf16"),
              dict(out="f32", bias=True, res="f32", act="relu"))
    for entry in ("splitk", "splitk_fused"):
        for tile in (64, 96, 128, 176, 512):
            if tile == 512 and entry == "splitk":
                continue
            # (fused: a forced 512 is remapped to 128 x 128, the documented behaviour of that entry point)
            kern = (GEMM_TILE, 128, 128) if tile == 512 else KERNEL[(tile, "bf16")]
            for splits in (2, 3, 4):
                for i, kw in enumerate(combos):
                    K = {2: 384, 3: 192, 4: 768}[splits] if kw.get("panel") else {2: 192, 3: 384, 4: 768}[splits]
                    if tile == 512 and i not in (0, 3):
                        continue
                    yield Case("D", 300, 328, K, tile, "bf16", entry=entry, splits=splits, kernel=kern, **kw)


def group_e():
    """K-panel layouts of A, W and C (kstep > rows * 64), alone and together"""
    for tile in (64, 128, 256, 512):
        for K in (64, 192, 448):
            for i, panel in enumerate(("A", "W", "C", "AWC")):
                epi = ("plain", "bias", "gelu")[(i + K // 64) % 3]
                out = "16" if "C" in panel else ("f32" if i == 0 else "16")
                vals = "int" if epi != "gelu" else ("pos" if out == "16" else "act")
                yield Case("E", 300, 384, K, tile, "bf16", out, "gelu" if epi == "gelu" else "none", "panel", bias=epi != "plain",
                           panel=panel, vals=vals, kernel=KERNEL[(tile, "bf16")])


# the one shape that provably splits: 32 x 9 = 288 tiles of 256^2 -> 2048 columns on the 8-phase kernel + a 256-column strip
F_SHAPE = (8192, 2304, 2048)


def group_f():
    M, N, K = F_SHAPE
    two = lambda f32: ((GEMM_256P, 256, 256, 0, f32, 0), (GEMM_TILE, 128, 64, 0, f32, 0))
    yield Case("F", M, N, K, out="f32", res="f32", routes=two(1))
    yield Case("F", M, N, K, out="16", bias=True, routes=two(0))
    yield Case("F", M, N, K, out="16", entry="panel", panel="C", routes=two(0))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for gen in (group_a, group_b, group_c, group_d, group_e, group_f):
        out += list(gen())
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:4]
    return tuple(out)


def cases_of(group):
    return [c for c in cases() if c.group == group]


# ---- operands, reference ------------------------------------------------------------------------------------------------------------
SENT16, SENT32, SENT8 = 0x7B5A, 0x7B5A7B5A, 0x5A  # sentinel bit patterns of untouched output (finite values no case produces)


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64).double()


@functools.lru_cache(maxsize=64)
def _operands(M, N, K, vals, a_split, probe, opk, seed):
    """-> x [M, K], w [N, K] (float64, exact in the operand format), granule of their products"""
    gen = torch.Generator().manual_seed(seed)
    if vals == "int":
        w, gw = _ints(gen, (N, K), -3, 3), 1.0
        if a_split:  # fp32 activations n + j 2^-10: hi = n, lo = j 2^-10 in either 16-bit format
            n = _ints(gen, (M, K), 4, 7) * (2.0 * _ints(gen, (M, K), 0, 1) - 1.0)
            x, gx = n + _ints(gen, (M, K), -1, 1) * 2.0 ** -10, 2.0 ** -10
            w = _ints(gen, (N, K), -2, 2)
        elif probe:
            x, gx = torch.zeros(M, K, dtype=torch.float64), 1.0
            x[torch.arange(M), torch.arange(M) % K] = 1.0
            w = _ints(gen, (N, K), -4, 4) + (torch.arange(N).double()[:, None] % 5)  # asymmetric
        else:
            x, gx = _ints(gen, (M, K), -4, 4), 1.0
    else:
        x, gx = _ints(gen, (M, K), -3, 3), 1.0
        w, gw = _ints(gen, (N, K), -1, 1) * 0.125, 0.125
        if vals == "pos":  # z >= ~1.5: non-negative operands, thinned so that z stays small
            x = _ints(gen, (M, K), 0, 1) * _ints(gen, (M, K), 0, 1)
            w = _ints(gen, (N, K), 0, 1) * 0.125
        if opk == "e4m3":  # (the per-tensor scales of the e4m3 cases multiply by 2^-3; K is twice as long: narrower x)
            w, gw = w * 8.0, 1.0
            if vals == "act":
                x = _ints(gen, (M, K), -2, 2)
    return x, w, gx * gw


@functools.lru_cache(maxsize=16)
def _product(M, N, K, vals, a_split, probe, opk, seed):
    x, w, g = _operands(M, N, K, vals, a_split, probe, opk, seed)
    return x @ w.T  # float64: exact (every partial sum is below 2^24 granules)


def act_f64(z, act):
    """the true function on float64"""
    if act == "gelu":
        return 0.5 * z * torch.erfc(-z / math.sqrt(2.0))
    if act == "quick_gelu":
        return z * torch.sigmoid(1.702 * z)
    if act == "relu":
        return torch.clamp(z, min=0.0)
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "sigmoid":
        return torch.sigmoid(z)
    if act == "swiglu":
        g, u = z[..., 0::2], z[..., 1::2]
        return g * torch.sigmoid(g) * u
    return z


def _dt16(c):
    """the 16-bit output format: fp16 for fp16 operands, bf16 otherwise - and bf16 for the 16-bit store of an activation (the fp16
    spacing is 8 x finer: an fp32 error of the activation's bound crosses its rounding ties in more than 0.1 % of an output; the
    fp16 pack itself is compared exactly in groups A and B)"""
    return torch.float16 if c.opk == "fp16" and not (c.vals != "int" and c.out == "16") else torch.bfloat16


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _sentinel(n, dtype):
    if dtype == torch.uint8:
        return torch.full((n,), SENT8, dtype=torch.uint8)
    if dtype == torch.float32:
        return torch.full((n,), SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full((n,), SENT16, dtype=torch.int16).view(dtype)


def split_planes(v, dtype):
    """[hi | lo] of an fp32-exact value: hi = dtype(v), lo = dtype(v - hi)"""
    hi = v.to(dtype)
    return hi, (v - hi.double()).to(dtype)


def encode(c, v):
    """float64 result -> the stored planes (one tensor, or hi and lo)"""
    if c.out == "f32":
        return (v.float(),)
    if c.out == "16":
        return (v.to(_dt16(c)),)
    if c.out == "split":
        return split_planes(v, _dt16(c))
    return (torch.clamp(v / SCALE_OUT, -448.0, 448.0).float().to(torch.float8_e4m3fn).view(torch.uint8),)


SCALE_A, SCALE_W, SCALE_OUT = 0.5, 0.25, 0.5  # the per-tensor scales of the e4m3 cases (powers of two: exact)


@dataclasses.dataclass
class Built:
    case: Case
    A: torch.Tensor            # operand buffers as the call takes them (16-bit / uint8, flat)
    W: torch.Tensor
    bias: torch.Tensor | None
    res: torch.Tensor | None   # None also when the residual IS the output buffer (in-place scatter)
    c_init: torch.Tensor       # flat output buffer before the call (sentinel; the residual stream when in place)
    a_rows: torch.Tensor | None
    out_rows: torch.Tensor | None
    idx: torch.Tensor          # [batch, M, n_out] flat element offset of every result in the output buffer, -1 = dropped
    z: torch.Tensor | None     # exact pre-activation incl. bias [batch, M, N] float64 (None: too large for the CPU, group F)
    rsd: torch.Tensor | None   # residual term of every result [batch, M, n_out] float64
    ref: torch.Tensor | None   # act(z) + residual, float64
    args: dict                 # strides and the like
    granule: float
    budget: float              # max (sum |x||w| + |bias| + |residual|) / granule: < 2^24

    def expected(self):
        """the whole output buffer after the call, bit for bit (exact cases)"""
        planes = encode(self.case, self.ref)
        full = self.c_init.clone()
        ok = self.idx >= 0
        for p, off in zip(planes, (0, self.args["c_lo"])):
            full[self.idx[ok] + off] = p[ok]
        return full


def make_case(c: Case, with_ref=True) -> Built:
    M, N, K, B = c.M, c.N, c.K, c.batch
    fp8 = c.opk == "e4m3"
    dt = torch.float8_e4m3fn if fp8 else (torch.float16 if c.opk == "fp16" else torch.bfloat16)
    seed = (M * 31 + N * 17 + K * 7 + len(c.vals)) & 0xffff
    gen = torch.Generator().manual_seed(seed + 1)
    Msrc = M + 37 if c.gather else M
    xs, ws, zs = [], [], []
    for b in range(B):
        key = (Msrc, N, K, c.vals, c.a_split, c.probe, c.opk, seed + 101 * b)
        x, w, g_prod = _operands(*key)
        xs.append(x), ws.append(w)
        if with_ref:
            zs.append(_product(*key))
    assert not fp8 or max(float(x.abs().max()), float(w.abs().max())) <= 8.0
    alpha = SCALE_A * SCALE_W if fp8 else 1.0
    act_vals = c.vals != "int"
    granule = min(g_prod * alpha, 0.0625) if act_vals else g_prod * alpha  # (activation cases: the bias is on a 2^-4 grid)
    a_rows = torch.randint(0, Msrc, (M,), generator=gen, dtype=torch.int32) if c.gather else None

    # ---- A: rows [hi | lo] for a split operand; junk behind every row where the rows are strided --------------------------------
    Kw = 2 * K if c.a_split else K
    gran = 16 if fp8 else 8
    lda, ldw = (Kw + 3 * gran, K + gran) if c.strided == 8 else (Kw, K)
    junk = 6.0
    def rows(mat, ld):
        buf = torch.full((mat.shape[0], ld), junk, dtype=torch.float64)
        buf[:, :mat.shape[1]] = mat
        return buf
    a_kstep = w_kstep = 0
    A_parts, W_parts = [], []
    for x, w in zip(xs, ws):
        if c.a_split:
            hi, lo = split_planes(x, dt)
            assert torch.equal(hi.double() + lo.double(), x), "hi + lo must be the fp32 value exactly"
            x = torch.cat([hi.double(), lo.double()], 1)
        if "A" in c.panel:  # element (r, k) at (k / 64) * kstep + r * 64 + k % 64, kstep > 64 rows
            a_kstep = 64 * Msrc + 64
            p = torch.full((K // 64, a_kstep), junk, dtype=torch.float64)
            p[:, :64 * Msrc] = x.view(Msrc, K // 64, 64).permute(1, 0, 2).reshape(K // 64, -1)
            A_parts.append(p.flatten())
        else:
            A_parts.append(rows(x, lda).flatten())
        if c.panel in ("w",) or "W" in c.panel:
            w_kstep = 64 * N + (0 if c.panel == "w" else 128)  # (the flag form has kstep = 64 N by definition)
            p = torch.full((K // 64, w_kstep), junk, dtype=torch.float64)
            p[:, :64 * N] = w.view(N, K // 64, 64).permute(1, 0, 2).reshape(K // 64, -1)
            W_parts.append(p.flatten())
        else:
            W_parts.append(rows(w, ldw).flatten())
    pad = torch.full((gran * 2,), junk, dtype=torch.float64)  # batch strides larger than the matrices
    strideA, strideW = A_parts[0].numel() + pad.numel(), W_parts[0].numel() + pad.numel()
    A = torch.cat([t for p in A_parts for t in (p, pad)]).to(dt)
    W = torch.cat([t for p in W_parts for t in (p, pad)]).to(dt)

    # ---- epilogue operands ------------------------------------------------------------------------------------------------------
    bias = None
    if c.bias:
        bias = (_ints(gen, (N,), -16, 16) * 0.0625) if act_vals else _ints(gen, (N,), -8, 8) * granule
        if c.vals == "pos":
            bias = bias.abs() + 1.5
    n_out = c.n_out
    Mc = M + 40 if c.scatter else M
    out_rows = None
    dst = torch.arange(M)
    if c.scatter:
        dst = torch.randperm(Mc, generator=gen)[:M]
        dst[torch.rand(M, generator=gen) < 0.1] = -1
        dst[-1] = -1  # (the last row of a ragged row tile is dropped)
        out_rows = dst.to(torch.int32)
    inplace = c.scatter and c.res == "f32" and c.out == "f32"
    planes = 2 if c.out == "split" else 1
    padc = {0: 8, 8: 24, 2: 6}[c.strided]
    if c.out == "e4m3":  # (an e4m3 output needs ldc % 4 == 0)
        padc += -(n_out + padc) % 4
    ldc = planes * n_out + padc
    if c.strided == 2:
        assert N % 4 == 0 and ldc % 4 == 2
    ldr = ldc if inplace else N + padc
    Mr = c.res_mod if c.res_mod else Mc
    rdt = torch.float32 if c.res == "f32" else torch.bfloat16
    odt = {"f32": torch.float32, "16": _dt16(c), "split": _dt16(c), "e4m3": torch.uint8}[c.out]
    R = None
    if c.res:
        rv = _ints(gen, (B, Mr, N), -1000 if c.res == "f32" else -64, 1000 if c.res == "f32" else 64) * (granule if not act_vals else 0.0625)
        R = torch.empty(B, Mr + 1, ldr, dtype=rdt)  # (one spare row = the batch stride is larger than the matrix)
        R.view(-1)[:] = _sentinel(R.numel(), rdt)
        R[:, :Mr, :N] = rv.to(rdt)
        assert torch.equal(R[:, :Mr, :N].double(), rv)
    strideR = (Mr + 1) * ldr
    # ---- C: spare rows, spare columns, sentinel; flat offsets of the results ----------------------------------------------------
    c_panel = 0
    m_i, n_i = torch.arange(M)[:, None], torch.arange(n_out)[None, :]
    if "C" in c.panel:
        c_panel = 64 * M + 192  # a gap between the panels
        numel = (N // 64) * c_panel + 64
        idx = ((n_i >> 6) * c_panel + m_i * 64 + (n_i & 63))[None]
        strideC = numel
    else:
        strideC = (Mc + 3) * ldc
        numel = B * strideC
        base = torch.where(dst[:, None] >= 0, dst[:, None] * ldc + n_i, -1)
        idx = torch.stack([torch.where(base >= 0, base + b * strideC, base) for b in range(B)])
    if inplace:  # the fp32 residual stream is the output
        assert B == 1
        c_init = R[0].flatten().clone()
        c_init = torch.cat([c_init, _sentinel(numel - c_init.numel(), odt)])
        R = None
    else:
        c_init = _sentinel(numel, odt)

    # ---- reference and budget ---------------------------------------------------------------------------------------------------
    rsd = None
    if c.res:
        rrow = dst.clamp(min=0)
        rrow = rrow % c.res_mod if c.res_mod else rrow
        rsd = rv[:, rrow, :]
    amax = lambda t: 0.0 if t is None else float(t.abs().max())
    xmax = max(amax(x) for x in xs) + (2.0 ** -10 if c.a_split else 0.0)
    # (sum_k |x||w| <= K max|x| max|w|: the bound, not the sum - it also covers any grouping of partial sums)
    budget = (K * xmax * max(amax(w) for w in ws) * alpha + amax(bias) + (amax(rv) if c.res else 0.0)) / granule
    assert budget < 2 ** 24, (c.id, budget)
    for t in (bias, rsd):
        assert t is None or torch.equal(torch.round(t / granule) * granule, t), c.id
    z = ref = None
    if with_ref:
        z = torch.stack(zs)
        if c.gather:
            z = z[:, a_rows.long(), :]
        z = z * alpha + (bias if c.bias else 0.0)
        assert torch.equal(z.float().double(), z)
        ref = act_f64(z, c.act) + (rsd if c.res else 0.0)
    bias16 = None
    if c.bias:
        bias16 = torch.cat([bias, torch.full((8,), 99.0, dtype=torch.float64)]).to(torch.bfloat16)
        assert torch.equal(bias16[:N].double(), bias)
    args = dict(lda=lda, ldw=ldw, ldc=ldc, ldr=ldr, a_kstep=a_kstep, w_kstep=w_kstep, c_panel=c_panel, strideA=strideA, strideW=strideW,
                strideC=strideC, strideR=strideR, c_lo=n_out, inplace=inplace, odt=odt)
    return Built(c, A.view(torch.uint8) if fp8 else A, W.view(torch.uint8) if fp8 else W, bias16, R, c_init, a_rows, out_rows, idx, z, rsd,
                 ref, args, granule, budget)


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def flags_of(c):
    f = RES_F32 if c.res == "f32" else 0
    if c.opk == "fp16":
        f |= F16 | (OUT_F16 if c.out in ("16", "split") and _dt16(c) == torch.float16 else 0)
    if c.a_split:
        f |= A_SPLIT
    if c.out == "split":
        f |= OUT_SPLIT
    if c.panel == "w":
        f |= W_PANEL
    return f


def out_kind_of(c):
    if c.entry == "fp8":  # IVLM_F32 0 | IVLM_BF16 1 | 2 = e4m3
        return {"f32": 0, "16": 1, "e4m3": 2}[c.out]
    return int(c.out == "f32")


def query_args(c, a):
    """the 21 leading arguments of ivlm_gemm_route_query for the call ``run_case`` makes (a = Built.args)"""
    return (ENTRY[c.entry], c.M, c.N, c.K, a["lda"], 64 if c.panel == "w" else a["ldw"], a["ldc"], a["ldr"], a["a_kstep"],
            0 if c.panel == "w" else a["w_kstep"], a["c_panel"], ACT[c.act], out_kind_of(c), int(c.bias), int(bool(c.res)), c.res_mod,
            c.batch, flags_of(c), int(c.scatter), int(c.gather), c.splits)


class hooks:
    """the case's hooks for the duration of a block; always restored"""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c

    def __enter__(self):
        self.prev = self.lib.ivlm_gemm_tile_override(self.c.tile)
        self.lib.ivlm_gemm_nsplit(self.c.nsplit)

    def __exit__(self, *exc):
        self.lib.ivlm_gemm_tile_override(self.prev)
        self.lib.ivlm_gemm_nsplit(1)


def route_records(lib, c, a):
    """what the call would launch: [(family, BM, BN, operand kind, fp32 epilogue, act)], or [(-1, rc)] for a rejected call"""
    buf = (ctypes.c_int32 * (9 * 8))()
    with hooks(lib, c):
        n = lib.ivlm_gemm_route_query(*query_args(c, a), ctypes.cast(buf, ctypes.c_void_p), 8)
    assert 1 <= n <= 8, (c.id, n)
    return [tuple(buf[9 * r:9 * r + (2 if buf[9 * r] == -1 else 6)]) for r in range(n)]


def run_case(lib, b: Built, dev, stream=0, scratch=None, repeat=1):
    """Upload, launch (``repeat`` times into fresh copies of the output buffer), -> (return code, [flat output buffers on the device])."""
    c, a = b.case, b.args
    up = lambda t: None if t is None else t.to(dev)
    A, W, bias, R, ar, orow = up(b.A), up(b.W), up(b.bias), up(b.res), up(b.a_rows), up(b.out_rows)
    p = lambda t: 0 if t is None else t.data_ptr()
    fl, ok = flags_of(c), out_kind_of(c)
    outs, rc = [], OK
    with hooks(lib, c):
        for _ in range(repeat):
            C = b.c_init.to(dev)
            Rp = C.data_ptr() if a["inplace"] else p(R)
            ldw = 64 if c.panel == "w" else a["ldw"]
            if c.entry == "gemm":
                rc = lib.ivlm_gemm_bf16(p(A), a["lda"], p(W), ldw, p(C), a["ldc"], p(bias), Rp, a["ldr"], c.res_mod, c.M, c.N, c.K, ACT[c.act],
                                        ok, c.batch, a["strideA"], a["strideW"], a["strideC"], a["strideR"], 0, 0.0, fl, p(orow), p(ar), stream)
            elif c.entry == "panel":
                rc = lib.ivlm_gemm_bf16_panel(p(A), a["lda"], a["a_kstep"], p(W), a["ldw"], a["w_kstep"], p(C), a["ldc"], a["c_panel"], p(bias),
                                              Rp, a["ldr"], c.M, c.N, c.K, ACT[c.act], ok, fl, p(orow), p(ar), stream)
            elif c.entry == "fp8":
                sc = scratch["scales"]
                rc = lib.ivlm_gemm_fp8(p(A), a["lda"], p(W), a["ldw"], p(C), a["ldc"], p(bias), Rp, a["ldr"], c.M, c.N, c.K, ACT[c.act], ok,
                                       sc[0:1].data_ptr(), sc[1:2].data_ptr(), sc[2:3].data_ptr(), fl, p(orow), p(ar), stream)
            else:
                ws = scratch["ws"]
                assert ws.numel() * 4 >= lib.ivlm_gemm_splitk_workspace_bytes(c.M, c.N, c.splits)
                common = (p(A), a["lda"], p(W), ldw, p(C), a["ldc"], p(bias), Rp, a["ldr"], c.res_mod, c.M, c.N, c.K, ACT[c.act], ok, c.splits,
                          ws.data_ptr(), ws.numel() * 4)
                if c.entry == "splitk":
                    rc = lib.ivlm_gemm_bf16_splitk(*common, fl, stream)
                else:
                    rc = lib.ivlm_gemm_bf16_splitk_fused(*common, scratch["counters"].data_ptr(), fl, stream)
            outs.append(C)
            if rc != OK:
                break
    return rc, outs


# ---- activations: the tolerance covers the activation formula alone --------------------------------------------------------------------
# max |got - ref| / max(1, |ref|) of the fp32 result against float64 of the true function on the exact pre-activation, measured on an
# MI355X over every case of groups C and E (all kernels, operand kinds and entry points give the same figures: one epilogue), and the
# committed bound = 4 x that.  No bound may exceed 2^-16.
ACT_MEASURED = {"gelu": 2.112e-7, "quick_gelu": 1.036e-7, "silu": 9.947e-8, "sigmoid": 8.524e-8, "swiglu": 3.050e-7}
ACT_BOUND = {a: 4.0 * m for a, m in ACT_MEASURED.items()}
assert max(ACT_BOUND.values()) <= 2.0 ** -16


def decode(c, t):
    """stored 16-bit / e4m3 / fp32 values -> float64"""
    return (t.view(torch.float8_e4m3fn).float().double() * SCALE_OUT) if c.out == "e4m3" else t.double()


def rounded_window(c, ref, bound):
    """the stored values of ref -+ bound * max(1, |ref|), as float64: rounding is monotonic, so an fp32 result within the bound of
    ``ref`` is stored as a value inside [lo, hi] - and as the rounded reference itself wherever lo == hi."""
    d = bound * torch.clamp(ref.abs(), min=1.0)
    return decode(c, encode(c, ref - d)[0]), decode(c, encode(c, ref + d)[0])
