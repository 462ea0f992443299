"""The tile GEMM kernels against an exact integer reference (tests/_gemm_exact.py): every kernel of the build x output kind, every
epilogue and addressing feature per kernel, split-K through both entry points, the K-panel layouts and the column split.  Operands are
chosen so that fp32 accumulation is exact in any order: outputs are compared BIT FOR BIT over the whole output buffer (spare rows,
spare columns and dropped rows must keep their sentinel), and only the nonlinear activations keep a tolerance - the measured error of
the activation formula (ACT_BOUND in _gemm_exact.py), not of the GEMM.  tests/test_gemm_exact_cases_cpu.py shows that every case
reaches the kernel it names."""
import dataclasses

import pytest
import torch

import _gemm_exact as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scratch(cuda):
    return {"scales": torch.tensor([G.SCALE_A, G.SCALE_W, G.SCALE_OUT], dtype=torch.float32, device=cuda),
            "ws": torch.empty(4 * 513 * 640, dtype=torch.float32, device=cuda),
            "counters": torch.zeros(4096, dtype=torch.int32, device=cuda)}


def _launch(lib, cuda, scratch, b, repeat=1):
    """run_case; a HIP error (a fault is sticky: nothing after it on this device means anything) ends the session at once"""
    rc, outs = G.run_case(lib, b, cuda, scratch=scratch, repeat=repeat)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after {b.case.id}: {e}", returncode=3)
    assert rc == G.OK, (b.case.id, rc)
    return outs


def _explain(b, got, want):
    """where a buffer differs: inside the result region or outside it (a canary)"""
    diff = (got != want).nonzero().flatten()
    inside = torch.zeros(want.numel(), dtype=torch.bool, device=want.device)
    ok = (b.idx >= 0)
    for off in ((0, b.args["c_lo"]) if b.case.out == "split" else (0,)):
        inside[(b.idx[ok] + off).to(want.device)] = True
    n_in = int(inside[diff].sum())
    first = int(diff[0])
    return (f"{b.case.id}: {diff.numel()} elements differ ({n_in} results, {diff.numel() - n_in} outside the result region); first at flat "
            f"offset {first} (ldc {b.args['ldc']}): got {int(got[first]):#x}, want {int(want[first]):#x}")


def _run_exact(lib, cuda, scratch, c, repeat=1):
    b = G.make_case(c)
    outs = _launch(lib, cuda, scratch, b, repeat)
    want = G._bits(b.expected()).to(cuda)
    for C in outs:
        got = G._bits(C)
        assert torch.equal(got, want), _explain(b, got, want)
    return b


def _run_act(lib, cuda, scratch, c):
    """an activation case: the fp32 result within ACT_BOUND of float64 of the true function; a 16-bit / e4m3 store equal to the rounded
    reference except where that error crosses a rounding tie (<= 0.1 % of the output); [hi | lo] planes that add up to such a value.
    Everything outside the result region keeps its bits.  -> the measured max |got - ref| / max(1, |ref|) (fp32 outputs)"""
    b = G.make_case(c)
    C, = _launch(lib, cuda, scratch, b)
    bound = G.ACT_BOUND[c.act]
    C = C.cpu()
    ref, idx = b.ref, b.idx
    untouched = torch.ones(C.numel(), dtype=torch.bool)
    for off in ((0, b.args["c_lo"]) if c.out == "split" else (0,)):
        untouched[idx.flatten() + off] = False
    assert torch.equal(G._bits(C)[untouched], G._bits(b.c_init)[untouched]), f"{c.id}: a value outside the result region changed"
    got = C[idx]
    scale = torch.clamp(ref.abs(), min=1.0)
    err = None
    if c.out == "f32" and c.res:
        # the bound is the activation's, relative to max(1, |act(z)|); the residual is then added in fp32: one more rounding of the sum
        act = G.act_f64(b.z, c.act)
        excess = (got.double() - ref).abs() - (bound * torch.clamp(act.abs(), min=1.0) + 2.0 ** -24 * ref.abs())
        assert float(excess.max()) <= 0.0, (c.id, float(excess.max()))
    elif c.out == "f32":
        err = float(((got.double() - ref).abs() / scale).max())
        print(f"[gemm-exact] {c.id}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (c.id, err, bound)
    elif c.out == "split":
        hi, lo = got.double(), C[idx + b.args["c_lo"]].double()
        # the planes carry 16 (bf16) / 22 (fp16) significant bits of the fp32 value: hi + lo is within 2^-17 / 2^-23 of it
        plane = 2.0 ** (-17 if C.dtype == torch.bfloat16 else -23)
        e = float((((hi + lo) - ref).abs() / scale - plane * ref.abs() / scale).max())
        assert e <= bound, (c.id, e, bound)
        lo_w, hi_w = G.rounded_window(c, ref, bound)  # (and hi is the 16-bit store of such a value)
        assert bool(((hi >= lo_w) & (hi <= hi_w)).all()), (c.id, int(((hi < lo_w) | (hi > hi_w)).sum()))
    else:
        lo, hi = G.rounded_window(c, ref, bound)
        val = G.decode(c, got)
        assert bool(((val >= lo) & (val <= hi)).all()), (c.id, int(((val < lo) | (val > hi)).sum()))
        moved = float((val != G.decode(c, G.encode(c, ref)[0])).double().mean())
        assert moved <= 1e-3, (c.id, moved)
    return err


def _key_cases(group, key):
    return [c for c in G.cases_of(group) if (c.tile, c.opk, c.out) == key]


A_KEYS = sorted({(c.tile, c.opk, c.out) for c in G.cases_of("A")})


@pytest.mark.parametrize("tile,opk,out", A_KEYS, ids=[f"{t}-{k}-{o}" for t, k, o in A_KEYS])
def test_plain_product_is_exact(hip_lib, cuda, scratch, tile, opk, out):
    """Group A: one kernel x operand kind x output kind over M in {300, 513} x N in {328, 640} x K of one tile, two tiles + a tail and
    an odd tile count + a tail (ReLU too for bf16 operands), and the transposition probe."""
    for c in _key_cases("A", (tile, opk, out)):
        _run_exact(hip_lib, cuda, scratch, c)


B_KEYS = sorted({(c.tile, c.opk) for c in G.cases_of("B")})


@pytest.mark.parametrize("tile,opk", B_KEYS, ids=[f"{t}-{k}" for t, k in B_KEYS])
def test_epilogue_and_addressing_features_are_exact(hip_lib, cuda, scratch, tile, opk):
    """Group B: bias / bf16 / fp32 / row-modulo residuals, the out_rows scatter (in place on the fp32 stream, dropped rows), the a_rows
    gather, strided rows (ldc, ldr multiples of 8; and 2 mod 4, which the direct epilogue must take), batch 3, split A, N = 330 through
    the scalar tail, their combination; e4m3 operands: the e4m3 output."""
    for c in G.cases_of("B"):
        if (c.tile, c.opk) == (tile, opk):
            _run_exact(hip_lib, cuda, scratch, c)


def test_split_rows_gives_the_planes_the_cases_use(hip_lib, cuda):
    """the split A operands of group B are built on the CPU; ops.split_rows gives the same [hi | lo] bits"""
    from interactvlm_amd import ops

    x, _, _ = G._operands(300, 328, 136, "int", True, False, "bf16", 7)
    assert torch.equal(x.float().double(), x)
    hi, lo = G.split_planes(x, torch.bfloat16)
    got = ops.split_rows(x.float().to(cuda)).cpu()
    assert torch.equal(G._bits(got), G._bits(torch.cat([hi, lo], 1)))


C_KEYS = sorted({(c.tile, c.opk) for c in G.cases_of("C")})


@pytest.mark.parametrize("tile,opk", C_KEYS, ids=[f"{t}-{k}" for t, k in C_KEYS])
def test_activations_against_float64(hip_lib, cuda, scratch, tile, opk):
    """Group C: GELU, quick-GELU, SiLU, sigmoid and SwiGLU (fp32, 16-bit, split, e4m3-pair outputs) on exact pre-activations in about
    +-8 (both signs, zero, the tails), against float64 of the true function."""
    for c in G.cases_of("C"):
        if (c.tile, c.opk) == (tile, opk):
            _run_act(hip_lib, cuda, scratch, c)


D_KEYS = sorted({(c.entry, c.tile) for c in G.cases_of("D")})


@pytest.mark.parametrize("entry,tile", D_KEYS, ids=[f"{e}-{t}" for e, t in D_KEYS])
def test_split_k_is_exact(hip_lib, cuda, scratch, entry, tile):
    """Group D: 2, 3 and 4 K slices through ivlm_gemm_bf16_splitk and ivlm_gemm_bf16_splitk_fused against the integer reference (not
    against each other); every case twice on the same counters, which every fused call must leave at zero."""
    for c in G.cases_of("D"):
        if (c.entry, c.tile) == (entry, tile):
            _run_exact(hip_lib, cuda, scratch, c, repeat=2)
            assert not bool(scratch["counters"].any()), c.id


@pytest.mark.parametrize("tile", [64, 128, 256, 512])
def test_k_panel_layouts_are_exact(hip_lib, cuda, scratch, tile):
    """Group E: a_kstep, w_kstep and c_panel (each larger than rows x 64: the gaps keep their sentinel), alone and together."""
    for c in G.cases_of("E"):
        if c.tile == tile:
            (_run_exact if c.vals == "int" else _run_act)(hip_lib, cuda, scratch, c)


@pytest.mark.parametrize("i", range(3), ids=["f32-res_f32", "16-bias", "16-c_panel"])
def test_column_split_is_exact(hip_lib, cuda, scratch, i):
    """Group F: 8192 x 2304 x 2048 runs as 2048 columns on the 8-phase kernel + a 256-column strip on 128 x 64 tiles (the CPU test shows
    the two launches): the W, C, bias and residual offsets of the strip.  Exactness makes the float64 product independent of who
    computes it: it is computed on the device.  Both the split and the ivlm_gemm_nsplit(0) launch must equal it bit for bit."""
    c = G.cases_of("F")[i]
    b = G.make_case(c, with_ref=False)
    M, N, K = c.M, c.N, c.K
    A = b.A[:M * K].view(M, K).to(cuda).double()
    W = b.W[:N * K].view(N, K).to(cuda).double()
    ref = A @ W.T
    if c.bias:
        ref += b.bias[:N].to(cuda).double()
    if c.res:
        ref += b.rsd[0].to(cuda)
    assert float(ref.abs().max()) / b.granule < 2 ** 24
    want = b.c_init.to(cuda)
    want[b.idx[0].to(cuda)] = G.encode(c, ref)[0]
    want = G._bits(want)
    for nsplit in (1, 0):
        C, = _launch(hip_lib, cuda, scratch, dataclasses.replace(b, case=dataclasses.replace(c, nsplit=nsplit)))
        assert torch.equal(G._bits(C), want), f"nsplit {nsplit}: " + _explain(b, G._bits(C), want)
