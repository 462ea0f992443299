"""The weight-streaming linears (gemv.hip, gemv_p12.hip, gemv_mfma.hip) share their prologue and finish code (gemv_common.h).  These
cases sit where shared finish code can go wrong and that the model-size tests do not reach: blocks whose last waves own no row in front of
the SwiGLU barrier, K halves of unequal length, the clamped last row of the two-rows-per-wave form, broadcast residual rows, tiles and
row pointers past N, every activation / bias / residual / output-type arm.  Every case: a few thousand weights, forced onto its kernel
with the library's tuning hooks, against torch fp64 on the same operands, launched twice (bit-equal).

Tolerances are those of the model-size tests of the same kernel, e of the output range (max |reference|):
  fp32 rows on bf16 weights (exact products), on bf16 or 12-bit weights with the hi + lo operand split (M <= 16)   3e-5  (test_dense_gpu.py)
  gemv1_p12_kernel and gemv1_p12m_kernel (M = 1 on 12-bit weights)   3e-6  (test_dense_gpu.py, test_gemv_bf12_staging_gpu.py)
  e4m3 weights, against the dequantised matrix                                            2e-5 of max(1, range)  (test_fp8_gpu.py)
  bf16 rows (operand-rounded RMS prologue): atol 2e-3, rtol 1e-3 for fp32 output, atol 2e-2, rtol 1.6e-2 for bf16 output
A bf16 OUTPUT of an fp32-row kernel is the round-to-nearest bf16 (8 significant bits: unit roundoff 2^-8) of a value v within e of the
reference y: |out - y| <= |v| 2^-8 + e <= e (1 + 2^-8) + |y| 2^-8, which is what such a case asserts.

Planted patches (12-bit weights): in three rows - the gate / up pair (2, 3) and row 21 of the next 16-row tile - one weight of 64 ends
the row's exponent window at 64 x 2^-14 = 3.9e-3 and one of 2e-3 falls under it.  The 64 meets x = 0.25: + 16, so neither ReLU nor the
SwiGLU pairing hides the row.  The patch meets x = 8: 1.6e-2 in the row's sum, far above e, and the case asserts that the reference
WITHOUT the patches misses the bound."""
from collections import namedtuple

import pytest

pytestmark = pytest.mark.gpu

EPS = 1e-5
Case = namedtuple("Case", "name route M N K act bias rms res res_mod out_f32 x_bf16 plant hooks tol")
Case.__new__.__defaults__ = ("none", False, False, None, 0, True, False, 0, (), 3e-5)

# (hook, arguments that force the route, arguments that restore the default)
KS2 = (("ivlm_gemv1_tuning", (2,), (0,)),)
LEGACY = (("ivlm_gemv_tuning", (-1, 0), (0, 0)),)      # M = 1 fp32 rows also take the persistent gemv_kernel
ROWS2 = (("ivlm_gemv_tuning", (-1, 16), (0, 0)),)      # ... and two weight rows per wave from N > 16 on
WAVES8 = (("ivlm_gemv1_bf12m_tuning", (0,), (256,)),)  # no grid is "at most 0 blocks": the 8-wave form


def _skinny(t):  # the skinny MFMA kernel for every M, t tiles per block (0 = its rule)
    return (("ivlm_gemv_mfma_min_m", (1,), (0,)), ("ivlm_skinny_tuning", (t,), (0,)))


def _tiles12(t):
    return (("ivlm_gemv16_bf12m_tuning", (t,), (0,)),)


def _legacy(tag, M, x_bf16):
    kw = dict(M=M, x_bf16=x_bf16, hooks=LEGACY if M == 1 else ())
    rows2 = dict(kw, hooks=ROWS2)
    return [
        Case(f"legacy-{tag}-gelu-bias-rms", "gemv", N=33, K=64, act="gelu", bias=True, rms=True, **kw),
        Case(f"legacy-{tag}-swiglu", "gemv", N=34, K=64, act="swiglu", **kw),
        Case(f"legacy-{tag}-rows2-odd-n", "gemv", N=33, K=64, act="relu", bias=True, res="f32", **rows2),  # rows (32, 32): clamped
        Case(f"legacy-{tag}-rows2-bf16-out", "gemv", N=33, K=64, res="bf16", out_f32=False, **rows2),
    ]


CASES = [
    # gemv1_kernel (M = 1, fp32 row, 16 rows per block)
    Case("gemv1-swiglu-rms-dead-waves", "gemv", 1, 40, 64, act="swiglu", rms=True),  # last block: 8 live waves, 8 dead ones
    Case("gemv1-relu-bias-bf16-res-bf16-out", "gemv", 1, 24, 72, act="relu", bias=True, res="bf16", out_f32=False),
    Case("gemv1-ks2-f32-res", "gemv", 1, 17, 2112, res="f32", hooks=KS2),  # 264 chunks: K halves of 192 and 72
    # the persistent gemv_kernel: M = 1 fp32 by hook, M = 3 fp32 rows and M = 2 bf16 rows by shape
    *_legacy("m1-f32", 1, False), *_legacy("m3-f32", 3, False), *_legacy("m2-bf16", 2, True),
    Case("legacy-m3-f32-res-mod", "gemv", 3, 33, 64, act="silu", bias=True, res="f32", res_mod=2),
    Case("legacy-m2-bf16-res-mod", "gemv", 2, 33, 64, bias=True, res="bf16", res_mod=1),
    # e4m3 weights
    Case("fp8w-swiglu-rms-dead-waves", "fp8w", 1, 40, 64, act="swiglu", rms=True, tol=2e-5),
    # 12-bit weights, row layout (VALU kernel): shapes the fragment layout does not take; planted patches
    Case("p12-swiglu-rms", "bf12", 1, 40, 80, act="swiglu", rms=True, plant=1, tol=3e-6),
    Case("p12-relu-bias-bf16-res", "bf12", 1, 24, 48, act="relu", bias=True, res="bf16", plant=1, tol=3e-6),
    # 12-bit weights, fragment layout, M = 1 (gemv1_p12m_kernel)
    Case("p12m-16-waves", "bf12", 1, 32, 320, act="relu", bias=True, res="bf16", out_f32=False, tol=3e-6),
    Case("p12m-8-waves", "bf12", 1, 32, 320, act="relu", bias=True, res="bf16", out_f32=False, hooks=WAVES8, tol=3e-6),
    # skinny_mfma_kernel (takes N, K >= 1024 only: the smallest ragged shape - 64.5 tiles, 32.25 k-steps)
    *[Case(f"skinny-{'bf16' if xb else 'f32'}-t{t}", "gemv", 3, 1032, 1032, act="gelu", bias=True, x_bf16=xb, hooks=_skinny(t))
      for xb in (False, True) for t in (0, 2, 3)],  # t = 2, 3: the last block's row pointers clamp past N
    Case("skinny-bf16-swiglu-rms-bf16-out", "gemv", 3, 1032, 1032, act="swiglu", rms=True, x_bf16=True, out_f32=False, hooks=_skinny(3)),
    Case("skinny-f32-res-mod", "gemv", 3, 1032, 1032, bias=True, res="f32", res_mod=2, hooks=_skinny(2)),
    # skinny_p12m_kernel: 5 tiles; T = 2, 3: the last block owns a tile past N
    *[Case(f"skinny-p12m-swiglu-rms-t{t}", "bf12", 5, 80, 128, act="swiglu", rms=True, plant=1, hooks=_tiles12(t))
      for t in (1, 2, 3)],  # (patches under RMS: times gamma, in front of the row scale)
    *[Case(f"skinny-p12m-relu-bias-res-patches-t{t}", "bf12", 5, 80, 128, act="relu", bias=True, res="f32", plant=1, hooks=_tiles12(t))
      for t in (1, 2, 3)],
]
PLANT_ROWS = (2, 3, 21)


def _act(y, act):
    import torch
    import torch.nn.functional as F

    if act == "swiglu":
        return F.silu(y[:, 0::2]) * y[:, 1::2]
    return {"none": lambda v: v, "gelu": F.gelu, "relu": torch.relu, "silu": F.silu}[act](y)


def run_case(lib, dev, c):
    """-> (first launch, second launch, fp64 reference on the same operands, the reference without the planted patches or None)"""
    import torch

    from interactvlm_amd import ops

    g = torch.Generator().manual_seed(1000 * c.M + 7 * c.N + c.K)
    w = (torch.randn(c.N, c.K, generator=g) / c.K ** 0.5).bfloat16()
    x = torch.randn(c.M, c.K, generator=g) * 2.0
    if c.plant:
        x[:, 1] = 0.25
        for r in PLANT_ROWS:
            w[r, 1], w[r, 9 + r] = 64.0, 2e-3
            x[:, 9 + r] = 8.0
    if c.x_bf16:
        x = x.bfloat16()
    gam = (1 + 0.1 * torch.randn(c.K, generator=g)).bfloat16()
    b = (0.1 * torch.randn(c.N, generator=g)).bfloat16() if c.bias else None
    res = None
    if c.res:
        res = torch.randn(c.res_mod or c.M, c.N, generator=g)
        res = res.bfloat16() if c.res == "bf16" else res
    dv = lambda t: None if t is None else t.to(dev)
    kw = dict(bias=dv(b), act=c.act, residual=dv(res), out_f32=c.out_f32, rms=(dv(gam), EPS) if c.rms else None)
    wd = w.double()
    if c.route == "gemv":
        xg, wg = dv(x), dv(w)
        call = lambda: ops.linear(xg, wg, res_mod=c.res_mod, **kw)
    elif c.route == "fp8w":
        xg = dv(x)
        wq, sw = ops.quantize_fp8(dv(w))
        wd = wq.cpu().view(torch.float8_e4m3fn).float().double() * float(sw)
        call = lambda: ops.linear_fp8w(xg, wq, sw, **kw)
    else:
        xg, wp = dv(x), ops.PackedBf12(dv(w))
        assert wp.frag == ops.PackedBf12.takes(c.N, c.K) and wp.n_patches >= (len(PLANT_ROWS) if c.plant else 0)
        call = lambda: ops.linear_bf12(xg, wp, **kw)
    xd = x.double()
    if c.rms:
        rstd = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS)
        # (bf16 rows: the kernels round x * gamma to the bf16 operand of the product)
        xd = (x.float() * gam.float()).bfloat16().double() * rstd if c.x_bf16 else xd * gam.double() * rstd

    def ref(wd):
        y = xd @ wd.T
        if c.bias:
            y = y + b.double()
        y = _act(y, c.act)
        if c.res:
            rd = res.double()
            y = y + (rd[torch.arange(c.M) % c.res_mod] if c.res_mod else rd)
        return y

    y, y_unpatched = ref(wd), None
    if c.plant:
        w0 = wd.clone()
        for r in PLANT_ROWS:
            w0[r, 9 + r] = 0.0
        y_unpatched = ref(w0)
    try:
        for name, on, _ in c.hooks:
            getattr(lib, name)(*on)
        got, again = call(), call()
        torch.cuda.synchronize()
    finally:
        for name, _, off in c.hooks:
            getattr(lib, name)(*off)
    return got, again, y, y_unpatched


def _within(got, y, c):
    """the case's bound (module docstring) -> (holds, max error)"""
    err = (got.double().cpu() - y).abs()
    rng = float(y.abs().max())
    if c.x_bf16:
        atol, rtol = (2e-3, 1e-3) if c.out_f32 else (2e-2, 1.6e-2)
        return bool((err <= atol + rtol * y.abs()).all()), float(err.max())
    e = c.tol * (max(1.0, rng) if c.route == "fp8w" else rng)
    if c.out_f32:
        return float(err.max()) < e, float(err.max())
    return bool((err <= e * (1 + 2.0 ** -8) + y.abs() * 2.0 ** -8).all()), float(err.max())


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_gemv_family_finish(hip_lib, cuda, c):
    import torch

    got, again, y, y_unpatched = run_case(hip_lib, cuda, c)
    n_out = c.N // 2 if c.act == "swiglu" else c.N
    assert got.shape == (c.M, n_out) and got.dtype == (torch.float32 if c.out_f32 else torch.bfloat16)
    assert torch.equal(got, again)
    assert bool(torch.isfinite(got).all())
    ok, err = _within(got, y, c)
    print(f"\n[gemv family {c.name}] max err {err:.3e} = {err / float(y.abs().max()):.2e} of range")
    assert ok
    if y_unpatched is not None:  # the planted patches matter: without them the result is out of bounds
        missed, err0 = _within(got, y_unpatched, c)
        print(f"[gemv family {c.name}] against the reference without the patches: {err0:.3e}")
        assert not missed
