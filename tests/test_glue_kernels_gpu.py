"""The kernels between the GEMMs and the attentions, each against a plain CPU reference (tests/_glue_ref.py, itself pinned by
tests/test_glue_ref_cpu.py): the RoPE table, rope_kv (bf16 / fp16 / table-less / split), both im2cols, mask_dot, dense_pe, the row
kernels, the norms at the limits of norm.hip, argmax with its position bump and the accept step of a verify pass.

Inputs are asymmetric (no square grids) and seeded.  Where a kernel writes into a larger buffer that buffer is pre-filled with a
sentinel (NaN for fp32, the bit pattern 0x7fff for 16-bit types) and everything outside the specified region must come back bit for
bit.  One case per grid-stride kernel is large enough (more than 8192 blocks of 256 threads) to enter the second iteration of the
loop.  The tolerances are derived from fp32 arithmetic on the reference's values and the rounding of the output type, not from what
the kernels return; the one exception, dense_pe, says so in its docstring."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _glue_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F16, F32, I16, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int16, torch.int32
_id = lambda v: str(v).replace("torch.", "").replace(" ", "")


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _sentinel(shape, dtype, device="cpu"):
    """NaN for fp32, the 16-bit pattern 0x7fff (a NaN in both bf16 and fp16) otherwise"""
    if dtype == F32:
        return torch.full(shape, float("nan"), dtype=F32, device=device)
    return torch.full(shape, 0x7FFF, dtype=I16, device=device).view(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(I32 if t.dtype == F32 else I16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _is_sentinel(t):
    return bool((_bits(t) == _bits(_sentinel((1,), t.dtype))).all())


# ---- RoPE table -------------------------------------------------------------------------------------------------------------
_TABLE_C = {1e4: 8.0, 1e6: 24.0}  # units of 2^-24 * max(ang, 1): ~4x what HF's fp32 table needs (test_glue_ref_cpu: 2.5 and 7)


@pytest.mark.parametrize("T,D,theta", [(4096, 128, 1e4), (4096, 64, 1e4), (2048, 80, 1e6), (1, 2, 1e4)])
def test_rope_table_vs_fp64(hip_lib, cuda, T, D, theta):
    """rope_table_kernel against cos / sin of pos * theta^(-2j/D) in fp64: |err| <= C * 2^-24 * max(ang, 1) per element, C = 8 at
    theta 1e4 and 24 at theta 1e6 (about 4x the error of HF's fp32 table on the host, see test_glue_ref_cpu: the device's powf, sinf
    and cosf may each be a few ulp off; a wrong exponent or position base is off by O(1)).  Row 0 is exactly (1, 0).
    Measured on an MI355X: cos 2.50 / sin 2.48 units at (4096, 128, 1e4) and at (4096, 64, 1e4), cos 5.08 / sin 3.87 units at
    (2048, 80, 1e6), 0 at (1, 2, 1e4)."""
    from interactvlm_amd import ops

    cos, sin = ops.rope_table(T, D, theta, cuda)
    assert cos.shape == (T, D // 2) == sin.shape and cos.dtype == F32 == sin.dtype
    cos, sin = cos.cpu().double(), sin.cpu().double()
    ang = R.rope_angles_ref(T, D, theta)
    rc, rs = R.rope_table_ref(T, D, theta)
    unit = 2.0 ** -24 * ang.clamp_min(1.0)
    uc, us = (cos - rc).abs() / unit, (sin - rs).abs() / unit
    print(f"rope_table (T={T}, D={D}, theta={theta:g}): cos {float(uc.max()):.2f} units, sin {float(us.max()):.2f} units")
    assert bool((cos[0] == 1).all()) and bool((sin[0] == 0).all())
    C = _TABLE_C[theta]
    assert float(uc.max()) <= C and float(us.max()) <= C
    pos = torch.arange(T, dtype=torch.float64)  # column 0: the angle is the position itself
    assert bool(((cos[:, 0] - pos.cos()).abs() <= C * unit[:, 0]).all()) and bool(((sin[:, 0] - pos.sin()).abs() <= C * unit[:, 0]).all())


# ---- rope_kv ----------------------------------------------------------------------------------------------------------------
# (T, H, D, pos0, columns past 3HD, Tmax, theta); the last has 1100 * 30 * 64 = 2,112,000 pairs > 8192 * 256
ROPE_CASES = [(5, 2, 8, 0, 0, 8, 1e4), (37, 4, 128, 11, 16, 64, 1e4), (9, 3, 80, 3, 0, 16, 1e6), (1100, 30, 128, 0, 0, 1100, 1e4)]


def _pair_sum(x):
    """|x_j| + |x_{j + D/2}| at both places of the pair: x [..., D]"""
    half = x.shape[-1] // 2
    s = x[..., :half].abs() + x[..., half:].abs()
    return torch.cat([s, s], -1)


def _rope_inputs(case, dtype):
    T, H, D, pos0, extra, Tmax, theta = case
    g = _gen(T, H, D, pos0)
    x = torch.randn(T, 3, H, D, generator=g).to(dtype)
    buf = _sentinel((T, 3 * H * D + extra), dtype)
    buf[:, : 3 * H * D] = x.view(T, -1)
    return x, buf


def _check_rope_qkv(case, dtype, x, got, table64, extra_units=0.0):
    """got [T, ld] after the call against fp64 on the same table values and the same 16-bit inputs:
    |err| <= u |ref| + 2^-22 (|x_j| + |x_{j+D/2}|) (+ 2^-25 for fp16): one rounding of the output type plus the fp32 rounding of the two
    products and their sum; extra_units: what a table computed on the device may add, in units of 2^-24 max(ang, 1) per |x| of the pair.
    v and the columns past 3HD are bit-unchanged.  -> the worst err / bound"""
    T, H, D, pos0, extra, Tmax, theta = case
    W = 3 * H * D
    pos = torch.arange(pos0, pos0 + T)
    g3 = got[:, :W].view(T, 3, H, D)
    u = 2.0 ** -8 if dtype == BF16 else 2.0 ** -11
    worst = 0.0
    for part in (0, 1):
        ref = R.rope_apply_ref(x[:, part], table64[0], table64[1], pos)
        ps = _pair_sum(x[:, part].double())
        bound = u * ref.abs() + 2.0 ** -22 * ps + (2.0 ** -25 if dtype == F16 else 0.0)
        if extra_units:
            ang = R.rope_angles_ref(pos0 + T, D, theta)[pos].clamp_min(1.0)[:, None, :]
            bound = bound + ps * extra_units * 2.0 ** -24 * torch.cat([ang, ang], -1)
        err = (g3[:, part].double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), f"{'qk'[part]}: worst err / bound {worst:.3f}"
    assert _same_bits(g3[:, 2], x[:, 2]), "v columns changed"
    assert _is_sentinel(got[:, W:]), "columns past 3HD changed"
    return worst


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
@pytest.mark.parametrize("case", ROPE_CASES, ids=_id)
def test_rope_kv_table_vs_fp64(hip_lib, cuda, case, dtype):
    """ops.rope_kv with a table built by the test (fp64 cos / sin rounded to fp32), with and without the cache append: the rotation
    against fp64 (bound in _check_rope_qkv), v / the extra columns / the cache rows outside [pos0, pos0 + T) untouched, the appended
    rows bit-equal to what now stands in qkv."""
    from interactvlm_amd import ops

    T, H, D, pos0, extra, Tmax, theta = case
    W = 3 * H * D
    x, buf = _rope_inputs(case, dtype)
    tab64 = tuple(t.float() for t in R.rope_table_ref(Tmax, D, theta))
    tab = tuple(t.to(cuda) for t in tab64)
    kc, vc = _sentinel((Tmax, H, D), dtype, cuda), _sentinel((Tmax, H, D), dtype, cuda)
    q1 = buf.to(cuda)
    ops.rope_kv(q1[:, :W] if extra else q1, H, D, pos0, theta, kc, vc, table=tab)
    q2 = buf.to(cuda)
    ops.rope_kv(q2[:, :W] if extra else q2, H, D, pos0, theta, table=tab)
    q1, q2, kc, vc = q1.cpu(), q2.cpu(), kc.cpu(), vc.cpu()
    worst = max(_check_rope_qkv(case, dtype, x, q1, tab64), _check_rope_qkv(case, dtype, x, q2, tab64))
    print(f"rope_kv {_id(dtype)} {case}: worst err / bound {worst:.3f}")
    assert _same_bits(q1, q2)
    g3 = q1[:, :W].view(T, 3, H, D)
    assert _is_sentinel(kc[:pos0]) and _is_sentinel(kc[pos0 + T:]) and _is_sentinel(vc[:pos0]) and _is_sentinel(vc[pos0 + T:])
    assert _same_bits(kc[pos0: pos0 + T], g3[:, 1]) and _same_bits(vc[pos0: pos0 + T], x[:, 2])


@pytest.mark.parametrize("case", ROPE_CASES[1:3], ids=_id)
def test_rope_kv_tableless_vs_fp64(hip_lib, cuda, case):
    """table=None: the kernel computes powf / cosf / sinf itself.  Against fp64 with the fp64 table; the bound of the table form plus
    (|x_j| + |x_{j+D/2}|) * C * 2^-24 * max(ang, 1), C as for rope_table (8 at theta 1e4, 24 at 1e6).
    Measured on an MI355X: the worst element uses 0.994 of that bound at (37, 4, 128, pos0 11) and 0.986 at (9, 3, 80, pos0 3)
    (the rounding of the bf16 result dominates); beyond the table form's own bound the device's table costs 0.38 units of
    2^-24 max(ang, 1) in the first case and nothing in the second."""
    from interactvlm_amd import ops

    T, H, D, pos0, extra, Tmax, theta = case
    W = 3 * H * D
    x, buf = _rope_inputs(case, BF16)
    kc, vc = _sentinel((Tmax, H, D), BF16, cuda), _sentinel((Tmax, H, D), BF16, cuda)
    q = buf.to(cuda)
    ops.rope_kv(q[:, :W] if extra else q, H, D, pos0, theta, kc, vc)
    q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()
    tab64 = R.rope_table_ref(Tmax, D, theta)
    loose = _check_rope_qkv(case, BF16, x, q, tab64, extra_units=_TABLE_C[theta])
    # what the device's table costs: the units needed on top of the table form's own bound
    need = 0.0
    pos = torch.arange(pos0, pos0 + T)
    ang = R.rope_angles_ref(Tmax, D, theta)[pos].clamp_min(1.0)[:, None, :]
    for part in (0, 1):
        ref = R.rope_apply_ref(x[:, part], tab64[0], tab64[1], pos)
        ps = _pair_sum(x[:, part].double())
        over = ((q[:, :W].view(T, 3, H, D)[:, part].double() - ref).abs() - 2.0 ** -8 * ref.abs() - 2.0 ** -22 * ps).clamp_min(0)
        need = max(need, float((over / (ps * 2.0 ** -24 * torch.cat([ang, ang], -1)).clamp_min(1e-300)).max()))
    print(f"rope_kv table-less {case}: worst err / bound {loose:.3f}; {need:.2f} units beyond the table form's bound")
    g3 = q[:, :W].view(T, 3, H, D)
    assert _is_sentinel(kc[:pos0]) and _is_sentinel(kc[pos0 + T:]) and _is_sentinel(vc[:pos0]) and _is_sentinel(vc[pos0 + T:])
    assert _same_bits(kc[pos0: pos0 + T], g3[:, 1]) and _same_bits(vc[pos0: pos0 + T], x[:, 2])


@pytest.mark.parametrize("case", ROPE_CASES[:3], ids=_id)
def test_rope_kv_split_vs_fp64(hip_lib, cuda, case):
    """ops.rope_kv_split on [hi | lo] rows: the reference rotates the hi + lo values actually fed (read back before the call);
    |err| <= 2^-16 |ref| + 2^-22 (|x_j| + |x_{j+D/2}|) on hi + lo of the result.  The four cache planes: sentinel outside
    [pos0, pos0 + T), bit-equal to the planes of qkv inside; v hi and lo copied bit for bit."""
    from interactvlm_amd import ops

    T, H, D, pos0, extra, Tmax, theta = case
    W = 3 * H * D
    g = _gen(T, H, D, pos0, 1)
    x32 = torch.randn(T, W, generator=g)
    hi = x32.to(BF16)
    lo = (x32 - hi.float()).to(BF16)
    buf = _sentinel((T, 2 * W + extra), BF16)
    buf[:, :W], buf[:, W: 2 * W] = hi, lo
    q = buf.to(cuda)
    fed = q.cpu()
    xin = (fed[:, :W].double() + fed[:, W: 2 * W].double()).view(T, 3, H, D)
    tab64 = tuple(t.float() for t in R.rope_table_ref(Tmax, D, theta))
    caches = tuple(_sentinel((Tmax, H, D), BF16, cuda) for _ in range(4))  # k, k_lo, v, v_lo
    ops.rope_kv_split(q[:, : 2 * W] if extra else q, H, D, pos0, caches, tuple(t.to(cuda) for t in tab64))
    q = q.cpu()
    kc, kcl, vc, vcl = (c.cpu() for c in caches)
    ghi, glo = q[:, :W].view(T, 3, H, D), q[:, W: 2 * W].view(T, 3, H, D)
    pos = torch.arange(pos0, pos0 + T)
    worst = 0.0
    for part in (0, 1):
        ref = R.rope_apply_ref(xin[:, part], tab64[0], tab64[1], pos)
        bound = 2.0 ** -16 * ref.abs() + 2.0 ** -22 * _pair_sum(xin[:, part])
        err = (ghi[:, part].double() + glo[:, part].double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), worst
    print(f"rope_kv_split {case}: worst err / bound {worst:.3f}")
    fhi, flo = fed[:, :W].view(T, 3, H, D), fed[:, W: 2 * W].view(T, 3, H, D)
    assert _same_bits(ghi[:, 2], fhi[:, 2]) and _same_bits(glo[:, 2], flo[:, 2]) and _is_sentinel(q[:, 2 * W:])
    for c in (kc, kcl, vc, vcl):
        assert _is_sentinel(c[:pos0]) and _is_sentinel(c[pos0 + T:])
    assert _same_bits(kc[pos0: pos0 + T], ghi[:, 1]) and _same_bits(kcl[pos0: pos0 + T], glo[:, 1])
    assert _same_bits(vc[pos0: pos0 + T], fhi[:, 2]) and _same_bits(vcl[pos0: pos0 + T], flo[:, 2])


def test_rope_host_guards(hip_lib, cuda):
    """What the kernels cannot see is rejected before any launch: a table or a cache shorter than pos0 + T rows, a table of the wrong
    width / dtype / layout, a qkv row narrower than 3HD (6HD).  (Only the rejection is tested: the out-of-range access is never run.)"""
    from interactvlm_amd import ops

    T, H, D, Tmax = 4, 2, 8, 8
    W = 3 * H * D
    tab = tuple(t.float().to(cuda) for t in R.rope_table_ref(Tmax, D, 1e4))
    mk = lambda rows=Tmax: torch.zeros(rows, H, D, dtype=BF16, device=cuda)
    qkv = torch.zeros(T, W, dtype=BF16, device=cuda)
    qs = torch.zeros(T, 2 * W, dtype=BF16, device=cuda)
    ops.rope_kv(qkv, H, D, 4, 1e4, mk(), mk(), table=tab)  # pos0 + T == Tmax: the last legal position
    ops.rope_kv_split(qs, H, D, 4, (mk(), mk(), mk(), mk()), tab)
    bad_tables = [tuple(t[:7] for t in tab),                                     # too short for pos0 = 4
                  tuple(t.double() for t in tab),                                # not fp32
                  tuple(torch.zeros(Tmax, D, device=cuda)[:, : D // 2] for _ in tab),  # not contiguous
                  tuple(torch.zeros(Tmax, D, device=cuda) for _ in tab)]         # D columns, not D/2
    for bad in bad_tables:
        with pytest.raises(AssertionError):
            ops.rope_kv(qkv, H, D, 4, 1e4, mk(), mk(), table=bad)
        with pytest.raises(AssertionError):
            ops.rope_kv_split(qs, H, D, 4, (mk(), mk(), mk(), mk()), bad)
    with pytest.raises(AssertionError):
        ops.rope_kv(qkv, H, D, 5, 1e4, table=tab)  # position 8 of an 8-row table
    with pytest.raises(AssertionError):
        ops.rope_kv(qkv[:, : W - 8], H, D, 0, 1e4, table=tab)
    with pytest.raises(AssertionError):
        ops.rope_kv(qkv, H, D, 4, 1e4, mk(), mk(7), table=tab)
    with pytest.raises(AssertionError):
        ops.rope_kv(qkv, H, D, 4, 1e4, mk(7), mk())  # the table-less form checks its caches too
    with pytest.raises(AssertionError):
        ops.rope_kv_split(qs[:, : 2 * W - 8], H, D, 0, None, tab)
    with pytest.raises(AssertionError):
        ops.rope_kv_split(qs, H, D, 4, (mk(), mk(7), mk(), mk()), tab)
    torch.cuda.synchronize()


# ---- im2col -----------------------------------------------------------------------------------------------------------------
# K = 588 pads to 640 and 588 % 8 == 4 (one 8-group straddles K), trailing pixels that fill no patch; K = 768 unpadded; explicit
# kpad; stride != ks; 265,225 rows x 8 groups > 8192 * 256
IM2COL_CASES = [(2, 3, 31, 45, 14, 14, None), (1, 3, 32, 48, 16, 16, None), (2, 3, 28, 42, 14, 14, 704), (1, 5, 9, 11, 3, 2, None),
                (1, 8, 1030, 1030, 2, 2, None)]


@pytest.mark.parametrize("case", IM2COL_CASES, ids=_id)
def test_im2col_nchw_bit_equal(hip_lib, cuda, case):
    from interactvlm_amd import ops

    B, C, H, W, ks, stride, kpad = case
    x = torch.randn(B, C, H, W, generator=_gen(*case[:6])).to(BF16)
    ref = R.im2col_nchw_ref(x, ks, stride, kpad)
    got = ops.im2col_nchw(x.to(cuda), ks, stride, kpad)
    assert _same_bits(got, ref)


def test_im2col_nchw_writes_its_pad_columns_and_rejects_bad_kpad(hip_lib, cuda):
    """The pad columns 588 .. 639 are written as zeros (not left to the allocator); kpad not a multiple of 8 or below K is refused."""
    from interactvlm_amd import ops

    B, C, H, W, ks, stride, _ = IM2COL_CASES[0]
    x = torch.randn(B, C, H, W, generator=_gen(*IM2COL_CASES[0][:6])).to(BF16)
    ref = R.im2col_nchw_ref(x, ks, stride, 640)
    out = _sentinel(ref.shape, BF16, cuda)
    xd = x.to(cuda)
    rc = hip_lib.ivlm_im2col_nchw(xd.data_ptr(), out.data_ptr(), B, C, H, W, ks, stride, 640, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert _same_bits(out, ref) and bool((out[:, 588:].cpu().float() == 0).all())
    for kpad in (590, 584):
        with pytest.raises(ops.IvlmError):
            ops.im2col_nchw(xd, ks, stride, kpad)
    torch.cuda.synchronize()


# the last: 93,000 rows x 9 taps x 3 groups = 2,511,000 > 8192 * 256
IM2COL3_CASES = [(2, 5, 7, 8), (1, 1, 1, 24), (1, 1, 6, 16), (3, 4, 3, 256), (1, 300, 310, 24)]


@pytest.mark.parametrize("case", IM2COL3_CASES, ids=_id)
def test_im2col3x3_nhwc_bit_equal(hip_lib, cuda, case):
    from interactvlm_amd import ops

    x = torch.randn(*case, generator=_gen(*case)).to(BF16)
    ref = R.im2col3x3_ref(x)
    got = ops.im2col3x3_nhwc(x.to(cuda))
    assert _same_bits(got, ref)
    if case[1:3] == (1, 1):  # a single pixel: only the centre tap is not padding
        C = case[3]
        assert bool((got.cpu().float()[:, : 4 * C] == 0).all()) and bool((got.cpu().float()[:, 5 * C:] == 0).all())


@pytest.mark.parametrize("case", [IM2COL3_CASES[0], IM2COL3_CASES[3]], ids=_id)
def test_im2col3x3_nhwc_split_bit_equal(hip_lib, cuda, case):
    """[hi | lo] rows from ops.split_rows: columns [:9C] are the unfold of the hi plane, [9C:] that of the lo plane."""
    from interactvlm_amd import ops

    B, H, W, C = case
    x = torch.randn(B * H * W, C, generator=_gen(*case, 2))
    xs = ops.split_rows(x.to(cuda))
    planes = xs.cpu()
    got = ops.im2col3x3_nhwc_split(xs, B, H, W, C)
    assert got.shape == (B * H * W, 18 * C)
    assert _same_bits(got[:, : 9 * C], R.im2col3x3_ref(planes[:, :C].reshape(B, H, W, C)))
    assert _same_bits(got[:, 9 * C:], R.im2col3x3_ref(planes[:, C:].reshape(B, H, W, C)))
    assert bool((planes[:, C:].float() != 0).any())


def test_im2col3x3_rejects_channels_not_multiple_of_8(hip_lib, cuda):
    from interactvlm_amd import ops

    with pytest.raises(ops.IvlmError):
        ops.im2col3x3_nhwc(torch.zeros(1, 2, 3, 12, dtype=BF16, device=cuda))
    torch.cuda.synchronize()


# ---- mask_dot ---------------------------------------------------------------------------------------------------------------
# the last: 370 * 360 * 16 = 2,131,200 outputs > 8192 * 256 (up: 68 MB of fp32)
@pytest.mark.parametrize("B,gh,gw,C,dtype", [(2, 3, 5, 32, F32), (2, 3, 5, 32, BF16), (1, 1, 1, 8, F32), (1, 370, 360, 8, F32)], ids=_id)
def test_mask_dot_vs_fp64(hip_lib, cuda, B, gh, gw, C, dtype):
    """|err| <= 2^-21 * sum_c |up_c * hyper_c|: fp32 accumulation over C <= 32 terms.  bf16 operands: the reference uses the
    bf16-rounded values (their products are exact in fp32), same bound."""
    from interactvlm_amd import ops

    g = _gen(B, gh, gw, C)
    up = torch.randn(B * gh * gw * 16, C, generator=g).to(dtype)
    hyper = torch.randn(B, C, generator=g).to(dtype)
    got = ops.mask_dot(up.to(cuda), hyper.to(cuda), B, gh, gw).cpu()
    assert got.shape == (B, 4 * gh, 4 * gw) and got.dtype == F32
    ref = R.mask_dot_ref(up, hyper, B, gh, gw)
    bound = 2.0 ** -21 * R.mask_dot_ref(up.abs(), hyper.abs(), B, gh, gw)
    err = (got.double() - ref).abs()
    print(f"mask_dot {(B, gh, gw, C)} {_id(dtype)}: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---- dense_pe ---------------------------------------------------------------------------------------------------------------
DENSE_PE_C = 2.484  # see test_dense_pe_vs_fp64


@pytest.mark.parametrize("h,w,F_", [(5, 7, 16), (1, 3, 4), (64, 64, 128)])
def test_dense_pe_vs_fp64(hip_lib, cuda, h, w, F_):
    """fp32 output: |err| <= DENSE_PE_C * 2^-21 (1 + |t|), t the fp64 phase (the kernel forms it in about five fp32 operations);
    bf16 output: that plus 2^-8.  x pairs with gauss[0] and w, y with gauss[1] and h.
    DENSE_PE_C = 2.484 is twice the worst case measured on an MI355X at (64, 64, 128), in units of 2^-21 (1 + |t|): 1.242
    (|err| 2.53e-6 at t = 0.047; (5, 7, 16): 0.797, (1, 3, 4): 0.042).  The plain 2^-21 (1 + |t|) is tighter than fp32 allows, and
    not because of the device's sinf / cosf: the same five fp32 operations on the host, followed by an fp64 sine, are 1.239 units
    off at that very element.  Its two products, 2 pi cx g[0] and 2 pi cy g[1], are each of size 2 pi |g| (|g[0]| + |g[1]| = 3.1
    there) and cancel to 0.047, so their roundings, which scale with |g|, are not covered by a bound that scales with |t|."""
    from interactvlm_amd import ops

    gauss = torch.randn(2, F_, generator=_gen(h, w, F_))
    ref = R.dense_pe_ref(gauss, h, w)
    t = R.dense_pe_phase_ref(gauss, h, w).abs()
    bound = DENSE_PE_C * 2.0 ** -21 * (1.0 + torch.cat([t, t], -1))
    got = ops.dense_pe(gauss.to(cuda), h, w).cpu()
    assert got.shape == (h * w, 2 * F_) and got.dtype == F32
    err = (got.double() - ref).abs()
    print(f"dense_pe ({h}, {w}, {F_}) fp32: worst |err| {float(err.max()):.3e}, {float((err / bound).max() * DENSE_PE_C):.3f} units of 2^-21 (1 + |t|)")
    assert bool((err <= bound).all())
    got_b = ops.dense_pe(gauss.to(cuda), h, w, dtype=BF16).cpu()
    assert got_b.dtype == BF16 and bool(((got_b.double() - ref).abs() <= bound + 2.0 ** -8).all())


# ---- gather_rows / add_rows / fill_rows -------------------------------------------------------------------------------------
def _gather_ref(src, idx, add=None):
    out = torch.where(idx[:, None] >= 0, src.float()[idx.clamp(min=0).long()], torch.zeros(1))
    return out if add is None else out + add.float()


def test_gather_rows_strided_repeated_and_split(hip_lib, cuda):
    """Copies and single fp32 additions: exact.  src, add and out are column windows of wider buffers (row stride 96 for 64 columns);
    the out buffer is NaN outside the window before and after."""
    from interactvlm_amd import ops

    g = _gen(31)
    src_buf, add_buf = torch.randn(20, 96, generator=g), torch.randn(9, 96, generator=g)
    idx = torch.tensor([3, 3, -1, 19, 0, 3, -1, 7, 19], dtype=I32)  # repeated and dropped rows
    out_buf = _sentinel((9, 96), F32, cuda)
    sd, ad = src_buf.to(cuda), add_buf.to(cuda)
    ret = ops.gather_rows(sd[:, 8:72], idx.to(cuda), add=ad[:, 8:72], out=out_buf[:, 8:72])
    assert ret.data_ptr() == out_buf[:, 8:72].data_ptr()
    got = out_buf.cpu()
    assert torch.equal(got[:, 8:72], _gather_ref(src_buf[:, 8:72], idx, add_buf[:, 8:72]))
    assert _is_sentinel(got[:, :8]) and _is_sentinel(got[:, 72:])
    # the same windows in bf16, into a bf16 window
    sb, ab = src_buf.to(BF16), add_buf.to(BF16)
    out_b = _sentinel((9, 96), BF16, cuda)
    ops.gather_rows(sb.to(cuda)[:, 8:72], idx.to(cuda), add=ab.to(cuda)[:, 8:72], out=out_b[:, 8:72])
    got = out_b.cpu()
    assert _same_bits(got[:, 8:72], _gather_ref(sb[:, 8:72], idx, ab[:, 8:72]).to(BF16))
    assert _is_sentinel(got[:, :8]) and _is_sentinel(got[:, 72:])
    # bf16 src + bf16 add -> split: hi = bf16(sum), lo = bf16(sum - hi)
    s = _gather_ref(sb[:, 8:72], idx, ab[:, 8:72])
    sp = ops.gather_rows(sb.to(cuda)[:, 8:72], idx.to(cuda), add=ab.to(cuda)[:, 8:72], out_kind="split").cpu()
    assert sp.shape == (9, 128) and _same_bits(sp[:, :64], s.to(BF16)) and _same_bits(sp[:, 64:], (s - s.to(BF16).float()).to(BF16))


def test_gather_rows_second_grid_stride_iteration(hip_lib, cuda):
    """2100 rows x 1000 groups = 2,100,000 > 8192 * 256: fp32 -> bf16 through a random index with dropped rows"""
    from interactvlm_amd import ops

    g = _gen(2100, 8000)
    src = torch.randn(300, 8000, generator=g)
    idx = torch.randint(-1, 300, (2100,), generator=g, dtype=I32)
    assert bool((idx == -1).any())
    got = ops.gather_rows(src.to(cuda), idx.to(cuda), out_kind="bf16").cpu()
    assert _same_bits(got, _gather_ref(src, idx).to(BF16))


def test_add_rows_mixed_dtypes_and_row_modulo(hip_lib, cuda):
    from interactvlm_amd import ops

    g = _gen(41)
    a, b = torch.randn(12, 72, generator=g), torch.randn(5, 72, generator=g)
    ab, bb = a.to(BF16), b.to(BF16)
    rows = torch.arange(12) % 5
    got = ops.add_rows(ab.to(cuda), b.to(cuda)).cpu()  # bf16 a + fp32 b -> bf16 (a's dtype)
    assert _same_bits(got, (ab.float() + b[rows]).to(BF16))
    got = ops.add_rows(a.to(cuda), bb.to(cuda)).cpu()  # fp32 a + bf16 b -> fp32
    assert got.dtype == F32 and torch.equal(got, a + bb.float()[rows])
    got = ops.add_rows(a.to(cuda), bb.to(cuda), op="mul", out_kind="bf16").cpu()
    assert _same_bits(got, (a * bb.float()[rows]).to(BF16))
    assert torch.equal(ops.add_rows(a.to(cuda), b[:1].contiguous().to(cuda)).cpu(), a + b[:1])  # b_rows = 1
    assert torch.equal(ops.add_rows(a[:4].contiguous().to(cuda), b.to(cuda)).cpu(), a[:4] + b[:4])  # b_rows > rows


@pytest.mark.parametrize("cols", [8, 1280])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
def test_fill_rows_strided_duplicates_and_empty(hip_lib, cuda, dtype, cols):
    """A 16-bit copy into the listed rows of a column window: every other row and every column past ``cols`` stays bit for bit."""
    from interactvlm_amd import ops

    g = _gen(cols, 3)
    before = torch.randn(10, cols + 16, generator=g).to(dtype)
    row = torch.randn(cols, generator=g).to(dtype)
    idx = torch.tensor([3, 7, 3, 0], dtype=I32)  # one duplicate
    buf = before.to(cuda)
    ops.fill_rows(buf[:, :cols], idx.to(cuda), row.to(cuda))
    exp = before.clone()
    exp[idx.long(), :cols] = row
    assert _same_bits(buf, exp)
    ops.fill_rows(buf[:, :cols], torch.empty(0, dtype=I32, device=cuda), row.to(cuda))  # nothing listed: nothing changes
    assert _same_bits(buf, exp)


# ---- norms at the limits of norm.hip ----------------------------------------------------------------------------------------
def _norm_params(cols, g):
    return (1 + 0.1 * torch.randn(cols, generator=g)).to(BF16), (0.1 * torch.randn(cols, generator=g)).to(BF16)


def _ln64(x, w, b, eps):
    import torch.nn.functional as F

    return F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps)


# 8: one chunk, 63 idle lanes; 64: the mask decoder's up_ln; 2048 / 2056: the last width of the 4-chunk kernel and the first of the
# 16-chunk kernel; 8192: the widest row
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [8, 64, 2048, 2056, 8192])
def test_norms_at_the_width_limits(hip_lib, cuda, cols, rows):
    from interactvlm_amd import ops

    g = _gen(cols, rows)
    x = torch.randn(rows, cols, generator=g) * 3 + 0.5
    w, b = _norm_params(cols, g)
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    ref = _ln64(x, w, b, 1e-6)
    got = ops.layernorm(xd, wd, bd, 1e-6, out_f32=True).cpu()
    assert got.dtype == F32 and bool(((got.double() - ref).abs() <= 2e-5 + 1e-5 * ref.abs()).all())
    got_b = ops.layernorm(xd, wd, bd, 1e-6).cpu()
    assert got_b.dtype == BF16 and float((got_b.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())
    x64 = x.double()
    ref_r = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + 1e-5) * w.double()
    got_r = ops.rmsnorm(xd, wd, 1e-5, out_f32=True).cpu()
    assert got_r.dtype == F32 and bool(((got_r.double() - ref_r).abs() <= 2e-5 + 1e-5 * ref_r.abs()).all())
    got_rb = ops.rmsnorm(xd, wd, 1e-5).cpu()
    assert got_rb.dtype == BF16 and float((got_rb.double() - ref_r).abs().max()) <= 2.0 ** -8 * float(ref_r.abs().max())
    # a constant row has no spread: every output is the bias itself, exactly
    const = torch.full((rows, cols), 3.25, device=cuda)
    assert _same_bits(ops.layernorm(const, wd, bd, 1e-6), b.expand(rows, cols))


@pytest.mark.parametrize("cols", [64, 2048])
def test_layernorm_gelu_vs_fp64(hip_lib, cuda, cols):
    import torch.nn.functional as F

    from interactvlm_amd import ops

    g = _gen(cols, 9)
    x = torch.randn(5, cols, generator=g) * 3 + 0.5
    w, b = _norm_params(cols, g)
    ref = F.gelu(_ln64(x, w, b, 1e-6))
    got = ops.layernorm(x.to(cuda), w.to(cuda), b.to(cuda), 1e-6, gelu=True, out_f32=True).cpu()
    err = float((got.double() - ref).abs().max())
    print(f"layernorm + gelu, {cols} columns: worst |err| {err:.3e}")
    assert got.dtype == F32 and err <= 3e-5


def test_layernorm_row_with_a_large_mean(hip_lib, cuda):
    """x = 100 + randn over 1280 columns, fp32 in and out: |err| <= 16 * 2^-24 * 100 * rstd * |w| + 2e-5.  The first term is what the
    fp32 rounding of the mean (a sum of values near 100) may shift every output by when the variance is taken around that mean in a
    second pass; a one-pass E[x^2] - mean^2 cancels 10^4 against 10^4 and misses the bound by orders of magnitude."""
    from interactvlm_amd import ops

    cols = 1280
    g = _gen(cols, 100)
    x = 100 + torch.randn(5, cols, generator=g)
    w, b = _norm_params(cols, g)
    ref = _ln64(x, w, b, 1e-6)
    rstd = torch.rsqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-6)
    bound = 16 * 2.0 ** -24 * 100 * rstd * w.double().abs() + 2e-5
    got = ops.layernorm(x.to(cuda), w.to(cuda), b.to(cuda), 1e-6, out_f32=True).cpu()
    err = (got.double() - ref).abs()
    print(f"layernorm, mean 100: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_norm_host_rejections(hip_lib, cuda):
    from interactvlm_amd import ops

    def call(cols, **kw):
        g = _gen(cols)
        w, b = _norm_params(cols, g)
        return ops.layernorm(torch.randn(2, cols, generator=g).to(cuda), w.to(cuda), b.to(cuda), 1e-6, **kw)

    one = torch.ones(1, device=cuda)
    for cols, kw in ((8200, {}), (12, {}), (2056, dict(gelu=True)), (64, dict(gelu=True, fp8_scale=one))):
        with pytest.raises(ops.IvlmError):
            call(cols, **kw)
    for cols in (8200, 12):
        with pytest.raises(ops.IvlmError):
            ops.rmsnorm(torch.zeros(2, cols, device=cuda), torch.ones(cols, dtype=BF16, device=cuda))
    torch.cuda.synchronize()


# ---- argmax with the position bump, spec_accept -----------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [7, 32003])
def test_argmax_bump(hip_lib, cuda, cols):
    from interactvlm_amd import ops

    x = torch.randn(3, cols, generator=_gen(cols, 5))
    xd = x.to(cuda)
    bump = torch.tensor([5, 0, -1], dtype=I32, device=cuda)
    exp = torch.argmax(x, -1).to(I32)
    assert torch.equal(ops.argmax(xd).cpu(), exp)
    assert torch.equal(ops.argmax(xd, bump=bump).cpu(), exp) and bump.cpu().tolist() == [6, 1, 0]
    assert torch.equal(ops.argmax(xd, bump=bump).cpu(), exp) and bump.cpu().tolist() == [7, 2, 1]


_FULL = list(range(100, 116))
SPEC_CASES = {
    "k1": ([7], [3], 0),
    "k16_all_accepted": (_FULL, [1] + _FULL[:15], 15),
    "mismatch_at_0": ([4, 5, 6, 9], [1, 8, 5, 6], 3),
    "mismatch_in_the_middle": ([4, 5, 6, 9, 2, 3], [1, 4, 5, 8, 9, 2], 5),
    "mismatch_at_the_last_draft": ([4, 5, 6, 9], [1, 4, 5, 8], 3),
    "n_draft_clamped": ([4, 5, 6, 9], [1, 4, 5, 6], 9),
    "n_draft_0_ignores_a_matching_draft": ([4, 5, 6, 9], [1, 4, 5, 6], 0),
}


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_spec_accept_vs_ref(hip_lib, cuda, name):
    from interactvlm_amd import ops

    amax, fed, nd = SPEC_CASES[name]
    dev = lambda v: torch.tensor(v, dtype=I32, device=cuda)
    n_acc, tok, pos = dev([-7]), dev([-7]), dev([41])
    ops.spec_accept(dev(amax), dev(fed), dev([nd]), n_acc, tok, pos)
    n, t, adv = R.spec_accept_ref(amax, fed, nd)
    assert (int(n_acc), int(tok), int(pos)) == (n, t, 41 + adv)
