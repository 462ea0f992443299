"""Pins the CPU references of tests/_glue_ref.py against independent formulations of the same operations, so that a failure of
tests/test_glue_kernels_gpu.py can be blamed on the kernel and not on its yardstick.  No GPU, a few seconds."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _glue_ref as R  # noqa: E402


def _hf_table(T, D, theta):
    """HF LlamaRotaryEmbedding, restated: everything in fp32"""
    inv_freq = 1.0 / (theta ** (torch.arange(0, D, 2).float() / D))
    freqs = torch.outer(torch.arange(T).float(), inv_freq)
    return freqs.cos(), freqs.sin()


@pytest.mark.parametrize("T,D,theta,ceiling", [(4096, 128, 1e4, 2.5), (4096, 64, 1e4, 2.5), (2048, 80, 1e6, 7.0)])
def test_rope_table_ref_vs_hf_fp32(T, D, theta, ceiling):
    """rope_table_ref (fp64) against HF's fp32 table, in units of 2^-24 * max(ang, 1) per element: the rounding of an fp32 angle
    of that size.  Measured: 2.11 units at (4096, 128, 1e4) and (4096, 64, 1e4), where 2j/D is exact in fp32, and 6.2 units at
    (2048, 80, 1e6), where the rounded exponent is multiplied by ln(1e6); the ceilings are those figures rounded up.  The bound
    that tests/test_glue_kernels_gpu.py sets for rope_table_kernel (8 and 24 units) is derived from these ceilings: about 4x,
    because device powf / sinf / cosf may each be a few ulp off where the host's are nearly correctly rounded."""
    ang = R.rope_angles_ref(T, D, theta)
    cos, sin = R.rope_table_ref(T, D, theta)
    assert cos.dtype == torch.float64 and cos.shape == (T, D // 2) == sin.shape
    hc, hs = _hf_table(T, D, theta)
    unit = 2.0 ** -24 * ang.clamp_min(1.0)
    worst = max(float(((hc.double() - cos).abs() / unit).max()), float(((hs.double() - sin).abs() / unit).max()))
    print(f"rope_table_ref vs HF fp32 (T={T}, D={D}, theta={theta:g}): {worst:.2f} units")
    assert worst <= ceiling, worst
    # the formula itself, spelled out for two entries: position 0 and the exponent 2j/D (not j/D)
    assert bool((cos[0] == 1).all()) and bool((sin[0] == 0).all())
    j, pos = D // 2 - 1, T - 1
    assert abs(float(ang[pos, j]) - pos * theta ** (-2.0 * j / D)) <= 1e-12 * pos


def test_rope_apply_ref_vs_hf_rotate_half():
    g = torch.Generator().manual_seed(11)
    T, H, D = 7, 3, 10
    x = torch.randn(T, H, D, generator=g, dtype=torch.float64)
    pos = torch.tensor([4, 0, 9, 9, 1, 12, 3])
    cos, sin = R.rope_table_ref(13, D, 1e4)

    def rotate_half(t):
        return torch.cat([-t[..., D // 2:], t[..., : D // 2]], -1)

    c = torch.cat([cos, cos], -1)[pos][:, None, :]  # HF: emb = cat(freqs, freqs)
    s = torch.cat([sin, sin], -1)[pos][:, None, :]
    exp = x * c + rotate_half(x) * s
    got = R.rope_apply_ref(x, cos, sin, pos)
    assert got.dtype == torch.float64 and float((got - exp).abs().max()) <= 1e-12


@pytest.mark.parametrize("B,C,H,W,ks,stride,kpad", [(2, 3, 31, 45, 14, 14, None), (1, 5, 9, 11, 3, 2, None), (2, 2, 8, 13, 4, 4, 40)])
def test_im2col_nchw_ref_is_conv2d(B, C, H, W, ks, stride, kpad):
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    wt = torch.randn(6, C, ks, ks, generator=g, dtype=torch.float64)
    K = C * ks * ks
    cols = R.im2col_nchw_ref(x, ks, stride, kpad)
    assert cols.dtype == x.dtype and cols.shape[1] == (kpad or (K + 63) // 64 * 64) and bool((cols[:, K:] == 0).all())
    conv = F.conv2d(x, wt, stride=stride)  # [B, N, gh, gw]
    exp = conv.permute(0, 2, 3, 1).reshape(-1, 6)
    assert cols.shape[0] == exp.shape[0]
    assert float((cols[:, :K] @ wt.reshape(6, -1).T - exp).abs().max()) <= 1e-12


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 8), (1, 1, 6, 3), (1, 4, 1, 2)])
def test_im2col3x3_ref_is_conv2d_padding_1(B, H, W, C):
    g = torch.Generator().manual_seed(H + 10 * W)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    wt = torch.randn(5, C, 3, 3, generator=g, dtype=torch.float64)
    cols = R.im2col3x3_ref(x)
    assert cols.shape == (B * H * W, 9 * C)
    exp = F.conv2d(x.permute(0, 3, 1, 2), wt, padding=1).permute(0, 2, 3, 1).reshape(-1, 5)
    assert float((cols @ wt.permute(0, 2, 3, 1).reshape(5, -1).T - exp).abs().max()) <= 1e-12


def test_mask_dot_ref_is_two_pixel_unshuffles():
    """The two kernel-2 stride-2 transposed convolutions each place their 2 x 2 outputs at (2y + dy, 2x + dx): written out with
    loops, one stage after the other, on a 2 x 3 grid."""
    g = torch.Generator().manual_seed(5)
    B, gh, gw, C = 2, 2, 3, 4
    up = torch.randn(B, gh, gw, 2, 2, 2, 2, C, generator=g, dtype=torch.float64)
    hyper = torch.randn(B, C, generator=g, dtype=torch.float64)
    stage1 = torch.zeros(B, 2 * gh, 2 * gw, 2, 2, C, dtype=torch.float64)  # after the first un-shuffle: [b, Y, X, dy2, dx2, c]
    for b in range(B):
        for y in range(gh):
            for x in range(gw):
                for dy in range(2):
                    for dx in range(2):
                        stage1[b, 2 * y + dy, 2 * x + dx] = up[b, y, x, dy, dx]
    stage2 = torch.zeros(B, 4 * gh, 4 * gw, C, dtype=torch.float64)
    for b in range(B):
        for Y in range(2 * gh):
            for X in range(2 * gw):
                for dy2 in range(2):
                    for dx2 in range(2):
                        stage2[b, 2 * Y + dy2, 2 * X + dx2] = stage1[b, Y, X, dy2, dx2]
    exp = torch.zeros(B, 4 * gh, 4 * gw, dtype=torch.float64)
    for b in range(B):
        exp[b] = stage2[b] @ hyper[b]
    got = R.mask_dot_ref(up.reshape(-1, C), hyper, B, gh, gw)
    assert got.shape == exp.shape and float((got - exp).abs().max()) <= 1e-12


def test_dense_pe_ref_entries():
    """Single entries written out by hand: x pairs with gauss[0] and w, y with gauss[1] and h; sin first, then cos."""
    import math

    g = torch.Generator().manual_seed(6)
    h, w, nf = 3, 5, 4
    gauss = torch.randn(2, nf, generator=g)
    pe = R.dense_pe_ref(gauss, h, w)
    assert pe.shape == (h * w, 2 * nf) and pe.dtype == torch.float64
    for y, x, f in ((0, 0, 0), (2, 4, 3), (1, 3, 2), (2, 0, 1)):
        t = 2 * math.pi * ((2 * (x + 0.5) / w - 1) * float(gauss[0, f]) + (2 * (y + 0.5) / h - 1) * float(gauss[1, f]))
        assert abs(float(pe[y * w + x, f]) - math.sin(t)) <= 1e-12 and abs(float(pe[y * w + x, nf + f]) - math.cos(t)) <= 1e-12


@pytest.mark.parametrize("amax,fed,nd,exp", [
    ([7], [3], 0, (0, 7, 1)),                                  # k = 1: nothing to accept
    ([7], [3], 5, (0, 7, 1)),                                  # k = 1, n_draft clamped to 0
    ([4, 5, 6, 9], [1, 4, 5, 6], 3, (3, 9, 4)),                # every draft accepted
    ([4, 5, 6, 9], [1, 8, 5, 6], 3, (0, 4, 1)),                # first mismatch at index 0
    ([4, 5, 6, 9], [1, 4, 8, 6], 3, (1, 5, 2)),                # ... in the middle
    ([4, 5, 6, 9], [1, 4, 5, 8], 3, (2, 6, 3)),                # ... at the last draft
    ([4, 5, 6, 9], [1, 4, 5, 6], 9, (3, 9, 4)),                # n_draft > k - 1: clamped
    ([4, 5, 6, 9], [1, 4, 5, 6], 0, (0, 4, 1)),                # n_draft = 0: a matching draft is ignored
    ([4, 5, 6, 9], [1, 4, 5, 6], 2, (2, 6, 3)),                # only n_draft ids are looked at
    ([4, 4, 4, 4], [4, 4, 4, 4], 3, (3, 4, 4)),                # fed[0] is the last emitted token, never compared
])
def test_spec_accept_ref_table(amax, fed, nd, exp):
    assert R.spec_accept_ref(amax, fed, nd) == exp
    assert R.spec_accept_ref(torch.tensor(amax, dtype=torch.int32), torch.tensor(fed, dtype=torch.int32), nd) == exp
