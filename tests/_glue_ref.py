"""Plain torch restatements, on the CPU, of the kernels that sit between the GEMMs and the attentions: the RoPE table and its
application, both im2cols, mask_dot, dense_pe and the accept step of a verify pass.  fp64 where there is arithmetic, exact copies
where there is none.  Nothing here calls into interactvlm_amd: tests/test_glue_ref_cpu.py pins these functions against independent
formulations (HF's RoPE, F.conv2d, loop-written pixel un-shuffles), tests/test_glue_kernels_gpu.py holds the kernels to them.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def rope_angles_ref(T, D, theta):
    """fp64 [T, D/2]: ang[pos, j] = pos * theta ** (-2j / D)"""
    j = torch.arange(D // 2, dtype=torch.float64)
    inv_freq = torch.tensor(float(theta), dtype=torch.float64) ** (-2.0 * j / D)
    return torch.arange(T, dtype=torch.float64)[:, None] * inv_freq[None, :]


def rope_table_ref(T, D, theta):
    """-> (cos, sin) fp64 [T, D/2] of rope_angles_ref"""
    ang = rope_angles_ref(T, D, theta)
    return torch.cos(ang), torch.sin(ang)


def rope_apply_ref(x, cos, sin, pos):
    """Rotate-half RoPE in fp64: x [T, H, D], cos / sin [rows, D/2], pos [T] (long) the table row of each x row.  Pairs (j, j + D/2):
    out[j] = x[j] * c - x[j + D/2] * s, out[j + D/2] = x[j + D/2] * c + x[j] * s."""
    x = x.detach().cpu().double()
    half = x.shape[-1] // 2
    pos = torch.as_tensor(pos, dtype=torch.long)
    c = cos.detach().cpu().double()[pos][:, None, :]
    s = sin.detach().cpu().double()[pos][:, None, :]
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def _wide(x):
    """16-bit images are unfolded as fp32 (F.unfold has no 16-bit CPU path everywhere); a copy either way: exact"""
    return x if x.dtype in (torch.float32, torch.float64) else x.float()


def im2col_nchw_ref(x, ks, stride, kpad=None):
    """x [B, C, H, W] -> [(b, gy, gx), (c, ky, kx)] in x's dtype, zero columns up to kpad (default: the next multiple of 64).
    Pixels that do not fill a patch are dropped (F.unfold)."""
    x = x.detach().cpu()
    B, C = x.shape[:2]
    K = C * ks * ks
    kpad = kpad or (K + 63) // 64 * 64
    cols = F.unfold(_wide(x), ks, stride=stride)  # [B, (c, ky, kx), (gy, gx)]
    out = torch.zeros(B * cols.shape[-1], kpad, dtype=x.dtype)
    out[:, :K] = cols.transpose(1, 2).reshape(-1, K).to(x.dtype)
    return out


def im2col3x3_ref(x_nhwc):
    """x [B, H, W, C] -> [(b, y, x), (ky, kx, c)] in x's dtype: the 3 x 3 neighbourhood with zero padding 1"""
    x = x_nhwc.detach().cpu()
    B, H, W, C = x.shape
    cols = F.unfold(_wide(x).permute(0, 3, 1, 2), 3, padding=1)  # [B, (c, ky, kx), (y, x)]
    cols = cols.view(B, C, 9, H * W).permute(0, 3, 2, 1)  # [B, (y, x), (ky, kx), c]
    return cols.reshape(B * H * W, 9 * C).to(x.dtype)


def mask_dot_ref(up, hyper, B, gh, gw):
    """up [B, gh, gw, dy, dx, dy2, dx2, C] (any shape with that order) . hyper [B, C] in fp64 -> low fp64 [B, 4gh, 4gw] at
    (4y + 2dy + dy2, 4x + 2dx + dx2)"""
    hyper = hyper.detach().cpu().double().view(B, -1)
    u = up.detach().cpu().double().view(B, gh, gw, 2, 2, 2, 2, hyper.shape[-1])
    d = torch.einsum("byxpqrsc,bc->byxpqrs", u, hyper)  # p = dy, q = dx, r = dy2, s = dx2
    return d.permute(0, 1, 3, 5, 2, 4, 6).reshape(B, 4 * gh, 4 * gw)  # [b, (y, dy, dy2), (x, dx, dx2)]


def dense_pe_phase_ref(gauss, h, w):
    """fp64 [h * w, F]: t[(y, x), f] = 2 pi ((2 (x + .5) / w - 1) gauss[0, f] + (2 (y + .5) / h - 1) gauss[1, f])"""
    g = gauss.detach().cpu().double()
    cx = 2.0 * (torch.arange(w, dtype=torch.float64) + 0.5) / w - 1.0
    cy = 2.0 * (torch.arange(h, dtype=torch.float64) + 0.5) / h - 1.0
    t = cx[None, :, None] * g[0][None, None, :] + cy[:, None, None] * g[1][None, None, :]
    return (2.0 * math.pi * t).reshape(h * w, -1)


def dense_pe_ref(gauss, h, w):
    """fp64 [h * w, 2F]: columns c < F hold sin(t), columns c >= F hold cos(t) of dense_pe_phase_ref"""
    t = dense_pe_phase_ref(gauss, h, w)
    return torch.cat([torch.sin(t), torch.cos(t)], -1)


def spec_accept_ref(amax, fed, nd):
    """-> (n_acc, tok, pos advance): the leading draft ids fed[1 .. nd] that equal the previous row's argmax, the next token
    amax[n_acc], and n_acc + 1 positions consumed; nd is clamped to the k - 1 drafts a pass of k rows can hold."""
    amax, fed = [int(v) for v in amax], [int(v) for v in fed]
    nd = min(int(nd), len(amax) - 1)
    n = 0
    while n < nd and fed[n + 1] == amax[n]:
        n += 1
    return n, amax[n], n + 1
