"""float64 reference, derived error bound, inputs and case tables for the mask-resampling kernels.  No GPU in this module.

The kernels under test share one piece of arithmetic (csrc/bilinear.h: axis_src / stage1 / postprocess_at):
``postprocess_kernel`` (csrc/postprocess.hip), ``lift_plan_lowres_kernel`` (csrc/lift.hip) and ``resize_bilinear_kernel``
(csrc/heads.hip).  ``resize64`` / ``post64`` restate the operation in numpy float64 from its definition (bilinear,
align_corners=False), NOT from the kernels' coordinate arithmetic; tests/test_resample_ref_cpu.py pins them to torch's float64
interpolate.  ``bound`` is the error an fp32 evaluation may have against them; it is derived below, not measured, and it is the
only tolerance of tests/test_resample_gpu.py (besides the 1e-6 of the sigmoid and the 1e-3 of the lift, both taken from
tests/test_lift_gpu.py)."""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
SIGMOID_ATOL = 1e-6     # the atol test_postprocess_vs_oracle uses for the sigmoid
GUARD = 64              # guard floats in front of and behind an output buffer
GUARD_BITS = 0x7B5A7B5A  # their bit pattern (a finite value no case produces)


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _axis64(n_in, n_out):
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def resize64(x, oh, ow):
    """x [..., h, w] -> float64 [..., oh, ow]: bilinear, align_corners=False"""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly0, ly1 = _axis64(x.shape[-2], int(oh))
    x0, x1, lx0, lx1 = _axis64(x.shape[-1], int(ow))
    rows = x[..., y0, :] * ly0[:, None] + x[..., y1, :] * ly1[:, None]
    return rows[..., x0] * lx0 + rows[..., x1] * lx1


def post64(low, img, ins, orig):
    """Sam.postprocess_masks in float64: resize to img x img, crop to ins, resize to orig unless ins == orig"""
    m = resize64(low, img, img)[..., : int(ins[0]), : int(ins[1])]
    if tuple(ins) == tuple(orig):
        return m
    return resize64(m, orig[0], orig[1])


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


# ---- bound -------------------------------------------------------------------------------------------------------------------------
def _grad(low):
    """G: the largest |difference| of horizontally or vertically adjacent pixels, per image -> [n, 1, 1]"""
    low = np.asarray(low, dtype=np.float64)
    g = np.zeros(low.shape[:-2])
    if low.shape[-1] > 1:
        g = np.maximum(g, np.abs(np.diff(low, axis=-1)).max(axis=(-2, -1)))
    if low.shape[-2] > 1:
        g = np.maximum(g, np.abs(np.diff(low, axis=-2)).max(axis=(-2, -1)))
    return g[..., None, None]


def bound(low, img=None, ins=None, orig=None, sigmoid=False):
    """|fp32 evaluation - post64| <= bound, per image ([..., 1, 1], broadcasts over the output).  img = None: one resize (resize64).

    An fp32 source coordinate (d + 0.5) * scale - 0.5 is off by at most 4u * max(1, extent) source pixels: the rounding of the scale,
    of the product and of the subtraction, fused or not.  Moving a sample by t pixels along one axis changes a bilinear surface by at
    most G t (G = the largest step between adjacent pixels); the tap index may change with it, the surface is continuous.  Two axes:
    e1 = 2 G 4u max(1, h, w).  The img x img intermediate has steps of at most G max(h, w) / img, and the second resize samples it
    at coordinates off by 4u max(1, in_h, in_w): e2 = 2 G max(h, w) / img 4u max(1, in_h, in_w).  The weights (1 - l1, l1), the
    products and the sums of the taps of both stages round at most 16 times relative to max|low|: 16u max|low|.  The slope of the
    sigmoid is at most 1/4."""
    low = np.asarray(low, dtype=np.float64)
    h, w = low.shape[-2:]
    g = _grad(low)
    e = 2.0 * g * 4.0 * U * max(1, h, w)
    if img is not None and tuple(ins) != tuple(orig):
        e = e + 2.0 * g * max(h, w) / img * 4.0 * U * max(1, int(ins[0]), int(ins[1]))
    e = e + 16.0 * U * np.abs(low).max(axis=(-2, -1))[..., None, None]
    return e / 4.0 + SIGMOID_ATOL if sigmoid else e


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smooth(n, h, w, seed=0):
    """[n, h, w] float32: per image a sum of four sinusoids, spatial frequency <= 0.08 cycles / pixel, amplitudes 1 .. 3.  The
    coordinate term of ``bound`` stays small, a one-tap mistake is of order 1."""
    rng = np.random.default_rng(1000 * seed + 7)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w))
    for i in range(n):
        for _ in range(4):
            f, th = rng.uniform(0.02, 0.08), rng.uniform(0.0, 2.0 * np.pi)
            out[i] += rng.uniform(1.0, 3.0) * np.sin(2.0 * np.pi * f * (np.cos(th) * x + np.sin(th) * y) + rng.uniform(0.0, 2.0 * np.pi))
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ramp(n, h, w):
    """[n, h, w] float32: 100 y + x + 1000 n - asymmetric in the axes and in the image index (exact in fp32 and in bf16 up to 256)"""
    i, y, x = np.mgrid[0:n, 0:h, 0:w]
    out = (100.0 * y + x + 1000.0 * i).astype(np.float32)
    out.setflags(write=False)
    return out


def impulse(h, w, r, c):
    out = np.zeros((h, w), dtype=np.float32)
    out[r, c] = 1.0
    return out


def visible_impulse(case):
    """(r, c) of the low-res pixel that weighs most in the centre output pixel of a geometry (the LAST such pixel along each axis, so
    that a shift by +1 strictly lowers its weight): a coarse output samples few low-res pixels, an impulse elsewhere is invisible"""
    h, w, img, ins, orig = case
    site = []
    for axis, n in ((0, h), (1, w)):
        basis = np.eye(n)[:, :, None] if axis == 0 else np.eye(n)[:, None, :]
        one = lambda k: (k, 1) if axis == 0 else (1, k)
        m = resize64(basis, *one(img))
        m = m[:, : ins[0], :] if axis == 0 else m[:, :, : ins[1]]
        if tuple(ins) != tuple(orig):
            m = resize64(m, *one(orig[axis]))
        wgt = m.reshape(n, -1)[:, orig[axis] // 2]
        site.append(int(np.flatnonzero(wgt >= wgt.max() - 1e-9)[-1]))
    return tuple(site)


def worst(err, e):
    """max err / e (0 / 0 = 0: a zero image has a zero bound and must come out as zeros)"""
    return float(np.max(np.asarray(err) / np.maximum(e, 1e-300)))


def impulse_sites(h, w):
    """the four corners, one mid-edge pixel per side, one interior pixel"""
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1), (h // 2, w // 3)]


def make_input(kind, n, h, w):
    """smooth | ramp | smooth24: ``smooth`` + 24, the input of the bf16-output test (values in about 12 .. 36, across two binades,
    where the bf16 spacing of 2^-4 .. 2^-3 is far above the bound: few stored values have a window of two bf16 values)"""
    return {"smooth": lambda: smooth(n, h, w), "ramp": lambda: ramp(n, h, w), "smooth24": lambda: smooth(n, h, w) + np.float32(24.0)}[kind]()


def to_bf16(a):
    """round-to-nearest-even to bf16, back as float32 (torch's conversion)"""
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
N_IMAGES = 3  # the image stride is exercised

# (h, w, img, (in_h, in_w), (oh, ow)).  postprocess_kernel stores a group of four pixels either as one float4 (ow % 4 == 0) or pixel
# by pixel ("scalar": ow % 4 != 0, every group of the row), and runs (ow + 1023) / 1024 blocks of 1024 pixels along x.
POST_CASES = (
    [
        (8, 8, 32, (32, 32), (32, 32)),        # identity second resize; FLOAT4 stores
        (8, 8, 32, (32, 21), (32, 21)),        # identity second resize behind a crop; ow = 21: SCALAR stores, tail of 1
        (8, 8, 32, (32, 21), (47, 31)),        # both resizes, odd sizes; scalar stores, tail of 3
    ]
    # every tail length against both store paths: k = 4, 8 float4; the rest scalar
    + [(8, 8, 32, (32, 32), (2, k)) for k in range(1, 10)]
    + [
        (8, 8, 32, (32, 32), (4, 1022)),       # ow even, no multiple of 4: scalar stores, the last group holds 2 pixels
        (16, 12, 64, (64, 43), (5, 1027)),     # h != w; TWO BLOCKS in x (gridDim.x = 2), scalar stores
        (16, 16, 64, (64, 64), (3, 2048)),     # float4 stores across TWO BLOCKS in x
        (16, 16, 64, (48, 64), (3, 2049)),     # THREE BLOCKS in x, the third holds one pixel
        (16, 16, 64, (64, 43), (31, 21)),      # down-scaling second resize
        (4, 4, 16, (16, 16), (1, 1)),          # one-pixel output
        (1, 1, 8, (8, 8), (5, 6)),             # one-pixel input: every tap is clamped
        (256, 256, 1024, (1024, 683), (7, 1367)),   # real coordinate magnitudes, few rows; two blocks, scalar stores
        (256, 256, 1024, (1024, 1024), (5, 1023)),
    ]
)
assert len(POST_CASES) == 21 and len(set(POST_CASES)) == 21

IMPULSE_CASES = [c for c in POST_CASES if c[:3] == (8, 8, 32) and c[4][1] >= 21 and c[4][0] >= 32] + [(16, 12, 64, (64, 43), (5, 1027))]
VALID_CASES = [c for c in POST_CASES if c[4] in ((32, 21), (47, 31), (5, 1027))]
LIFT_CASES = [c for c in POST_CASES if c[4] in ((47, 31), (5, 1027), (3, 2049))]
assert len(IMPULSE_CASES) == 4 and len(VALID_CASES) == 3 and len(LIFT_CASES) == 3

# ops.resize_bilinear: (h, w) -> (oh, ow)
RESIZE_CASES = [((8, 8), (2, k)) for k in range(1, 10)] + [((16, 12), (5, 1027)), ((64, 64), (33, 47)), ((64, 64), (1, 1)), ((12, 16), (7, 5))]
BF16_STRADDLE_MAX = 0.02  # share of pixels whose window [bf16(ref - e), bf16(ref + e)] holds two bf16 values


def case_id(c):
    if len(c) == 2:
        (h, w), (oh, ow) = c
        return f"{h}x{w}-to{oh}x{ow}"
    h, w, img, ins, orig = c
    return f"{h}x{w}-img{img}-in{ins[0]}x{ins[1]}-to{orig[0]}x{orig[1]}"


def gt_mask(n, oh, ow, ignore=-1.0):
    """ground-truth mask [n, oh, ow] float32: ``ignore`` in a checkerboard, in one whole row and in the last column; 0, 1 and 0.5
    elsewhere"""
    i, y, x = np.mgrid[0:n, 0:oh, 0:ow]
    gt = np.choose((y * 7 + x * 3 + i) % 3, [0.0, 1.0, 0.5]).astype(np.float32)
    gt[(x + y + i) % 2 == 0] = ignore
    gt[:, oh // 2, :] = ignore
    gt[:, :, ow - 1] = ignore
    return gt


@functools.lru_cache(maxsize=None)
def post_reference(case, kind, bf16):
    """-> (low float32 [n, h, w] (bf16 values when ``bf16``), post64 of it, bound, sigmoid bound); computed once, read-only"""
    h, w, img, ins, orig = case
    low = make_input(kind, N_IMAGES, h, w)
    if bf16:
        low = to_bf16(low)
    ref = post64(low, img, ins, orig)
    out = (low, ref, bound(low, img, ins, orig), bound(low, img, ins, orig, sigmoid=True))
    for a in out:
        a.setflags(write=False)
    return out


def bf16_window(ref, e):
    """[bf16(ref - e), bf16(ref + e)] as float64: rounding is monotonic, so an fp32 value within e of ref is stored inside it"""
    return to_bf16(ref - e).astype(np.float64), to_bf16(ref + e).astype(np.float64)
