"""The rigid transform of the object-pose fit for B poses in one launch, with an analytic backward (csrc/pose.hip), and the starts
of a multi-start fit: ``fit.apply_transformation`` as a HIP kernel pair, so that B starts cost three launches per step instead of
about forty small ones per start.

    R = rot6d_to_matrix(rot6d)  (Gram-Schmidt of the two interleaved columns, the third their cross product)
    y_n = (s v_n) R + t         (row vectors, as the reference has them)

Not the reference's: the reference runs one start from one pose (optim/fit.py); ``cube_rotations``, ``axis_rotations`` and
``pose_starts`` produce the starts of ``fit.search_object_pose``, a deliberate addition.  There is no CPU fallback.
"""
from __future__ import annotations

import itertools
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._args import check_devices, check_points
from ._lib import check, header_constant

# Error model of the kernels, in units of 2^-24 (IVLM_POSE_* of include/ivlm_hip.h); tests derive their bounds from these.
POSE_CHUNK = header_constant("IVLM_POSE_CHUNK")     # vertices per block of the backward's partial sums: a function of nothing but the build
L_CHAIN = header_constant("IVLM_POSE_CHAIN")        # every term is converted to fp64 before it is added
FWD_ULPS = header_constant("IVLM_POSE_FWD_ULPS")    # |delta y_nj| <= FWD_ULPS 2^-24 (s sum_i |v_ni| |R_ij| + |t_j|)
GRAD_ULPS = header_constant("IVLM_POSE_GRAD_ULPS")  # |delta dL/dtheta| <= GRAD_ULPS 2^-24 sum_n |d y_n / d theta| |g_n|


def gram_schmidt_backward(rot6d, grad_R):
    """The chain of the finish kernel, written once in torch as its documentation: rot6d [6] and dL/dR [3,3] -> dL/drot6d [6], in
    the dtype of its inputs (the kernel does this in fp64).  With a1_i = rot6d[2 i], a2_i = rot6d[2 i + 1]:

        b1 = a1 / n1, n1 = max(|a1|, 1e-12);  d = b1 . a2;  u2 = a2 - d b1;  b2 = u2 / n2, n2 = max(|u2|, 1e-12);  b3 = b1 x b2
        R = [b1 b2 b3] by columns, so dL/db_k is column k of dL/dR

    backwards: b3 = b1 x b2 gives gb1 += b2 x gb3, gb2 += gb3 x b1;  b2 = u2 / n2 gives gu2 = (gb2 - b2 (b2 . gb2)) / n2 (a clamped
    norm is a constant: gu2 = gb2 / n2);  u2 = a2 - d b1 gives ga2 = gu2, gd = -(b1 . gu2), gb1 -= d gu2;  d = b1 . a2 gives
    gb1 += gd a2, ga2 += gd b1;  b1 = a1 / n1 as b2."""
    a = rot6d.reshape(3, 2)
    a1, a2 = a[:, 0], a[:, 1]
    eps = 1e-12
    l1 = a1.norm()
    n1 = l1.clamp_min(eps)
    b1 = a1 / n1
    d = (b1 * a2).sum()
    u2 = a2 - d * b1
    l2 = u2.norm()
    n2 = l2.clamp_min(eps)
    b2 = u2 / n2
    gb1, gb2, gb3 = grad_R[:, 0], grad_R[:, 1], grad_R[:, 2]
    gb1 = gb1 + torch.linalg.cross(b2, gb3)
    gb2 = gb2 + torch.linalg.cross(gb3, b1)
    gu2 = (gb2 - b2 * ((b2 * gb2).sum() if float(l2) > eps else 0.0)) / n2
    gd = -(b1 * gu2).sum()
    gb1 = gb1 + gd * a2 - d * gu2
    ga2 = gu2 + gd * b1
    ga1 = (gb1 - b1 * ((b1 * gb1).sum() if float(l1) > eps else 0.0)) / n1
    return torch.stack((ga1, ga2), dim=-1).reshape(6)


def pose_arguments(vertices, rot6d, translation, scaling, name="vertices"):
    """The arguments of a call that poses ``vertices`` [N,3] (a constant: it must not require grad) B times: rot6d [B,6] with
    translation [B,3] and scaling a number, [B] or [B,1], or one pose ([6], [3], a scalar).  Raises before anything touches the
    library; -> (r6 [B,6], t [B,3], s [B], batched)."""
    check_points(vertices, name, batch=False)
    if vertices.requires_grad:
        raise ValueError(f"{name}: requires_grad is set, and it is a constant of this call: it must not require grad (detach it)")
    if not isinstance(rot6d, torch.Tensor):
        raise ValueError(f"rot6d: expected a tensor, got {type(rot6d).__name__}")
    if rot6d.dim() not in (1, 2) or rot6d.shape[-1] != 6 or rot6d.shape[0] < 1:
        raise ValueError(f"rot6d: expected [6] or [B,6] with B >= 1, got {tuple(rot6d.shape)}")
    if rot6d.dtype != torch.float32:
        raise ValueError(f"rot6d: expected float32, got {rot6d.dtype}")
    batched = rot6d.dim() == 2
    B = rot6d.shape[0] if batched else 1
    want = (B, 3) if batched else (3,)
    if not isinstance(translation, torch.Tensor):
        raise ValueError(f"translation: expected a tensor, got {type(translation).__name__}")
    if tuple(translation.shape) != want:
        raise ValueError(f"translation: expected {list(want)} (one per pose of rot6d), got {tuple(translation.shape)}")
    if translation.dtype != torch.float32:
        raise ValueError(f"translation: expected float32, got {translation.dtype}")
    named = [(vertices, name, 2), (rot6d, "rot6d", 1), (translation, "translation", 1)]
    if isinstance(scaling, torch.Tensor):
        if scaling.numel() not in (1, B) or scaling.dim() > 2 or (scaling.dim() == 2 and scaling.shape[1] != 1):
            raise ValueError(f"scaling: expected a number, [{B}] or [{B},1], got {tuple(scaling.shape)}")
        if scaling.dtype != torch.float32:
            raise ValueError(f"scaling: expected float32, got {scaling.dtype}")
        named.append((scaling, "scaling", 0))
    else:
        try:
            ok = math.isfinite(float(scaling))
        except (TypeError, ValueError):
            raise ValueError(f"scaling: expected a number or a tensor, got {scaling!r}") from None
        if not ok:
            raise ValueError(f"scaling: expected a finite number, got {scaling!r}")
    check_devices(named)
    if isinstance(scaling, torch.Tensor):
        s = scaling.reshape(-1).expand(B)
    else:
        s = torch.full((B,), float(scaling), dtype=torch.float32, device=vertices.device)
    return (rot6d, translation, s, True) if batched else (rot6d.unsqueeze(0), translation.unsqueeze(0), s, False)


class _PoseTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, rot6d, trans, scale):
        lib = _lib.load()
        v, r6, t, s = verts.contiguous(), rot6d.contiguous(), trans.contiguous(), scale.contiguous()
        B, N = r6.shape[0], v.shape[0]
        _lib.workspace(lib.ivlm_pose_transform_workspace_bytes, "pose_transform", None, B=B, N=N)  # (the forward needs none: the check)
        dev = v.device
        with torch.cuda.device(dev):
            out = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
            check(lib.ivlm_pose_transform_forward(v.data_ptr(), r6.data_ptr(), t.data_ptr(), s.data_ptr(), B, N, out.data_ptr(),
                                                  _lib.stream()), "pose_transform_forward")
        ctx.save_for_backward(v, r6, s)
        return out

    @staticmethod
    @once_differentiable  # the backward is a kernel, not a graph: a double backward raises instead of returning wrong derivatives
    def backward(ctx, grad_out):
        v, r6, s = ctx.saved_tensors
        need_r, need_t, need_s = ctx.needs_input_grad[1:4]
        if not (need_r or need_t or need_s):
            return None, None, None, None
        lib = _lib.load()
        B, N = r6.shape[0], v.shape[0]
        g = grad_out.to(torch.float32).contiguous()
        dev = v.device
        with torch.cuda.device(dev):
            ws, nbytes = _lib.workspace(lib.ivlm_pose_transform_workspace_bytes, "pose_transform", dev, B=B, N=N)
            g_r = torch.empty(B, 6, dtype=torch.float32, device=dev) if need_r else None
            g_t = torch.empty(B, 3, dtype=torch.float32, device=dev) if need_t else None
            g_s = torch.empty(B, dtype=torch.float32, device=dev) if need_s else None
            p = _lib.ptr
            check(lib.ivlm_pose_transform_backward(v.data_ptr(), r6.data_ptr(), s.data_ptr(), g.data_ptr(), B, N, p(g_r), p(g_t), p(g_s),
                                                   ws.data_ptr(), nbytes, _lib.stream()), "pose_transform_backward")
        return None, g_r, g_t, g_s


def pose_transform(vertices, rot6d, translation, scaling=1.0):
    """``fit.apply_transformation`` for B poses in one launch: (vertices * scaling) @ R(rot6d) + translation, row vectors.

    vertices [N,3] (fp32, GPU, constant: it must not require grad), rot6d [B,6] with translation [B,3] and scaling a number, [B] or
    [B,1] -> [B,N,3]; rot6d [6] with translation [3] and a scalar scaling -> [N,3].  Differentiable in rot6d, translation and a tensor
    scaling, once: a double backward raises.  The backward is two launches (fp64 partial sums per ``POSE_CHUNK`` vertices, then one
    small block per pose that adds them in order and chains through the Gram-Schmidt, ``gram_schmidt_backward``); a parameter that
    does not require grad is not computed.  No atomics and no host read: the same bits every call, for a pose whatever the batch
    around it and its place in it.  Documented errors: ``FWD_ULPS`` and ``GRAD_ULPS``."""
    r6, t, s, batched = pose_arguments(vertices, rot6d, translation, scaling)
    out = _PoseTransform.apply(vertices, r6, t, s)
    return out if batched else out.view(vertices.shape[0], 3)


def cube_rotations():
    """-> [24,3,3] fp32: the proper rotations of the cube, the signed permutation matrices of determinant +1.  Row i of matrix
    (perm, sign) is sign[i] e_perm[i]; the order is perm over the permutations of (0, 1, 2) in lexicographic order, then sign over
    ``itertools.product((1, -1), repeat=3)``, keeping determinant +1 (four sign triples per permutation).  Index 0 is the identity."""
    out = []
    for perm in itertools.permutations(range(3)):
        parity = 1
        for i in range(3):
            for j in range(i + 1, 3):
                if perm[i] > perm[j]:
                    parity = -parity
        for sign in itertools.product((1, -1), repeat=3):
            if parity * sign[0] * sign[1] * sign[2] != 1:
                continue
            q = torch.zeros(3, 3, dtype=torch.float32)
            for i in range(3):
                q[i, perm[i]] = sign[i]
            out.append(q)
    return torch.stack(out)


def axis_rotations(k, axis=(0.0, 1.0, 0.0)):
    """-> [k,3,3] fp32: the rotations by 2 pi j / k, j = 0 .. k - 1, about ``axis`` (Rodrigues, I + sin K + (1 - cos) K^2, evaluated in
    fp64), for an object whose up direction is known.  Index 0 is the identity."""
    if not isinstance(k, int) or k < 1:
        raise ValueError(f"k: expected an integer >= 1, got {k!r}")
    a = torch.as_tensor(axis, dtype=torch.float64).reshape(-1)
    if a.numel() != 3 or not bool(torch.isfinite(a).all()) or float(a.norm()) == 0.0:
        raise ValueError(f"axis: expected three finite numbers, not all zero, got {axis!r}")
    x, y, z = (a / a.norm()).tolist()
    K = torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=torch.float64)
    eye = torch.eye(3, dtype=torch.float64)
    out = [eye + math.sin(2 * math.pi * j / k) * K + (1 - math.cos(2 * math.pi * j / k)) * (K @ K) for j in range(k)]
    out[0] = eye
    return torch.stack(out).float()


def compose_rotations(rotations, R0):
    """rotations [K,3,3], R0 [3,3] -> rotations[k] @ R0 [K,3,3], elementwise: entry (i, j) is ((q_i0 R0_0j + q_i1 R0_1j) + q_i2 R0_2j).
    For a signed permutation matrix two of the three products are zeros and the third is +-R0_pj exactly, and adding zeros to it is
    exact, so every entry is bit-equal to plus or minus an entry of R0 (finite R0) - what a library GEMM does not promise."""
    q = rotations
    return (q[:, :, 0:1] * R0[0] + q[:, :, 1:2] * R0[1]) + q[:, :, 2:3] * R0[2]


def check_rotations(rotations):
    if not isinstance(rotations, torch.Tensor):
        raise ValueError(f"rotations: expected a tensor, got {type(rotations).__name__}")
    if rotations.dim() != 3 or tuple(rotations.shape[1:]) != (3, 3) or rotations.shape[0] < 1:
        raise ValueError(f"rotations: expected [K,3,3] with K >= 1, got {tuple(rotations.shape)}")
    if rotations.dtype != torch.float32:
        raise ValueError(f"rotations: expected float32, got {rotations.dtype}")


def check_start(R0, T0, s0, device):
    """-> (R0 [3,3], T0 [3], s0 0-dim) fp32 on ``device``, the identity where None"""
    if R0 is None:
        R0 = torch.eye(3)
    if T0 is None:
        T0 = torch.zeros(3)
    for t, name, shape in ((R0, "R0", (3, 3)), (T0, "T0", (3,))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {list(shape)}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: expected float32, got {t.dtype}")
    if isinstance(s0, torch.Tensor):
        if s0.numel() != 1 or s0.dtype != torch.float32:
            raise ValueError(f"s0: expected a number or one float32 element, got {tuple(s0.shape)} {s0.dtype}")
        s0 = s0.detach().reshape(())
    else:
        try:
            s0 = torch.tensor(float(s0), dtype=torch.float32)
        except (TypeError, ValueError):
            raise ValueError(f"s0: expected a number, got {s0!r}") from None
    return R0.detach().to(device), T0.detach().to(device), s0.to(device)


def pose_starts(rotations, R0=None, T0=None, s0=1.0):
    """The K starts of a multi-start fit around one pose: start k is R_k = rotations[k] @ R0 with the translation T0 and the scale s0
    of that pose.  In the row-vector convention v R_k = (v rotations[k]) R0: the extra rotation turns the object in its own frame,
    about the mesh origin (the centroid, where the reference's optim/data_io.py puts it), so T0 is shared by the starts.

    rotations [K,3,3] (fp32), R0 [3,3], T0 [3], s0 a number (None: the identity, zero) -> (rot6d [K,6], T [K,3], s [K]) on the device
    of ``rotations``.  The product is ``compose_rotations``: exact for ``cube_rotations``, whose starts are signed row permutations
    of R0."""
    from .fit import matrix_to_rot6d

    check_rotations(rotations)
    R0, T0, s0 = check_start(R0, T0, s0, rotations.device)
    K = rotations.shape[0]
    R = compose_rotations(rotations.detach(), R0)
    return matrix_to_rot6d(R), T0.expand(K, 3).contiguous(), s0.expand(K).contiguous()
