"""Signed distance to a closed triangle mesh and the penetration term of the object-pose fit, as hand-written HIP
(csrc/mesh_sdf.hip).  NOT the reference's: ``ObjPose_Opt.forward`` has three terms and none of them knows inside from outside.

    c(x)  the closest point of the surface, per face by Ericson's region classification;  d(x) = |x - c(x)|
    k(x)  a face that attains d(x); among faces whose fp32 squared distance compares equal, the lowest index
    w(x)  = (1 / 4 pi) sum_f Omega_f(x),  Omega_f = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|),
            a, b, c = v0 - x, v1 - x, v2 - x;  inside(x) <=> w(x) > 0.5;  sdf(x) = -d inside, +d outside
    L     = (1 / N) sum_i inside(x_i) d(x_i)^2,  dL/dx_i = inside(x_i) 2 (x_i - c(x_i)) / N  (exact almost everywhere)

The mesh is closed and consistently oriented, outward, where a sign is wanted; a face of zero area contributes to neither sum;
no gradient flows to the mesh vertices (the human is a constant of the fit, as in the reference).  No [N, F] array exists
anywhere.  The same bits every call, and for a pose whatever the batch around it.  There is no CPU fallback.
"""
from __future__ import annotations

import re

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import IvlmError, check


def _header_constant(name):
    m = re.search(rf"#define\s+{name}\s+(\d+)", open(_lib.HEADER_PATH).read())
    if not m:
        raise IvlmError(f"include/ivlm_hip.h does not define {name}")
    return int(m.group(1))


TILE = _header_constant("IVLM_MESH_SDF_TILE")    # faces per LDS tile
CHUNK = _header_constant("IVLM_MESH_SDF_CHUNK")  # faces per grid chunk: the longest serial fp32 accumulation of the winding sum


def _check_points(points):
    """-> batched; raises before anything touches the library"""
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"points: expected a tensor, got {type(points).__name__}")
    if points.dim() not in (2, 3) or points.shape[-1] != 3 or points.shape[-2] < 1 or points.shape[0] < 1:
        raise ValueError(f"points: expected [N,3] or [B,N,3] with N >= 1, got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise ValueError(f"points: expected float32, got {points.dtype}")
    _lib.require_gpu(((points, "points"),))
    return points.dim() == 3


class MeshSDF:
    """A mesh prepared for ``query`` and ``penetration``: vertices [N_h,3] fp32, faces [F,3] int32, on the GPU.  The constructor
    validates shapes and dtypes and that faces lies within [0, N_h) - ONE device read, here and before any loop, the convention
    of ``fit_object_pose``'s own one-time reads - refuses vertices.requires_grad (no gradient flows to the mesh), and writes the
    plan (per-face records, the zero-area marks, the bounding box) with one launch sequence.  The plan is reused by every call."""

    def __init__(self, vertices, faces):
        for t, name in ((vertices, "vertices"), (faces, "faces")):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
            if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"{name}: expected [{'N_h' if name == 'vertices' else 'F'},3] with at least one row, got {tuple(t.shape)}")
        if vertices.dtype != torch.float32:
            raise ValueError(f"vertices: expected float32, got {vertices.dtype}")
        if faces.dtype != torch.int32:
            raise ValueError(f"faces: expected int32, got {faces.dtype}")
        if vertices.requires_grad:
            raise ValueError("vertices: requires_grad is set, and no gradient flows to the mesh (detach it: the human is a constant)")
        _lib.require_gpu(((vertices, "vertices"), (faces, "faces")))
        if vertices.device != faces.device:
            raise ValueError(f"vertices and faces must be on one device, got {vertices.device} and {faces.device}")
        n_h, n_f = vertices.shape[0], faces.shape[0]
        lo, hi = (int(v) for v in torch.stack((faces.min(), faces.max())).tolist())  # the one device read
        if lo < 0 or hi >= n_h:
            raise ValueError(f"faces: indices must lie in [0, {n_h}), got [{lo}, {hi}]")
        lib = _lib.load()
        self.device = vertices.device
        self.num_vertices, self.num_faces = n_h, n_f
        v, f = vertices.detach().contiguous(), faces.contiguous()
        with torch.cuda.device(self.device):
            self.plan, nbytes = _lib.workspace(lib.ivlm_mesh_sdf_plan_bytes, "MeshSDF", self.device, N_h=n_h, F=n_f)
            check(lib.ivlm_mesh_sdf_prepare(v.data_ptr(), f.data_ptr(), n_h, n_f, self.plan.data_ptr(), nbytes, _lib.stream()),
                  "mesh_sdf_prepare")

    def _workspace(self, lib, points, B, N):
        if points.device != self.device:
            raise ValueError(f"points: expected a tensor on {self.device}, got {points.device}")
        return _lib.workspace(lib.ivlm_mesh_sdf_workspace_bytes, "mesh_sdf", self.device, B=B, N=N, F=self.num_faces)

    def query(self, points):
        """points [N,3] or [B,N,3] (fp32, GPU) -> (sdf [..,N] fp32, closest [..,N,3] fp32, face [..,N] int32, winding [..,N] fp32).
        No autograd: the outputs are constants."""
        batched = _check_points(points)
        lib = _lib.load()
        p = (points if batched else points.unsqueeze(0)).detach().contiguous()
        B, N = p.shape[0], p.shape[1]
        with torch.cuda.device(self.device):
            ws, nbytes = self._workspace(lib, p, B, N)
            sdf = torch.empty(B, N, dtype=torch.float32, device=self.device)
            closest = torch.empty(B, N, 3, dtype=torch.float32, device=self.device)
            face = torch.empty(B, N, dtype=torch.int32, device=self.device)
            winding = torch.empty(B, N, dtype=torch.float32, device=self.device)
            check(lib.ivlm_mesh_sdf_query(self.plan.data_ptr(), p.data_ptr(), B, N, sdf.data_ptr(), closest.data_ptr(), face.data_ptr(),
                                          winding.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "mesh_sdf_query")
        out = (sdf, closest, face, winding)
        return out if batched else tuple(t[0] for t in out)

    def _penetration(self, p, want_grad):
        """p [B,N,3] contiguous -> (L [B], dL/dp [B,N,3] | None)"""
        lib = _lib.load()
        B, N = p.shape[0], p.shape[1]
        with torch.cuda.device(self.device):
            ws, nbytes = self._workspace(lib, p, B, N)
            value = torch.empty(B, dtype=torch.float32, device=self.device)
            grad = torch.empty(B, N, 3, dtype=torch.float32, device=self.device) if want_grad else None
            check(lib.ivlm_mesh_sdf_penetration(self.plan.data_ptr(), p.data_ptr(), B, N, value.data_ptr(), _lib.ptr(grad),
                                                ws.data_ptr(), nbytes, _lib.stream()), "mesh_sdf_penetration")
        return value, grad

    def penetration(self, points):
        """points [N,3] or [B,N,3] (fp32, GPU) -> L = mean over the points of inside(x) d(x)^2, shape [] or [B].  Differentiable in
        points, once: the forward launch computes dL/dpoints when points requires grad and saves it as a constant, so a double
        backward (create_graph=True) raises.  Points outside the mesh's bounding box cost no face sweep and get an exact zero row."""
        batched = _check_points(points)
        value = _Penetration.apply(points, self)
        return value if batched else value[0]


class _Penetration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, mesh):
        p = (points if points.dim() == 3 else points.unsqueeze(0)).contiguous()
        value, grad = mesh._penetration(p, ctx.needs_input_grad[0])
        ctx.grad = grad  # dL/dpoints per pose: backward only scales it
        ctx.shape = tuple(points.shape)
        return value

    @staticmethod
    @once_differentiable  # the saved gradient is a constant: a double backward raises instead of returning wrong second derivatives
    def backward(ctx, grad_value):
        if not ctx.needs_input_grad[0]:
            return None, None
        return (grad_value.reshape(-1, 1, 1) * ctx.grad).reshape(ctx.shape), None


def mesh_signed_distance(points, vertices, faces):
    """``MeshSDF(vertices, faces).query(points)``: prepare the mesh (one device read) and query it once"""
    _check_points(points)
    return MeshSDF(vertices, faces).query(points)


def penetration_loss(points, mesh_or_vertices, faces=None):
    """``mesh.penetration(points)`` for a prepared ``MeshSDF``, or for ``MeshSDF(vertices, faces)`` prepared here (one device read:
    prepare the mesh once yourself when this runs in a loop)"""
    _check_points(points)
    if isinstance(mesh_or_vertices, MeshSDF):
        if faces is not None:
            raise ValueError("faces: not expected with a prepared MeshSDF")
        return mesh_or_vertices.penetration(points)
    if faces is None:
        raise ValueError("faces: expected [F,3] int32 with vertices (or pass a prepared MeshSDF)")
    return MeshSDF(mesh_or_vertices, faces).penetration(points)
