"""Signed distance to a closed triangle mesh and the penetration term of the object-pose fit, as hand-written HIP
(csrc/mesh_sdf.hip).  NOT the reference's: ``ObjPose_Opt.forward`` has three terms and none of them knows inside from outside.

    c(x)  the closest point of the surface, per face by Ericson's region classification;  d(x) = |x - c(x)|
    k(x)  a face that attains d(x); among faces whose fp32 squared distance compares equal, the lowest index
    w(x)  = (1 / 4 pi) sum_f Omega_f(x),  Omega_f = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|),
            a, b, c = v0 - x, v1 - x, v2 - x;  inside(x) <=> w(x) > 0.5;  sdf(x) = -d inside, +d outside
    L     = (1 / N) sum_i inside(x_i) d(x_i)^2,  dL/dx_i = inside(x_i) 2 (x_i - c(x_i)) / N  (exact almost everywhere)

The other direction, ``MeshSDF.intrusion``: the prepared mesh is the OBJECT (closed, outward, constant; ``check_closed``) under B poses
(rot6d, t, s), y = (s v) R + t, and the points are the human's vertices h_j [N,3], shared by the batch:

    x_j = ((h_j - t) R^T) / s   the human vertex in the object's canonical frame;  c_j, d_j, inside_j = the query at x_j
    e_j = s (x_j - c_j) R       the world-frame vector from the object's surface to h_j
    L   = (1 / N) sum_j inside_j |e_j|^2 = (1 / N) sum_j inside_j (s d_j)^2
    dL/dt = -(2 / N) sum inside e;  dL/ds = -(2 / N) sum inside e . (c R);  dL/dR_ik = -(2 s / N) sum inside c_i e_k, then to rot6d

(c_j is a constant of the derivative, by the envelope theorem.)  13 fp64 sums per pose; no [B, N, 3] gradient array exists.

The mesh is closed and consistently oriented, outward, where a sign is wanted; a face of zero area contributes to neither sum;
no gradient flows to the mesh vertices (the human is a constant of the fit, as in the reference).  No [N, F] array exists
anywhere.  The same bits every call, and for a pose whatever the batch around it.  There is no CPU fallback.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import _lib
from ._args import ValueWithGradients, check_devices, check_points, side
from ._lib import check, header_constant
from .pose import pose_arguments

TILE = header_constant("IVLM_MESH_SDF_TILE")    # faces per LDS tile
CHUNK = header_constant("IVLM_MESH_SDF_CHUNK")  # faces per grid chunk: the longest serial fp32 accumulation of the winding sum


def _check_points(points):
    """-> batched; raises before anything touches the library"""
    check_points(points, "points")
    check_devices([(points, "points", 2)])
    return points.dim() == 3


def check_closed(vertices, faces):
    """A one-time host check that (vertices [N_v,3], faces [F,3]) is a closed, consistently oriented, outward mesh - what a signed
    distance to it means anything for.  Tensors (copied to the host: one device read) or arrays.  Raises ValueError naming the first
    defect, in this order: an index outside [0, N_v); a face with a repeated index; a directed edge that occurs twice (two
    neighbours wound against each other); a directed edge whose reverse does not occur exactly once (a hole, or an edge of three
    faces); a signed volume <= 0 (inward).  Pure numpy: usable without a GPU."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"vertices: expected [N_v,3] with at least one row, got {tuple(v.shape)}")
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected integers [F,3] with at least one row, got {f.dtype} {tuple(f.shape)}")
    v, f = v.astype(np.float64), f.astype(np.int64)
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f"faces: indices must lie in [0, {v.shape[0]}), got [{int(f.min())}, {int(f.max())}]")
    repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    if repeated.any():
        k = int(np.nonzero(repeated)[0][0])
        raise ValueError(f"faces: face {k} = {f[k].tolist()} repeats an index (a zero-area face: the mesh is not a closed surface)")
    n = v.shape[0]
    a, b = f.reshape(-1), f[:, (1, 2, 0)].reshape(-1)  # the directed edges a -> b, three per face, in face order
    key, rev = a * n + b, b * n + a
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    if (count > 1).any():
        e = int(first[count > 1].min())
        raise ValueError(f"faces: the directed edge {int(a[e])} -> {int(b[e])} (face {e // 3}) occurs {int(count[uniq == key[e]][0])} times: "
                         "two faces are wound against each other (or the edge has more than two faces)")
    at = np.searchsorted(uniq, rev)
    found = (at < len(uniq)) & (uniq[np.minimum(at, len(uniq) - 1)] == rev)
    if not found.all():
        e = int(np.nonzero(~found)[0][0])
        raise ValueError(f"faces: the directed edge {int(a[e])} -> {int(b[e])} (face {e // 3}) has no reverse {int(b[e])} -> {int(a[e])}: "
                         "the mesh is open there")
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float((v0 * np.cross(v1, v2)).sum() / 6.0)
    if not volume > 0.0:
        raise ValueError(f"faces: the signed volume is {volume:.6g}, not > 0: the faces are wound inward (flip them)")


class MeshSDF:
    """A mesh prepared for ``query``, ``penetration`` and ``intrusion``: vertices [N_h,3] fp32, faces [F,3] int32, on the GPU.  The constructor
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
        p, _ = side(points.detach(), 2)
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

    def _penetration(self, points, need):
        """-> (L [B], dL/dpoints per pose [B,N,3] | None)"""
        lib = _lib.load()
        p, _ = side(points, 2)
        B, N = p.shape[0], p.shape[1]
        with torch.cuda.device(self.device):
            ws, nbytes = self._workspace(lib, p, B, N)
            value = torch.empty(B, dtype=torch.float32, device=self.device)
            grad = torch.empty(B, N, 3, dtype=torch.float32, device=self.device) if need[0] else None
            check(lib.ivlm_mesh_sdf_penetration(self.plan.data_ptr(), p.data_ptr(), B, N, value.data_ptr(), _lib.ptr(grad),
                                                ws.data_ptr(), nbytes, _lib.stream()), "mesh_sdf_penetration")
        return value, grad

    def penetration(self, points):
        """points [N,3] or [B,N,3] (fp32, GPU) -> L = mean over the points of inside(x) d(x)^2, shape [] or [B].  Differentiable in
        points, once: the forward launch computes dL/dpoints when points requires grad and saves it as a constant, so a double
        backward (create_graph=True) raises.  Points outside the mesh's bounding box cost no face sweep and get an exact zero row."""
        batched = _check_points(points)
        value = ValueWithGradients.apply(self._penetration, points)
        return value if batched else value[0]

    def _intrusion(self, h, r6, t, s, need):
        """h [N,3] contiguous, r6 [B,6], t [B,3], s [B] -> (L [B], dL/drot6d | None, dL/dt | None, dL/ds | None)"""
        lib = _lib.load()
        r6, t, s = r6.contiguous(), t.contiguous(), s.contiguous()
        B, N = r6.shape[0], h.shape[0]
        dev = self.device
        with torch.cuda.device(dev):
            ws, nbytes = _lib.workspace(lib.ivlm_mesh_sdf_intrusion_workspace_bytes, "mesh_sdf_intrusion", dev, B=B, N=N, F=self.num_faces)
            value = torch.empty(B, dtype=torch.float32, device=dev)
            grads = [torch.empty(*shape, dtype=torch.float32, device=dev) if want else None
                     for want, shape in zip(need, ((B, 6), (B, 3), (B,)))]
            check(lib.ivlm_mesh_sdf_intrusion(self.plan.data_ptr(), h.data_ptr(), r6.data_ptr(), t.data_ptr(), s.data_ptr(), B, N,
                                              value.data_ptr(), _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]),
                                              ws.data_ptr(), nbytes, _lib.stream()), "mesh_sdf_intrusion")
        return (value, *grads)

    def intrusion(self, points, rot6d, translation, scaling=1.0):
        """This mesh is the object, posed B times by (rot6d [B,6], translation [B,3], scaling a number, [B] or [B,1]) as
        ``pose.pose_transform`` poses it (or one pose: [6], [3], a scalar); points [N,3] (fp32, GPU) are the human's vertices, shared
        by the batch and constant (requires_grad is refused).  -> L = mean over the points of inside (s d)^2 with d the distance of
        the un-posed point to this mesh, shape [B] or [].  Differentiable in rot6d, translation and a tensor scaling, once: the
        forward launch computes the gradients that are needed and saves them as constants, so a double backward raises.  A pose
        whose scaling is not > 0 gets NaN.  The mesh must be closed and outward (``check_closed``)."""
        r6, t, s, batched = pose_arguments(points, rot6d, translation, scaling, name="points")
        if points.device != self.device:
            raise ValueError(f"points: expected a tensor on {self.device}, got {points.device}")
        value = ValueWithGradients.apply(functools.partial(self._intrusion, points.contiguous()), r6, t, s)
        return value if batched else value[0]


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
