"""Occlusion-aware image terms for the object-pose fit: the z-buffer of a posed mesh in the camera of ``soft_silhouette`` and a
depth-order term on it (csrc/depth_order.hip).  NOT the reference's: PHOSA's "occlusion-aware silhouette" and "ordinal depth" losses
are the usual formulation.  The reference's ``SSRenderer`` has an unused ``h_vertices`` path, which renders a union silhouette - a
different thing.

    u = fx X / Z + px,  v = fy Y / Z + py;  pixel (row i, col j) has its centre q at (j + 0.5, i + 0.5)
    a face (a, b, c) covers the pixel when e_a = cross(c - b, q - b), e_b = cross(a - c, q - c), e_c = cross(b - a, q - a) are all > 0
    or all < 0; there z = 1 / sum_i (w_i / Z_i) with w_i = e_i / (e_a + e_b + e_c); depth = the smallest z, +inf where no face covers
    x = sign(c) (D_o - D_h) / tau at pixels with c != 0 and D_o, D_h finite;  L = (tau / n) sum |c| softplus(x),  n = sum |c|

A face with zero screen area or a vertex at Z <= 1e-6 is skipped whole, as in the silhouette.  There is no CPU fallback.
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib, silhouette
from ._args import check_devices, side
from ._lib import check, header_constant

L_CHAIN = header_constant("IVLM_DEPTH_ORDER_CHAIN")  # fp32 additions per lane of the backward before fp64 takes over
DEFAULT_TAU = 0.01  # scene units: 1 cm on metric meshes.  A default nobody has measured on data.


def validate(verts, faces, focal, principal, image_size):
    """-> (fx, fy, px, py, H, W): the silhouette's checks of a mesh and a camera; raises before anything touches the library"""
    return silhouette.validate(verts, faces, focal, principal, image_size, 1.0, 0.0)[:6]


def check_image(x, name, shape, dtypes=(torch.float32,)):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(x).__name__}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: expected [{shape[0]},{shape[1]}] (one image, shared by the batch), got {tuple(x.shape)}")
    if x.dtype not in dtypes:
        raise ValueError(f"{name}: expected {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {x.dtype}")


def check_tau(tau):
    try:
        tau = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"tau: expected a number, got {tau!r}") from None
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"tau: expected a finite number > 0, got {tau}")
    return tau


def faces_int32(faces, n):
    """faces [F,3] -> int32, contiguous, every index checked to lie in [0, n) (one host read): all the z-buffer needs of a topology
    (``silhouette.topology_of`` also builds the incidence lists of the backward, which ``depth_image`` never reads)"""
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= n:
        raise ValueError(f"faces: vertex indices must lie in [0, {n}), got [{lo}, {hi}]")
    return faces.to(torch.int32).contiguous()


def depth_image(verts, faces, focal, principal, image_size):
    """The z-buffer of a posed triangle mesh seen by the pinhole camera of ``soft_silhouette``.

    verts [N,3] or [B,N,3] (fp32, GPU, camera coordinates: +Z forward), faces [F,3] (int32 or int64, shared by the batch), focal = f or
    (fx, fy), principal = (px, py), image_size = (H, W) -> (depth [B,H,W] fp32: the perspective-correct depth of the nearest covering
    face, +inf where none covers; face_id [B,H,W] int32: that face, the lowest index among equal depths, -1 where none).  Always with a
    batch axis.  Not differentiable.  The faces' indices are range-checked on every call (one host read: the call is made once per
    scene, not per step); everything else is enqueued on the current stream.  The same bits every call, for a pose whatever the batch
    around it."""
    fx, fy, px, py, H, W = validate(verts, faces, focal, principal, image_size)
    lib = _lib.load()
    v, _ = side(verts.detach(), 2)
    B, N = v.shape[0], v.shape[1]
    f32 = faces_int32(faces, N)
    F = f32.shape[0]
    dev = v.device
    with torch.cuda.device(dev):
        ws, nbytes = _lib.workspace(lib.ivlm_depth_image_workspace_bytes, "depth_image", dev, B=B, N=N, F=F, H=H, W=W)
        depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        face_id = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        check(lib.ivlm_depth_image(v.data_ptr(), f32.data_ptr(), B, N, F, H, W, fx, fy, px, py, depth.data_ptr(), face_id.data_ptr(),
                                   ws.data_ptr(), nbytes, _lib.stream()), "depth_image")
    return depth, face_id


class _DepthOrder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, occ, cw, cam, tau):
        fx, fy, px, py, H, W = cam
        lib = _lib.load()
        v, _ = side(verts, 2)
        B, N = v.shape[0], v.shape[1]
        f32, offsets, slots = silhouette.topology_of(faces, N)
        F = f32.shape[0]
        dev = v.device
        with torch.cuda.device(dev):
            ws, nbytes = _lib.workspace(lib.ivlm_depth_order_workspace_bytes, "depth_order", dev, B=B, N=N, F=F, H=H, W=W)
            value = torch.empty(B, dtype=torch.float32, device=dev)
            check(lib.ivlm_depth_order_forward(v.data_ptr(), f32.data_ptr(), occ.data_ptr(), cw.data_ptr(), B, N, F, H, W, fx, fy, px, py,
                                               tau, value.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "depth_order_forward")
        # the workspace keeps the z-buffer, the winners and the projected faces for the backward; verts through save_for_backward, so
        # that an in-place change of them before the backward raises
        ctx.save_for_backward(verts, offsets, slots, ws, occ, cw)
        ctx.sizes = (nbytes, F)
        ctx.cam, ctx.tau = cam, tau
        ctx.shape = tuple(verts.shape)
        return value

    @staticmethod
    @once_differentiable  # the backward is a kernel, not a graph: a double backward raises instead of returning wrong derivatives
    def backward(ctx, grad_value):
        fx, fy, px, py, H, W = ctx.cam
        verts, offsets, slots, ws, occ, cw = ctx.saved_tensors
        v, _ = side(verts, 2)
        nbytes, F = ctx.sizes
        lib = _lib.load()
        B, N = v.shape[0], v.shape[1]
        g = grad_value.to(torch.float32).expand(B).contiguous()
        with torch.cuda.device(v.device):
            gv = torch.empty(B, N, 3, dtype=torch.float32, device=v.device)
            check(lib.ivlm_depth_order_backward(v.data_ptr(), offsets.data_ptr(), slots.data_ptr(), occ.data_ptr(), cw.data_ptr(),
                                                g.data_ptr(), B, N, F, H, W, fx, fy, px, py, ctx.tau, gv.data_ptr(), ws.data_ptr(), nbytes,
                                                _lib.stream()), "depth_order_backward")
        return gv.reshape(ctx.shape), None, None, None, None, None


def depth_order(verts, faces, occluder_depth, signed_weight, focal, principal, tau=DEFAULT_TAU):
    """The depth-order term: where the photo says which of the mesh and an occluder is in front, a soft penalty on the wrong order.

    verts [N,3] or [B,N,3] (fp32, GPU) and faces [F,3] as ``depth_image`` takes them; occluder_depth [H,W] fp32 (D_h: the occluder's
    ``depth_image``, +inf where it covers nothing) and signed_weight [H,W] fp32 (c > 0: the photo says the mesh is in front here, c < 0:
    the occluder is, 0: ignored), both constant over a fit and shared by the batch; the image size is theirs.  -> [B] (always with a
    batch axis): L = (tau / n) sum |c| softplus(sign(c) (D_o - D_h) / tau) over the pixels with c != 0 where both depths are finite,
    n = sum |c| over the whole image; an exact 0 when n == 0.  tau is in scene units; its default, 0.01 (1 cm on metric meshes), is a
    default nobody has measured on data.  Continuous across a change of the winning face; it jumps only where a pixel enters or leaves
    the mesh's coverage.  Differentiable in verts, once (the winner of every pixel held fixed: the gradient almost everywhere; nothing
    flows through the coverage edge or through occluder_depth); a double backward raises.  The same bits every call, for a pose
    whatever the batch around it."""
    if not isinstance(occluder_depth, torch.Tensor) or occluder_depth.dim() != 2:
        raise ValueError("occluder_depth: expected a tensor [H,W]")
    H, W = occluder_depth.shape
    check_image(occluder_depth, "occluder_depth", (H, W))
    check_image(signed_weight, "signed_weight", (H, W))
    tau = check_tau(tau)
    cam = validate(verts, faces, focal, principal, (H, W))  # (shapes and dtypes of the mesh, then its devices)
    check_devices([(verts, "verts", 2), (occluder_depth, "occluder_depth", 2), (signed_weight, "signed_weight", 2)])
    return _DepthOrder.apply(verts, faces, occluder_depth.detach().contiguous(), signed_weight.detach().contiguous(), cam, tau)


def occluder_maps(human_verts, human_faces, target_mask, focal, principal, human_mask=None):
    """What an occlusion-aware fit needs of the occluder, made once: -> (D_h [H,W], signed_weight [H,W], valid [H,W]), all fp32.

    human_verts [N_h,3] (fp32, GPU, in the frame the object is rendered in), human_faces [F_h,3]; target_mask [H,W] (the object's
    VISIBLE pixels: non-zero = object); human_mask [H,W] (optional: the photo's person mask).  D_h = the human's ``depth_image``;
    cover = isfinite(D_h), or human_mask != 0 when it is given; signed_weight = +1 on cover & target (the object is seen: it is in
    front), -1 on cover & ~target (the body is seen), 0 elsewhere; valid = 1 - (cover & ~target): the don't-care image of the silhouette
    terms (an object pixel hidden by the body is neither wanted nor penalised).  target * valid == target."""
    if not isinstance(target_mask, torch.Tensor) or target_mask.dim() != 2:
        raise ValueError("target_mask: expected a tensor [H,W]")
    H, W = target_mask.shape
    if not isinstance(human_verts, torch.Tensor) or human_verts.dim() != 2:
        raise ValueError("human_verts: expected a tensor [N_h,3] (no batch axis)")
    if human_mask is not None:
        check_image(human_mask, "human_mask", (H, W), (torch.float32, torch.bool, torch.uint8))
    validate(human_verts, human_faces, focal, principal, (H, W))
    check_devices([(human_verts, "human_verts", 2), (target_mask, "target_mask", 2)]
                  + ([] if human_mask is None else [(human_mask, "human_mask", 2)]))
    depth, _ = depth_image(human_verts, human_faces, focal, principal, (H, W))
    return maps_from_depth(depth[0], target_mask, human_mask)


def maps_from_depth(occluder_depth, target_mask, human_mask=None):
    """the image arithmetic of ``occluder_maps`` (plain torch; any device)"""
    target = target_mask != 0
    cover = torch.isfinite(occluder_depth) if human_mask is None else human_mask != 0
    hidden = cover & ~target
    signed = (cover & target).to(torch.float32) - hidden.to(torch.float32)
    return occluder_depth, signed, 1.0 - hidden.to(torch.float32)
