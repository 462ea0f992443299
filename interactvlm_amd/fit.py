"""The object-pose fit of the reference's joint fitting stage (optim/optimizer.py ``ObjPose_Opt``, optim/fit.py:217-290): the thin
loop that composes ``contact_icp`` (the start), ``soft_silhouette`` + ``silhouette_terms`` (mask and centroid terms) and
``contact_distance`` (the contact term), for B starts at once.

Not the reference's: no Phong render, no depth image, no logging or video.  The rigid transform is applied pose by pose with the
operations of a single-pose run, so that every start of a batch computes the bits of its own unbatched run.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .contact_icp import contact_icp
from .contact_pair import contact_distance
from .silhouette import silhouette_terms, soft_silhouette

# optim/cfg/fit.yaml
DEFAULT_LOSS_WEIGHTS = {
    "mask_loss": {"w": 5.0, "kick_in": 0},
    "centroid_loss": {"w": 1e-4, "kick_in": 0},
    "contact_loss": {"w": 10.0, "kick_in": 0},
}


def matrix_to_rot6d(matrix):
    """[...,3,3] -> [B,6]: the first two COLUMNS, interleaved as the reference's ``stack((a1, a2), -1).view(-1, 6)`` has them"""
    matrix = matrix.reshape(-1, 3, 3)
    return torch.stack((matrix[:, :, 0], matrix[:, :, 1]), dim=-1).reshape(-1, 6)


def rot6d_to_matrix(rot_6d):
    """[B,6] (or [6]) -> [B,3,3]: Gram-Schmidt of the two columns, the third is their cross product"""
    rot_6d = rot_6d.reshape(-1, 3, 2)
    a1, a2 = rot_6d[:, :, 0], rot_6d[:, :, 1]
    b1 = F.normalize(a1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    b3 = torch.linalg.cross(b1, b2)
    return torch.stack((b1, b2, b3), dim=-1)


def _transform_one(vertices, rot6d, translation, scaling):
    R = rot6d_to_matrix(rot6d)[0]
    x = vertices * scaling
    # x R, elementwise: no library GEMM whose summation order could depend on the shapes around it
    return x[:, 0:1] * R[0] + x[:, 1:2] * R[1] + x[:, 2:3] * R[2] + translation


def apply_transformation(vertices, rot6d, translation, scaling=1.0):
    """The reference's row-vector convention: (vertices * scaling) @ R(rot6d) + translation.

    vertices [N,3]; rot6d [6] with translation [3] and a scalar scaling -> [N,3]; rot6d [B,6] with translation [B,3] and scaling a
    number, [B] or [B,1] -> [B,N,3], each pose transformed by the operations of the unbatched call."""
    if rot6d.dim() == 1:
        return _transform_one(vertices, rot6d, translation, scaling)
    B = rot6d.shape[0]

    def scale_of(b):
        if not isinstance(scaling, torch.Tensor) or scaling.dim() == 0:
            return scaling
        return scaling.reshape(-1)[b if scaling.numel() > 1 else 0]

    return torch.stack([_transform_one(vertices, rot6d[b], translation[b], scale_of(b)) for b in range(B)])


def mask_bbox_centre(mask):
    """(row, col) centre of the bounding box of the non-zero pixels, as ``ObjPose_Opt.__init__`` has it ((min + max) / 2), without
    ``nonzero``; an empty mask gives the image centre"""
    H, W = mask.shape
    on = mask != 0
    out = []
    for hit, n in ((on.any(1), H), (on.any(0), W)):
        idx = torch.arange(n, device=mask.device)
        lo = torch.where(hit, idx, n).min()
        hi = torch.where(hit, idx, -1).max()
        out.append(torch.where(hi >= 0, (lo + hi).to(torch.float32) / 2.0, torch.tensor(n / 2.0, device=mask.device)))
    return torch.stack(out)


class ObjectPoseFit(nn.Module):
    """The terms of ``ObjPose_Opt.forward`` for B starts at once, with its quirks: the silhouette is rendered on the object moved by
    ``hum_centroid_offset`` while the contact term is taken on the un-offset vertices; the target centroid is the centre of the
    target mask's bounding box; a term counts when ``kick_in >= 0 and step >= kick_in``.

    rotation_init [B,6] (or [6]), translation_init [B,3], scaling_init a number or [B]; obj_vertices [N,3], obj_faces [F,3],
    human_vertices [N_h,3], obj_contact_probs [N], human_contact_probs [N_h], target_mask [H,W]; focal / principal as
    ``soft_silhouette`` takes them.  ``vars`` selects what is optimised: "pose", "scale" or both.
    forward(loss_weights, step=None) -> (total [B], {term: [B]})."""

    def __init__(self, rotation_init, translation_init, scaling_init, obj_vertices, obj_faces, human_vertices, obj_contact_probs,
                 human_contact_probs, target_mask, focal, principal, hum_centroid_offset=None, vars=("pose",), sigma=1e-4,
                 blur_radius=None):
        super().__init__()
        unknown = set(vars) - {"pose", "scale"}
        if unknown:
            raise ValueError(f"vars: expected a subset of ('pose', 'scale'), got {sorted(unknown)}")
        rot = rotation_init.detach().clone().float().reshape(-1, 6)
        B = rot.shape[0]
        trans = translation_init.detach().clone().float().reshape(-1, 3)
        if trans.shape[0] != B:
            raise ValueError(f"translation_init: expected [{B},3], got {tuple(translation_init.shape)}")
        scale = torch.as_tensor(scaling_init, dtype=torch.float32, device=rot.device).detach().clone().reshape(-1)
        if scale.numel() not in (1, B):
            raise ValueError(f"scaling_init: expected a number or [{B}], got {tuple(scale.shape)}")
        scale = scale.expand(B).contiguous()
        self.rotation = nn.Parameter(rot, requires_grad="pose" in vars)
        self.translation = nn.Parameter(trans, requires_grad="pose" in vars)
        if "scale" in vars:
            self.scale = nn.Parameter(scale, requires_grad=True)
        else:
            self.register_buffer("scale", scale)
        self.step = 0
        self.camera = (focal, principal)
        self.sigma, self.blur_radius = sigma, blur_radius
        self.register_buffer("obj_vertices", obj_vertices.detach().float())
        self.register_buffer("obj_faces", obj_faces.detach())
        self.register_buffer("human_vertices", human_vertices.detach().float())
        self.register_buffer("object_contact_probs", obj_contact_probs.detach())
        self.register_buffer("human_contact_probs", human_contact_probs.detach())
        off = torch.zeros(3) if hum_centroid_offset is None else hum_centroid_offset.detach().float()
        self.register_buffer("hum_centroid_offset", off.to(obj_vertices.device))
        mask = (target_mask != 0).float()
        self.register_buffer("target_mask", mask)
        self.register_buffer("target_mask_centroid", mask_bbox_centre(mask))

    def object_vertices(self):
        return apply_transformation(self.obj_vertices, self.rotation, self.translation, self.scale)

    def forward(self, loss_weights=None, step=None):
        weights = DEFAULT_LOSS_WEIGHTS if loss_weights is None else loss_weights
        step = self.step if step is None else step

        def on(key):
            return key in weights and weights[key]["kick_in"] >= 0 and step >= weights[key]["kick_in"]

        obj = self.object_vertices()
        terms = {}
        if on("mask_loss") or on("centroid_loss"):
            H, W = self.target_mask.shape
            alpha = soft_silhouette(obj + self.hum_centroid_offset, self.obj_faces, self.camera[0], self.camera[1], (H, W),
                                    self.sigma, self.blur_radius)
            mask_loss, centroid = silhouette_terms(alpha, self.target_mask)
            if on("mask_loss"):
                terms["mask_loss"] = mask_loss
            if on("centroid_loss"):
                d = centroid - self.target_mask_centroid
                terms["centroid_loss"] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if on("contact_loss"):
            terms["contact_loss"] = contact_distance(obj, self.human_vertices, self.object_contact_probs, self.human_contact_probs)
        total = torch.zeros(self.rotation.shape[0], dtype=torch.float32, device=self.rotation.device)
        for key, val in terms.items():
            total = total + val * weights[key]["w"]
        self.step = step + 1
        return total, terms


def fit_object_pose(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask, focal, principal,
                    init=None, hum_centroid_offset=None, vars=("pose",), loss_weights=None, max_iter=250, early_stop=False,
                    sigma=1e-4, blur_radius=None, icp_threshold=(0.3, 0.5), icp_max_iterations=10):
    """The loop of optim/fit.py:217-290: Adam with lr 5e-2 for the rotation, 1e-2 for the translation and 1e-2 for the scale.

    init = (R6 [B,6], T [B,3], s number or [B]) gives the B starts; None takes one start from ``contact_icp`` between the object
    vertices of contact probability > icp_threshold[0] and the human vertices of probability > icp_threshold[1] (selecting them
    reads the device once, before the loop).  early_stop ends the loop when every start has |previous - current| < 1e-6: the only
    host read of the loop, made only when asked for.
    -> dict(rotation [B,6], translation [B,3], scale [B], object_vertices [B,N,3], history [iterations,B] (device tensor))."""
    if not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"max_iter: expected an integer >= 1, got {max_iter!r}")
    if init is None:
        o_sel = obj_vertices[obj_contact_probs.float() > icp_threshold[0]]
        h_sel = human_vertices[human_contact_probs.float() > icp_threshold[1]]
        if o_sel.shape[0] < 1 or h_sel.shape[0] < 1:
            raise ValueError("init=None needs contact vertices above icp_threshold on both meshes for contact_icp")
        icp = contact_icp(o_sel.float(), h_sel.float(), max_iterations=icp_max_iterations)
        init = (matrix_to_rot6d(icp.R), icp.T, 1.0)
    model = ObjectPoseFit(init[0], init[1], init[2], obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs,
                          target_mask, focal, principal, hum_centroid_offset, vars, sigma, blur_radius)
    groups = []
    if "pose" in vars:
        groups += [{"params": [model.rotation], "lr": 5e-2}, {"params": [model.translation], "lr": 1e-2}]
    if "scale" in vars:
        groups.append({"params": [model.scale], "lr": 1e-2})
    if not groups:
        raise ValueError("vars: nothing to optimise")
    optimizer = torch.optim.Adam(groups)
    history = []
    prev = None
    for i in range(max_iter):
        optimizer.zero_grad()
        total, _ = model(loss_weights, step=i)
        total.sum().backward()  # the starts are independent: the sum's gradient is each start's own
        optimizer.step()
        history.append(total.detach())
        if early_stop:
            if prev is not None and bool(((prev - history[-1]).abs() < 1e-6).all()):
                break
            prev = history[-1]
    with torch.no_grad():
        verts = model.object_vertices()
    return {"rotation": model.rotation.detach(), "translation": model.translation.detach(), "scale": model.scale.detach(),
            "object_vertices": verts, "history": torch.stack(history)}
