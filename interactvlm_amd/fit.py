"""The object-pose fit of the reference's joint fitting stage (optim/optimizer.py ``ObjPose_Opt``, optim/fit.py:217-290): the thin
loop that composes ``contact_icp`` (the start), ``soft_silhouette`` + ``silhouette_terms`` (mask and centroid terms) and
``contact_distance`` (the contact term), for B starts at once.

Not the reference's: no Phong render, no depth image of the reference's (``occlusion=True`` renders z-buffers of its own for the
occlusion-aware terms, see ``ObjectPoseFit``), no logging or video.  The rigid transform is applied pose by pose with the
operations of a single-pose run, so that every start of a batch computes the bits of its own unbatched run; with
``fused_transform=True`` it is ``pose.pose_transform`` (csrc/pose.hip), which keeps that property in three launches per step.
``search_object_pose`` (many starts, one loop, the winner picked on the device) is an addition: the reference fits one start.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, contact_pair, silhouette
from .contact_icp import contact_icp
from .contact_pair import contact_distance
from .mesh_sdf import MeshSDF, check_closed
from .occlusion import DEFAULT_TAU, check_tau, depth_order, occluder_maps
from .pose import check_rotations, check_start, compose_rotations, cube_rotations, pose_arguments, pose_transform
from .silhouette import silhouette_terms, soft_silhouette

# optim/cfg/fit.yaml
DEFAULT_LOSS_WEIGHTS = {
    "mask_loss": {"w": 5.0, "kick_in": 0},
    "centroid_loss": {"w": 1e-4, "kick_in": 0},
    "contact_loss": {"w": 10.0, "kick_in": 0},
}
# Every term of ``ObjectPoseFit``, in the order they are added up: key -> its bit of ivlm_fit_step's terms_on (a row of term_history),
# or None for a term that the device loop's launch sequence does not run.  The None terms are NOT the reference's and not in
# DEFAULT_LOSS_WEIGHTS: mesh_sdf's penetration of the object vertices into the human mesh (the model needs human_faces), the other
# direction, mesh_sdf's intrusion of the human vertices into the posed object (the model needs intrusion=True), and occlusion's depth
# order of the object against the human's z-buffer (the model needs occlusion=True).
TERMS = {"mask_loss": _lib.FIT_MASK, "centroid_loss": _lib.FIT_CENTROID, "contact_loss": _lib.FIT_CONTACT,
         "penetration_loss": None, "intrusion_loss": None, "depth_order_loss": None}
TERM_KEYS = tuple(k for k, bit in TERMS.items() if bit is not None)


def _host_term(key):
    """a key of ``TERMS`` whose value is None, looked up by name"""
    if TERMS[key] is not None:
        raise KeyError(f"{key}: a term of the device loop")
    return key


PENETRATION_KEY, INTRUSION_KEY, DEPTH_ORDER_KEY = (_host_term(k) for k in ("penetration_loss", "intrusion_loss", "depth_order_loss"))
DEFAULT_LRS = (5e-2, 1e-2, 1e-2)  # rotation, translation, scale (optim/fit.py)


def term_configured(key, weights):
    """weights holds the term and does not switch it off (kick_in = -1: never)"""
    return key in weights and weights[key]["kick_in"] >= 0


def term_counts(key, weights, i):
    """the term counts at iteration i: configured, and i >= kick_in (0: from the start, k: from iteration k on)"""
    return key in weights and 0 <= weights[key]["kick_in"] <= i


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


class FitScene:
    """The constants of a fit, prepared once and shared by every model and loop over them: the float, detached buffers, the binarised
    target and the centre of its bounding box, the camera, sigma and blur radius, the centroid offset, with human_faces the human's
    ``MeshSDF`` and with intrusion=True the object checked closed (``mesh_sdf.check_closed``, on a host copy) and prepared as a
    ``MeshSDF`` - every host read of a fit's preparation but the silhouette's topology cache, which is keyed by the tensor object
    ``obj_faces`` kept here and so hits after the first use.  With occlusion=True (it needs human_faces) the human moved by the centroid
    offset - the silhouette's frame - is rendered once (``occlusion.occluder_maps``) into occluder_depth, signed_weight and valid.  The
    arguments are ``ObjectPoseFit``'s (here occlusion, human_mask and depth_tau come after human_faces)."""

    def __init__(self, obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask, focal, principal,
                 hum_centroid_offset=None, sigma=1e-4, blur_radius=None, intrusion=False, human_faces=None, occlusion=False,
                 human_mask=None, depth_tau=DEFAULT_TAU):
        if not isinstance(target_mask, torch.Tensor) or target_mask.dim() != 2:
            raise ValueError("target_mask: expected [H,W]")
        if occlusion_flag(occlusion) and human_faces is None:
            raise ValueError("occlusion=True needs human_faces: the occluder's depth image is rendered from the human's triangles")
        self.depth_tau = check_tau(depth_tau)
        self.camera = (focal, principal)
        self.sigma, self.blur_radius = sigma, blur_radius
        self.obj_vertices = obj_vertices.detach().float()
        self.obj_faces = obj_faces.detach()
        self.human_vertices = human_vertices.detach().float()
        self.object_contact_probs = obj_contact_probs.detach()
        self.human_contact_probs = human_contact_probs.detach()
        off = torch.zeros(3) if hum_centroid_offset is None else hum_centroid_offset.detach().float()
        self.hum_centroid_offset = off.to(obj_vertices.device)
        self.target_mask = (target_mask != 0).float()
        self.target_mask_centroid = mask_bbox_centre(self.target_mask)
        # the penetration term's prepared mesh (one device read, here); the plan belongs to this device
        self.human_sdf = None if human_faces is None else MeshSDF(self.human_vertices, human_faces.detach())
        # the intrusion term's prepared mesh: the object in its canonical frame, checked closed and outward on a host copy first
        self.object_sdf = None
        if intrusion:
            check_closed(self.obj_vertices, self.obj_faces)
            self.object_sdf = MeshSDF(self.obj_vertices, self.obj_faces.to(torch.int32))
        # the occlusion-aware terms' constants: the human in the silhouette's frame (the reference's off_h_verts), rendered once
        self.occluder_depth = self.signed_weight = self.valid = None
        if occlusion:
            self.occluder_depth, self.signed_weight, self.valid = occluder_maps(
                self.human_vertices + self.hum_centroid_offset, human_faces.detach(), self.target_mask, focal, principal, human_mask)

    BUFFERS = ("obj_vertices", "obj_faces", "human_vertices", "object_contact_probs", "human_contact_probs", "hum_centroid_offset",
               "target_mask", "target_mask_centroid")
    OCCLUSION_BUFFERS = ("occluder_depth", "signed_weight", "valid")  # tensors with occlusion=True, else None
    _DEFAULTS = (None,) * 8 + (1e-4, None, False, None, False, None, DEFAULT_TAU)  # of the arguments after obj_vertices

    @classmethod
    def of(cls, first, *rest):
        """``first`` when it is a scene given in place of obj_vertices (nothing else of a scene may come with it), else the scene of
        the arguments"""
        if not isinstance(first, cls):
            return cls(first, *rest)
        if not all(v is d or (not isinstance(v, torch.Tensor) and v == d) for v, d in zip(rest, cls._DEFAULTS)):
            raise ValueError("obj_vertices is a FitScene: no other argument of the scene may be given with it")
        return first

    def validate(self, rotation, translation, scale):
        """What ``DevicePoseFit`` checks before the library loads, by the modules whose kernels run: shapes, dtypes and devices of the
        scene with the pose parameters rotation [B,6], translation [B,3], scale [B] -> the camera tuple of ``silhouette.validate``"""
        H, W = self.target_mask.shape
        pose_arguments(self.obj_vertices, rotation, translation, scale)
        cam = silhouette.validate(self.obj_vertices, self.obj_faces, *self.camera, (H, W), self.sigma, self.blur_radius)
        contact_pair.validate(self.obj_vertices, self.human_vertices, self.object_contact_probs, self.human_contact_probs)
        silhouette.validate_terms(self.target_mask.new_empty(H, W), self.target_mask)
        if self.hum_centroid_offset.shape != (3,):
            raise ValueError(f"hum_centroid_offset: expected [3], got {tuple(self.hum_centroid_offset.shape)}")
        return cam


class ObjectPoseFit(nn.Module):
    """The terms of ``ObjPose_Opt.forward`` for B starts at once, with its quirks: the silhouette is rendered on the object moved by
    ``hum_centroid_offset`` while the contact term is taken on the un-offset vertices; the target centroid is the centre of the
    target mask's bounding box; a term counts when ``kick_in >= 0 and step >= kick_in``.

    rotation_init [B,6] (or [6]), translation_init [B,3], scaling_init a number or [B]; obj_vertices [N,3] (or a ``FitScene``
    in its place, and then none of the scene's other arguments), obj_faces [F,3],
    human_vertices [N_h,3], obj_contact_probs [N], human_contact_probs [N_h], target_mask [H,W]; focal / principal as
    ``soft_silhouette`` takes them.  ``vars`` selects what is optimised: "pose", "scale" or both.  fused_transform=True moves the
    object with ``pose.pose_transform`` (one launch for the batch, two for its backward) instead of the pose-by-pose torch
    operations of ``apply_transformation``: the same transform within the documented errors of that kernel, not the same bits.
    human_faces [F_h,3] int32 (closed, outward) prepares one ``MeshSDF`` of the human and allows one more term, NOT the reference's:
    "penetration_loss" = ``MeshSDF.penetration`` of the un-offset object vertices (the frame of the contact term), gated and weighted
    like the others when loss_weights holds the key (``DEFAULT_LOSS_WEIGHTS`` does not); on without human_faces it raises.
    intrusion=True checks that the object is closed and outward (``mesh_sdf.check_closed``, on a host copy) and prepares one
    ``MeshSDF`` of it (its one device read; both here, before any loop) for the term "intrusion_loss" = ``MeshSDF.intrusion`` of the
    un-offset human vertices under the B poses: the penetration term's other direction, for a coarse object none of whose vertices
    lies inside the body while a limb passes through one of its faces.  Gated and weighted like the others, not in
    ``DEFAULT_LOSS_WEIGHTS`` either; on without intrusion=True it raises.
    occlusion=True (it needs human_faces; NOT the reference's) makes the image terms occlusion-aware: target_mask is then the object's
    VISIBLE pixels, the human moved by ``hum_centroid_offset`` is rendered once (``occlusion.occluder_maps``; human_mask [H,W] is the
    photo's person mask, when there is one), ``mask_loss`` and ``centroid_loss`` are taken on alpha * valid - an object pixel hidden by
    the body is neither wanted nor penalised - and one more term is allowed: "depth_order_loss" = ``occlusion.depth_order`` of the
    offset object against the human's z-buffer with tau = depth_tau (scene units; 0.01 is a default nobody has measured on data),
    gated and weighted like the others, not in ``DEFAULT_LOSS_WEIGHTS``; on without occlusion=True it raises.  (occlusion, human_mask
    and depth_tau stand before human_faces, which stays the last parameter.)
    forward(loss_weights, step=None) -> (total [B], {term: [B]})."""

    def __init__(self, rotation_init, translation_init, scaling_init, obj_vertices, obj_faces=None, human_vertices=None,
                 obj_contact_probs=None, human_contact_probs=None, target_mask=None, focal=None, principal=None, hum_centroid_offset=None,
                 vars=("pose",), sigma=1e-4, blur_radius=None, fused_transform=False, intrusion=False, occlusion=False, human_mask=None,
                 depth_tau=DEFAULT_TAU, human_faces=None):
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
        self.fused_transform = bool(fused_transform)
        self.scene = scene = FitScene.of(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask,
                                         focal, principal, hum_centroid_offset, sigma, blur_radius, intrusion, human_faces, occlusion,
                                         human_mask, depth_tau)
        self.camera, self.sigma, self.blur_radius = scene.camera, scene.sigma, scene.blur_radius
        for name in FitScene.BUFFERS + FitScene.OCCLUSION_BUFFERS:  # the scene's own tensor objects (None without occlusion=True:
            self.register_buffer(name, getattr(scene, name))         # a None buffer is in no state_dict), so .to() moves them too
        self.depth_tau = scene.depth_tau
        self.human_sdf, self.object_sdf = scene.human_sdf, scene.object_sdf  # plain attributes: a plan belongs to its device

    def object_vertices(self):
        if self.fused_transform:
            return pose_transform(self.obj_vertices, self.rotation, self.translation, self.scale)
        return apply_transformation(self.obj_vertices, self.rotation, self.translation, self.scale)

    def forward(self, loss_weights=None, step=None):
        weights = DEFAULT_LOSS_WEIGHTS if loss_weights is None else loss_weights
        step = self.step if step is None else step

        def on(key):
            return term_counts(key, weights, step)

        obj = self.object_vertices()
        terms = {}
        if on(DEPTH_ORDER_KEY) and self.valid is None:
            raise ValueError(f"{DEPTH_ORDER_KEY} is on, but the model was built without occlusion=True: the term needs the human's "
                             "depth image")
        if on("mask_loss") or on("centroid_loss"):
            H, W = self.target_mask.shape
            alpha = soft_silhouette(obj + self.hum_centroid_offset, self.obj_faces, self.camera[0], self.camera[1], (H, W),
                                    self.sigma, self.blur_radius)
            if self.valid is not None:  # occlusion=True: a pixel where the body hides the object is a don't-care
                alpha = alpha * self.valid
            mask_loss, centroid = silhouette_terms(alpha, self.target_mask)
            if on("mask_loss"):
                terms["mask_loss"] = mask_loss
            if on("centroid_loss"):
                d = centroid - self.target_mask_centroid
                terms["centroid_loss"] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if on("contact_loss"):
            terms["contact_loss"] = contact_distance(obj, self.human_vertices, self.object_contact_probs, self.human_contact_probs)
        if on(PENETRATION_KEY):
            if self.human_sdf is None:
                raise ValueError(f"{PENETRATION_KEY} is on, but the model was built without human_faces: the signed distance needs the "
                                 "human's triangles")
            terms[PENETRATION_KEY] = self.human_sdf.penetration(obj)
        if on(INTRUSION_KEY):
            if self.object_sdf is None:
                raise ValueError(f"{INTRUSION_KEY} is on, but the model was built without intrusion=True: the term needs the object "
                                 "checked closed and prepared as a MeshSDF")
            terms[INTRUSION_KEY] = self.object_sdf.intrusion(self.human_vertices, self.rotation, self.translation, self.scale)
        if on(DEPTH_ORDER_KEY):
            terms[DEPTH_ORDER_KEY] = depth_order(obj + self.hum_centroid_offset, self.obj_faces, self.occluder_depth,
                                                 self.signed_weight, self.camera[0], self.camera[1], self.depth_tau)
        total = torch.zeros(self.rotation.shape[0], dtype=torch.float32, device=self.rotation.device)
        for key, val in terms.items():
            total = total + val * weights[key]["w"]
        self.step = step + 1
        return total, terms


def refuse_terms_the_device_loop_lacks(loss_weights):
    for key, bit in TERMS.items():
        if bit is None and loss_weights is not None and term_configured(key, loss_weights):
            raise ValueError(f"{key}: not available with device_loop=True (the device loop's launch sequence does not run the "
                             "term; configure kick_in = -1 or use the torch loop)")


def occlusion_flag(occlusion):
    """-> bool; anything but a bool is refused by name.  occlusion, human_mask and depth_tau stand before human_faces in the public
    signatures, so a tensor here is a human_faces that was passed by position."""
    if not isinstance(occlusion, bool):
        raise ValueError(f"occlusion: expected True or False, got {type(occlusion).__name__} (human_faces is the last parameter: pass "
                         "it by keyword)")
    return occlusion


def refuse_occlusion_in_the_device_loop(occlusion):
    if occlusion_flag(occlusion):
        raise ValueError("occlusion=True: not available with device_loop=True (the device loop's launch sequence takes the image terms "
                         "on alpha itself and has no depth image; use the torch loop)")


def fit_phases(loss_weights, max_iter):
    """-> [(first iteration, end, bits)]: the runs of iterations over which the same terms count (``term_counts``).  ``bits`` holds
    the ``TERMS`` bit of each of them.  ``kick_in`` is a host number, so the phases are known before the loop: at most four of them."""
    weights = DEFAULT_LOSS_WEIGHTS if loss_weights is None else loss_weights
    kicks = {weights[k]["kick_in"] for k in TERM_KEYS if term_configured(k, weights)}
    edges = sorted({0, max_iter} | {k for k in kicks if 0 < k < max_iter})
    return [(lo, hi, sum(TERMS[k] for k in TERM_KEYS if term_counts(k, weights, lo))) for lo, hi in zip(edges[:-1], edges[1:])]


def adam_reference(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """One step of torch's Adam (amsgrad off, no weight decay) in fp64, as csrc/fit_step.hip evaluates it per element: t is the
    1-based step.  -> (p, m, v) in fp64; the kernel stores each rounded to fp32 once."""
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    beta1, beta2 = betas
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


def _f32(x):
    """a Python number rounded to fp32 the way torch rounds a scalar operand of an fp32 tensor"""
    return float(torch.tensor(float(x), dtype=torch.float32))


class DevicePoseFit:
    """The loop of ``fit_object_pose`` on the device: one ``ivlm_fit_step`` (csrc/fit_step.hip) per iteration - the fused transform,
    the silhouette and contact kernels, the loss arithmetic, every backward and Adam as one launch sequence without a host read or
    an allocation; each phase (``fit_phases``) has its own launch sequence.  The launches are eager: replaying the sequence as
    a HIP graph is NOT built (DESIGN 4.42 says what was tried and why it was taken out).  Iteration i computes the total, the
    terms and the gradients of ``ObjectPoseFit(fused_transform=True)`` at step i bit for bit; the update is torch's Adam evaluated
    in fp64 per element (``adam_reference``), so later iterations follow the torch loop within Adam's rounding, not bit for bit.

    The constructor takes ``ObjectPoseFit``'s arguments (a ``FitScene`` too; the transform is always fused) and loss_weights, max_iter,
    lrs = (rotation, translation, scale), betas, eps > 0.  It owns rotation [B,6], translation [B,3], scale [B], the moments, the device step
    counter, history [max_iter,B] (the total BEFORE update i), term_history [max_iter,3,B] (``TERM_KEYS``; an exact 0 for a term
    that does not count), the workspace and the topology lists (from the silhouette module's cache: the one host read, here).
    occlusion=True, or a scene prepared with it, is refused by name: the launch sequence has no don't-care image and no depth image.
    step() runs one iteration, run(n=None) the remaining ones (or n).  rotation_grad / translation_grad / scale_grad are the last
    step's gradients."""

    def __init__(self, rotation_init, translation_init, scaling_init, obj_vertices, obj_faces=None, human_vertices=None,
                 obj_contact_probs=None, human_contact_probs=None, target_mask=None, focal=None, principal=None, hum_centroid_offset=None,
                 vars=("pose",), sigma=1e-4, blur_radius=None, loss_weights=None, max_iter=250, lrs=DEFAULT_LRS, betas=(0.9, 0.999),
                 eps=1e-8, occlusion=False):
        if not isinstance(max_iter, int) or isinstance(max_iter, bool) or max_iter < 1:
            raise ValueError(f"max_iter: expected an integer >= 1, got {max_iter!r}")
        if not set(vars):
            raise ValueError("vars: nothing to optimise")
        try:
            lrs = tuple(float(x) for x in lrs)
            betas = tuple(float(x) for x in betas)
            eps = float(eps)
        except (TypeError, ValueError):
            raise ValueError(f"lrs / betas / eps: expected numbers, got {lrs!r}, {betas!r}, {eps!r}") from None
        if len(lrs) != 3 or len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas) or not eps > 0.0:
            raise ValueError(f"expected three learning rates, two betas in [0, 1) and eps > 0, got {lrs}, {betas}, {eps}")
        refuse_terms_the_device_loop_lacks(loss_weights)
        refuse_occlusion_in_the_device_loop(occlusion or (isinstance(obj_vertices, FitScene) and obj_vertices.valid is not None))
        weights = DEFAULT_LOSS_WEIGHTS if loss_weights is None else loss_weights
        self.phases = fit_phases(weights, max_iter)
        for lo, _, bits in self.phases:
            if bits == 0:
                raise ValueError(f"loss_weights: no term counts at iteration {lo}: nothing to descend")
        self.scene = scene = FitScene.of(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask,
                                         focal, principal, hum_centroid_offset, sigma, blur_radius)
        self.model = model = ObjectPoseFit(rotation_init, translation_init, scaling_init, scene, vars=vars, fused_transform=True)
        self.rotation, self.translation, self.scale = model.rotation.data, model.translation.data, model.scale.data
        cam = scene.validate(self.rotation, self.translation, self.scale)  # before the library loads
        self.max_iter, self.iteration = max_iter, 0
        dev = self.rotation.device
        (H, W), B = scene.target_mask.shape, self.rotation.shape[0]
        N, F, N_h = scene.obj_vertices.shape[0], scene.obj_faces.shape[0], scene.human_vertices.shape[0]
        self.sizes = (B, N, F, H, W, N_h)
        lib = _lib.load()
        p, q, p_dtype = contact_pair.one_dtype(scene.object_contact_probs, scene.human_contact_probs)
        optimise = (_lib.FIT_POSE if "pose" in vars else 0) | (_lib.FIT_SCALE if "scale" in vars else 0)
        with torch.cuda.device(dev):
            self.workspace, nbytes = _lib.workspace(lib.ivlm_fit_step_workspace_bytes, "DevicePoseFit", dev,
                                                    B=B, N=N, F=F, H=H, W=W, N_h=N_h)
            f32, offsets, slots = silhouette.topology_of(scene.obj_faces, N)
            zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
            self._moments = [zeros(B, 6), zeros(B, 3), zeros(B), zeros(B, 6), zeros(B, 3), zeros(B)]
            self._grads = [zeros(B, 6), zeros(B, 3), zeros(B)]
            self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
            self.history, self.term_history = zeros(max_iter, B), zeros(max_iter, 3, B)
        self._keep = (f32, offsets, slots, p, q, scene.obj_vertices.contiguous(), scene.human_vertices.contiguous(),
                      scene.target_mask.contiguous(), scene.target_mask_centroid.contiguous(), scene.hum_centroid_offset.contiguous())
        f32, offsets, slots, p, q, verts, hum, target, target_c, off = self._keep
        a = _lib.FitStepArgs()
        for name, t in (("obj_verts", verts), ("faces", f32), ("vert_face_offsets", offsets), ("vert_face_list", slots),
                        ("human_verts", hum), ("obj_probs", p), ("human_probs", q), ("target", target), ("target_centroid", target_c),
                        ("centroid_offset", off), ("rotation", self.rotation), ("translation", self.translation), ("scale", self.scale),
                        ("step", self.counter), ("history", self.history), ("term_history", self.term_history),
                        ("workspace", self.workspace)):
            setattr(a, name, t.data_ptr())
        for name, t in zip(("m_rotation", "m_translation", "m_scale", "v_rotation", "v_translation", "v_scale"), self._moments):
            setattr(a, name, t.data_ptr())
        for name, t in zip(("grad_rotation", "grad_translation", "grad_scale"), self._grads):
            setattr(a, name, t.data_ptr())
        a.workspace_bytes = nbytes
        a.lr_rotation, a.lr_translation, a.lr_scale = lrs
        a.beta1, a.beta2, a.eps = betas[0], betas[1], eps
        a.B, a.N, a.F, a.H, a.W, a.N_h = self.sizes
        a.p_dtype = p_dtype
        a.max_iter, a.optimise = max_iter, optimise
        a.fx, a.fy, a.px, a.py, _, _, a.sigma, a.blur_radius = cam
        a.w_mask, a.w_centroid, a.w_contact = (_f32(weights[k]["w"]) if k in weights else 0.0 for k in TERM_KEYS)
        self._args, self._lib = a, lib
        self._vars = tuple(vars)

    def _grad(self, k, name):
        if name not in self._vars:
            return None
        return self._grads[k].detach()

    rotation_grad = property(lambda self: self._grad(0, "pose"))
    translation_grad = property(lambda self: self._grad(1, "pose"))
    scale_grad = property(lambda self: self._grad(2, "scale"))

    def _state(self):
        return [self.rotation, self.translation, self.scale, *self._moments, *self._grads, self.counter, self.history, self.term_history]

    def _launch(self, bits):
        self._args.terms_on = bits
        with torch.cuda.device(self.rotation.device):
            _lib.check(self._lib.ivlm_fit_step(ctypes.byref(self._args), _lib.stream()), "fit_step")

    def step(self):
        """one iteration: the total of the current parameters into history[i], then the update"""
        i = self.iteration
        if i >= self.max_iter:
            raise RuntimeError(f"DevicePoseFit: all {self.max_iter} iterations have run")
        bits = next(b for lo, hi, b in self.phases if lo <= i < hi)
        self._launch(bits)
        self.iteration = i + 1

    def run(self, n=None):
        """the remaining iterations, or n of them"""
        left = self.max_iter - self.iteration
        if n is not None and (not isinstance(n, int) or n < 0 or n > left):
            raise ValueError(f"n: expected an integer in [0, {left}], got {n!r}")
        for _ in range(left if n is None else n):
            self.step()
        return self

    def result(self):
        """-> the dict of ``fit_object_pose`` plus term_history, at the current parameters"""
        with torch.no_grad():
            verts = self.model.object_vertices()
        done = self.iteration
        return {"rotation": self.rotation, "translation": self.translation, "scale": self.scale, "object_vertices": verts,
                "history": self.history[:done], "term_history": self.term_history[:done]}


_UNSET = object()  # fused_transform was not passed: False for the torch loop, implied by device_loop


def fit_object_pose(obj_vertices, obj_faces=None, human_vertices=None, obj_contact_probs=None, human_contact_probs=None, target_mask=None,
                    focal=None, principal=None, init=None, hum_centroid_offset=None, vars=("pose",), loss_weights=None, max_iter=250,
                    early_stop=False, sigma=1e-4, blur_radius=None, icp_threshold=(0.3, 0.5), icp_max_iterations=10, fused_transform=_UNSET,
                    device_loop=False, intrusion=False, occlusion=False, human_mask=None, depth_tau=DEFAULT_TAU, human_faces=None):
    """The loop of optim/fit.py:217-290: Adam with lr 5e-2 for the rotation, 1e-2 for the translation and 1e-2 for the scale.

    The scene is ``ObjectPoseFit``'s (obj_vertices may be a ``FitScene``); it is prepared once, before the loop.
    init = (R6 [B,6], T [B,3], s number or [B]) gives the B starts; None takes one start from ``contact_icp`` between the object
    vertices of contact probability > icp_threshold[0] and the human vertices of probability > icp_threshold[1] (selecting them
    reads the device once, before the loop).  early_stop ends the loop when every start has |previous - current| < 1e-6: the only
    host read of the loop, made only when asked for.  fused_transform: see ``ObjectPoseFit``.  device_loop=True runs the loop as
    ``DevicePoseFit`` does (one launch sequence per iteration, Adam as a kernel): it implies the fused
    transform, refuses early_stop (a host read per iteration) and adds term_history [iterations,3,B] to the result.
    human_faces [F_h,3] int32 (the human's triangles, closed and outward) is what the term "penetration_loss" of loss_weights needs
    (``ObjectPoseFit``, ``mesh_sdf``: NOT the reference's); device_loop=True refuses that term when it is configured (kick_in >= 0).
    intrusion=True is what the term "intrusion_loss" needs (``ObjectPoseFit``: the object is checked closed and prepared once, before
    the loop); device_loop=True refuses that term in the same way.
    occlusion=True, human_mask and depth_tau are ``ObjectPoseFit``'s (the human is rendered once, before the loop; the term
    "depth_order_loss" needs it); device_loop=True refuses occlusion=True and that term by name.
    -> dict(rotation [B,6], translation [B,3], scale [B], object_vertices [B,N,3], history [iterations,B] (device tensor))."""
    if not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"max_iter: expected an integer >= 1, got {max_iter!r}")
    if device_loop:
        if early_stop:
            raise ValueError("early_stop: not available with device_loop=True (it reads the device every iteration)")
        if fused_transform is not _UNSET and not fused_transform:
            raise ValueError("fused_transform=False: not available with device_loop=True (the device loop runs the fused transform)")
        refuse_terms_the_device_loop_lacks(loss_weights)
        refuse_occlusion_in_the_device_loop(occlusion)
    fused_transform = bool(device_loop) if fused_transform is _UNSET else fused_transform
    # (the device loop runs neither extra term, so a scene made here for it prepares neither mesh)
    scene = FitScene.of(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask, focal, principal,
                        hum_centroid_offset, sigma, blur_radius, intrusion and not device_loop, None if device_loop else human_faces,
                        occlusion, human_mask, depth_tau)
    if init is None:
        o_sel = scene.obj_vertices[scene.object_contact_probs.float() > icp_threshold[0]]
        h_sel = scene.human_vertices[scene.human_contact_probs.float() > icp_threshold[1]]
        if o_sel.shape[0] < 1 or h_sel.shape[0] < 1:
            raise ValueError("init=None needs contact vertices above icp_threshold on both meshes for contact_icp")
        icp = contact_icp(o_sel, h_sel, max_iterations=icp_max_iterations)
        init = (matrix_to_rot6d(icp.R), icp.T, 1.0)
    if device_loop:
        return DevicePoseFit(*init, scene, vars=vars, loss_weights=loss_weights, max_iter=max_iter).run().result()
    model = ObjectPoseFit(*init, scene, vars=vars, fused_transform=fused_transform)
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


def select_best(scores):
    """scores [K] -> the index of the smallest finite score, a 0-dim int64 tensor on the scores' device.  A non-finite score (NaN,
    +-inf) ranks last, ties go to the lowest index, and scores that are all non-finite give 0.  No host read: the minimum, then the
    smallest index among the elements equal to it.  Works on CPU tensors too."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 1 or scores.shape[0] < 1 or not scores.is_floating_point():
        raise ValueError(f"scores: expected a floating-point [K] with K >= 1, got "
                         f"{tuple(scores.shape) if isinstance(scores, torch.Tensor) else type(scores).__name__}")
    K = scores.shape[0]
    key = torch.where(torch.isfinite(scores), scores, torch.full_like(scores, float("inf")))
    idx = torch.arange(K, dtype=torch.int64, device=scores.device)
    return torch.where(key == key.min(), idx, torch.full_like(idx, K)).min()


_SEARCH_FIT_KWARGS = ("hum_centroid_offset", "vars", "loss_weights", "max_iter", "sigma", "blur_radius", "icp_threshold",
                      "icp_max_iterations")


def search_object_pose(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask, focal, principal,
                       rotations=None, init=None, icp=True, chunk=None, obj_normals=None, human_normals=None, device_loop=False,
                       intrusion=False, occlusion=False, human_mask=None, depth_tau=DEFAULT_TAU, human_faces=None, **fit_kwargs):
    """A multi-start ``fit_object_pose``: K starts around one pose, fitted in one loop with the fused transform, scored and ranked on
    the device.  NOT the reference's, which runs one start (optim/fit.py): contact patches and a silhouette leave rotational
    ambiguities that a local fit from one start does not resolve.

    rotations [K,3,3] (None: the 24 ``pose.cube_rotations()``); init = (R0 [3,3], T0 [3], s0) (None: identity, zero, 1): start k is
    ``pose.pose_starts``' R_k = rotations[k] @ R0 at T0, s0.  icp=True first runs ONE ``contact_icp`` call with init = (R_k, T0, s0)
    for all K starts, between the object vertices of contact probability > icp_threshold[0] and the human vertices of probability >
    icp_threshold[1] (the selection of ``fit_object_pose(init=None)``: it reads the device once, before anything else), with
    obj_normals [N,3] / human_normals [N_h,3] of the whole meshes forwarded when given, and takes R, T of every start from its result.
    Then ``fit_object_pose(init=starts, fused_transform=True, **fit_kwargs)``; fit_kwargs are that function's hum_centroid_offset,
    vars, loss_weights, max_iter, sigma, blur_radius, icp_threshold, icp_max_iterations (early_stop is refused: it ends a loop
    when all of ITS starts have settled).  The score of a start is one more forward at its returned parameters, without gradients,
    with every configured term (kick_in >= 0) on; history[-1] is the total BEFORE the last update and is not the score.

    device_loop=True runs every loop on the device (``fit_object_pose(device_loop=True)``, ``DevicePoseFit``) and adds term_history
    [iterations,3,K]; the scoring stays the forward described above.  One ``FitScene`` is prepared with human_faces and intrusion and
    serves every loop and every scoring model, so that the score holds "penetration_loss" and "intrusion_loss" whenever loss_weights
    configures them (device_loop=True refuses that, see ``fit_object_pose``).  occlusion=True, human_mask and depth_tau go to that scene
    too: every loop and every score then takes the image terms on alpha * valid, and the score holds "depth_order_loss" when it is
    configured - a start whose object sits on the wrong side of the body ranks behind its twin on the right side (device_loop=True
    refuses occlusion=True by name).

    chunk=None fits all K starts in one loop; an integer fits them in loops of at most that many starts, to bound memory.  A start
    computes the bits of its own run whatever the batch around it, so chunk does not change a single bit of the result.

    -> the dict of ``fit_object_pose`` for all K starts (rotation [K,6], translation [K,3], scale [K], object_vertices [K,N,3],
    history [iterations,K]) plus scores [K], best_index (0-dim int64 device tensor, ``select_best``) and best = {rotation [6],
    translation [3], scale [], object_vertices [N,3]} gathered with index_select.  The only host reads are made once per search,
    before the first loop: the contact selection for icp, the ``FitScene`` (the closedness check and the two ``MeshSDF`` when asked
    for) and the silhouette's topology cache at the first step."""
    if chunk is not None and (not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1):
        raise ValueError(f"chunk: expected None or an integer >= 1, got {chunk!r}")
    if device_loop:
        refuse_terms_the_device_loop_lacks(fit_kwargs.get("loss_weights"))
        refuse_occlusion_in_the_device_loop(occlusion)
    if "early_stop" in fit_kwargs:
        raise ValueError("early_stop: not available in search_object_pose (it would make a start's result depend on chunk)")
    unknown = sorted(set(fit_kwargs) - set(_SEARCH_FIT_KWARGS))
    if unknown:
        raise ValueError(f"unexpected arguments {unknown}: expected a subset of {list(_SEARCH_FIT_KWARGS)} (the transform is always fused)")
    if not isinstance(obj_vertices, torch.Tensor) or obj_vertices.dim() != 2 or obj_vertices.shape[1] != 3:
        raise ValueError(f"obj_vertices: expected [N,3], got "
                         f"{tuple(obj_vertices.shape) if isinstance(obj_vertices, torch.Tensor) else type(obj_vertices).__name__}")
    if (obj_normals is None) != (human_normals is None):
        raise ValueError("normals must be given for both sides or for neither")
    dev = obj_vertices.device
    if rotations is None:
        rotations = cube_rotations()
    check_rotations(rotations)
    if init is None:
        init = (None, None, 1.0)
    if not isinstance(init, (tuple, list)) or len(init) != 3:
        raise ValueError("init: expected (R0 [3,3], T0 [3], s0)")
    R0, T0, s0 = init
    R0, T0, s0 = check_start(R0, T0, s0, dev)
    K = rotations.shape[0]
    R = compose_rotations(rotations.detach().to(dev), R0)
    T, s = T0.expand(K, 3).contiguous(), s0.expand(K).contiguous()
    if icp:
        threshold = fit_kwargs.get("icp_threshold", (0.3, 0.5))
        o_on, h_on = obj_contact_probs.float() > threshold[0], human_contact_probs.float() > threshold[1]
        o_sel, h_sel = obj_vertices[o_on], human_vertices[h_on]
        if o_sel.shape[0] < 1 or h_sel.shape[0] < 1:
            raise ValueError("icp=True needs contact vertices above icp_threshold on both meshes for contact_icp")
        normals = (obj_normals[o_on].float(), human_normals[h_on].float()) if obj_normals is not None else (None, None)
        found = contact_icp(o_sel.float(), h_sel.float(), normals[0], normals[1], init=(R, T, s),
                            max_iterations=fit_kwargs.get("icp_max_iterations", 10))
        R, T = found.R, found.T
    R6 = matrix_to_rot6d(R)
    weights = fit_kwargs.get("loss_weights")
    configured = DEFAULT_LOSS_WEIGHTS if weights is None else weights
    every_term = max([0] + [configured[k]["kick_in"] for k in configured if term_configured(k, configured)])  # every key that is held
    scene = FitScene(obj_vertices, obj_faces, human_vertices, obj_contact_probs, human_contact_probs, target_mask, focal, principal,
                     fit_kwargs.pop("hum_centroid_offset", None), fit_kwargs.pop("sigma", 1e-4), fit_kwargs.pop("blur_radius", None),
                     intrusion, human_faces, occlusion, human_mask, depth_tau)
    step = K if chunk is None else chunk
    parts, scores = [], []
    for lo in range(0, K, step):
        sel = slice(lo, min(lo + step, K))
        out = fit_object_pose(scene, init=(R6[sel], T[sel], s[sel]), fused_transform=True, device_loop=device_loop, **fit_kwargs)
        final = ObjectPoseFit(out["rotation"], out["translation"], out["scale"], scene, vars=fit_kwargs.get("vars", ("pose",)),
                              fused_transform=True)
        with torch.no_grad():
            scores.append(final(weights, step=every_term)[0])
        parts.append(out)
    result = {k: torch.cat([p[k] for p in parts], dim={"history": 1, "term_history": 2}.get(k, 0)) for k in parts[0]}
    result["scores"] = torch.cat(scores)
    best = select_best(result["scores"])
    result["best_index"] = best
    result["best"] = {k: result[k].index_select(0, best.reshape(1))[0] for k in ("rotation", "translation", "scale", "object_vertices")}
    return result
