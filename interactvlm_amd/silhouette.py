"""Differentiable soft silhouette of a posed mesh and the two image losses built on it: what the reference's joint fitting stage
(optim/optimizer.py ``ObjPose_Opt.forward``) gets from pytorch3d's ``SoftSilhouetteShader`` for its ``mask_loss`` and
``centroid_loss``, as HIP kernels (csrc/silhouette.hip) with an analytic backward and no [H W, F] array.

    u = fx X / Z + px,  v = fy Y / Z + py;  pixel (row i, col j) has its centre at (j + 0.5, i + 0.5);  kappa = (2 / min(H, W))^2
    d_k = smallest squared distance (pixels^2) from the pixel centre to the three edge segments of face k
    the face counts if the pixel is strictly inside it or kappa d_k < blur_radius;  s_k = -/+ kappa d_k (inside / outside)
    p_k = sigmoid(-s_k / sigma),  alpha = 1 - prod_k (1 - p_k) over every counted face

Deliberately not the reference's: no cap at the 100 faces nearest in depth (so alpha does not depend on depth order), a face with
zero screen area or a vertex at Z <= 1e-6 is skipped whole, no Phong render and no depth image.  There is no CPU fallback.
"""
from __future__ import annotations

import math
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._args import check_devices, check_points, side
from ._lib import check, header_constant

# Error model of the kernels, in units of 2^-24 (IVLM_SILHOUETTE_* of include/ivlm_hip.h); tests derive their bounds from these.
# With M = the largest of H, W, |u|, |v|, |u - px|, |v - py| over a face's vertices:
POS_ULPS = header_constant("IVLM_SILHOUETTE_POS_ULPS")        # |delta sqrt(d_k)| <= POS_ULPS 2^-24 M
REL_ULPS = header_constant("IVLM_SILHOUETTE_REL_ULPS")        # plus a relative REL_ULPS 2^-24 on d_k
EXP_ULPS = header_constant("IVLM_SILHOUETTE_EXP_ULPS")        # plus an absolute EXP_ULPS 2^-24 on the exponent argument s_k / sigma
T_ULPS = header_constant("IVLM_SILHOUETTE_T_ULPS")            # |delta t| <= T_ULPS 2^-24 |p - a| / |b - a| (gradients only)
L_CHAIN = header_constant("IVLM_SILHOUETTE_CHAIN")            # fp32 additions per lane of the backward before fp64 takes over
TERMS_CHAIN = header_constant("IVLM_SILHOUETTE_TERMS_CHAIN")  # silhouette_terms converts every element to fp64 before it is added
TERMS_WORKSPACE_ROW_BYTES = 40  # IVLM_SILHOUETTE_TERMS_WORKSPACE(B, H) = B H x this: five fp64 sums per image row

# id(faces tensor) -> (weak reference to that tensor, its version, N, (faces int32, vertex -> face-slot offsets, slots)).  An entry
# belongs to ONE tensor object: a hit needs that very object, unmodified, and the entry goes when the tensor does (or as the oldest
# of more than _TOPOLOGY_MAX), so a different mesh that the allocator places at a freed tensor's address can never match.
_topology = {}
_TOPOLOGY_MAX = 8


def default_blur_radius(sigma):
    """the reference's ``np.log(1.0 / 1e-4 - 1.0) * sigma``: a face at the cut-off contributes p = 1e-4"""
    return float(sigma) * math.log(1.0 / 1e-4 - 1.0)


def validate(verts, faces, focal, principal, image_size, sigma, blur_radius):
    """-> (fx, fy, px, py, H, W, sigma, blur_radius): raises before anything touches the library"""
    check_points(verts, "verts")
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"faces: expected a tensor, got {type(faces).__name__}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"faces: expected [F,3] with F >= 1 (one topology shared by the batch), got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces: expected int32 or int64 vertex indices, got {faces.dtype}")

    def pair(x, name, kind):
        try:
            a, b = (kind(v) for v in (x if isinstance(x, (tuple, list)) else (x, x)))
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected one number or a pair, got {x!r}") from None
        return a, b

    fx, fy = pair(focal, "focal", float)
    px, py = pair(principal, "principal", float)
    H, W = pair(image_size, "image_size", int)
    if H < 1 or W < 1:
        raise ValueError(f"image_size: expected (H, W) >= 1, got {(H, W)}")
    if not all(math.isfinite(v) for v in (fx, fy, px, py)):
        raise ValueError(f"focal / principal: expected finite numbers, got {(fx, fy)}, {(px, py)}")
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"sigma: expected a finite number > 0, got {sigma}")
    blur_radius = default_blur_radius(sigma) if blur_radius is None else float(blur_radius)
    if not (blur_radius >= 0 and math.isfinite(blur_radius)):
        raise ValueError(f"blur_radius: expected a finite number >= 0, got {blur_radius}")
    check_devices([(verts, "verts", 2), (faces, "faces", 2)])
    return fx, fy, px, py, H, W, sigma, blur_radius


def topology_of(faces, n):
    """faces [F,3] -> (faces int32 contiguous, offsets int32 [N+1], slots int32 [3F]): per vertex the slots (face * 3 + corner) of
    its incident faces in ascending order.  Built once per faces tensor (this is where the indices are range-checked, the one host
    read) and kept while that tensor object lives and its version counter stands (a write that autograd's counter does not see,
    such as one through a raw pointer, is not noticed: pass a new tensor for a new mesh)."""
    key = id(faces)
    hit = _topology.get(key)
    if hit is not None and hit[0]() is faces and hit[1] == faces._version and hit[2] == n:
        return hit[3]
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= n:
        raise ValueError(f"faces: vertex indices must lie in [0, {n}), got [{lo}, {hi}]")
    f32 = faces.to(torch.int32).contiguous()
    flat = f32.reshape(-1).long()
    order = torch.sort(flat, stable=True).indices  # stable: ascending slot within a vertex
    counts = torch.bincount(flat, minlength=n)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=faces.device)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    value = (f32, offsets, order.to(torch.int32).contiguous())
    _topology.pop(key, None)  # (a stale entry of this tensor: re-inserted as the newest)
    while len(_topology) >= _TOPOLOGY_MAX:
        _topology.pop(next(iter(_topology)))  # the oldest
    # (the table is bound here: a tensor that dies at interpreter exit finds the module's globals already cleared)
    _topology[key] = (weakref.ref(faces, lambda _, key=key, table=_topology: table.pop(key, None)), faces._version, n, value)
    return value


_topology_of = topology_of  # its name before fit.DevicePoseFit became a caller from outside this module


class _SoftSilhouette(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, cam):
        fx, fy, px, py, H, W, sigma, blur = cam
        lib = _lib.load()
        v, _ = side(verts, 2)
        B, N = v.shape[0], v.shape[1]
        f32, offsets, slots = topology_of(faces, N)
        F = f32.shape[0]
        dev = v.device
        with torch.cuda.device(dev):
            ws, nbytes = _lib.workspace(lib.ivlm_soft_silhouette_workspace_bytes, "soft_silhouette", dev, B=B, N=N, F=F, H=H, W=W)
            alpha = torch.empty(B, H, W, dtype=torch.float32, device=dev)
            check(lib.ivlm_soft_silhouette_forward(v.data_ptr(), f32.data_ptr(), B, N, F, H, W, fx, fy, px, py, sigma, blur,
                                                   alpha.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "soft_silhouette_forward")
        # the workspace keeps 1 - alpha and the projected faces for the backward; verts through save_for_backward, so that an
        # in-place change of them before the backward raises instead of chaining through other coordinates
        ctx.save_for_backward(verts, offsets, slots, ws)  # (the input itself, not the view of it made here)
        ctx.sizes = (nbytes, F)
        ctx.cam = cam
        ctx.shape = tuple(verts.shape)
        return alpha if verts.dim() == 3 else alpha.view(H, W)  # (not alpha[0] outside: its backward would allocate an image)

    @staticmethod
    @once_differentiable  # the backward is a kernel, not a graph: a double backward raises instead of returning wrong derivatives
    def backward(ctx, grad_alpha):
        fx, fy, px, py, H, W, sigma, blur = ctx.cam
        verts, offsets, slots, ws = ctx.saved_tensors
        v, _ = side(verts, 2)
        nbytes, F = ctx.sizes
        lib = _lib.load()
        B, N = v.shape[0], v.shape[1]
        g = grad_alpha.to(torch.float32).expand(B, H, W).contiguous()
        with torch.cuda.device(v.device):
            gv = torch.empty(B, N, 3, dtype=torch.float32, device=v.device)
            check(lib.ivlm_soft_silhouette_backward(v.data_ptr(), offsets.data_ptr(), slots.data_ptr(), g.data_ptr(), B, N, F, H, W,
                                                    fx, fy, px, py, sigma, blur, gv.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
                  "soft_silhouette_backward")
        return gv.reshape(ctx.shape), None, None


def soft_silhouette(verts, faces, focal, principal, image_size, sigma=1e-4, blur_radius=None):
    """The soft silhouette (alpha channel) of a posed triangle mesh seen by an OpenCV pinhole camera.

    verts [N,3] or [B,N,3] (fp32, GPU, camera coordinates: +Z forward), faces [F,3] (int32 or int64, shared by the batch), focal =
    f or (fx, fy) and principal = (px, py) in pixels, image_size = (H, W) -> alpha [H,W] or [B,H,W], fp32.  sigma and blur_radius
    have pytorch3d's meaning (NDC units); blur_radius defaults to sigma ln(1 / 1e-4 - 1).  Differentiable in verts, once: a double
    backward raises.  The vertex-to-face incidence lists of a faces tensor are built (and its indices range-checked, one host read)
    on first use and reused while that tensor object lives unmodified; everything else is enqueued on the current stream without host
    synchronisation.  The same bits every call, for a pose whatever the batch around it."""
    cam = validate(verts, faces, focal, principal, image_size, sigma, blur_radius)
    return _SoftSilhouette.apply(verts, faces, cam)


def validate_terms(alpha, target_mask):
    if not isinstance(alpha, torch.Tensor):
        raise ValueError(f"alpha: expected a tensor, got {type(alpha).__name__}")
    if alpha.dim() not in (2, 3) or min(alpha.shape) < 1:
        raise ValueError(f"alpha: expected [H,W] or [B,H,W], got {tuple(alpha.shape)}")
    if alpha.dtype != torch.float32:
        raise ValueError(f"alpha: expected float32, got {alpha.dtype}")
    if not isinstance(target_mask, torch.Tensor):
        raise ValueError(f"target_mask: expected a tensor, got {type(target_mask).__name__}")
    if target_mask.dim() not in (2, 3) or tuple(target_mask.shape[-2:]) != tuple(alpha.shape[-2:]):
        raise ValueError(f"target_mask: expected [{alpha.shape[-2]},{alpha.shape[-1]}] (or with a batch axis), "
                         f"got {tuple(target_mask.shape)}")
    if target_mask.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise ValueError(f"target_mask: expected float32, bool or uint8, got {target_mask.dtype}")
    ba = alpha.shape[0] if alpha.dim() == 3 else 1
    bt = target_mask.shape[0] if target_mask.dim() == 3 else 1
    if bt not in (1, ba):  # (not batch_size: a batch of targets does not make a batch of one alpha)
        raise ValueError(f"target_mask: batch size {bt} does not broadcast with {ba}")
    check_devices([(alpha, "alpha", 2), (target_mask, "target_mask", 2)])


def _terms_call(lib, shape, a, t, sums, loss, centroid, g_loss, g_centroid, g_alpha, ws):
    """the forward (g_alpha None) or the backward (a, loss, centroid, ws None) of ivlm_silhouette_terms"""
    B, H, W = shape
    p = _lib.ptr
    check(lib.ivlm_silhouette_terms(p(a), t.data_ptr(), H * W if t.shape[0] > 1 else 0, B, H, W, p(loss), p(centroid), sums.data_ptr(),
                                    p(g_loss), p(g_centroid), p(g_alpha), p(ws), 0 if ws is None else ws.numel(), _lib.stream()),
          "silhouette_terms")


class _SilhouetteTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, target):
        lib = _lib.load()
        a, _ = side(alpha, 2)
        B, H, W = a.shape
        dev = a.device
        with torch.cuda.device(dev):
            ws = torch.empty(B * H * TERMS_WORKSPACE_ROW_BYTES, dtype=torch.uint8, device=dev)
            sums = torch.empty(B, 5, dtype=torch.float64, device=dev)
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            centroid = torch.empty(B, 2, dtype=torch.float32, device=dev)
            _terms_call(lib, (B, H, W), a, target, sums, loss, centroid, None, None, None, ws)
        ctx.saved = (target, sums, (B, H, W), tuple(alpha.shape))
        ctx.mark_non_differentiable(sums)
        return loss, centroid, sums

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_centroid, _g_sums):
        target, sums, (B, H, W), shape = ctx.saved
        lib = _lib.load()
        dev = sums.device
        with torch.cuda.device(dev):
            gl = g_loss.to(torch.float32).contiguous()
            gc = g_centroid.to(torch.float32).contiguous()
            g_alpha = torch.empty(B, H, W, dtype=torch.float32, device=dev)
            _terms_call(lib, (B, H, W), None, target, sums, None, None, gl, gc, g_alpha, None)
        return g_alpha.reshape(shape), None


def silhouette_terms(alpha, target_mask):
    """The two image terms of the reference's fit from one reduction over alpha and the target mask.

    alpha [H,W] or [B,H,W] (fp32, GPU), target_mask [H,W] or [B,H,W] (fp32, bool or uint8; constant) -> (mask_loss, centroid):
    mask_loss = 1 - sum(alpha t) / (sum alpha + sum t), shape [] or [B] - the reference's "union" is the sum of both images, which
    is mirrored; it is 1 when both images are empty.  centroid [2] or [B,2] = (sum i alpha, sum j alpha) / sum alpha in integer
    (row, col) index units as ``calculate_centroid`` has it; the image centre (H / 2, W / 2) with zero gradient when sum alpha ==
    0.  Sums are fp64 in a fixed order; no ``nonzero``, no host synchronisation.  Differentiable in alpha, once."""
    validate_terms(alpha, target_mask)
    t, _ = side(target_mask.detach().to(torch.float32), 2)
    loss, centroid, _ = _SilhouetteTerms.apply(alpha, t)
    return (loss, centroid) if alpha.dim() == 3 else (loss[0], centroid[0])
