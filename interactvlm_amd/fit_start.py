"""The start of the object-pose fit: what the reference computes between "two meshes, two contact vectors, one mask" and the
(rotation_init, translation_init, scaling_init) its optimiser starts from - the device part of optim/data_io.py ``load_params`` and
optim/fit.py:99-193 - as HIP kernels (csrc/fit_start.hip), without pytorch3d or trimesh.

    vertex_normals     area-weighted vertex normals (pytorch3d ``Meshes.verts_normals_list``, then normalised: data_io.py:40-42)
    surface_centroid   area-weighted centroid of the surface (trimesh ``Trimesh.centroid``: data_io.py:175)
    mask_stats         count, bounding box, index sums and the first two non-zero pixels of a mask
    contact_depth      count and mean z of the vertices above a contact threshold
    osx_camera         ``get_camera_params_torch`` (data_io.py:96-109)
    centre_meshes      both meshes centred as ``load_params`` centres them, with their normals
    centroid_start     the stage-1 translation (optim/fit.py:119-135)
    reference_start    the whole chain: stage 1, selections, normal filter, ICP -> ``fit_object_pose(init=...)``

The pytorch3d and trimesh definitions are taken from their documentation; neither library exists for this stack, so no golden from
either exists: tests/_fit_start_ref.py restates the definitions in fp64.  Deliberately not the reference's: a vertex whose face normals
sum to zero gets (0, 0, 0), not NaN; an empty selection or a mask without the pixels stage 1 reads raises ``ValueError`` by name, not
``IndexError`` / NaN.  Loading the meshes, masks and detections from files stays out of scope.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib
from ._args import check_devices, check_points, check_vector
from ._lib import check, header_constant
from .constants import OSX_FOCAL_VIRTUAL, OSX_INPUT_BODY_SHAPE, OSX_PRINCPT
from .contact_icp import ICPResult, contact_icp, contact_normal_filter
from .contact_pair import IVLM_BF16, IVLM_F32
from .silhouette import topology_of

MASK_RECORD, DEPTH_RECORD = header_constant("IVLM_MASK_RECORD"), header_constant("IVLM_DEPTH_RECORD")
(M_COUNT, M_ROW_MIN, M_ROW_MAX, M_COL_MIN, M_COL_MAX, M_ROW_SUM, M_COL_SUM, M_FIRST_ROW, M_SECOND_ROW) = (
    header_constant(f"IVLM_MASK_{k}") for k in ("COUNT", "ROW_MIN", "ROW_MAX", "COL_MIN", "COL_MAX", "ROW_SUM", "COL_SUM", "FIRST_ROW",
                                                "SECOND_ROW"))
EMPTY_MASK, FEW_PIXELS, NO_CONTACT, NO_AREA = (header_constant(f"IVLM_START_{k}")
                                               for k in ("EMPTY_MASK", "FEW_PIXELS", "NO_CONTACT", "NO_AREA"))
# the one device record of a stage-1 chain: the mask record, the depth record, the translation's status word
_AT_MASK, _AT_DEPTH, _AT_T, _RECORD = 0, MASK_RECORD, MASK_RECORD + DEPTH_RECORD, MASK_RECORD + DEPTH_RECORD + 1
PROB_DTYPES = (torch.float32, torch.bfloat16)  # what contact_pair.one_dtype takes
MASK_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32,
               torch.float64)


class MaskStats(NamedTuple):
    """device tensors, int64; a field that no pixel defines is -1"""
    count: torch.Tensor    # []
    row_min: torch.Tensor  # []
    row_max: torch.Tensor  # []
    col_min: torch.Tensor  # []
    col_max: torch.Tensor  # []
    row_sum: torch.Tensor  # []
    col_sum: torch.Tensor  # []
    first: torch.Tensor    # [2]: (row, col) of the first non-zero pixel in row-major order
    second: torch.Tensor   # [2]: of the second


class ContactDepth(NamedTuple):
    count: torch.Tensor  # int64 []
    z_sum: torch.Tensor  # fp64 []
    z: torch.Tensor      # fp32 []: z_sum / count rounded once, 0 when count is 0


class CentredMeshes(NamedTuple):
    human_vertices: torch.Tensor       # [N_h,3]: minus hum_centroid_offset
    obj_vertices: torch.Tensor         # [N_o,3]: minus its surface centroid, then y and z negated
    hum_centroid_offset: torch.Tensor  # [3]
    human_normals: torch.Tensor        # [N_h,3], of the centred meshes
    obj_normals: torch.Tensor          # [N_o,3]


class ReferenceStart(NamedTuple):
    init: tuple                      # (R6 [1,6], T [1,3], s): ready for fit_object_pose(init=...)
    obj_contact_probs: torch.Tensor  # [N_o]: every entry that is not kept set to 0 (optim/fit.py:166-167)
    kept: torch.Tensor               # bool [N_o]
    obj_normals: torch.Tensor        # [N_o,3]
    human_normals: torch.Tensor      # [N_h,3]
    icp: ICPResult | None            # None with icp=False
    stage1_translation: torch.Tensor  # [3]: the translation ICP started from


# ---- argument checks (all of them before the library loads) ---------------------------------------------------------------------------

def check_faces(faces, name="faces"):
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(faces).__name__}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"{name}: expected [F,3] with F >= 1, got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: expected int32 or int64 vertex indices, got {faces.dtype}")


def check_mesh(verts, faces, vname="verts", fname="faces"):
    check_points(verts, vname, batch=False)
    check_faces(faces, fname)


def check_mask(mask, name="mask"):
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(mask).__name__}")
    if mask.dim() != 2 or min(mask.shape) < 1:
        raise ValueError(f"{name}: expected [H,W], got {tuple(mask.shape)}")
    if mask.dtype not in MASK_DTYPES:
        raise ValueError(f"{name}: expected a bool, integer or floating-point mask, got {mask.dtype}")


def check_threshold(t, name="threshold"):
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t):
        raise ValueError(f"{name}: expected a finite number, got {t!r}")
    return float(t)


def check_offset(off, name="hum_centroid_offset"):
    if off is None:
        return
    if not isinstance(off, torch.Tensor) or tuple(off.shape) != (3,) or off.dtype != torch.float32:
        raise ValueError(f"{name}: expected a float32 tensor [3] or None, got "
                         f"{(tuple(off.shape), off.dtype) if isinstance(off, torch.Tensor) else type(off).__name__}")


def check_camera(focal, principal):
    """focal = f, (fx, fy) or a tensor of one or two elements, principal = (px, py) or a tensor [2]; numbers must be finite (a tensor's
    values are not read)"""
    for x, name, sizes in ((focal, "focal", (1, 2)), (principal, "principal", (2,))):
        if isinstance(x, torch.Tensor):
            if x.numel() not in sizes or not x.dtype.is_floating_point:
                raise ValueError(f"{name}: expected a floating-point tensor of {' or '.join(map(str, sizes))} elements, got "
                                 f"{tuple(x.shape)} {x.dtype}")
            continue
        try:
            vals = [float(v) for v in (x if isinstance(x, (tuple, list)) else (x,))]
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected a number, a pair or a tensor, got {x!r}") from None
        if len(vals) not in sizes or not all(math.isfinite(v) for v in vals):
            raise ValueError(f"{name}: expected {' or '.join(map(str, sizes))} finite numbers, got {x!r}")


def camera_tensor(focal, principal, device):
    """-> f32 [4] on ``device``: (fx, fy, px, py).  Tensors stay on the device (no host read)."""
    def part(x):
        if isinstance(x, torch.Tensor):
            x = x.detach().reshape(-1).to(device=device, dtype=torch.float32)
        else:
            x = torch.tensor([float(v) for v in (x if isinstance(x, (tuple, list)) else (x,))], dtype=torch.float32, device=device)
        return x.expand(2) if x.numel() == 1 else x
    return torch.cat([part(focal), part(principal)]).contiguous()


def _raise_for(status, mask_name="mask", probs_name="human_contact_probs", threshold=None, mesh_name="faces"):
    """the IVLM_START_* bits of a status word read from the device -> ValueError by name"""
    if status & FEW_PIXELS:
        raise ValueError(f"{mask_name}: fewer than two non-zero pixels: mirror_reference=True reads the first two (the reference raises "
                         "IndexError here)")
    if status & EMPTY_MASK:
        raise ValueError(f"{mask_name}: no non-zero pixel")
    if status & NO_CONTACT:
        raise ValueError(f"{probs_name}: no vertex above the threshold{'' if threshold is None else f' {threshold}'} (the reference's "
                         "mean over none is NaN)")
    if status & NO_AREA:
        raise ValueError(f"{mesh_name}: no face has an area: the surface centroid is undefined")


# ---- launches (arguments already checked; ``status`` / ``record`` are int64 views the kernels write) ----------------------------------

def _normals(lib, verts, faces):
    v = verts.detach().contiguous()
    n = v.shape[0]
    f32, offsets, slots = topology_of(faces, n)
    out = torch.empty(n, 3, dtype=torch.float32, device=v.device)
    check(lib.ivlm_mesh_vertex_normals(v.data_ptr(), f32.data_ptr(), offsets.data_ptr(), slots.data_ptr(), n, f32.shape[0],
                                       out.data_ptr(), _lib.stream()), "mesh_vertex_normals")
    return out


def _centroid(lib, verts, faces, status):
    v = verts.detach().contiguous()
    n = v.shape[0]
    f32, _, _ = topology_of(faces, n)  # (the int32 copy and the range check; a cache hit after vertex_normals of the same tensor)
    F = f32.shape[0]
    ws, nbytes = _lib.workspace(lib.ivlm_mesh_surface_centroid_workspace_bytes, "surface_centroid", v.device, F=F)
    out = torch.empty(3, dtype=torch.float32, device=v.device)
    check(lib.ivlm_mesh_surface_centroid(v.data_ptr(), f32.data_ptr(), n, F, out.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes,
                                         _lib.stream()), "mesh_surface_centroid")
    return out


def _mask_record(lib, mask, record):
    on = (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8)
    H, W = on.shape
    ws, nbytes = _lib.workspace(lib.ivlm_mask_stats_workspace_bytes, "mask_stats", on.device, H=H, W=W)
    check(lib.ivlm_mask_stats(on.data_ptr(), H, W, record.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "mask_stats")


def _depth(lib, verts, probs, threshold, record):
    v = verts.detach().contiguous()
    p = probs.detach().contiguous()
    n = v.shape[0]
    ws, nbytes = _lib.workspace(lib.ivlm_contact_depth_workspace_bytes, "contact_depth", v.device, N=n)
    z_sum = torch.empty((), dtype=torch.float64, device=v.device)
    z = torch.empty((), dtype=torch.float32, device=v.device)
    check(lib.ivlm_contact_depth(v.data_ptr(), p.data_ptr(), IVLM_BF16 if p.dtype == torch.bfloat16 else IVLM_F32, n, threshold,
                                 record.data_ptr(), z_sum.data_ptr(), z.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
          "contact_depth")
    return z_sum, z


def _stage1(lib, mask, human_vertices, human_contact_probs, focal, principal, offset, threshold, mirror, rec):
    """the three launches of the stage-1 translation; ``rec`` is the chain's record -> T [3]"""
    dev = human_vertices.device
    _mask_record(lib, mask, rec[_AT_MASK:_AT_DEPTH])
    _, z = _depth(lib, human_vertices, human_contact_probs, threshold, rec[_AT_DEPTH:_AT_T])
    cam = camera_tensor(focal, principal, dev)
    off = None if offset is None else offset.detach().contiguous()
    T = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib.ivlm_start_translation(rec[_AT_MASK:].data_ptr(), rec[_AT_DEPTH:].data_ptr(), z.data_ptr(), cam.data_ptr(), _lib.ptr(off),
                                     int(bool(mirror)), T.data_ptr(), rec[_AT_T:].data_ptr(), _lib.stream()), "start_translation")
    return T


# ---- the public functions ------------------------------------------------------------------------------------------------------------

def vertex_normals(verts, faces):
    """Unit vertex normals of a triangle mesh, area-weighted (pytorch3d's documented weighting, then ``normals /= norm`` as
    data_io.py:40-42 has it).

    verts [N,3] (fp32, GPU, any strides), faces [F,3] (int32 or int64) -> [N,3] fp32: the sum over the vertex's faces of
    cross(b - a, c - a), fp64 from the fp32 coordinates, added in ascending (face, corner) order, divided by its fp64 length and rounded
    once.  A vertex whose sum is zero - no face, or only zero-area faces - gets (0, 0, 0); the reference gives NaN there.  One launch;
    the incidence lists of a faces tensor are built on first use (``silhouette.topology_of``: the index range check, one host read)
    and reused.  The same bits every call.  Not differentiable."""
    check_mesh(verts, faces)
    check_devices([(verts, "verts", 2), (faces, "faces", 2)])
    lib = _lib.load()
    with torch.cuda.device(verts.device):
        return _normals(lib, verts, faces)


def surface_centroid(verts, faces):
    """The area-weighted centroid of a mesh's surface (trimesh's documented ``Trimesh.centroid``): sum_f A_f (a + b + c) / 3 / sum_f A_f.

    verts [N,3] (fp32, GPU), faces [F,3] (int32 or int64) -> [3] fp32; fp64 sums in a fixed order (256 faces per block, then the block
    sums), one division per axis, rounded once.  Two launches.  Reads one status word back: a mesh none of whose faces has an area
    raises ``ValueError``."""
    check_mesh(verts, faces)
    check_devices([(verts, "verts", 2), (faces, "faces", 2)])
    lib = _lib.load()
    with torch.cuda.device(verts.device):
        status = torch.zeros(1, dtype=torch.int64, device=verts.device)
        c = _centroid(lib, verts, faces, status)
        _raise_for(int(status[0]))
    return c


def mask_stats(mask) -> MaskStats:
    """What the fit's start reads off a mask, in one pass: mask [H,W] (bool, integer or floating point, GPU; a pixel is on when it is
    != 0) -> ``MaskStats`` of int64 device tensors, exact.  An empty mask gives count 0 and -1 elsewhere (the sums are 0).  Two
    launches, no host read."""
    check_mask(mask)
    check_devices([(mask, "mask", 2)])
    lib = _lib.load()
    with torch.cuda.device(mask.device):
        rec = torch.zeros(MASK_RECORD, dtype=torch.int64, device=mask.device)
        _mask_record(lib, mask, rec)
    return MaskStats(rec[M_COUNT], rec[M_ROW_MIN], rec[M_ROW_MAX], rec[M_COL_MIN], rec[M_COL_MAX], rec[M_ROW_SUM], rec[M_COL_SUM],
                     rec[M_FIRST_ROW:M_FIRST_ROW + 2], rec[M_SECOND_ROW:M_SECOND_ROW + 2])


def contact_depth(verts, probs, threshold) -> ContactDepth:
    """Count, fp64 sum and mean of z over the vertices whose contact probability is strictly above ``threshold``.

    verts [N,3] (fp32, GPU), probs [N] (fp32 or bf16; compared in fp32, against the threshold rounded to fp32 as torch's
    ``probs.float() > threshold`` compares) -> ``ContactDepth`` of device tensors; the mean is the fp64 sum (256 vertices per block,
    then the block sums) over the count, rounded once, and 0 when no vertex is selected.  Two launches, no host read."""
    check_points(verts, "verts", batch=False)
    check_vector(probs, verts.shape[0], "probs", PROB_DTYPES)
    threshold = check_threshold(threshold)
    check_devices([(verts, "verts", 2), (probs, "probs", 1)])
    lib = _lib.load()
    with torch.cuda.device(verts.device):
        rec = torch.zeros(DEPTH_RECORD, dtype=torch.int64, device=verts.device)
        z_sum, z = _depth(lib, verts, probs, threshold, rec)
    return ContactDepth(rec[0], z_sum, z)


def osx_camera(bbox):
    """``get_camera_params_torch`` (data_io.py:96-109): bbox = (x, y, w, h) of the person, a tensor [4] or four numbers ->
    (focal [2], principal [2]) fp32 on the box's device, by the reference's operations in its order:
    focal = (5000 / 192 * w, 5000 / 256 * h), principal = (96 / 192 * w + x, 128 / 256 * h + y)."""
    if not isinstance(bbox, torch.Tensor):
        try:
            bbox = torch.tensor([float(v) for v in bbox], dtype=torch.float32)
        except (TypeError, ValueError):
            raise ValueError(f"bbox: expected a tensor [4] or four numbers, got {bbox!r}") from None
    if bbox.numel() != 4 or bbox.dim() != 1:
        raise ValueError(f"bbox: expected (x, y, w, h), got {tuple(bbox.shape)}")

    def c(v):
        return torch.tensor(v, dtype=torch.float32, device=bbox.device)

    fv, bs, pt = OSX_FOCAL_VIRTUAL, OSX_INPUT_BODY_SHAPE, OSX_PRINCPT
    focal = torch.stack([c(fv[0]) / c(bs[1]) * bbox[2], c(fv[1]) / c(bs[0]) * bbox[3]], dim=0)
    principal = torch.stack([c(pt[0]) / c(bs[1]) * bbox[2] + bbox[0], c(pt[1]) / c(bs[0]) * bbox[3] + bbox[1]], dim=0)
    return focal, principal


def centre_meshes(human_vertices, human_faces, obj_vertices, obj_faces) -> CentredMeshes:
    """The device part of ``load_params`` (data_io.py:173-194): the human minus its surface centroid (returned as
    hum_centroid_offset), the object minus its surface centroid and then its y and z negated, and the normals of both, taken after
    those steps.  The subtraction is fp32 (the reference subtracts in fp64 and rounds: half an ulp apart at most).  Six launches and
    three elementwise torch operations; reads one record back (both centroids' status words): a mesh without area raises."""
    check_mesh(human_vertices, human_faces, "human_vertices", "human_faces")
    check_mesh(obj_vertices, obj_faces, "obj_vertices", "obj_faces")
    check_devices([(human_vertices, "human_vertices", 2), (human_faces, "human_faces", 2), (obj_vertices, "obj_vertices", 2),
                   (obj_faces, "obj_faces", 2)])
    lib = _lib.load()
    dev = human_vertices.device
    with torch.cuda.device(dev):
        status = torch.zeros(2, dtype=torch.int64, device=dev)
        offset = _centroid(lib, human_vertices, human_faces, status[0:])
        obj_c = _centroid(lib, obj_vertices, obj_faces, status[1:])
        human = human_vertices.detach() - offset
        obj = (obj_vertices.detach() - obj_c) * torch.tensor([1.0, -1.0, -1.0], device=dev)
        h_n, o_n = _normals(lib, human, human_faces), _normals(lib, obj, obj_faces)
        bad = status.cpu().tolist()
        _raise_for(bad[0], mesh_name="human_faces")
        _raise_for(bad[1], mesh_name="obj_faces")
    return CentredMeshes(human, obj, offset, h_n, o_n)


def _check_stage1(mask, human_vertices, human_contact_probs, focal, principal, hum_centroid_offset, threshold, mask_name="mask"):
    check_mask(mask, mask_name)
    check_points(human_vertices, "human_vertices", batch=False)
    check_vector(human_contact_probs, human_vertices.shape[0], "human_contact_probs", PROB_DTYPES)
    check_camera(focal, principal)
    check_offset(hum_centroid_offset)
    return check_threshold(threshold)


def centroid_start(mask, human_vertices, human_contact_probs, focal, principal, hum_centroid_offset=None, threshold=0.5,
                   mirror_reference=True):
    """The stage-1 translation of optim/fit.py:119-135 -> T [3] fp32.

    mask [H,W] (the object's mask, as ``mask_stats`` takes it), human_vertices [N_h,3] (centred: minus hum_centroid_offset),
    human_contact_probs [N_h] (fp32 or bf16), focal = f, (fx, fy) or a tensor, principal = (px, py) or a tensor [2] (tensors are not
    read on the host), hum_centroid_offset [3] or None.  z = the mean z of the human vertices with probability > threshold.

    mirror_reference=True repeats the reference as written, in fp32 and in its operation order, T = ((cx z) / fx, (cy z) / fy, z):
    ``nonzero(mask)[1]`` indexes a PIXEL, not the column axis, so cx = the mean of (row, col) of the SECOND non-zero pixel in
    row-major order minus principal[0], and cy = the mean of (row, col) of the FIRST one minus principal[1].  hum_centroid_offset is
    not used.  Fewer than two non-zero pixels raise ``ValueError`` (the reference: ``IndexError``), no human vertex above the
    threshold raises ``ValueError`` (the reference: NaN).

    mirror_reference=False is the evident intent and NOT the reference's: the object's origin is put on the camera ray through the
    centre of the mask's mean pixel, (sum of columns / count + 0.5, sum of rows / count + 0.5) in ``silhouette``'s convention
    u = fx X / Z + px, at depth Z = z + hum_centroid_offset[2], and expressed in the fit's frame, that is minus hum_centroid_offset,
    because the silhouette renders vertices + offset.  fp64, rounded once.  An empty mask raises.

    Five launches on the current stream; one status word is read back."""
    threshold = _check_stage1(mask, human_vertices, human_contact_probs, focal, principal, hum_centroid_offset, threshold)
    named = [(mask, "mask", 2), (human_vertices, "human_vertices", 2), (human_contact_probs, "human_contact_probs", 1)]
    if hum_centroid_offset is not None:
        named.append((hum_centroid_offset, "hum_centroid_offset", 1))
    check_devices(named)
    lib = _lib.load()
    dev = human_vertices.device
    with torch.cuda.device(dev):
        rec = torch.zeros(_RECORD, dtype=torch.int64, device=dev)
        T = _stage1(lib, mask, human_vertices, human_contact_probs, focal, principal, hum_centroid_offset, threshold, mirror_reference, rec)
        _raise_for(int(rec[_AT_T]), threshold=threshold)
    return T


def _parse_filter(filter_contacts):
    """(False, ...) -> None; (True, a) -> (a, None); (True, a, b) -> (a, b): the reference's ``icp.filter_contacts`` list"""
    try:
        parts = tuple(filter_contacts)
        on = bool(parts[0])
        angles = tuple(float(a) for a in parts[1:3]) if on else ()
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"filter_contacts: expected (False,), (True, angle) or (True, angle, negative angle), got {filter_contacts!r}") from None
    if not on:
        return None
    if len(parts) not in (2, 3) or not all(math.isfinite(a) for a in angles):
        raise ValueError(f"filter_contacts: expected (False,), (True, angle) or (True, angle, negative angle), got {filter_contacts!r}")
    return angles[0], (angles[1] if len(angles) == 2 else None)


def reference_start(obj_vertices, obj_faces, human_vertices, human_faces, obj_contact_probs, human_contact_probs, target_mask, focal,
                    principal, hum_centroid_offset=None, scale=1.0, thresholds=(0.3, 0.5), translation_hum_centroid=True, icp=True,
                    filter_contacts=(True, 90, -90), estimate_scale=False, icp_max_iterations=10, mirror_reference=True,
                    obj_normals=None, human_normals=None) -> ReferenceStart:
    """The start the reference's fit begins from: optim/fit.py:99-193 in its order, for meshes centred as ``centre_meshes`` centres
    them.

      1. translation_hum_centroid: T1 = ``centroid_start`` (``mirror_reference`` chooses its mode), else 0; R = I, s = ``scale``
      2. the selections obj_contact_probs > thresholds[0] and human_contact_probs > thresholds[1] (compared in fp32)
      3. filter_contacts = (True, angle[, negative angle]): ``contact_normal_filter`` on the selected normals (it negates the human's
         itself); ``kept`` = the selected object vertices that pass, and EVERY other entry of the object contact vector is set to 0,
         as optim/fit.py:166-167 does - that vector is what the reference's ``contact_loss`` then sees.  (False,): nothing changes
      4. the object selection again, from the filtered vector
      5. icp: ``contact_icp`` with both selections' normals from init = (I, T1, scale), ``requery=False`` (the reference's loop);
         R, T come from it, the scale stays ``scale`` whatever ``estimate_scale`` found, as in the reference

    obj_normals / human_normals [N,3]: computed with ``vertex_normals`` when None (human_faces is needed only then, and may be None
    when human_normals is given).  -> ``ReferenceStart``; ``fit_object_pose(..., obj_contact_probs=start.obj_contact_probs,
    init=start.init)`` continues as the reference does.

    Host reads: the topology cache of each faces tensor on first use, the one status / count record (before the selections), and
    the boolean selections themselves, as in ``fit_object_pose(init=None)``.  Raises ``ValueError`` by name for what stage 1 cannot
    read (see ``centroid_start``) and for a selection that is empty, before or after the filter."""
    check_mesh(obj_vertices, obj_faces, "obj_vertices", "obj_faces")
    check_points(human_vertices, "human_vertices", batch=False)
    if human_normals is None or human_faces is not None:
        check_faces(human_faces, "human_faces")
    check_vector(obj_contact_probs, obj_vertices.shape[0], "obj_contact_probs", PROB_DTYPES)
    if not isinstance(thresholds, (tuple, list)) or len(thresholds) != 2:
        raise ValueError(f"thresholds: expected (object threshold, human threshold), got {thresholds!r}")
    threshold_o = check_threshold(thresholds[0], "thresholds[0]")
    check_threshold(thresholds[1], "thresholds[1]")
    threshold_h = _check_stage1(target_mask, human_vertices, human_contact_probs, focal, principal, hum_centroid_offset, thresholds[1],
                                "target_mask")
    scale = check_threshold(scale, "scale")
    angles = _parse_filter(filter_contacts)
    if not isinstance(icp_max_iterations, int) or icp_max_iterations < 1:
        raise ValueError(f"icp_max_iterations: expected an integer >= 1, got {icp_max_iterations!r}")
    named = [(obj_vertices, "obj_vertices", 2), (obj_faces, "obj_faces", 2), (human_vertices, "human_vertices", 2),
             (obj_contact_probs, "obj_contact_probs", 1), (human_contact_probs, "human_contact_probs", 1), (target_mask, "target_mask", 2)]
    for normals, name, verts in ((obj_normals, "obj_normals", obj_vertices), (human_normals, "human_normals", human_vertices)):
        if normals is not None:
            check_points(normals, name, batch=False)
            if normals.shape[0] != verts.shape[0]:
                raise ValueError(f"{name}: expected one normal per vertex, [{verts.shape[0]},3], got {tuple(normals.shape)}")
            named.append((normals, name, 2))
    if human_faces is not None:
        named.append((human_faces, "human_faces", 2))
    if hum_centroid_offset is not None:
        named.append((hum_centroid_offset, "hum_centroid_offset", 1))
    check_devices(named)
    lib = _lib.load()
    from .fit import matrix_to_rot6d  # (here: fit imports the term modules, this module is a caller of both)

    dev = obj_vertices.device
    with torch.cuda.device(dev):
        o_v, h_v = obj_vertices.detach(), human_vertices.detach()
        o_n = _normals(lib, o_v, obj_faces) if obj_normals is None else obj_normals.detach()
        h_n = _normals(lib, h_v, human_faces) if human_normals is None else human_normals.detach()
        if translation_hum_centroid:
            rec = torch.zeros(_RECORD, dtype=torch.int64, device=dev)
            T1 = _stage1(lib, target_mask, h_v, human_contact_probs, focal, principal, hum_centroid_offset, threshold_h, mirror_reference,
                         rec)
            _raise_for(int(rec[_AT_T]), "target_mask", threshold=threshold_h)  # the one record read
        else:
            T1 = torch.zeros(3, dtype=torch.float32, device=dev)
        probs = obj_contact_probs.detach()
        o_on = probs.float() > threshold_o
        h_on = human_contact_probs.detach().float() > threshold_h
        h_sel, h_sel_n = h_v[h_on], h_n[h_on]
        if h_sel.shape[0] < 1:
            raise ValueError(f"human_contact_probs: no vertex above the threshold {threshold_h}")
        if not bool(o_on.any()):
            raise ValueError(f"obj_contact_probs: no vertex above the threshold {threshold_o}")
        kept = o_on
        if angles is not None and icp:  # (the reference filters inside its ``if icp_opt.run``)
            passed = contact_normal_filter(o_n[o_on], h_sel_n, angles[0], angles[1])
            kept = o_on.clone()
            kept[o_on] = passed
            probs = torch.where(kept, probs, torch.zeros((), dtype=probs.dtype, device=dev))
            o_on = probs.float() > threshold_o  # "extract contacts again since they might've changed"
        o_sel = o_v[o_on]
        if o_sel.shape[0] < 1:
            raise ValueError("obj_contact_probs: no selected vertex passes filter_contacts: nothing is left for contact_icp")
        R6 = matrix_to_rot6d(torch.eye(3, dtype=torch.float32, device=dev))
        T, found = T1[None], None
        if icp:
            found = contact_icp(o_sel, h_sel, o_n[o_on], h_sel_n,
                                init=(torch.eye(3, dtype=torch.float32, device=dev)[None], T1[None],
                                      torch.full((1,), scale, dtype=torch.float32, device=dev)),
                                max_iterations=icp_max_iterations, estimate_scale=bool(estimate_scale), requery=False)
            R6, T = matrix_to_rot6d(found.R), found.T
    return ReferenceStart((R6, T, scale), probs, kept, o_n, h_n, found, T1)
