"""The scene of the multi-start search tests and its fp64 restatement (shared by tests/test_pose_gpu.py and
tests/golden/make_golden_pose_search.py; nothing here needs a GPU or the library).

An object without rotational symmetry (a warped 8 x 12 sphere, centred), posed by the cube rotation of index 7, beside a human
stand-in (a 6 x 8 sphere); contact on the facing patches; the target mask is the fp64 render of the true pose.  All 24 starts sit
at the same translation, a few centimetres off the truth.
"""
import functools

import torch

import _silhouette_ref as ref
from interactvlm_amd import fit, pose

TRUE_INDEX = 7
MAX_ITER = 20
GOLDEN = "pose_search_fp64.json"


@functools.lru_cache(maxsize=None)
def search_scene():
    """-> cam, obj fp32 [86,3], faces [168,3], hum fp32 [50,3], p_obj [86], p_hum [50], target bool [48,48], T_start fp32 [3]"""
    cam = ref.camera(48, 48)
    v, faces = ref.uv_sphere(8, 12)
    x, y, z = v.unbind(-1)
    obj = torch.stack((x + 0.8 * y * y, 0.6 * y + 0.6 * z * z, 0.4 * z + 0.6 * x * y), -1)
    obj = (obj - obj.mean(0)).float()  # what the kernels are given; fp64 copies of these values are the reference's input
    R_true = pose.cube_rotations()[TRUE_INDEX].double()
    T_true = torch.tensor([0.1, -0.05, 3.0], dtype=torch.float64)
    posed = obj.double() @ R_true + T_true
    hum = (ref.uv_sphere(6, 8)[0] + torch.tensor([1.05, -0.05, 3.1], dtype=torch.float64)).float()
    p_obj = ((posed[:, 0] - 0.1) > 0.25).float() * 0.8
    p_hum = ((hum.double()[:, 0] - 1.05) < -0.3).float() * 0.6
    with torch.no_grad():
        target = ref.render(posed, faces, cam, 1e-4) > 0.5
    T_start = (T_true + torch.tensor([0.05, -0.04, 0.06], dtype=torch.float64)).float()
    return cam, obj, faces, hum, p_obj, p_hum, target, T_start


def total_fp64(r6, t, weights=None):
    """the total of ``ObjectPoseFit.forward`` (every term on, no centroid offset, scale 1) from the fp64 definitions"""
    cam, obj, faces, hum, p_obj, p_hum, target, _ = search_scene()
    w = fit.DEFAULT_LOSS_WEIGHTS if weights is None else weights
    moved = fit.apply_transformation(obj.double(), r6, t)
    mask_loss, centroid = ref.terms(ref.render(moved, faces, cam, 1e-4), target)
    centroid_loss = ((centroid - fit.mask_bbox_centre(target.float()).double()) ** 2).sum()
    d = (moved[:, None, :] - hum.double()[None]).norm(dim=-1)
    pq = p_obj.double()[:, None] * p_hum.double()[None]
    contact = (pq * d).sum() / pq.sum()
    return w["mask_loss"]["w"] * mask_loss + w["centroid_loss"]["w"] * centroid_loss + w["contact_loss"]["w"] * contact


def fit_fp64(k, max_iter=MAX_ITER):
    """start k of the search in fp64: torch.optim.Adam with the learning rates of ``fit_object_pose`` -> (history, final total)"""
    T_start = search_scene()[7]
    r6 = torch.nn.Parameter(fit.matrix_to_rot6d(pose.cube_rotations()[k].double())[0])
    t = torch.nn.Parameter(T_start.double())
    opt = torch.optim.Adam([{"params": [r6], "lr": 5e-2}, {"params": [t], "lr": 1e-2}])
    history = []
    for _ in range(max_iter):
        opt.zero_grad()
        total = total_fp64(r6, t)
        total.backward()
        opt.step()
        history.append(float(total.detach()))
    with torch.no_grad():
        return history, float(total_fp64(r6, t))
