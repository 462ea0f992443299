"""mesh_sdf without a GPU: the module imports, arguments are validated before the library is touched, the C ABI declares the entry
points and the constants the Python side uses, and the yardstick of the GPU tests (tests/_mesh_sdf_ref.py) is itself checked: against
the analytic signed distance of a cube in all 27 regions, and its analytic penetration gradient against central differences."""
import inspect
import re

import numpy as np
import pytest
import torch

import _mesh_sdf_ref as ref
from interactvlm_amd import _lib, fit
from interactvlm_amd import mesh_sdf as ms
from interactvlm_amd.synthetic import body_mesh

ENTRY_POINTS = {"ivlm_mesh_sdf_plan_bytes": ("size_t", 2), "ivlm_mesh_sdf_prepare": ("int", 7),
                "ivlm_mesh_sdf_workspace_bytes": ("size_t", 3), "ivlm_mesh_sdf_query": ("int", 11),
                "ivlm_mesh_sdf_penetration": ("int", 9)}


def test_module_imports_without_gpu():
    assert callable(ms.mesh_signed_distance) and callable(ms.penetration_loss)
    assert all(callable(getattr(ms.MeshSDF, n)) for n in ("query", "penetration"))
    assert isinstance(ms.TILE, int) and isinstance(ms.CHUNK, int) and 0 < ms.TILE <= ms.CHUNK and ms.CHUNK % ms.TILE == 0


def test_header_declares_the_entry_points_and_constants():
    protos = _lib.header_prototypes()
    for name, (ret, nargs) in ENTRY_POINTS.items():
        assert name in protos, name
        assert protos[name][0] == ret and len(protos[name][1]) == nargs, (name, protos[name])
    txt = open(_lib.HEADER_PATH).read()
    for name, value in (("IVLM_MESH_SDF_TILE", ms.TILE), ("IVLM_MESH_SDF_CHUNK", ms.CHUNK)):
        m = re.search(rf"#define\s+{name}\s+(\d+)", txt)
        assert m and int(m.group(1)) == value


def test_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.ivlm_abi_version() == 5
    assert lib.ivlm_mesh_sdf_prepare(None, None, 8, 12, None, 0, None) == -1
    assert lib.ivlm_mesh_sdf_query(None, None, 1, 4, None, None, None, None, None, 0, None) == -1
    assert lib.ivlm_mesh_sdf_penetration(None, None, 1, 4, None, None, None, 0, None) == -1
    fake = 4096  # pointers that are never followed: the refusals below come before any launch
    assert lib.ivlm_mesh_sdf_prepare(fake, fake, 0, 12, fake, 1 << 20, None) == -1
    assert lib.ivlm_mesh_sdf_prepare(fake, fake, 8, 12, fake, 16, None) == -2
    assert lib.ivlm_mesh_sdf_query(fake, fake, 0, 4, fake, fake, fake, fake, fake, 1 << 20, None) == -1
    assert lib.ivlm_mesh_sdf_query(fake, fake, 1, 4, None, None, None, None, fake, 1 << 20, None) == -1
    assert lib.ivlm_mesh_sdf_query(fake, fake, 1, 4, fake, fake, fake, fake, fake, 64, None) == -2
    assert lib.ivlm_mesh_sdf_penetration(fake, fake, 1, -4, fake, None, fake, 1 << 20, None) == -1
    assert lib.ivlm_mesh_sdf_penetration(fake, fake, 1, 4, None, None, fake, 1 << 20, None) == -1
    assert lib.ivlm_mesh_sdf_penetration(fake, fake, 1, 4, fake, None, fake, 64, None) == -2
    assert lib.ivlm_mesh_sdf_plan_bytes(6890, 13776) == 256 + 48 * 13776
    assert lib.ivlm_mesh_sdf_plan_bytes(0, 12) == 0 and lib.ivlm_mesh_sdf_plan_bytes(8, 0) == 0
    assert lib.ivlm_mesh_sdf_workspace_bytes(1, 64, 12) > 0
    for bad in ((0, 64, 12), (1, 0, 12), (1, 64, 0), (-1, 64, 12)):
        assert lib.ivlm_mesh_sdf_workspace_bytes(*bad) == 0


def test_workspace_is_far_below_one_dense_array_per_pose():
    lib = _lib.load()
    B, N, F = 24, 2048, 13776
    nbytes = lib.ivlm_mesh_sdf_workspace_bytes(B, N, F)
    chunks = -(-F // ms.CHUNK)
    assert nbytes <= B * N * (24 * chunks + 8) + B * 8 * -(-N // 256) + 8 * 256 + 8 * B  # the formula of the header, with its padding
    assert nbytes < (N * F * 4) // 3  # all 24 poses together: a third of ONE pose's dense [N, F] fp32 array (32.2 MB against 112.9 MB)


def test_validation_raises_before_touching_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    v, f = torch.zeros(8, 3), torch.zeros(12, 3, dtype=torch.int32)
    pts = torch.zeros(5, 3)
    with pytest.raises(_lib.IvlmError):  # CPU tensors: no CPU fallback
        ms.MeshSDF(v, f)
    with pytest.raises(_lib.IvlmError):
        ms.penetration_loss(pts, v, f)
    with pytest.raises(_lib.IvlmError):
        ms.mesh_signed_distance(pts, v, f)
    with pytest.raises(ValueError):
        ms.MeshSDF(v.double(), f)
    with pytest.raises(ValueError):
        ms.MeshSDF(v, f.long())
    with pytest.raises(ValueError):
        ms.MeshSDF(torch.zeros(8, 2), f)
    with pytest.raises(ValueError):
        ms.MeshSDF(v, torch.zeros(12, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ms.MeshSDF(v.clone().requires_grad_(True), f)
    with pytest.raises(ValueError):
        ms.MeshSDF([[0.0, 0.0, 0.0]], f)
    with pytest.raises(ValueError):
        ms.penetration_loss(pts.double(), v, f)
    with pytest.raises(ValueError):
        ms.penetration_loss(torch.zeros(5, 2), v, f)
    with pytest.raises(ValueError):
        ms.mesh_signed_distance(torch.zeros(2, 2, 5, 3), v, f)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def cube_sdf(p, half=0.5):
    q = np.abs(p) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


def test_reference_reproduces_the_cube_in_all_27_regions():
    v, f = ref.cube_mesh()
    assert abs(ref.signed_volume(v, f) - 1.0) < 1e-12
    # one generic coordinate per side of each axis: below the cube, within it, above it -> 27 regions (face, edge, corner, inside)
    sides = [(-0.93, 0.11, 0.77), (-0.71, -0.23, 0.88), (-1.2, 0.31, 0.64)]
    pts = np.array([[x, y, z] for x in sides[0] for y in sides[1] for z in sides[2]])
    inner = np.array([[0.41, 0.1, -0.2], [0.43, 0.46, 0.05], [-0.44, -0.47, 0.42], [0.02, -0.03, 0.01]])  # near a face, an edge, a corner, the centre
    pts = np.concatenate([pts, inner])
    r = ref.query(pts, v, f)
    want = cube_sdf(pts)
    assert int((want < 0).sum()) == 5 and int((want > 0).sum()) == 26
    assert np.abs(r["sdf"] - want).max() < 1e-14
    assert np.abs(r["winding"] - (want < 0)).max() < 1e-12
    assert np.abs(np.linalg.norm(r["closest"] - pts, axis=1) - np.abs(want)).max() < 1e-14
    # the fp32 mode is the same function
    r32 = ref.query(pts, v, f, dtype=np.float32)
    assert r32["sdf"].dtype == np.float32 and np.abs(r32["sdf"] - want).max() < 1e-6 and (r32["inside"] == (want < 0)).all()


def test_reference_ignores_zero_area_faces_and_keeps_the_lowest_face_on_ties():
    v, f = ref.named_mesh("body_12_11")
    vz, fz = ref.named_mesh("body_12_11+zero")
    assert len(fz) == len(f) + 2 and ref.corners(vz, fz)[3].sum() == len(f)
    pts = ref.point_cube(centre=(0.0, 0.4, 0.22))
    a, b = ref.query(pts, v, f), ref.query(pts, vz, fz)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    cv, cf = ref.cube_mesh()
    assert ref.query(np.array([[0.9, 0.0, 0.0]]), cv, cf)["face"][0] == 2  # the x = +0.5 side is faces 2 and 3, equidistant here


@pytest.mark.parametrize("centre,seen", [((0.0, 0.4, 0.22), 1.4e-12), ((0.2, -0.5, 0.1), 4.4e-12)])
def test_reference_gradient_matches_central_differences(centre, seen):
    """relative errors seen with h = 1e-5: 1.4e-12 and 4.4e-12; asserted: 1e-8"""
    v, f = (t.numpy() for t in body_mesh(12, 11))
    assert ref.signed_volume(v, f) > 0
    pts = ref.point_cube(centre=centre)
    n, h = pts.shape[0], 1e-5
    L, g, _ = ref.penetration(pts, v, f)
    assert L > 0 and 0 < ref.query(pts, v, f)["inside"].sum() < n
    # L is a sum over points: the derivative in a coordinate of point i needs the term of point i alone
    moved = np.repeat(pts[:, None, None, :], 3, 1).repeat(2, 2)  # [n, axis, sign, 3]
    for ax in range(3):
        moved[:, ax, 0, ax] -= h
        moved[:, ax, 1, ax] += h
    r = ref.query(moved.reshape(-1, 3), v, f)
    term = np.where(r["inside"], r["dd"], 0.0).reshape(n, 3, 2) / n
    fd = (term[:, :, 1] - term[:, :, 0]) / (2 * h)
    rel = np.abs(fd - g).max() / np.abs(g).max()
    print(f"centre {centre}: relative error {rel:.2e} (seen {seen:.1e})")
    assert rel < 1e-8


def test_object_pose_fit_signature():
    params = list(inspect.signature(fit.ObjectPoseFit.__init__).parameters.values())
    assert params[-1].name == "human_faces" and params[-1].default is None
    for fn in (fit.fit_object_pose, fit.search_object_pose):
        named = [p for p in inspect.signature(fn).parameters.values() if p.kind is not inspect.Parameter.VAR_KEYWORD]
        assert named[-1].name == "human_faces" and named[-1].default is None
    assert fit.DEFAULT_LOSS_WEIGHTS == {"mask_loss": {"w": 5.0, "kick_in": 0}, "centroid_loss": {"w": 1e-4, "kick_in": 0},
                                        "contact_loss": {"w": 10.0, "kick_in": 0}}
    assert fit.TERM_KEYS == ("mask_loss", "centroid_loss", "contact_loss")
    weights = {"penetration_loss": {"w": 1.0, "kick_in": 0}}
    with pytest.raises(ValueError, match="penetration_loss"):
        fit.fit_object_pose(*[None] * 8, init=(None, None, 1.0), loss_weights=weights, device_loop=True)
    with pytest.raises(ValueError, match="penetration_loss"):
        fit.search_object_pose(*[None] * 8, loss_weights=weights, device_loop=True)
