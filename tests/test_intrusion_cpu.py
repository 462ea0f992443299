"""The intrusion term without a GPU: the C ABI declares the two entry points and still is version 5, the calls refuse bad arguments
and short workspaces before touching a device, the workspace formula, the yardstick of the GPU tests (tests/_intrusion_ref.py) checked
against central differences, a hand-computed cube case and a rigid motion of the whole scene, ``check_closed``, and the fit's
signatures and refusals."""
import inspect

import numpy as np
import pytest
import torch

import _intrusion_ref as ir
import _mesh_sdf_ref as ref
from interactvlm_amd import _lib, fit
from interactvlm_amd import mesh_sdf as ms

INT = "intrusion_loss"


def test_header_declares_the_entry_points_and_the_abi_is_still_5():
    protos = _lib.header_prototypes()
    assert protos["ivlm_mesh_sdf_intrusion_workspace_bytes"] == ("size_t", ["int B", "int N", "int F"])
    ret, args = protos["ivlm_mesh_sdf_intrusion"]
    assert ret == "int" and len(args) == 14
    assert [a.split()[-1].lstrip("*") for a in args] == ["plan", "points", "rot6d", "translation", "scale", "B", "N", "value", "grad_rot6d",
                                                         "grad_translation", "grad_scale", "workspace", "workspace_bytes", "stream"]
    assert _lib.load().ivlm_abi_version() == 5
    assert callable(ms.MeshSDF.intrusion) and callable(ms.check_closed)


def test_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    call = lib.ivlm_mesh_sdf_intrusion
    fake = 4096  # pointers that are never followed: the refusals below come before any launch
    big = 1 << 20
    assert call(None, None, None, None, None, 1, 4, None, None, None, None, None, 0, None) == -1
    ok = [fake, fake, fake, fake, fake, 1, 4, fake, None, None, None, fake, big, None]
    for at in (0, 1, 2, 3, 4, 7, 11):  # plan, points, rot6d, translation, scale, value, workspace
        bad = list(ok)
        bad[at] = None
        assert call(*bad) == -1, at
    for at, v in ((5, 0), (5, -1), (6, 0), (6, -4)):
        bad = list(ok)
        bad[at] = v
        assert call(*bad) == -1, (at, v)
    bad = list(ok)
    bad[0] = fake + 8  # a plan off its 16-byte alignment
    assert call(*bad) == -1
    # short workspaces: nothing, the penetration's own size (no room for x and the partials), one byte less than one chunk's
    one_chunk = lib.ivlm_mesh_sdf_intrusion_workspace_bytes(1, 4, 12)
    for nbytes in (0, 64, lib.ivlm_mesh_sdf_workspace_bytes(1, 4, 12), one_chunk - 1):
        bad = list(ok)
        bad[12] = nbytes
        assert call(*bad) == -2, nbytes
    bad = list(ok)
    bad[11] = fake + 4  # a workspace off its alignment
    assert call(*bad) == -2
    bad = list(ok)
    bad[6] = (1 << 20) + 1  # N beyond the limit
    bad[12] = 1 << 40
    assert call(*bad) == -4


def test_workspace_formula():
    lib = _lib.load()
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    for B, N, F in ((1, 1, 4), (3, 257, 516), (24, 6890, 500), (2, 1025, 13776)):
        base = lib.ivlm_mesh_sdf_workspace_bytes(B, N, F)
        assert lib.ivlm_mesh_sdf_intrusion_workspace_bytes(B, N, F) == base + pad(12 * B * N) + pad(14 * 8 * B * -(-N // 256))
    for bad in ((0, 64, 12), (1, 0, 12), (1, 64, 0), (-1, 64, 12), (1, (1 << 20) + 1, 12), (65536, 64, 12)):
        assert lib.ivlm_mesh_sdf_intrusion_workspace_bytes(*bad) == 0


def test_validation_raises_before_touching_the_library(monkeypatch):
    mesh = object.__new__(ms.MeshSDF)  # no constructor: it would need a GPU; validation comes before the mesh is looked at
    mesh.device, mesh.num_faces = torch.device("cpu"), 12

    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    pts, r6, t = torch.zeros(5, 3), torch.tensor([ir.IDENTITY6]), torch.zeros(1, 3)
    with pytest.raises(_lib.IvlmError):  # CPU tensors: no CPU fallback
        mesh.intrusion(pts, r6, t, 1.0)
    with pytest.raises(ValueError, match="requires_grad"):
        mesh.intrusion(pts.clone().requires_grad_(True), r6, t, 1.0)
    for bad in (pts.double(), torch.zeros(2, 5, 3), torch.zeros(5, 2), torch.zeros(0, 3), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match="points"):
            mesh.intrusion(bad, r6, t, 1.0)
    with pytest.raises(ValueError, match="rot6d"):
        mesh.intrusion(pts, torch.zeros(1, 5), t, 1.0)
    with pytest.raises(ValueError, match="rot6d"):
        mesh.intrusion(pts, r6.double(), t, 1.0)
    with pytest.raises(ValueError, match="translation"):
        mesh.intrusion(pts, r6, torch.zeros(2, 3), 1.0)
    with pytest.raises(ValueError, match="translation"):
        mesh.intrusion(pts, r6[0], t, 1.0)  # one pose: [6] goes with [3]
    with pytest.raises(ValueError, match="scaling"):
        mesh.intrusion(pts, r6, t, torch.ones(2))
    with pytest.raises(ValueError, match="scaling"):
        mesh.intrusion(pts, r6, t, float("nan"))


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def central(fn, n, h=1e-6):
    out = []
    for i in range(n):
        d = np.zeros(n)
        d[i] = h
        out.append((fn(d) - fn(-d)) / (2 * h))
    return np.array(out)


def test_reference_reproduces_the_numbers_of_the_issue():
    hv, hf, cv, cf = ir.fit_scene()
    w = ir.intrusion(hv, ir.IDENTITY6, ir.CUBE_CENTRE, 1.0, cv, cf, unique=True)
    world = ir.forward_pose(cv, ir.IDENTITY6, ir.CUBE_CENTRE, 1.0)
    assert int(ref.query(world, hv, hf)["inside"].sum()) == 0  # the penetration term sees nothing
    assert len(hv) == 134 and int(w["inside"].sum()) == 25
    assert abs(w["L"] - 1.6228e-3) < 5e-8 and w["r"]["unique"][w["inside"]].all() and abs(w["r"]["d"].min() - 5.1e-3) < 5e-5


def test_reference_gradients_match_central_differences():
    """h = 1e-6, a rotated and scaled pose (s = 1.1), 27 points inside.  Relative errors seen: translation 3.5e-11, scale 7.5e-11,
    rot6d 1.1e-9; asserted: 1e-6"""
    hv, _, cv, cf = ir.fit_scene()
    r6 = ir.axis_angle_rot6d((1, 2, 3), 0.3, (1.2, 0.9), 0.2).astype(np.float64)
    t, s = np.array(ir.CUBE_CENTRE), 1.1
    w = ir.intrusion(hv, r6, t, s, cv, cf)
    assert int(w["inside"].sum()) == 27
    gt = central(lambda d: ir.value_only(hv, r6, t + d, s, cv, cf), 3)
    gs = central(lambda d: ir.value_only(hv, r6, t, s + d[0], cv, cf), 1)
    gr = central(lambda d: ir.value_only(hv, r6 + d, t, s, cv, cf), 6)
    rel = (np.abs(gt - w["g_t"]).max() / np.abs(gt).max(), abs(gs[0] - w["g_s"]) / abs(gs[0]), np.abs(gr - w["g_r6"]).max() / np.abs(gr).max())
    print("relative errors (translation, scale, rot6d):", rel)
    assert max(rel) < 1e-6
    assert np.abs(w["g_r6"]).min() > 0 and abs(w["g_s"]) > 0
    # the Jacobian the rot6d tolerance scale is built from, against central differences of R itself
    J = ir.rotation_jacobian(r6)
    for m in range(6):
        d = np.zeros(6)
        d[m] = 1e-6
        fd = (ir.gram_schmidt(r6 + d)[0] - ir.gram_schmidt(r6 - d)[0]) / 2e-6
        assert np.abs(J[m] - fd).max() < 1e-8


def test_reference_on_a_hand_computed_cube_case():
    """The unit cube (half 0.5), s = 2, a quarter turn about z (row vectors: x R = (-x_1, x_0, x_2)), t = (1, 2, 3).  The canonical
    point x = (0.1, 0.2, 0.4) lies 0.1 under the face z = 0.5: c = (0.1, 0.2, 0.5), h = 2 (-0.2, 0.1, 0.4) + t = (0.6, 2.2, 3.8),
    e = 2 (0, 0, -0.1) R = (0, 0, -0.2).  N = 1: L = 0.04;  dL/dt = -2 e = (0, 0, 0.4);  dL/ds = -2 e . (c R) = -2 (-0.2)(0.5) = 0.2
    (also d/ds (0.5 s - 0.8)^2 at 2);  dL/dR = -2 s c^T e has the one column (0.08, 0.16, 0.4) at k = 2, i.e. gb3; with
    b1 = (0, -1, 0), b2 = (1, 0, 0) already orthonormal: gb1 = b2 x gb3 = (0, -0.4, 0.16), gb2 = gb3 x b1 = (0.4, 0, -0.08),
    ga2 = gb2 - b2 (b2 . gb2) = (0, 0, -0.08), ga1 = gb1 - b1 (b1 . gb1) = (0, 0, 0.16): rot6d gradient (0, 0, 0, 0, 0.16, -0.08)."""
    v, f = ref.cube_mesh()
    r6 = np.array([0.0, 1.0, -1.0, 0.0, 0.0, 0.0])
    R, _ = ir.gram_schmidt(r6)
    assert np.array_equal(R, np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))
    t, s = np.array([1.0, 2.0, 3.0]), 2.0
    h = np.array([[0.6, 2.2, 3.8]])
    assert np.abs(ir.forward_pose(np.array([[0.1, 0.2, 0.4]]), r6, t, s) - h).max() < 1e-15
    w = ir.intrusion(h, r6, t, s, v, f)
    assert w["inside"].all() and np.abs(w["x"] - [0.1, 0.2, 0.4]).max() < 1e-15
    assert abs(w["L"] - 0.04) < 1e-12 and abs(w["A"] - 0.04) < 1e-12
    assert np.abs(w["g_t"] - [0.0, 0.0, 0.4]).max() < 1e-12
    assert abs(w["g_s"] - 0.2) < 1e-12
    assert np.abs(w["g_r6"] - [0.0, 0.0, 0.0, 0.0, 0.16, -0.08]).max() < 1e-12
    # the tolerance scales of this case: |e| = 0.2;  |de/dt| = 1;  |de/ds| = |c|
    assert abs(w["s_t"] - 0.4) < 1e-12 and abs(w["s_s"] - 0.4 * np.sqrt(0.3)) < 1e-12
    # the fp32 mode is the same function
    w32 = ir.intrusion(h.astype(np.float32), r6, t, s, v, f, dtype=np.float32)
    assert w32["L"].dtype == np.float32 and abs(float(w32["L"]) - 0.04) < 1e-7 and np.abs(w32["g_r6"] - w["g_r6"]).max() < 1e-6


def test_reference_is_invariant_under_a_rigid_motion_of_the_whole_scene():
    hv, _, cv, cf = ir.fit_scene()
    r6 = ir.axis_angle_rot6d((1, 2, 3), 0.3).astype(np.float64)
    t, s = np.array(ir.CUBE_CENTRE), 1.1
    L = ir.intrusion(hv, r6, t, s, cv, cf)["L"]
    Q, _ = ir.gram_schmidt(ir.axis_angle_rot6d((-2, 1, 0.5), 1.9).astype(np.float64))
    tau = np.array([0.3, -1.2, 2.0])
    R, _ = ir.gram_schmidt(r6)
    RQ = R @ Q  # y Q + tau = (s v) (R Q) + (t Q + tau)
    moved = ir.intrusion(hv.astype(np.float64) @ Q + tau, np.stack([RQ[:, 0], RQ[:, 1]], 1).reshape(6), t @ Q + tau, s, cv, cf)
    assert L > 1e-4 and int(moved["inside"].sum()) == 27
    assert abs(moved["L"] - L) < 1e-12 * max(1.0, L)


def test_gpu_test_inputs_have_inside_points_and_flip_no_sign_in_fp32():
    """a sample of the GPU cases (the helper's __main__ runs them all)"""
    for name, n, b in (("tetra", 65, 3), ("cube", 257, 3), (ir.mesh_names(ms.TILE, ms.CHUNK)[-1], 64, 3)):
        v, f, h, poses, want = ir.make_case(name, n, b)
        assert all(0 < int(w["inside"].sum()) < n for w in want)  # every pose has points inside and points outside
        for (r6, t, s), w in zip(poses, want):
            got = ir.intrusion(h, r6, t, s, v, f, dtype=np.float32)
            assert np.array_equal(got["inside"], w["inside"])
    assert sorted(float(p[2]) for p in ir.POSES) == [np.float32(0.7), 1.0, np.float32(1.6)]


# ---- check_closed -----------------------------------------------------------------------------------------------------------------
def test_check_closed_passes_closed_outward_meshes():
    for name in ("cube", "tetra", "body_12_11"):
        v, f = ref.named_mesh(name)
        assert ms.check_closed(v, f) is None
        assert ms.check_closed(torch.from_numpy(v), torch.from_numpy(f)) is None


def test_check_closed_names_the_first_defect():
    v, f = ref.cube_mesh()
    with pytest.raises(ValueError, match="no reverse"):
        ms.check_closed(v, f[:-1])  # the cube minus one face
    one = f.copy()
    one[3] = one[3, ::-1]
    with pytest.raises(ValueError, match="occurs 2 times"):
        ms.check_closed(v, one)  # one face flipped
    with pytest.raises(ValueError, match="signed volume"):
        ms.check_closed(v, f[:, ::-1].copy())  # all faces flipped
    with pytest.raises(ValueError, match="repeats an index"):
        ms.check_closed(*ref.named_mesh("body_12_11+zero"))
    with pytest.raises(ValueError, match="indices"):
        ms.check_closed(v[:7], f)
    with pytest.raises(ValueError, match="faces"):
        ms.check_closed(v, f.astype(np.float32))


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def test_fit_signatures_and_keys():
    assert fit.INTRUSION_KEY == INT and INT not in fit.DEFAULT_LOSS_WEIGHTS and INT not in fit.TERM_KEYS
    for fn in (fit.ObjectPoseFit.__init__, fit.fit_object_pose, fit.search_object_pose):
        p = inspect.signature(fn).parameters
        assert "intrusion" in p and p["intrusion"].default is False


def test_fit_refusals_raise_before_the_library_loads(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    weights = {INT: {"w": 1.0, "kick_in": 0}}
    with pytest.raises(ValueError, match=INT):
        fit.fit_object_pose(*[None] * 8, init=(None, None, 1.0), loss_weights=weights, device_loop=True, intrusion=True)
    with pytest.raises(ValueError, match=INT):
        fit.search_object_pose(*[None] * 8, loss_weights=weights, device_loop=True, intrusion=True)
    with pytest.raises(ValueError, match=INT):
        fit.DevicePoseFit(*[None] * 11, loss_weights=weights)
    with pytest.raises(ValueError, match="penetration_loss"):  # the older refusal is unchanged
        fit.fit_object_pose(*[None] * 8, init=(None, None, 1.0), loss_weights={"penetration_loss": {"w": 1.0, "kick_in": 0}},
                            device_loop=True)
    # intrusion=True checks the object on the host before anything is prepared: an open cube is refused by name
    v, f = ref.cube_mesh(half=0.2)
    hv = torch.zeros(4, 3)
    args = (torch.tensor([ir.IDENTITY6]), torch.zeros(1, 3), 1.0, torch.from_numpy(v), torch.from_numpy(f[:-1]), hv, torch.zeros(8),
            torch.zeros(4), torch.zeros(8, 8), (10.0, 10.0), (4.0, 4.0))
    with pytest.raises(ValueError, match="no reverse"):
        fit.ObjectPoseFit(*args, intrusion=True)
    # on, on a model built without intrusion=True (CPU tensors: the refusal comes before any kernel)
    model = fit.ObjectPoseFit(*args)
    assert model.object_sdf is None
    with pytest.raises(ValueError, match="intrusion"):
        model(weights)
