"""soft_silhouette / silhouette_terms / fit without a GPU: validation (which raises before the library loads), the fit helpers
against fp64 restatements of the reference's formulas (optim/utils.py), tests/_silhouette_ref.py checked against itself, and the
C symbols of the built library."""
import ctypes
import math
import os

import pytest
import torch

import _silhouette_ref as ref
from interactvlm_amd import _lib, fit
from interactvlm_amd import silhouette as sil
from interactvlm_amd._lib import IvlmError


@pytest.fixture(autouse=True)
def grad_enabled():
    with torch.enable_grad():
        yield


@pytest.fixture
def no_library(monkeypatch):
    """validation must raise before anything touches the library"""
    def boom():
        raise AssertionError("the library was loaded before validation finished")

    monkeypatch.setattr(_lib, "load", boom)


def test_soft_silhouette_refusals(no_library):
    v, f = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    args = (100.0, (8.0, 8.0), (16, 16))
    for bad, match in ((v.double(), "float32"), (v[:, :2], r"\[N,3\]"), (torch.zeros(2, 2, 5, 3), r"\[N,3\]"), ([[0.0, 0.0, 1.0]], "tensor")):
        with pytest.raises(ValueError, match=match):
            sil.soft_silhouette(bad, f, *args)
    for bad, match in ((f.float(), "int32 or int64"), (f[:, :2], r"\[F,3\]"), (f[None], r"\[F,3\]"), (None, "tensor")):
        with pytest.raises(ValueError, match=match):
            sil.soft_silhouette(v, bad, *args)
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            sil.soft_silhouette(v, f, *args, sigma=sigma)
    with pytest.raises(ValueError, match="blur_radius"):
        sil.soft_silhouette(v, f, *args, blur_radius=-1e-3)
    with pytest.raises(ValueError, match="image_size"):
        sil.soft_silhouette(v, f, 100.0, (8.0, 8.0), (0, 16))
    with pytest.raises(ValueError, match="principal"):
        sil.soft_silhouette(v, f, 100.0, (8.0, 8.0, 1.0), (16, 16))
    with pytest.raises(IvlmError, match="GPU tensor"):  # everything else in order: there is no CPU fallback
        sil.soft_silhouette(v, f, *args)
    assert sil.default_blur_radius(1e-4) == pytest.approx(1e-4 * math.log(9999.0))


def test_silhouette_terms_refusals(no_library):
    a = torch.zeros(6, 7)
    for bad, match in ((a.double(), "float32"), (a[0], r"\[H,W\]"), (None, "tensor")):
        with pytest.raises(ValueError, match=match):
            sil.silhouette_terms(bad, a)
    for bad, match in ((torch.zeros(7, 6), "target_mask"), (a.double(), "target_mask"), (torch.zeros(2, 6, 7), "broadcast")):
        with pytest.raises(ValueError, match=match):
            sil.silhouette_terms(a, bad)
    with pytest.raises(IvlmError, match="GPU tensor"):
        sil.silhouette_terms(a, a)


def test_fit_refusals():
    with pytest.raises(ValueError, match="vars"):
        fit.ObjectPoseFit(torch.zeros(1, 6), torch.zeros(1, 3), 1.0, torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 3),
                          torch.zeros(4), torch.zeros(3), torch.zeros(8, 8), 10.0, (4.0, 4.0), vars=("pose", "shape"))
    with pytest.raises(ValueError, match="max_iter"):
        fit.fit_object_pose(None, None, None, None, None, None, 1.0, (0.0, 0.0), max_iter=0)


# ---- the fit helpers against the reference's formulas, restated in fp64 ------------------------------------------------------------
def _rot6d_to_matrix64(r6):
    """optim/utils.py rot6d_to_matrix: view(-1, 3, 2), Gram-Schmidt of the two columns, stack on the last axis"""
    r6 = r6.double().reshape(-1, 3, 2)
    a1, a2 = r6[:, :, 0], r6[:, :, 1]
    b1 = a1 / a1.norm(dim=1, keepdim=True)
    u2 = a2 - (b1 * a2).sum(1, keepdim=True) * b1
    b2 = u2 / u2.norm(dim=1, keepdim=True)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=1)), dim=-1)


def test_rot6d_round_trip_and_orthonormality():
    r6 = torch.randn(5, 6, generator=torch.Generator().manual_seed(0))
    R = fit.rot6d_to_matrix(r6)
    assert R.shape == (5, 3, 3)
    assert torch.allclose(R.double(), _rot6d_to_matrix64(r6), atol=1e-6)
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3).expand(5, 3, 3), atol=1e-6)
    assert torch.allclose(torch.linalg.det(R), torch.ones(5), atol=1e-6)
    # a rotation survives the round trip; its 6-D form is its first two columns, interleaved
    back = fit.rot6d_to_matrix(fit.matrix_to_rot6d(R))
    assert torch.allclose(back, R, atol=1e-6)
    assert torch.equal(fit.matrix_to_rot6d(R)[2], torch.stack((R[2, :, 0], R[2, :, 1]), -1).reshape(6))
    assert torch.equal(fit.matrix_to_rot6d(torch.eye(3))[0], torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]))


def test_apply_transformation_is_row_vector():
    g = torch.Generator().manual_seed(1)
    v, r6, t = torch.randn(7, 3, generator=g), torch.randn(3, 6, generator=g), torch.randn(3, 3, generator=g)
    s = torch.tensor([1.0, 0.5, 2.0])
    want = torch.stack([(v.double() * float(s[b])) @ _rot6d_to_matrix64(r6[b])[0] + t[b].double() for b in range(3)])
    got = fit.apply_transformation(v, r6, t, s)
    assert got.shape == (3, 7, 3)
    assert torch.allclose(got.double(), want, atol=1e-5)
    for b in range(3):  # a pose of the batch is its own unbatched call, bit for bit
        assert torch.equal(fit.apply_transformation(v, r6[b], t[b], s[b]), got[b])
    # x R, not R x: the row-vector product takes +x to R's first ROW
    R = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = fit.apply_transformation(torch.tensor([[1.0, 0.0, 0.0]]), fit.matrix_to_rot6d(R)[0], torch.zeros(3))
    assert torch.allclose(out, R[0][None])


def test_mask_bbox_centre():
    m = torch.zeros(9, 12)
    m[2:5, 3:10] = 1
    m[6, 4] = 1
    assert fit.mask_bbox_centre(m).tolist() == [4.0, 6.0]  # (min + max) / 2 of the non-zero (row, col) indices
    assert fit.mask_bbox_centre(torch.zeros(9, 12)).tolist() == [4.5, 6.0]


# ---- the definition against itself -----------------------------------------------------------------------------------------------
def test_ref_closed_form_gradient_matches_autograd():
    """d alpha / d s_k = -(1 - alpha) p_k / sigma, chained by hand through d and the projection, against autograd of the definition"""
    verts, faces, cam, blur, x = ref.case(6, 8, 40, 48, 4e-3, 3.0)
    g = torch.randn(cam.H, cam.W, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    v = verts.double().requires_grad_(True)
    (ref.render(v, faces, cam, 4e-3, blur) * g).sum().backward()
    # by hand: dL/dd = g d alpha / d s_k (+/- kappa); d d / d(edge start) = -2 (1 - t) r, d d / d(edge end) = -2 t r
    dLdd = g.reshape(-1, 1) * ref.dalpha_dsk(x) * x.kappa * (1 - 2 * x.inside.double())
    guv = torch.zeros(verts.shape[0], 2, dtype=torch.float64)
    P, F = x.d.shape
    for coef, corner in ((1 - x.t, x.m), (x.t, (x.m + 1) % 3)):
        vert = faces[torch.arange(F)[None].expand(P, F), corner]
        guv.index_add_(0, vert.reshape(-1), ((dLdd * -2 * coef)[..., None] * x.r).reshape(-1, 2))
    X, Y, Z = verts.double().unbind(-1)
    by_hand = torch.stack((guv[:, 0] * cam.fx / Z, guv[:, 1] * cam.fy / Z, -(guv[:, 0] * cam.fx * X + guv[:, 1] * cam.fy * Y) / Z ** 2), -1)
    assert float(v.grad.abs().max()) > 1
    assert torch.allclose(by_hand, v.grad, rtol=1e-9, atol=1e-9 * float(v.grad.abs().max()))


def test_ref_covering_triangle_is_opaque():
    cam = ref.camera(24, 32)
    z = 3.0
    uv = torch.tensor([(-4000.0, -3000.0), (5000.0, -3000.0), (16.0, 6000.0)], dtype=torch.float64)
    verts = torch.stack(((uv[:, 0] - cam.px) * z / cam.fx, (uv[:, 1] - cam.py) * z / cam.fy, torch.full((3,), z, dtype=torch.float64)), -1)
    alpha = ref.render(verts, torch.tensor([[0, 1, 2]]), cam, 1e-4)
    assert float((1 - alpha).abs().max()) <= 1e-12


def test_ref_union_quirk_and_centroid_units():
    alpha = torch.zeros(5, 7, dtype=torch.float64)
    alpha[1, 2], alpha[3, 6] = 0.5, 1.0
    target = torch.zeros(5, 7)
    target[3, 6] = target[0, 0] = 1
    loss, c = ref.terms(alpha, target)
    # "union" is sum(alpha + target) = 1.5 + 2, not the area of the union: an exact match would still lose 1/2
    assert float(loss) == pytest.approx(1 - 1.0 / 3.5)
    assert float(ref.terms(target.double(), target)[0]) == pytest.approx(0.5)
    # integer (row, col) index units, no half-pixel offset
    assert c.tolist() == pytest.approx([(1 * 0.5 + 3 * 1.0) / 1.5, (2 * 0.5 + 6 * 1.0) / 1.5])
    assert ref.terms(torch.zeros(5, 7, dtype=torch.float64), target)[1].tolist() == [2.5, 3.5]


def test_ref_scene_table():
    """the scenes are what the table says they exercise"""
    for (nlat, nlon, H, W, sigma), n_faces in zip(ref.SCENES, (80, 80, 352, 1472, 168)):
        verts, faces, cam, blur, x = ref.case(nlat, nlon, H, W, sigma, None)
        assert faces.shape[0] == n_faces and int(faces.max()) == verts.shape[0] - 1
        assert math.sqrt(x.blur / x.kappa) == pytest.approx(math.sqrt(sigma * math.log(9999.0)) * min(H, W) / 2)
    assert int(ref.case(24, 32, 64, 64, 1e-3, None)[4].counted.sum(1).max()) > 150
    x = ref.case(8, 12, 130, 97, 1e-3, None)[4]
    assert not bool(x.counted.reshape(130, 97, -1)[:16, :16].any())  # a tile the object never reaches


def test_abi_symbols_present():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.header_prototypes()
    for name in ("ivlm_soft_silhouette_workspace_bytes", "ivlm_soft_silhouette_forward", "ivlm_soft_silhouette_backward",
                 "ivlm_silhouette_terms"):
        assert name in protos, f"{name} is not declared in include/ivlm_hip.h"
        assert hasattr(lib, name), f"libivlm_hip.so does not export {name}"
    txt = open(_lib.HEADER_PATH).read()
    for const, value in (("IVLM_SILHOUETTE_CHAIN", sil.L_CHAIN), ("IVLM_SILHOUETTE_POS_ULPS", sil.POS_ULPS), ("IVLM_SILHOUETTE_REL_ULPS", sil.REL_ULPS),
                         ("IVLM_SILHOUETTE_EXP_ULPS", sil.EXP_ULPS), ("IVLM_SILHOUETTE_T_ULPS", sil.T_ULPS),
                         ("IVLM_SILHOUETTE_TERMS_CHAIN", sil.TERMS_CHAIN)):
        assert f"#define {const} {value}\n" in txt, f"{const} of the header and interactvlm_amd.silhouette differ"
    assert f"#define IVLM_SILHOUETTE_TERMS_WORKSPACE(B, H) ((size_t)(B) * (size_t)(H) * {sil.TERMS_WORKSPACE_ROW_BYTES})\n" in txt
    lib.ivlm_soft_silhouette_workspace_bytes.restype = ctypes.c_size_t
    assert lib.ivlm_soft_silhouette_workspace_bytes(2, 100, 200, 64, 48) >= 2 * (4 * 64 * 48 + 72 * 200 + 8 * 100)
    assert lib.ivlm_soft_silhouette_workspace_bytes(1, 100, 200, 1 << 20, 48) == 0


# ---- the topology cache ----------------------------------------------------------------------------------------------------------
def _expected_topology(faces, n):
    flat = faces.reshape(-1).tolist()
    lists = [[] for _ in range(n)]
    for slot, v in enumerate(flat):
        lists[v].append(slot)
    offsets = [0]
    for l in lists:
        offsets.append(offsets[-1] + len(l))
    return offsets, [slot for l in lists for slot in l]


def test_topology_cache_belongs_to_one_tensor():
    """a freed faces tensor's entry can never serve another mesh of the same shape, whatever address the allocator gives it"""
    n, gen = 50, torch.Generator().manual_seed(0)
    sil._topology.clear()
    for _ in range(40):
        a = torch.randint(n, (400, 3), generator=gen)
        f32, offsets, slots = sil._topology_of(a, n)
        assert torch.equal(f32.long(), a)
        want_off, want_slots = _expected_topology(a, n)
        assert offsets.tolist() == want_off and slots.tolist() == want_slots
        assert sil._topology_of(a, n)[0] is f32  # the same tensor object, unchanged: a hit
        del a
        assert len(sil._topology) == 0  # the entry went with its tensor
    # a write the version counter sees, and another N, rebuild; out-of-range indices are refused on every path
    a = torch.randint(n, (400, 3), generator=gen)
    first = sil._topology_of(a, n)
    a[7, 1] = (int(a[7, 1]) + 1) % n
    second = sil._topology_of(a, n)
    assert second[0] is not first[0] and torch.equal(second[0].long(), a)
    assert sil._topology_of(a, n + 3)[1].shape[0] == n + 4
    a[3, 2] = n
    with pytest.raises(ValueError, match="vertex indices"):
        sil._topology_of(a, n)
    # at most _TOPOLOGY_MAX live entries, the oldest leaves first
    keep = [torch.randint(n, (10, 3), generator=gen) for _ in range(sil._TOPOLOGY_MAX + 3)]
    for t in keep:
        sil._topology_of(t, n)
    assert len(sil._topology) == sil._TOPOLOGY_MAX
    assert id(keep[0]) not in sil._topology and id(keep[-1]) in sil._topology
    sil._topology.clear()
