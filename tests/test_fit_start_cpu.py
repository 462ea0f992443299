"""interactvlm_amd.fit_start without a GPU: every refusal by name before the library loads, ``osx_camera`` against its restatement,
the self-checks that pin tests/_fit_start_ref.py's definitions to closed forms, the intent mode's geometry, the chain fixture's
conditions on the restatement alone, and the host-only part of the C ABI (workspace sizes, invalid arguments)."""
import ctypes

import pytest
import torch

import _fit_start_ref as ref
import _silhouette_ref as sil_ref
from interactvlm_amd import _lib, fit_start as fs
from interactvlm_amd._lib import IvlmError

V, F = torch.zeros(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]])
HV, HF = torch.zeros(7, 3), torch.tensor([[0, 1, 2], [4, 5, 6]])
P5, P7 = torch.zeros(5), torch.zeros(7)
MASK = torch.ones(4, 6, dtype=torch.uint8)
CAM = ((50.0, 51.0), (3.0, 2.0))


@pytest.fixture
def no_library(monkeypatch):
    """a refusal must come before the library loads"""
    def load():
        raise AssertionError("the library was loaded before the argument checks were through")
    monkeypatch.setattr(_lib, "load", load)


def refused(match, fn, *args, **kwargs):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kwargs)


def test_refusals_mesh_functions(no_library):
    for fn in (fs.vertex_normals, fs.surface_centroid):
        refused("verts", fn, torch.zeros(5), F)
        refused("verts", fn, torch.zeros(2, 5, 3), F)  # no batch axis
        refused("verts", fn, V.double(), F)
        refused("verts", fn, [[0.0, 0.0, 0.0]], F)
        refused("faces", fn, V, torch.zeros(2, 4, dtype=torch.int64))
        refused("faces", fn, V, F.float())
        refused("faces", fn, V, torch.zeros(0, 3, dtype=torch.int64))
        refused("faces", fn, V, [[0, 1, 2]])
    refused("human_vertices", fs.centre_meshes, HV.half(), HF, V, F)
    refused("human_faces", fs.centre_meshes, HV, HF.float(), V, F)
    refused("obj_vertices", fs.centre_meshes, HV, HF, torch.zeros(5, 2), F)
    refused("obj_faces", fs.centre_meshes, HV, HF, V, torch.zeros(3, dtype=torch.int64))


def test_refusals_mask_and_depth(no_library):
    refused("mask", fs.mask_stats, torch.ones(4))
    refused("mask", fs.mask_stats, torch.ones(2, 4, 6))
    refused("mask", fs.mask_stats, torch.ones(4, 6, dtype=torch.complex64))
    refused("mask", fs.mask_stats, [[1, 0]])
    refused("verts", fs.contact_depth, torch.zeros(5, 2), P5, 0.5)
    refused("probs", fs.contact_depth, V, P7, 0.5)
    refused("probs", fs.contact_depth, V, P5.double(), 0.5)
    refused("threshold", fs.contact_depth, V, P5, float("nan"))
    refused("threshold", fs.contact_depth, V, P5, "0.5")


def test_refusals_centroid_start(no_library):
    ok = dict(mask=MASK, human_vertices=HV, human_contact_probs=P7, focal=CAM[0], principal=CAM[1])
    for key, bad, name in (("mask", torch.ones(4), "mask"), ("human_vertices", torch.zeros(7, 4), "human_vertices"),
                           ("human_contact_probs", P5, "human_contact_probs"), ("human_contact_probs", P7.half(), "human_contact_probs"),
                           ("focal", (1.0, 2.0, 3.0), "focal"), ("focal", float("inf"), "focal"), ("focal", "f", "focal"),
                           ("principal", 3.0, "principal"), ("principal", torch.zeros(3), "principal"),
                           ("hum_centroid_offset", torch.zeros(2), "hum_centroid_offset"),
                           ("hum_centroid_offset", torch.zeros(3, dtype=torch.float64), "hum_centroid_offset"),
                           ("threshold", None, "threshold")):
        refused(name, fs.centroid_start, **{**ok, key: bad})


def test_refusals_reference_start(no_library):
    ok = dict(obj_vertices=V, obj_faces=F, human_vertices=HV, human_faces=HF, obj_contact_probs=P5, human_contact_probs=P7,
              target_mask=MASK, focal=CAM[0], principal=CAM[1])
    for key, bad, name in (("obj_vertices", V.double(), "obj_vertices"), ("obj_faces", F.float(), "obj_faces"),
                           ("human_vertices", torch.zeros(7), "human_vertices"), ("human_faces", None, "human_faces"),
                           ("obj_contact_probs", P7, "obj_contact_probs"), ("human_contact_probs", P5, "human_contact_probs"),
                           ("target_mask", torch.ones(4), "target_mask"), ("focal", None, "focal"), ("principal", (1.0,), "principal"),
                           ("hum_centroid_offset", torch.zeros(4), "hum_centroid_offset"), ("scale", float("nan"), "scale"),
                           ("thresholds", 0.3, "thresholds"), ("thresholds", (0.3, None), "thresholds"),
                           ("filter_contacts", (True,), "filter_contacts"), ("filter_contacts", (True, "x"), "filter_contacts"),
                           ("filter_contacts", 90, "filter_contacts"), ("icp_max_iterations", 0, "icp_max_iterations"),
                           ("obj_normals", torch.zeros(4, 3), "obj_normals"), ("human_normals", HV.double(), "human_normals")):
        refused(name, fs.reference_start, **{**ok, key: bad})


def test_cpu_tensors_fail_loudly():
    """after the checks: no CPU fallback"""
    with pytest.raises(IvlmError):
        fs.vertex_normals(V, F)
    with pytest.raises(IvlmError):
        fs.surface_centroid(V, F)
    with pytest.raises(IvlmError):
        fs.mask_stats(MASK)
    with pytest.raises(IvlmError):
        fs.contact_depth(V, P5, 0.5)
    with pytest.raises(IvlmError):
        fs.centroid_start(MASK, HV, P7, *CAM)
    with pytest.raises(IvlmError):
        fs.reference_start(V, F, HV, HF, P5, P7, MASK, *CAM)


@pytest.mark.parametrize("bbox", [(120.0, 40.0, 210.0, 380.0), (13.25, 701.5, 97.0, 133.0)])
def test_osx_camera_against_the_restatement(bbox):
    focal, principal = fs.osx_camera(torch.tensor(bbox))
    want_f, want_p = ref.osx_camera(bbox)
    assert focal.dtype == torch.float32 and tuple(focal.shape) == (2,) and tuple(principal.shape) == (2,)
    assert [float(v) for v in focal] == [float(v) for v in want_f]
    assert [float(v) for v in principal] == [float(v) for v in want_p]
    again = fs.osx_camera(list(bbox))
    assert torch.equal(again[0], focal) and torch.equal(again[1], principal)
    with pytest.raises(ValueError, match="bbox"):
        fs.osx_camera((1.0, 2.0, 3.0))


def test_restatement_normals_on_the_sphere():
    """On the unit icosphere the fp64 normal of every vertex is its position, within 1e-12.  That is a theorem only where the ring of
    a vertex is symmetric about it - the icosahedron, the icosphere before any subdivision: the sum over a closed ring p_0 .. p_k-1 of
    cross(p_i - v, p_i+1 - v) is sum_i cross(p_i, p_i+1), twice the vector area of the ring, whatever v.  After a subdivision the
    rings are no longer symmetric and the area-weighted normal leaves the radius by up to 2e-2.  So the icosahedron is held to the
    issue's statement, and the subdivided sphere to the identity itself, which is the same check of the restatement for every ring."""
    v, f = ref.icosphere(0)
    assert tuple(v.shape) == (12, 3) and float((v.norm(dim=1) - 1).abs().max()) <= 1e-15
    assert float((ref.normals(v, f) - v).abs().max()) <= 1e-12
    v, f = ref.icosphere(2)
    assert tuple(v.shape) == (162, 3) and tuple(f.shape) == (320, 3)
    n = ref.normals(v, f)
    area = torch.zeros(162, 3, dtype=torch.float64)
    for k in range(3):  # the ring edge opposite corner k, in the face's orientation
        area.index_add_(0, f[:, k], torch.linalg.cross(v[f[:, (k + 1) % 3]], v[f[:, (k + 2) % 3]]))
    assert float((n - area / area.norm(dim=1, keepdim=True)).abs().max()) <= 1e-12
    assert float((n * v).sum(1).min()) > 0.99  # outward


def test_restatement_centroid_of_a_cube():
    for n in (1, 4):
        v, f = ref.box(n, (0.5, 0.3, 0.2))
        centre = torch.tensor([0.25, -1.5, 3.0], dtype=torch.float64)
        assert float((ref.centroid(v + centre, f) - centre).abs().max()) <= 1e-12
    v, f = ref.tetrahedron()  # (regular: the surface centroid is the vertex mean)
    assert float((ref.centroid(v, f) - v.mean(0)).abs().max()) <= 1e-12


@pytest.mark.parametrize("k", [0, 1, 2])
def test_intent_mode_lands_on_the_mean_pixel(k):
    H, W = ((48, 64), (120, 90), (33, 257))[k]
    cam = sil_ref.camera(H, W)
    focal, principal = (cam.fx, cam.fy * (1.0 + 0.03 * k)), (cam.px, cam.py)
    offset = [torch.tensor([0.1, -0.05, 3.0]), torch.tensor([-0.4, 0.3, 2.2]), torch.zeros(3)][k]
    mask = ref.blob_mask(H, W, (0.4 * H, 0.6 * W), (0.2 * H, 0.15 * W))
    z = (-0.11, 0.07, 1.9)[k]
    T = ref.stage1_intent(mask, z, focal, principal, offset)
    st = ref.mask_stats(mask)
    u, v = ref.project(T + offset.double(), focal, principal)
    # the centre of the mean pixel, in the convention of the silhouette: pixel (row i, col j) has its centre at (j + 0.5, i + 0.5)
    assert abs(float(u) - (st["col_sum"] / st["count"] + 0.5)) <= 1e-9
    assert abs(float(v) - (st["row_sum"] / st["count"] + 0.5)) <= 1e-9
    assert abs(float(T[2] + offset[2].double()) - (z + float(offset[2]))) <= 1e-12


def test_restatement_stage1_reads_pixels_not_columns():
    """``nonzero(mask)[1]`` is the second pixel: a mask whose first two pixels are (1, 4) and (2, 0) gives cx from (2 + 0) / 2"""
    mask = torch.zeros(4, 6)
    mask[1, 4] = mask[2, 0] = mask[3, 3] = 1
    hv = torch.tensor([[0.0, 0.0, 0.5], [0.0, 0.0, 1.5], [0.0, 0.0, 9.0]])
    T = ref.stage1_mirror(mask, hv, torch.tensor([0.9, 0.6, 0.5]), (8.0, 16.0), (0.25, 0.5))
    assert [float(t) for t in T] == [(1.0 - 0.25) * 1.0 / 8.0, (2.5 - 0.5) * 1.0 / 16.0, 1.0]  # (every step exact in fp32)


@pytest.mark.parametrize("filter_contacts", [(True, 90, -90), (True, 60), (False,)])
def test_chain_fixture_conditions_hold_for_the_restatement_alone(filter_contacts):
    """seed ``CHAIN_SEED``: the conditions the GPU test asserts, here with the restatement's own normals and stage-1 translation"""
    sc = ref.chain_scene()
    assert sc["human_vertices"].shape[0] == 162 and sc["obj_vertices"].shape[0] >= 98
    hn = ref.normals(sc["human_vertices"], sc["human_faces"]).float()
    on = ref.normals(sc["obj_vertices"], sc["obj_faces"]).float()
    T1 = ref.stage1_mirror(sc["mask"], sc["human_vertices"], sc["human_probs"], sc["focal"], sc["principal"])
    out = ref.chain(sc["obj_vertices"], sc["human_vertices"], on, hn, sc["obj_probs"], sc["human_probs"], T1, filter_contacts=filter_contacts)
    if filter_contacts[0]:
        assert ref.filter_margin(on, hn, sc["obj_probs"] > 0.3, out["h_on"], filter_contacts) > 1e-5
    assert ref.chain_conditions(out) == []
    assert int(out["kept"].sum()) >= 8 and int(out["h_on"].sum()) >= 8
    if filter_contacts == (True, 60):
        assert int(out["kept"].sum()) < int((sc["obj_probs"] > 0.3).sum())  # the filter removes something here


# ---- the C ABI, host only ---------------------------------------------------------------------------------------------------------------

def carve(nbytes):
    """fit_common.h's Carve: every region padded to 256 bytes"""
    return (nbytes + 255) & ~255


def blocks(n, per):
    return (n + per - 1) // per


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 65536, 65537, 1 << 22])
def test_workspace_queries_match_the_carve(n):
    lib = _lib.load()
    assert lib.ivlm_mesh_surface_centroid_workspace_bytes(n) == carve(blocks(n, 256) * 4 * 8)  # 8 blocks of 32 bytes: the 256-byte edge
    assert lib.ivlm_contact_depth_workspace_bytes(n) == carve(blocks(n, 256) * 2 * 8)        # 16 blocks of 16 bytes
    for H, W in ((1, n), (n, 1)) if n <= 16384 else ((n >> 8, 256),):
        assert lib.ivlm_mask_stats_workspace_bytes(H, W) == carve(blocks(H * W, 4096) * 9 * 8)


def test_workspace_queries_at_the_mask_edges_and_limits():
    lib = _lib.load()
    for H, W in ((1, 1), (64, 64), (64, 65), (1, 4097), (65, 257), (1024, 1024), (16384, 16384)):
        assert lib.ivlm_mask_stats_workspace_bytes(H, W) == carve(blocks(H * W, 4096) * 72)
    assert lib.ivlm_mask_stats_workspace_bytes(1024, 1024) == 256 * 72
    for bad in ((0, 4), (4, 0), (-1, 4), (16385, 1), (1, 16385)):
        assert lib.ivlm_mask_stats_workspace_bytes(*bad) == 0
    for fn in (lib.ivlm_mesh_surface_centroid_workspace_bytes, lib.ivlm_contact_depth_workspace_bytes):
        assert fn(0) == 0 and fn(-3) == 0 and fn((1 << 22) + 1) == 0


def test_invalid_arguments_return_minus_one_without_a_gpu():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15  # a host address: an invalid argument is refused before anything would touch it
    assert lib.ivlm_mesh_vertex_normals(None, p, p, p, 4, 4, p, None) == -1
    assert lib.ivlm_mesh_vertex_normals(p, p, p, p, 0, 4, p, None) == -1
    assert lib.ivlm_mesh_vertex_normals(p, p, p, p, 4, -1, p, None) == -1
    assert lib.ivlm_mesh_vertex_normals(p, p, p, p, 4, 4, None, None) == -1
    assert lib.ivlm_mesh_surface_centroid(p, None, 4, 4, p, p, p, 4096, None) == -1
    assert lib.ivlm_mesh_surface_centroid(p, p, 4, 0, p, p, p, 4096, None) == -1
    assert lib.ivlm_mesh_surface_centroid(p, p, 4, 4, p, None, p, 4096, None) == -1
    assert lib.ivlm_mask_stats(None, 4, 4, p, p, 4096, None) == -1
    assert lib.ivlm_mask_stats(p, 0, 4, p, p, 4096, None) == -1
    assert lib.ivlm_mask_stats(p, 4, 4, None, p, 4096, None) == -1
    assert lib.ivlm_contact_depth(p, None, 0, 4, 0.5, p, p, p, p, 4096, None) == -1
    assert lib.ivlm_contact_depth(p, p, 0, 0, 0.5, p, p, p, p, 4096, None) == -1
    assert lib.ivlm_contact_depth(p, p, 0, 4, float("nan"), p, p, p, p, 4096, None) == -1
    assert lib.ivlm_start_translation(None, p, p, p, None, 1, p, p, None) == -1
    assert lib.ivlm_start_translation(p, p, p, p, None, 2, p, p, None) == -1
    assert lib.ivlm_start_translation(p, p, p, p, None, 1, None, p, None) == -1
    # the other refusals that come before a launch: sizes past the limits, an unknown dtype, a workspace too small or misaligned
    assert lib.ivlm_mesh_vertex_normals(p, p, p, p, (1 << 22) + 1, 4, p, None) == -4
    assert lib.ivlm_mask_stats(p, 16385, 4, p, p, 4096, None) == -4
    assert lib.ivlm_contact_depth(p, p, 7, 4, 0.5, p, p, p, p, 4096, None) == -4
    assert lib.ivlm_mesh_surface_centroid(p, p, 4, 4, p, p, p, 255, None) == -2
    assert lib.ivlm_contact_depth(p, p, 0, 4, 0.5, p, p, p, p + 8, 2048, None) == -2
    assert lib.ivlm_abi_version() == 5
