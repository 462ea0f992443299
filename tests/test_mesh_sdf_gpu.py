"""mesh_sdf (csrc/mesh_sdf.hip) against its definitions in numpy fp64 (tests/_mesh_sdf_ref.py).

Meshes: a tetrahedron (F = 4), a cube (12), ``body_mesh(R, S)`` (F = 2 R S) with F nearest below, at and above one LDS tile
(IVLM_MESH_SDF_TILE) and one grid chunk (IVLM_MESH_SDF_CHUNK), (12, 11) (F = 264), (12, 11) with two zero-area faces appended, and
once the full (82, 84) (F = 13 776, N = 256, B = 2).  Points: N in {1, 63, 64, 65, 257} x B in {1, 3}, from the seeded generator
``_mesh_sdf_ref.make_points``: uniform in 1.4x the bounding box, face centroids pushed +-{1e-2, 1e-3, 1e-4} along the normal, points
beyond the box.  It rejects |sdf64| < 1e-4 and points whose closest point is not unique (a face within 1e-9 of the minimum distance
whose closest point lies further than 1e-6 from the winner's): conditions on the inputs, not tolerances - every generated point is
compared.  A placement on a symmetry plane of the mesh, such as the point cube centred at (0.625, 0, 0) on ``body_mesh``'s z = 0
plane, has two equidistant closest points per point; there the gradient is one-sided, and such placements are NOT inputs here.

Tolerances: k 2^-24 scale, with the scales of the issue - tol_d: the largest coordinate magnitude among mesh and points; tol_w: 1;
tol_L: the fp64 sum of the terms' absolute values; tol_g: 2 max d / N - and k = 8 x the worst ratio of the fp32 mode of
tests/_mesh_sdf_ref.py against its fp64 mode over exactly these inputs (``python tests/_mesh_sdf_ref.py 128 512 full``, on the CPU;
the kernel was not consulted).  The margin covers what numpy's fp32 does not model: the device's sqrt and atan2 and the order of
the winding sum.  Measured worst ratios and the constants:

    d 56.5 -> K_D = 452      w 47.7 -> K_W = 382      L 561.1 -> K_L = 4489      g 311.5 -> K_G = 2492      sign flips: 0 of 18 512 points

(L and g are large in these units because a pose with one or two inside points 1e-4 below the surface has d^2 of 1e-8, whose
relative error is 2 delta d / d.)
"""
import functools

import numpy as np
import pytest
import torch

import _mesh_sdf_ref as ref
from interactvlm_amd import mesh_sdf as ms
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu

K_D, K_W, K_L, K_G = 452.0, 382.0, 4489.0, 2492.0
MESHES = ref.mesh_names(ms.TILE, ms.CHUNK)
CASES = [(m, n, b) for m in MESHES for n in ref.POINT_COUNTS for b in ref.BATCHES]
FULL = ("body_82_84", 256, 2)
# The edges of the penetration's compaction (one block of 1024 threads per pose, a segment of ceil(N / 1024) points per thread) and of
# its fold blocks of 256: N = 1 (one thread has work), 1023 (segments of 1, the last thread idle), 1025 (segments of 2, half the
# threads idle) with exactly 0, 1, 256 and 257 points of a pose inside the bounding box ('box': inside and outside points mixed as
# the pool has them) or inside the mesh ('in': the kept list of the second compaction and the fold's count sit on 256 / 257).  The
# counted points are spread evenly from the first index to the last; a single one is the last.  name@kind:count of pose 0,of pose 1
PEN_EDGE_CASES = [("body_12_11@box:0,1", 1, 2), ("body_12_11@box:1,0", 1023, 2), ("body_12_11@box:256,257", 1023, 2),
                  ("body_12_11@box:0,1", 1025, 2), ("body_12_11@box:257,256", 1025, 2), ("body_12_11@in:256,257", 1025, 2)]


@pytest.fixture(autouse=True)
def grad_enabled():
    """These tests differentiate, and a whole-suite run reaches them with autograd switched off for the process (see the fixture of
    the same name in tests/test_contact_pair_gpu.py)."""
    with torch.enable_grad():
        yield


def test_the_meshes_sit_on_the_tile_and_chunk_boundaries():
    sizes = [len(ref.named_mesh(m)[1]) for m in MESHES]
    below_t, at_t, above_t = sizes[2:5]
    assert below_t < ms.TILE == at_t < above_t
    below_c, at_c, above_c = sizes[5:8]
    assert below_c < ms.CHUNK == at_c < above_c
    assert sizes[:2] == [4, 12] and sizes[8:] == [264, 266]
    assert all(ref.signed_volume(*ref.named_mesh(m)) > 0 for m in MESHES)


@functools.lru_cache(maxsize=None)
def case(name, n, b):
    """(vertices, faces, points [b,n,3] f32, the fp64 results per pose): computed once, shared by the tests, never modified"""
    if "@" in name:
        return edge_case(name, n, b)
    v, f = ref.named_mesh(name)
    pts, r64 = ref.make_points(v, f, n * b, ref.case_seed(name, n, b), spare=1.5 if name == FULL[0] else 3.0)
    poses = [{k: val[p * n:(p + 1) * n] for k, val in r64.items()} for p in range(b)]
    return v, f, pts.reshape(b, n, 3), poses


@functools.lru_cache(maxsize=None)
def edge_pool(name):
    """4000 points of ``make_points`` for the mesh, their fp64 results, and which lie in the bounding box of the fp32 vertices (the
    comparison the kernel makes: fp32 against fp32, exact): what the cases of PEN_EDGE_CASES draw from"""
    v, f = ref.named_mesh(name)
    pts, r64 = ref.make_points(v, f, 4000, ref.case_seed(name, 4000, 1))
    return v, f, pts, r64, ((pts >= v.min(0)) & (pts <= v.max(0))).all(1)


def edge_case(name, n, b):
    """``case`` for a name of PEN_EDGE_CASES: pose p has exactly counts[p] points in the box (kind 'box') or in the mesh ('in'), at
    evenly spread indices from 0 to n - 1 (one alone: at n - 1); every other point lies outside the box"""
    mesh, _, spec = name.partition("@")
    kind, _, counts = spec.partition(":")
    counts = [int(c) for c in counts.split(",")]
    assert len(counts) == b and kind in ("box", "in")
    v, f, pool, r64, box = edge_pool(mesh)
    counted = np.nonzero(box & r64["inside"] if kind == "in" else box)[0]
    rest = np.nonzero(~box)[0]
    assert len(counted) >= sum(counts) and len(rest) >= n
    idx = np.empty((b, n), dtype=np.int64)
    for p, c in enumerate(counts):
        at = np.zeros(n, dtype=bool)
        at[[n - 1] if c == 1 else np.linspace(0, n - 1, c).round().astype(np.int64)] = True
        assert int(at.sum()) == c
        idx[p, at] = counted[sum(counts[:p]):sum(counts[:p]) + c]
        idx[p, ~at] = np.roll(rest, -37 * p)[:n - c]
    return v, f, pool[idx], [{k: val[idx[p]] for k, val in r64.items()} for p in range(b)]


def assert_edge_counts(name, v, pts, poses):
    """on the CPU, from the numpy reference alone: the poses of an edge case have the in-box / inside counts its name states"""
    kind, _, counts = name.partition("@")[2].partition(":")
    for p, c in enumerate(int(c) for c in counts.split(",")):
        box = ((pts[p] >= v.min(0)) & (pts[p] <= v.max(0))).all(1)
        ins = poses[p]["inside"]
        assert not (ins & ~box).any()
        assert int((ins if kind == "in" else box).sum()) == c
        if kind == "in":
            assert int(box.sum()) == c
        if c >= 2:
            assert box[0] and box[-1]


@functools.lru_cache(maxsize=None)
def mesh_on(name, dev):
    v, f = ref.named_mesh(name.partition("@")[0])
    return ms.MeshSDF(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))


def as_result(out, p=None):
    sdf, closest, face, winding = (t.detach().cpu().numpy() if p is None else t[p].detach().cpu().numpy() for t in out)
    return {"d": np.abs(sdf), "inside": sdf < 0, "closest": closest, "face": face, "winding": winding, "sdf": sdf}


def check_query(name, n, b, dev):
    v, f, pts, poses = case(name, n, b)
    out = mesh_on(name, dev).query(torch.from_numpy(pts).to(dev))
    assert out[0].shape == (b, n) and out[1].shape == (b, n, 3) and out[2].shape == (b, n) and out[3].shape == (b, n)
    assert out[2].dtype == torch.int32
    compared = 0
    for p in range(b):
        got = as_result(out, p)
        assert np.isfinite(got["sdf"]).all() and (got["face"] >= 0).all() and (got["face"] < len(f)).all()
        assert np.array_equal(got["inside"], got["winding"] > 0.5)
        c = ref.compare(got, poses[p], pts[p], v, f)
        print(f"{name} N={n} pose {p}: d {c['d']:.1f} (<= {K_D}), w {c['w']:.1f} (<= {K_W}), sign flips {c['flips']}")
        assert c["flips"] == 0
        assert c["d"] <= K_D and c["w"] <= K_W
        compared += len(got["d"])
    assert compared == n * b  # every generated point was compared


def check_penetration(name, n, b, dev):
    v, f, pts, poses = case(name, n, b)
    if "@" in name:
        assert_edge_counts(name, v, pts, poses)
    mesh = mesh_on(name, dev)
    x = torch.from_numpy(pts).to(dev).requires_grad_(True)
    L = mesh.penetration(x)
    assert L.shape == (b,)
    L.sum().backward()
    face = mesh.query(x.detach())[2].cpu().numpy()
    value, grad = L.detach().cpu().numpy(), x.grad.cpu().numpy()
    compared = 0
    for p in range(b):
        ins = poses[p]["inside"]
        c = ref.compare_penetration(value[p], grad[p], face[p], poses[p], pts[p], v, f)
        print(f"{name} N={n} pose {p}: {int(ins.sum())} inside, L {c['L']:.1f} (<= {K_L}), g {c['g']:.1f} (<= {K_G})")
        assert c["L"] <= K_L and c["g"] <= K_G
        assert (grad[p][~ins] == 0).all()  # exactly: outside points, among them those beyond the bounding box
        beyond = ((pts[p] < v.min(0)) | (pts[p] > v.max(0))).any(1)
        assert not ins[beyond].any() and (grad[p][beyond] == 0).all()
        if not ins.any():
            assert value[p] == 0.0
        compared += len(ins)
    assert compared == n * b
    assert torch.equal(mesh.penetration(x.detach()), L.detach())  # forward only (no gradient asked of the kernel): the same value


@pytest.mark.parametrize("name,n,b", CASES)
def test_query_against_fp64(hip_lib, cuda, name, n, b):
    check_query(name, n, b, cuda)


@pytest.mark.parametrize("name,n,b", CASES + PEN_EDGE_CASES)
def test_penetration_against_fp64(hip_lib, cuda, name, n, b):
    check_penetration(name, n, b, cuda)


def test_full_body_mesh(hip_lib, cuda):
    assert len(ref.named_mesh(FULL[0])[1]) == 13776
    check_query(*FULL, cuda)
    check_penetration(*FULL, cuda)


def test_some_points_of_every_kind_are_present():
    v, f, pts, poses = case("body_12_11", 257, 3)
    ins = np.concatenate([p["inside"] for p in poses])
    d = np.concatenate([p["d"] for p in poses])
    beyond = ((pts.reshape(-1, 3) < v.min(0)) | (pts.reshape(-1, 3) > v.max(0))).any(1)
    assert ins.sum() > 50 and (~ins).sum() > 50 and beyond.sum() > 20 and (d < 2e-3).sum() > 20 and d.min() >= 1e-4


def test_zero_area_faces_change_no_output(hip_lib, cuda):
    v, f, pts, _ = case("body_12_11", 257, 3)
    x = torch.from_numpy(pts).to(cuda)
    plain, marked = mesh_on("body_12_11", cuda), mesh_on("body_12_11+zero", cuda)
    assert marked.num_faces == plain.num_faces + 2
    for a, b in zip(plain.query(x), marked.query(x)):
        assert torch.equal(a, b)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    La, Lb = plain.penetration(xa), marked.penetration(xb)
    La.sum().backward()
    Lb.sum().backward()
    assert torch.equal(La, Lb) and torch.equal(xa.grad, xb.grad) and bool((La > 0).all())


def test_all_outside_batch_is_exact_zeros(hip_lib, cuda):
    v, f = ref.named_mesh("body_12_11")
    mesh = mesh_on("body_12_11", cuda)
    g = torch.Generator().manual_seed(5)
    far = torch.rand(3, 65, 3, generator=g) + torch.tensor([2.0, 0.0, 0.0])  # beyond the bounding box: no sweep runs
    near = torch.from_numpy(v[:65] * 1.05).repeat(3, 1, 1)                  # in the box (mostly), outside the surface
    for pts in (far, near):
        x = pts.to(cuda).requires_grad_(True)
        L = mesh.penetration(x)
        L.sum().backward()
        assert bool((L == 0).all()) and bool((x.grad == 0).all())
    assert bool((mesh.query(far.to(cuda))[0] > 1.0).all())


def test_autograd_scales_the_saved_gradient_and_refuses_a_double_backward(hip_lib, cuda):
    v, f, pts, _ = case("body_12_11", 65, 3)
    mesh = mesh_on("body_12_11", cuda)
    x = torch.from_numpy(pts).to(cuda).requires_grad_(True)
    ms.penetration_loss(x, mesh).sum().backward()
    saved = x.grad.clone()
    assert bool((saved != 0).any())
    up = torch.tensor([0.5, -2.0, 3.0], device=cuda)
    x.grad = None
    (ms.penetration_loss(x, mesh) * up).sum().backward()
    assert torch.equal(x.grad, up.reshape(3, 1, 1) * saved)
    # the convenience that prepares the mesh itself, unbatched: [] and the first pose's gradient
    x0 = torch.from_numpy(pts[0]).to(cuda).requires_grad_(True)
    L0 = ms.penetration_loss(x0, torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda))
    assert L0.shape == ()
    L0.backward()
    assert torch.equal(x0.grad, saved[0])
    sdf = ms.mesh_signed_distance(x0.detach(), torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda))[0]
    assert sdf.shape == (65,) and not sdf.requires_grad
    x1 = torch.from_numpy(pts[0]).to(cuda).requires_grad_(True)
    L1 = mesh.penetration(x1)
    (g1,) = torch.autograd.grad(L1, x1, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_same_bits_every_call_and_whatever_the_batch(hip_lib, cuda):
    for name, n in (("body_12_11", 257), ("body_19_27", 65)):
        v, f, pts, _ = case(name, n, 3)
        mesh = mesh_on(name, cuda)

        def run(p):
            x = torch.from_numpy(p).to(cuda).requires_grad_(True)
            L = mesh.penetration(x)
            L.sum().backward()
            return L.detach(), x.grad

        L, g = run(pts)
        L2, g2 = run(pts)
        assert torch.equal(L, L2) and torch.equal(g, g2)
        q, q2 = mesh.query(torch.from_numpy(pts).to(cuda)), mesh.query(torch.from_numpy(pts).to(cuda))
        assert all(torch.equal(a, b) for a, b in zip(q, q2))
        for p in range(3):
            Lp, gp = run(pts[p])
            assert Lp.shape == () and torch.equal(Lp, L[p]) and torch.equal(gp, g[p])
            assert all(torch.equal(a, b[p]) for a, b in zip(mesh.query(torch.from_numpy(pts[p]).to(cuda)), q))
        Lr, gr = run(np.ascontiguousarray(pts[::-1]))  # another place in the batch
        assert torch.equal(Lr, L.flip(0)) and torch.equal(gr, g.flip(0))


def test_errors(hip_lib, cuda):
    v, f = (torch.from_numpy(t) for t in ref.cube_mesh())
    pts = torch.zeros(5, 3)
    with pytest.raises(IvlmError):
        ms.MeshSDF(v, f)  # CPU tensors
    with pytest.raises(IvlmError):
        ms.MeshSDF(v.to(cuda), f)
    vd, fd = v.to(cuda), f.to(cuda)
    mesh = ms.MeshSDF(vd, fd)
    with pytest.raises(IvlmError):
        mesh.query(pts)
    with pytest.raises(IvlmError):
        mesh.penetration(pts)
    for bad in (pts.double().to(cuda), torch.zeros(5, 2, device=cuda), torch.zeros(2, 2, 5, 3, device=cuda), torch.zeros(0, 3, device=cuda)):
        with pytest.raises(ValueError):
            mesh.query(bad)
        with pytest.raises(ValueError):
            mesh.penetration(bad)
    with pytest.raises(ValueError):
        ms.MeshSDF(vd.double(), fd)
    with pytest.raises(ValueError):
        ms.MeshSDF(vd, fd.long())
    with pytest.raises(ValueError):
        ms.MeshSDF(vd.reshape(-1), fd)
    with pytest.raises(ValueError):
        ms.MeshSDF(vd, fd.reshape(-1, 2))
    high, low = fd.clone(), fd.clone()
    high[3, 1] = 8
    low[0, 0] = -1
    for bad in (high, low):
        with pytest.raises(ValueError, match="indices"):
            ms.MeshSDF(vd, bad)
    with pytest.raises(ValueError, match="requires_grad"):
        ms.MeshSDF(vd.clone().requires_grad_(True), fd)
    with pytest.raises(ValueError):
        ms.penetration_loss(pts.to(cuda), mesh, fd)
    with pytest.raises(ValueError):
        ms.penetration_loss(pts.to(cuda), vd)


def test_c_calls_with_a_workspace_short_for_the_plan(hip_lib, cuda):
    """the C calls are not told F: a workspace that holds no chunk is refused (-2); one that holds fewer chunks than the plan has
    runs no sweep and gives NaN and face -1 - documented in include/ivlm_hip.h - and one with room to spare gives the usual bits"""
    name, n = "body_19_27", 65  # F = 1026: three chunks
    mesh = mesh_on(name, cuda)
    assert -(-mesh.num_faces // ms.CHUNK) >= 2
    x = torch.from_numpy(case(name, n, 1)[2]).to(cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=cuda)
        sdf, closest = torch.zeros(1, n, device=cuda), torch.zeros(1, n, 3, device=cuda)
        face, winding = torch.zeros(1, n, dtype=torch.int32, device=cuda), torch.zeros(1, n, device=cuda)
        value, grad = torch.zeros(1, device=cuda), torch.ones(1, n, 3, device=cuda)
        rq = hip_lib.ivlm_mesh_sdf_query(mesh.plan.data_ptr(), x.data_ptr(), 1, n, sdf.data_ptr(), closest.data_ptr(), face.data_ptr(),
                                         winding.data_ptr(), ws.data_ptr(), nbytes, stream)
        rp = hip_lib.ivlm_mesh_sdf_penetration(mesh.plan.data_ptr(), x.data_ptr(), 1, n, value.data_ptr(), grad.data_ptr(), ws.data_ptr(),
                                               nbytes, stream)
        return rq, rp, sdf, closest, face, winding, value, grad

    assert call(64)[:2] == (-2, -2)
    rq, rp, sdf, closest, face, winding, value, grad = call(hip_lib.ivlm_mesh_sdf_workspace_bytes(1, n, ms.CHUNK))  # one chunk of three
    assert (rq, rp) == (0, 0)
    assert bool(sdf.isnan().all()) and bool(closest.isnan().all()) and bool(winding.isnan().all()) and bool((face == -1).all())
    assert bool(value.isnan().all()) and bool((grad == 0).all())
    want = mesh.query(x)
    rq, rp, sdf, closest, face, winding, value, grad = call(hip_lib.ivlm_mesh_sdf_workspace_bytes(1, n, 8 * ms.CHUNK))  # room for eight
    assert (rq, rp) == (0, 0)
    assert all(torch.equal(a, b) for a, b in zip((sdf, closest, face, winding), want))
    xg = x.clone().requires_grad_(True)
    L = mesh.penetration(xg)
    L.sum().backward()
    assert torch.equal(value, L.detach()) and torch.equal(grad, xg.grad)
