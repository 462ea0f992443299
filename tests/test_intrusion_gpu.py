"""``MeshSDF.intrusion`` (csrc/mesh_sdf.hip) against its definition in numpy fp64 (tests/_intrusion_ref.py).

Objects: the tetrahedron (F = 4), the cube (12), ``body_mesh(R, S)`` with F nearest below, at and above one LDS tile
(IVLM_MESH_SDF_TILE) and one grid chunk (IVLM_MESH_SDF_CHUNK).  Points: N in {1, 63, 64, 65, 257} x B in {1, 3}; three poses with
distinct rotations (stretched and sheared six numbers) and s in {0.7, 1, 1.6}.  The points are ``_mesh_sdf_ref.make_points`` of the
object in its canonical frame - at least 1e-4 clear of the surface, unique closest points - taken to the world by the forward pose in
fp64 and rounded to fp32 (``_intrusion_ref.make_case``).  The points are shared by the poses of a batch, so point j is placed by pose
j mod B; that every inside (pose, point) pair has a unique closest point, and that the fp32 mode of the reference flips no sign,
are conditions on the inputs and asserted on the CPU.

Tolerances: k 2^-24 scale.  Scales: the fp64 sum of the terms' absolute values for L; (2 / N) sum_j |e_j| |d e_j / d theta| for each
parameter theta (|de/dt| = 1, |de/ds| = |c|, |de/drot6d_m| = s |c dR/drot6d_m|; fp64, ``_intrusion_ref.intrusion``).  k = 8 x the worst
ratio of the reference's fp32 mode against its fp64 mode over exactly these inputs (``python tests/_intrusion_ref.py 128 512``, on the
CPU; the kernel was not consulted).  Measured worst ratios and the constants:

    L 314.81 -> K_L = 2519      translation 168.87 -> K_T = 1351      scale 79.59 -> K_S = 637      rot6d 179.40 -> K_R = 1436
    sign flips: 0 of 14 400 (pose, point) pairs, 3 430 of them inside

(The ratios are large in these units for the reason given in tests/test_mesh_sdf_gpu.py: a pose whose few inside points lie 1e-4
under the surface has d^2 of 1e-8, whose relative error is 2 delta d / d.)
"""
import functools

import numpy as np
import pytest
import torch

import _intrusion_ref as ir
import _mesh_sdf_ref as ref
from interactvlm_amd import mesh_sdf as ms
from interactvlm_amd._lib import IvlmError

pytestmark = pytest.mark.gpu

K_L, K_T, K_S, K_R = 2519.0, 1351.0, 637.0, 1436.0
BOUNDS = {"L": K_L, "t": K_T, "s": K_S, "r": K_R}
CASES = ir.all_cases(ms.TILE, ms.CHUNK)


@pytest.fixture(autouse=True)
def grad_enabled():
    """see the fixture of the same name in tests/test_contact_pair_gpu.py"""
    with torch.enable_grad():
        yield


@functools.lru_cache(maxsize=None)
def case(name, n, b):
    """computed once, shared by the tests, never modified"""
    return ir.make_case(name, n, b)


@functools.lru_cache(maxsize=None)
def mesh_on(name, dev):
    v, f = ref.named_mesh(name)
    return ms.MeshSDF(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))


def pose_tensors(poses, dev, grad=True):
    r6 = torch.from_numpy(np.stack([p[0] for p in poses])).to(dev).requires_grad_(grad)
    t = torch.from_numpy(np.stack([p[1] for p in poses])).to(dev).requires_grad_(grad)
    s = torch.tensor([float(p[2]) for p in poses], dtype=torch.float32, device=dev).requires_grad_(grad)
    return r6, t, s


def run(mesh, h, poses, dev):
    """-> (L [B], dL/drot6d [B,6], dL/dt [B,3], dL/ds [B]) of the sum over the batch, which is each pose's own gradient"""
    r6, t, s = pose_tensors(poses, dev)
    L = mesh.intrusion(torch.from_numpy(h).to(dev), r6, t, s)
    L.sum().backward()
    return L.detach(), r6.grad, t.grad, s.grad


def test_the_objects_sit_on_the_tile_and_chunk_boundaries():
    sizes = [len(ref.named_mesh(m)[1]) for m in ir.mesh_names(ms.TILE, ms.CHUNK)]
    assert sizes[:2] == [4, 12] and sizes[2] < ms.TILE == sizes[3] < sizes[4] and sizes[5] < ms.CHUNK == sizes[6] < sizes[7]
    assert sizes[2:] == [126, 128, 130, 510, 512, 516]
    for m in ir.mesh_names(ms.TILE, ms.CHUNK):
        ms.check_closed(*ref.named_mesh(m))


@pytest.mark.parametrize("name,n,b", CASES)
def test_value_and_gradients_against_fp64(hip_lib, cuda, name, n, b):
    v, f, h, poses, want = case(name, n, b)
    mesh = mesh_on(name, cuda)
    L, g_r6, g_t, g_s = (x.cpu().numpy() for x in run(mesh, h, poses, cuda))
    assert L.shape == (b,) and g_r6.shape == (b, 6) and g_t.shape == (b, 3) and g_s.shape == (b,)
    for p, ((r6, t, s), w) in enumerate(zip(poses, want)):
        # on the CPU: the fp32 mode flips no sign on these inputs ...
        r32 = ir.intrusion(h, r6, t, s, v, f, dtype=np.float32)
        assert np.array_equal(r32["inside"], w["inside"])
        # ... and neither does the kernel, asked at the un-posed points the fp32 mode states
        inside = mesh.query(torch.from_numpy(r32["x"]).to(cuda))[0].cpu().numpy() < 0
        assert np.array_equal(inside, w["inside"])
        c = ir.compare({"L": L[p], "g_r6": g_r6[p], "g_t": g_t[p], "g_s": g_s[p]}, w)
        print(f"{name} N={n} pose {p} (s = {float(s):.1f}): {int(w['inside'].sum())} inside, "
              + ", ".join(f"{k} {c[k]:.1f} (<= {BOUNDS[k]:.0f})" for k in c))
        assert all(c[k] <= BOUNDS[k] for k in c)
        if not w["inside"].any():
            assert L[p] == 0.0 and (g_r6[p] == 0).all() and (g_t[p] == 0).all() and g_s[p] == 0.0
    # forward only (no gradient asked of the kernel): the same value
    r6, t, s = pose_tensors(poses, cuda, grad=False)
    assert torch.equal(mesh.intrusion(torch.from_numpy(h).to(cuda), r6, t, s).cpu(), torch.from_numpy(L))


def test_all_outside_poses_are_exact_zeros(hip_lib, cuda):
    v, f, h, poses, _ = case("body_7_9", 65, 3)
    mesh = mesh_on("body_7_9", cuda)
    far = [(r6, t + np.float32(5.0), s) for r6, t, s in poses]  # beyond the bounding box: no sweep runs
    L, g_r6, g_t, g_s = run(mesh, h, far, cuda)
    assert bool((L == 0).all()) and bool((g_r6 == 0).all()) and bool((g_t == 0).all()) and bool((g_s == 0).all())
    # in the box, outside the surface: the object's own vertices pushed outward, under the identity pose
    near = (v * 1.05).astype(np.float32)
    assert not ref.query(near, v, f)["inside"].any()
    L, g_r6, g_t, g_s = run(mesh, near, [(np.array(ir.IDENTITY6, dtype=np.float32), np.zeros(3, dtype=np.float32), np.float32(1.0))], cuda)
    assert bool((L == 0).all()) and bool((g_r6 == 0).all()) and bool((g_t == 0).all()) and bool((g_s == 0).all())


@pytest.mark.parametrize("name,n", [("cube", 257), ("body_7_9", 65), ("body_6_43", 257)])
def test_identity_pose_equals_penetration_bit_for_bit(hip_lib, cuda, name, n):
    v, f, h, _, _ = case(name, n, 3)
    mesh = mesh_on(name, cuda)
    x = torch.from_numpy(h).to(cuda)
    want = mesh.penetration(x)
    assert float(want) > 0
    eye = torch.tensor(ir.IDENTITY6, device=cuda)
    got = mesh.intrusion(x, eye, torch.zeros(3, device=cuda), 1.0)
    assert got.shape == () and torch.equal(got, want)
    batch = mesh.intrusion(x, eye.repeat(2, 1), torch.zeros(2, 3, device=cuda), torch.ones(2, device=cuda))
    assert torch.equal(batch, want.repeat(2))


def test_same_bits_every_call_and_whatever_the_batch(hip_lib, cuda):
    for name, n in (("body_6_43", 257), ("tetra", 65)):
        v, f, h, poses, want = case(name, n, 3)
        assert all(w["inside"].any() for w in want)
        mesh = mesh_on(name, cuda)
        first, again = run(mesh, h, poses, cuda), run(mesh, h, poses, cuda)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        for p in range(3):
            alone = run(mesh, h, poses[p:p + 1], cuda)
            assert all(torch.equal(a[0], b[p]) for a, b in zip(alone, first))
        flipped = run(mesh, h, poses[::-1], cuda)  # another place in the batch
        assert all(torch.equal(a, b.flip(0)) for a, b in zip(flipped, first))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_a_bad_scale_gives_nan_there_and_leaves_the_others_alone(hip_lib, cuda, bad):
    v, f, h, poses, _ = case("body_6_43", 257, 3)
    mesh = mesh_on("body_6_43", cuda)
    good = run(mesh, h, poses, cuda)
    broken = list(poses)
    broken[1] = (poses[1][0], poses[1][1], np.float32(bad))
    got = run(mesh, h, broken, cuda)
    for a, b in zip(got, good):
        assert bool(a[1].isnan().all())
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_autograd_scales_the_saved_gradients_and_refuses_a_double_backward(hip_lib, cuda):
    v, f, h, poses, _ = case("body_6_43", 65, 3)
    mesh = mesh_on("body_6_43", cuda)
    x = torch.from_numpy(h).to(cuda)
    _, g_r6, g_t, g_s = run(mesh, h, poses, cuda)
    assert bool((g_r6 != 0).any()) and bool((g_t != 0).any()) and bool((g_s != 0).any())
    up = torch.tensor([0.5, -2.0, 3.0], device=cuda)
    r6, t, s = pose_tensors(poses, cuda)
    (mesh.intrusion(x, r6, t, s) * up).sum().backward()
    assert torch.equal(r6.grad, up.reshape(3, 1) * g_r6) and torch.equal(t.grad, up.reshape(3, 1) * g_t) and torch.equal(s.grad, up * g_s)
    # only what requires grad is computed; a number for the scaling; one pose without a batch axis
    r6, t, _ = pose_tensors(poses[1:2], cuda)
    L = mesh.intrusion(x, r6[0].detach(), t[0], 1.0)
    assert L.shape == ()
    L.backward()
    assert r6.grad is None and torch.equal(t.grad[0], g_t[1])
    # a [B,1] scaling
    r6, t, s = pose_tensors(poses, cuda)
    s2 = s.detach().reshape(3, 1).requires_grad_(True)
    mesh.intrusion(x, r6, t, s2).sum().backward()
    assert torch.equal(s2.grad.reshape(3), g_s)
    r6, t, s = pose_tensors(poses, cuda)
    L = mesh.intrusion(x, r6, t, s)
    (g,) = torch.autograd.grad(L.sum(), t, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_errors(hip_lib, cuda):
    mesh = mesh_on("cube", cuda)
    pts = torch.zeros(5, 3, device=cuda)
    r6, t = torch.tensor([ir.IDENTITY6], device=cuda), torch.zeros(1, 3, device=cuda)
    assert mesh.intrusion(pts, r6, t, 1.0).shape == (1,)
    with pytest.raises(IvlmError):
        mesh.intrusion(pts.cpu(), r6, t, 1.0)
    with pytest.raises(IvlmError):
        mesh.intrusion(pts, r6.cpu(), t, 1.0)
    with pytest.raises(ValueError, match="requires_grad"):
        mesh.intrusion(pts.clone().requires_grad_(True), r6, t, 1.0)
    for bad in (pts.double(), torch.zeros(2, 5, 3, device=cuda), torch.zeros(5, 2, device=cuda), torch.zeros(0, 3, device=cuda)):
        with pytest.raises(ValueError, match="points"):
            mesh.intrusion(bad, r6, t, 1.0)
    with pytest.raises(ValueError, match="rot6d"):
        mesh.intrusion(pts, torch.zeros(1, 5, device=cuda), t, 1.0)
    with pytest.raises(ValueError, match="translation"):
        mesh.intrusion(pts, r6, torch.zeros(2, 3, device=cuda), 1.0)
    with pytest.raises(ValueError, match="scaling"):
        mesh.intrusion(pts, r6, t, torch.ones(2, device=cuda))
    with pytest.raises(ValueError, match="scaling"):
        mesh.intrusion(pts, r6, t, torch.ones(1, dtype=torch.float64, device=cuda))


def test_c_call_with_a_workspace_short_for_the_plan(hip_lib, cuda):
    """the C call is not told F: a workspace that holds no chunk is refused (-2); one that holds one chunk of the plan's three runs
    no sweep and gives NaN in every output; one with room to spare gives the usual bits"""
    name, n = "body_19_27", 65  # F = 1026: three chunks
    mesh = mesh_on(name, cuda)
    assert -(-mesh.num_faces // ms.CHUNK) == 3
    v, f = ref.named_mesh(name)
    r6, t, s = ir.POSES[0]
    canon, _ = ref.make_points(v, f, n, 11)
    h = ir.forward_pose(canon, r6, t, s).astype(np.float32)
    assert ir.intrusion(h, r6, t, s, v, f)["inside"].any()
    x = torch.from_numpy(h).to(cuda)
    r6d, td, sd = pose_tensors([ir.POSES[0]], cuda, grad=False)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=cuda)
        out = [torch.zeros(1, device=cuda), torch.zeros(1, 6, device=cuda), torch.zeros(1, 3, device=cuda), torch.zeros(1, device=cuda)]
        rc = hip_lib.ivlm_mesh_sdf_intrusion(mesh.plan.data_ptr(), x.data_ptr(), r6d.data_ptr(), td.data_ptr(), sd.data_ptr(), 1, n,
                                             *(o.data_ptr() for o in out), ws.data_ptr(), nbytes, stream)
        return rc, out

    assert call(64)[0] == -2
    assert call(hip_lib.ivlm_mesh_sdf_intrusion_workspace_bytes(1, n, ms.CHUNK) - 1)[0] == -2  # just short of one chunk
    rc, out = call(hip_lib.ivlm_mesh_sdf_intrusion_workspace_bytes(1, n, ms.CHUNK))  # one chunk of three
    assert rc == 0 and all(bool(o.isnan().all()) for o in out)
    rc, out = call(hip_lib.ivlm_mesh_sdf_intrusion_workspace_bytes(1, n, 8 * ms.CHUNK))  # room for eight
    want = run(mesh, h, [ir.POSES[0]], cuda)
    assert rc == 0 and float(out[0]) > 0 and all(torch.equal(a, b) for a, b in zip(out, want))
    rc, out = call(hip_lib.ivlm_mesh_sdf_intrusion_workspace_bytes(1, n, mesh.num_faces))  # exactly the plan's
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(out, want))
