"""The intrusion term of interactvlm_amd.mesh_sdf (``MeshSDF.intrusion``) restated in numpy on top of tests/_mesh_sdf_ref.py.

The object mesh (V_o, F_o) is closed, outward and constant; a pose is (rot6d, t, s) with y = (s v) R + t (row vectors); h_j are the
human's vertices, shared by the poses:

    x_j = ((h_j - t) R^T) / s;   c_j, d_j, inside_j = the query of the object mesh at x_j;   e_j = s (x_j - c_j) R
    L = (1 / N) sum_j inside_j |e_j|^2 = (1 / N) sum_j inside_j (s d_j)^2
    dL/dt = -(2 / N) sum inside e;  dL/ds = -(2 / N) sum inside e . (c R);  dL/dR_ik = -(2 s / N) sum inside c_i e_k, then to rot6d

``dtype=np.float64`` is the yardstick.  ``dtype=np.float32`` states what csrc/mesh_sdf.hip does, operation by operation: R from the
Gram-Schmidt in fp64, rounded to fp32 once; u = h - t and x_i = ((u_0 R_i0 + u_1 R_i1) + u_2 R_i2) / s in fp32; the fp32 query of
_mesh_sdf_ref; then everything in fp64 from the fp32 q, dd and x (c = x + q, e = -s (q R) with the unrounded R), each output rounded
to fp32 once.  The tolerance constants of tests/test_intrusion_gpu.py are measured with it against the fp64 mode, on the CPU
(``python tests/_intrusion_ref.py TILE CHUNK``), never against the kernel.
"""
import numpy as np

import _mesh_sdf_ref as ref

U = ref.U
EPS = 1e-12  # F.normalize's clamp of the norm


# ---- rot6d ----------------------------------------------------------------------------------------------------------------------
def gram_schmidt(r6):
    """six numbers (a1, a2 interleaved) -> R [3,3] fp64 with columns b1, b2, b3, and what the chain back needs"""
    a = np.asarray(r6, dtype=np.float64).reshape(3, 2)
    a1, a2 = a[:, 0], a[:, 1]
    l1 = np.sqrt(a1 @ a1)
    n1 = l1 if l1 > EPS else EPS
    b1 = a1 / n1
    d = b1 @ a2
    u2 = a2 - d * b1
    l2 = np.sqrt(u2 @ u2)
    n2 = l2 if l2 > EPS else EPS
    b2 = u2 / n2
    b3 = np.cross(b1, b2)
    return np.stack([b1, b2, b3], 1), dict(a2=a2, b1=b1, b2=b2, d=d, n1=n1, n2=n2, clamp1=not l1 > EPS, clamp2=not l2 > EPS)


def gram_schmidt_backward(frame, grad_R):
    """dL/dR [3,3] -> dL/drot6d [6] (pose.gram_schmidt_backward, in numpy fp64)"""
    f = frame
    gb1, gb2, gb3 = (np.array(grad_R[:, k], dtype=np.float64) for k in range(3))
    gb1 = gb1 + np.cross(f["b2"], gb3)
    gb2 = gb2 + np.cross(gb3, f["b1"])
    gu2 = (gb2 - f["b2"] * (0.0 if f["clamp2"] else f["b2"] @ gb2)) / f["n2"]
    gd = -(f["b1"] @ gu2)
    gb1 = gb1 + gd * f["a2"] - f["d"] * gu2
    ga2 = gu2 + gd * f["b1"]
    ga1 = (gb1 - f["b1"] * (0.0 if f["clamp1"] else f["b1"] @ gb1)) / f["n1"]
    return np.stack([ga1, ga2], 1).reshape(6)


def rotation_jacobian(r6):
    """-> J [6,3,3]: J[m] = dR / drot6d[m], from the chain applied to the nine unit matrices"""
    _, frame = gram_schmidt(r6)
    J = np.zeros((6, 3, 3))
    for i in range(3):
        for k in range(3):
            E = np.zeros((3, 3))
            E[i, k] = 1.0
            J[:, i, k] = gram_schmidt_backward(frame, E)
    return J


def axis_angle_rot6d(axis, angle, stretch=(1.0, 1.0), shear=0.0):
    """the rot6d of the rotation about ``axis`` by ``angle`` (Rodrigues, fp64), its columns stretched and sheared so that the
    Gram-Schmidt has work to do: a1 = stretch[0] b1, a2 = stretch[1] b2 + shear b1 -> f32 [6]"""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    a1, a2 = stretch[0] * R[:, 0], stretch[1] * R[:, 1] + shear * R[:, 0]
    return np.stack([a1, a2], 1).reshape(6).astype(np.float32)


def forward_pose(v, r6, t, s):
    """y = (s v) R + t in fp64"""
    R, _ = gram_schmidt(r6)
    return (float(s) * np.asarray(v, dtype=np.float64)) @ R + np.asarray(t, dtype=np.float64)


def unpose(h, r6, t, s, dtype=np.float64):
    """x = ((h - t) R^T) / s in dtype; the fp32 mode in the order of sdf_unpose_kernel"""
    R64, _ = gram_schmidt(r6)
    R = R64.astype(dtype)
    u = np.asarray(h, dtype=dtype) - np.asarray(t, dtype=dtype)
    sc = np.dtype(dtype).type(s)
    return np.stack([((u[:, 0] * R[i, 0] + u[:, 1] * R[i, 1]) + u[:, 2] * R[i, 2]) / sc for i in range(3)], 1)


# ---- the term -------------------------------------------------------------------------------------------------------------------
def intrusion(h, r6, t, s, vertices, faces, dtype=np.float64, unique=False):
    """h [N,3], one pose -> dict: L, g_r6 [6], g_t [3], g_s (rounded to dtype once), A = the sum of the terms' absolute values / N,
    and the tolerance scales of the gradients, s_t, s_s, s_r6 [6] = (2 / N) sum_j |e_j| |d e_j / d theta| (fp64, c held constant);
    x [N,3], the query r of x, inside [N]"""
    r6, t = np.asarray(r6), np.asarray(t)
    x = unpose(h, r6, t, s, dtype)
    r = ref.query(x, vertices, faces, dtype=dtype, unique=unique)
    n = x.shape[0]
    R, frame = gram_schmidt(r6)
    sc = float(np.float32(s)) if dtype == np.float32 else float(s)
    ins = r["inside"]
    q = r["q"].astype(np.float64)[ins]
    c = x.astype(np.float64)[ins] + q
    e = -sc * (q @ R)
    terms = (sc * sc) * r["dd"].astype(np.float64)[ins]
    cR = c @ R
    w = -2.0 / n
    g_t = w * e.sum(0)
    g_s = w * (e * cR).sum()
    g_R = (w * sc) * (c.T @ e)
    g_r6 = gram_schmidt_backward(frame, g_R)
    ne = np.linalg.norm(e, axis=1)
    J = rotation_jacobian(r6)
    out = {"L": terms.sum() / n, "g_r6": g_r6, "g_t": g_t, "g_s": g_s, "A": np.abs(terms).sum() / n,
           "s_t": 2.0 / n * ne.sum(), "s_s": 2.0 / n * (ne * np.linalg.norm(c, axis=1)).sum(),
           "s_r6": np.array([2.0 / n * (ne * sc * np.linalg.norm(c @ J[m], axis=1)).sum() for m in range(6)]),
           "x": x, "r": r, "inside": ins}
    if dtype == np.float32:
        for k in ("L", "g_r6", "g_t", "g_s"):
            out[k] = np.float32(out[k]) if np.ndim(out[k]) == 0 else out[k].astype(np.float32)
    return out


def value_only(h, r6, t, s, vertices, faces):
    """L in fp64 with the closest points queried afresh: what central differences differentiate"""
    x = unpose(h, r6, t, s)
    r = ref.query(x, vertices, faces)
    return float((np.where(r["inside"], r["dd"], 0.0) * float(s) ** 2).sum() / x.shape[0])


def compare(got, want):
    """the error ratios of a result (dict with L, g_r6, g_t, g_s: the fp32 mode here, or the kernel) against the fp64 result ``want``,
    in units of 2^-24 x the scale of each tolerance -> dict(L, t, s, r); a scale of 0 (no point inside) demands an exact 0"""
    def ratio(err, scale):
        err = float(np.max(np.abs(err)))
        if scale == 0.0:
            return 0.0 if err == 0.0 else float("inf")
        return err / (U * scale)

    g_r6 = np.asarray(got["g_r6"], dtype=np.float64)
    return {"L": ratio(float(got["L"]) - want["L"], want["A"]),
            "t": ratio(np.asarray(got["g_t"], dtype=np.float64) - want["g_t"], want["s_t"]),
            "s": ratio(float(got["g_s"]) - want["g_s"], want["s_s"]),
            "r": max(ratio(g_r6[m] - want["g_r6"][m], want["s_r6"][m]) for m in range(6))}


# ---- the inputs of tests/test_intrusion_gpu.py (and of the tolerance measurement below) ------------------------------------------
POINT_COUNTS = (1, 63, 64, 65, 257)
BATCHES = (1, 3)
# distinct rotations, stretched and sheared six numbers, s in {0.7, 1, 1.6}
POSES = (
    (axis_angle_rot6d((1.0, 2.0, 3.0), 0.4, (1.3, 0.8), 0.3), np.array([0.11, -0.07, 0.05], dtype=np.float32), np.float32(0.7)),
    (axis_angle_rot6d((-1.0, 0.5, 2.0), 1.1, (0.9, 1.2), -0.2), np.array([-0.06, 0.09, 0.12], dtype=np.float32), np.float32(1.0)),
    (axis_angle_rot6d((0.3, -1.0, 0.2), 2.5, (1.1, 0.7), 0.15), np.array([0.04, 0.13, -0.08], dtype=np.float32), np.float32(1.6)),
)


def mesh_names(tile, chunk):
    """the objects of the GPU tests: the tetrahedron, the cube, body meshes with F below / at / above one tile and one chunk"""
    return ref.mesh_names(tile, chunk)[:8]


def case_poses(n, b):
    """the poses of case (n, b): all three for b = 3; one, chosen by n, for b = 1"""
    return [POSES[(n + p) % 3] for p in range(b)] if b == 1 else list(POSES)


def make_case(name, n, b):
    """-> (vertices, faces, h f32 [n,3], poses, the fp64 ``intrusion`` per pose).  The n points are ``make_points`` of the object in
    its canonical frame (>= 1e-4 clear of the surface, unique closest points); point j is taken to the world by the forward pose
    (j mod b) in fp64 and rounded to fp32.  Every (pose, point) pair whose point is inside - also a point with a pose that did not
    place it - must have a unique closest point in fp64: asserted here, a condition on the inputs.  (A point outside adds an exact 0
    to every sum, whatever its closest point.)"""
    v, f = ref.named_mesh(name)
    canon, _ = ref.make_points(v, f, n, ref.case_seed(name, n, b) + 7)
    poses = case_poses(n, b)
    h = np.empty((n, 3), dtype=np.float32)
    for j in range(n):
        r6, t, s = poses[j % b]
        h[j] = forward_pose(canon[j:j + 1], r6, t, s)[0].astype(np.float32)
    want = [intrusion(h, r6, t, s, v, f, unique=True) for r6, t, s in poses]
    for p, w in enumerate(want):
        assert w["r"]["unique"][w["inside"]].all(), f"{name} n={n} b={b} pose {p}: an inside point with two closest points"
    return v, f, h, poses, want


def all_cases(tile, chunk):
    return [(m, n, b) for m in mesh_names(tile, chunk) for n in POINT_COUNTS for b in BATCHES]


# ---- the scene of the issue and of tests/test_fit_intrusion_gpu.py ---------------------------------------------------------------
CUBE_HALF, CUBE_CENTRE = 0.2, (0.05, 0.78, 0.03)
IDENTITY6 = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def fit_scene():
    """-> (human vertices, human faces, cube vertices (canonical, centred at the origin), cube faces) as numpy"""
    from interactvlm_amd.synthetic import body_mesh

    hv, hf = (a.numpy() for a in body_mesh(12, 11))
    cv, cf = ref.cube_mesh(half=CUBE_HALF)
    return hv, hf, cv, cf


if __name__ == "__main__":  # measure the constants: python tests/_intrusion_ref.py TILE CHUNK
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tile, chunk = int(sys.argv[1]), int(sys.argv[2])
    worst = {"L": 0.0, "t": 0.0, "s": 0.0, "r": 0.0}
    flips = pairs = inside = 0
    for name, n, b in all_cases(tile, chunk):
        v, f, h, poses, want = make_case(name, n, b)
        for (r6, t, s), w in zip(poses, want):
            got = intrusion(h, r6, t, s, v, f, dtype=np.float32)
            flips += int((got["inside"] != w["inside"]).sum())
            pairs += n
            inside += int(w["inside"].sum())
            for k, x in compare(got, w).items():
                worst[k] = max(worst[k], x)
        print(name, n, b, {k: round(float(x), 2) for k, x in worst.items()}, "flips", flips, flush=True)
    print("worst ratios:", worst, "sign flips:", flips, "of", pairs, "pairs,", inside, "inside")
