"""fp64 restatements on the CPU of what interactvlm_amd.fit_start computes, written from the definitions: pytorch3d's documented
area-weighted vertex normals, trimesh's documented surface centroid, the mask statistics with ``torch.nonzero``, stage 1 of the
reference's optim/fit.py:119-135 line by line, and the chain of optim/fit.py:137-193 on tests/_icp_ref.py.  Neither pytorch3d nor
trimesh exists for this stack, so there is no golden from either; the self-checks of tests/test_fit_start_cpu.py (sphere normals,
cube centroid) pin the two definitions to closed forms.  Also the small meshes and the chain scene the tests share.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _icp_ref as icp_ref

U = 2.0 ** -24
OSX = dict(focal_virtual=(5000, 5000), body_shape=(256, 192))  # optim/constants.py:6-7; princpt = (192 / 2, 256 / 2)


def f64(t):
    return t.detach().cpu().double()


# ---- the definitions ---------------------------------------------------------------------------------------------------------------

def face_cross(verts, faces):
    v, f = f64(verts), faces.detach().cpu().long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return torch.linalg.cross(b - a, c - a), (a, b, c)


def normals(verts, faces):
    """[N,3] fp64: the sum over the incident faces of cross(b - a, c - a), normalised; (0,0,0) where the sum is zero"""
    n, _ = face_cross(verts, faces)
    f = faces.detach().cpu().long()
    s = torch.zeros(verts.shape[0], 3, dtype=torch.float64)
    for k in range(3):
        s.index_add_(0, f[:, k], n)
    length = s.norm(dim=1, keepdim=True)
    return torch.where(length > 0, s / length.clamp_min(1e-300), torch.zeros_like(s))


def centroid(verts, faces):
    """[3] fp64: sum_f A_f (a + b + c) / 3 / sum_f A_f"""
    n, (a, b, c) = face_cross(verts, faces)
    area = 0.5 * n.norm(dim=1)
    return (area[:, None] * (a + b + c) / 3.0).sum(0) / area.sum()


def mask_stats(mask):
    """dict of Python integers (first / second: (row, col) or (-1, -1)), from ``torch.nonzero``"""
    idx = torch.nonzero(mask.detach().cpu() != 0)
    n = idx.shape[0]
    pix = lambda k: tuple(int(v) for v in idx[k]) if n > k else (-1, -1)  # noqa: E731
    r, c = idx[:, 0], idx[:, 1]
    return dict(count=n, row_min=int(r.min()) if n else -1, row_max=int(r.max()) if n else -1, col_min=int(c.min()) if n else -1,
                col_max=int(c.max()) if n else -1, row_sum=int(r.sum()), col_sum=int(c.sum()), first=pix(0), second=pix(1))


def contact_z(verts, probs, threshold):
    """-> (count, the mean z of the vertices with probs.float() > threshold: an exactly rounded fp64 sum over the count, rounded to fp32)"""
    sel = probs.detach().cpu().float() > threshold
    z = [float(v) for v in verts.detach().cpu()[sel, 2]]
    if not z:
        return 0, None
    return len(z), torch.tensor(math.fsum(z) / len(z), dtype=torch.float64).float()


def stage1_mirror(mask, human_vertices, human_probs, focal, principal, threshold=0.5):
    """optim/fit.py:119-135 line by line: fp32 tensors as the reference has them, the mean z from fp64"""
    obj_mask_indices = torch.nonzero(mask.detach().cpu() != 0).float()
    _, hum_centroid_z = contact_z(human_vertices, human_probs, threshold)
    focal_length = torch.tensor(focal, dtype=torch.float32)
    principal_point = torch.tensor(principal, dtype=torch.float32)
    cx = obj_mask_indices[1].mean() - principal_point[0]
    cy = obj_mask_indices[0].mean() - principal_point[1]
    translation_x = cx * hum_centroid_z / focal_length[0]
    translation_y = cy * hum_centroid_z / focal_length[1]
    return torch.stack([translation_x, translation_y, hum_centroid_z])


def project(point, focal, principal):
    """tests/_silhouette_ref.py's projection: u = fx X / Z + px, v = fy Y / Z + py (a pixel (row i, col j) has its centre at (j + 0.5, i + 0.5))"""
    return focal[0] * point[0] / point[2] + principal[0], focal[1] * point[1] / point[2] + principal[1]


def stage1_intent(mask, z, focal, principal, offset):
    """fp64: the point at depth z + offset[2] on the ray through the centre of the mask's mean pixel, minus the offset"""
    st = mask_stats(mask)
    u, v = st["col_sum"] / st["count"] + 0.5, st["row_sum"] / st["count"] + 0.5
    off = f64(torch.as_tensor(offset))
    Z = float(z) + float(off[2])
    return torch.tensor([(u - principal[0]) * Z / focal[0] - float(off[0]), (v - principal[1]) * Z / focal[1] - float(off[1]), float(z)],
                        dtype=torch.float64)


def osx_camera(bbox):
    """data_io.py:96-109 in numpy fp32 scalars, one operation at a time"""
    f = np.float32
    x, y, w, h = (f(v) for v in bbox)
    fv, bs = OSX["focal_virtual"], OSX["body_shape"]
    pt = (bs[1] / 2, bs[0] / 2)
    focal = (f(fv[0]) / f(bs[1]) * w, f(fv[1]) / f(bs[0]) * h)
    princpt = (f(pt[0]) / f(bs[1]) * w + x, f(pt[1]) / f(bs[0]) * h + y)
    return focal, princpt


def chain(obj_vertices, human_vertices, obj_normals, human_normals, obj_probs, human_probs, T1, scale=1.0, thresholds=(0.3, 0.5),
          filter_contacts=(True, 90, -90), icp_max_iterations=10, estimate_scale=False):
    """optim/fit.py:137-193 from given normals and a given stage-1 translation -> dict(kept, probs, R, T, idx, o_on, h_on)"""
    probs = obj_probs.detach().cpu().clone()
    o_on = probs.float() > thresholds[0]
    h_on = human_probs.detach().cpu().float() > thresholds[1]
    on, hn = obj_normals.detach().cpu(), human_normals.detach().cpu()
    kept = o_on.clone()
    if filter_contacts[0]:
        passed = icp_ref.normal_filter(on[o_on], hn[h_on], filter_contacts[1], filter_contacts[2] if len(filter_contacts) == 3 else None)
        kept[o_on.clone()] = passed
        probs[~kept] = 0.0
        o_on = probs.float() > thresholds[0]
    X, Y = obj_vertices.detach().cpu()[o_on], human_vertices.detach().cpu()[h_on]
    init = (torch.eye(3, dtype=torch.float64), f64(T1), torch.tensor(float(scale), dtype=torch.float64))
    out = icp_ref.icp_as_reference(X, Y, on[o_on], hn[h_on], init, max_iterations=icp_max_iterations, estimate_scale=estimate_scale)
    return dict(kept=kept, probs=probs, R=out["R"], T=out["T"], idx=out["idx"], o_on=o_on, h_on=h_on, X=X, Y=Y, Xn=on[o_on], Yn=hn[h_on],
                init=init)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def icosphere(level=2):
    """unit icosphere -> (verts fp64 [N,3], faces int64 [F,3], outward); level 2: N = 162, F = 320"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [tuple(c / math.sqrt(1 + t * t) for c in p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = [(a + b) / 2 for a, b in zip(v[i], v[j])]
                n = math.sqrt(sum(c * c for c in m))
                v.append(tuple(c / n for c in m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return torch.tensor(v, dtype=torch.float64), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def box(n=4, half=(0.5, 0.5, 0.5)):
    """the surface of a box cut into n x n quads per side, two outward triangles each -> (verts fp64 [(n+1)^3 - (n-1)^3, 3], faces);
    n = 1 is the cube of 8 vertices, n = 4 has 98"""
    index, verts, faces = {}, [], []

    def vid(i, j, k):
        if (i, j, k) not in index:
            index[(i, j, k)] = len(verts)
            verts.append(tuple(h * (2.0 * c / n - 1.0) for h, c in zip(half, (i, j, k))))
        return index[(i, j, k)]

    for axis in range(3):
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def p(da, db):
                        c = [0, 0, 0]
                        c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = side, a + da, b + db
                        return vid(*c)

                    q = [p(0, 0), p(1, 0), p(1, 1), p(0, 1)]  # counter-clockwise seen from +axis
                    if side == 0:
                        q.reverse()
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return torch.tensor(verts, dtype=torch.float64), torch.tensor(faces, dtype=torch.int64)


def tetrahedron():
    v = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]], dtype=torch.float64) * 0.37
    return v + torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64), torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def fan(valence):
    """a hub (vertex 0) above a closed ring of `valence` vertices of uneven radius and height: the hub has `valence` faces"""
    k = torch.arange(valence, dtype=torch.float64)
    a = 2 * math.pi * k / valence
    r = 1.0 + 0.2 * torch.sin(3 * a + 0.3)
    ring = torch.stack([r * torch.cos(a), r * torch.sin(a), 0.1 * torch.cos(5 * a)], 1)
    verts = torch.cat([torch.tensor([[0.03, -0.02, 0.4]], dtype=torch.float64), ring])
    i = torch.arange(valence)
    faces = torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % valence], 1)
    return verts, faces


def grid(rows, cols):
    """a bumpy height field of rows x cols vertices, two triangles per cell"""
    i, j = torch.meshgrid(torch.arange(rows, dtype=torch.float64), torch.arange(cols, dtype=torch.float64), indexing="ij")
    z = 0.3 * torch.sin(0.7 * i) * torch.cos(0.45 * j) + 0.01 * i
    verts = torch.stack([0.1 * j, 0.1 * i, z], -1).reshape(-1, 3)
    a = (torch.arange(rows - 1)[:, None] * cols + torch.arange(cols - 1)[None, :]).reshape(-1)
    faces = torch.cat([torch.stack([a, a + 1, a + cols + 1], 1), torch.stack([a, a + cols + 1, a + cols], 1)])
    return verts, faces


def random_rotation(seed):
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def blob_mask(H, W, centre, radii):
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return (((i - centre[0]) / radii[0]) ** 2 + ((j - centre[1]) / radii[1]) ** 2 <= 1.0).to(torch.uint8)


CHAIN_SEED = 0  # see chain_scene


@functools.lru_cache(maxsize=None)
def chain_scene(seed=CHAIN_SEED):
    """An icosphere "body" (162 vertices, radius 0.5, centred as ``centre_meshes`` leaves it) and a box object (98 vertices, rotated by a
    seeded rotation so that no normal is axis-aligned), with seeded contact vectors: a cap of the body towards (1, 0.4, -0.3) and the
    box vertices near one corner (three sides, so that the contact points are not coplanar), probabilities drawn in (0.55, 1) inside
    and (0, 0.25) outside.  All fp32 on the CPU.  The seed is the first for which the fp64 restatement ALONE meets the fixture
    conditions that tests/test_fit_start_gpu.py asserts, for the three filter settings; tests/test_fit_start_cpu.py asserts them too."""
    gen = torch.Generator().manual_seed(7000 + seed)
    hv, hf = icosphere(2)
    hv = (0.5 * hv) @ random_rotation(7100 + seed)
    ov, of = box(4, (0.16, 0.11, 0.07))
    corner = int(ov.sum(1).argmax())
    ov = ov @ random_rotation(7200 + seed)
    d = torch.tensor([1.0, 0.4, -0.3], dtype=torch.float64)
    d = d / d.norm()
    h_in = (hv / hv.norm(dim=1, keepdim=True)) @ d > 0.55
    o_in = (ov - ov[corner]).norm(dim=1) < 0.19

    def draw(inside):
        r = torch.rand(inside.shape[0], generator=gen)
        return torch.where(inside, 0.55 + 0.45 * r, 0.25 * r).float()

    H, W = 48, 64
    return dict(human_vertices=hv.float(), human_faces=hf, obj_vertices=ov.float(), obj_faces=of, human_probs=draw(h_in),
                obj_probs=draw(o_in), mask=blob_mask(H, W, (22.3, 35.1), (9.0, 12.0)), focal=(90.0, 92.0), principal=(31.5, 24.25),
                offset=torch.tensor([0.1, -0.05, 3.0]), H=H, W=W)


def chain_conditions(out):
    """The fixture conditions of the chain test but the filter's (``filter_margin``), in fp64 on the restatement's result ``out`` =
    chain(...): at least 8 vertices kept on each side; no nearest-neighbour near-tie inside the band of
    tests/test_contact_icp_gpu.py:288-289; the alignment's singular values as far apart as that file's 4u bound needs (its line 129).
    -> list of failures"""
    bad = []
    X, Y, Xn, Yn = (f64(out[k]) for k in ("X", "Y", "Xn", "Yn"))
    if X.shape[0] < 8 or Y.shape[0] < 8:
        bad.append(f"kept {X.shape[0]} object and {Y.shape[0]} human vertices, fewer than 8")
        return bad
    R, T, s = out["init"]
    q = torch.cat([icp_ref.apply(X, R, T, s), Xn], -1)
    t = torch.cat([Y, -Yn], -1)
    two = icp_ref.sqdist(q, t).topk(2, dim=1, largest=False).values
    delta = 8 * U * (abs(float(s)) * float(X.abs().sum(1).max()) + float(T.abs().max()))
    band = 16 * U * two[:, 1] + 2 * two[:, 1].sqrt() * delta
    if not bool((two[:, 1] - two[:, 0] > band).all()):
        bad.append("a nearest-neighbour query is inside the near-tie band")
    S = icp_ref.align(X, Y[out["idx"]], with_singular=True)[3]
    if not (float(S[0] / S[1]) >= 1.5 and float(S[1] / S[2]) >= 1.5 and float(S[2] / S[0]) >= 1e-3):
        bad.append(f"singular values {S.tolist()} too close or too small for the 4u bound")
    return bad


def filter_margin(obj_normals, human_normals, o_on, h_on, filter_contacts):
    """the smallest distance of a dot product of the selected normals (object against minus human, both normalised) from a threshold cosine"""
    on, hn = f64(obj_normals)[o_on], f64(human_normals)[h_on]
    o = on / on.norm(dim=1, keepdim=True).clamp_min(1e-12)
    h = -hn / hn.norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = o @ h.T
    return min(float((d - icp_ref.cos_threshold(a)).abs().min()) for a in filter_contacts[1:])
