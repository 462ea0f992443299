"""csrc/raster.hip, every pixel accounted for: the mesh and point rasterisers against the banded fp64 reference of tests/_raster_ref.py
(pinned by tests/test_raster_ref_cpu.py), plus the properties that need no reference - ties, order, winding, primitives that must draw
nothing, a face that straddles the camera plane, and the C ABI called directly.  Scenes: tests/_raster_scenes.py; every size is
non-square and both orientations occur.  Every scene exceeds one block of every kernel it runs (project 256 vertices, raster 64
primitives, resolve 256 pixels per block) except the 14-vertex / 7-face crossing scene, which is there for its geometry.

The reference names, per pixel, the set of answers fp32 arithmetic may give.  The kernel must answer inside the set everywhere; on
decided pixels (a set of one) it must give that face, that face's vertex ids, and barycentrics within the derived per-pixel bound.
Undecided pixels are at most 0.5 % of the covered ones, from the reference alone.

No vertex index outside [0, nv) may reach these tests: raster_faces_kernel does not validate indices (the caller owns the mesh), and
such a launch could fault the card.  That is stated here instead of being tested.

Measured on an MI355X (worst barycentric err / bound over the decided hits; pixels outside the allowed set; undecided / covered;
oracle/raster.py on the CPU uses 0.05 .. 0.18 of the bound on the same scenes, and |sum - 1| stays below 0.04 of it everywhere):
  sphere           err/bound 0.126   outside 0   undecided 0 / 2360
  overflow         err/bound 0.057   outside 0   undecided 0 / 8772
  crossing         err/bound 0.079   outside 0   undecided 0 / 2910
  body-topfront    err/bound 0.214   outside 0   undecided 4 / 3808
  body-topback     err/bound 0.192   outside 0   undecided 4 / 3808
  body-bottomfront err/bound 0.164   outside 0   undecided 5 / 3341
  body-bottomback  err/bound 0.151   outside 0   undecided 5 / 3341
  points sphere-r0.05 / sphere-r0.006 / box: outside 0 / 0 / 0, undecided 0 / 2231, 1 / 616, 0 / 5178
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _raster_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
IVLM_OK, IVLM_ERR_INVALID_ARG, IVLM_ERR_WORKSPACE = 0, -1, -2
S60 = float(np.float32(1.0 / np.tan(np.deg2rad(60.0) / 2.0)))


def _mesh(cuda, v, f, cam, size):
    """render.rasterize_mesh -> numpy (p2v, bary, p2f)"""
    from interactvlm_amd import render

    out = render.rasterize_mesh(torch.from_numpy(np.array(v, dtype=np.float32)).to(cuda),
                                torch.from_numpy(np.array(f, dtype=np.int32)).to(cuda), cam, size, want_faces=True)
    return tuple(o.cpu().numpy() for o in out)


def _points(cuda, p, cam, radius, size):
    from interactvlm_amd import render

    return render.rasterize_points(torch.from_numpy(np.array(p, dtype=np.float32)).to(cuda), cam, radius, size).cpu().numpy()


def _bit_equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))
               for x, y in zip(a, b))


def _well_formed(p2v, bary, p2f, faces, tol=None):
    hit = p2f >= 0
    assert p2f.min() >= -1 and p2f.max() < len(faces)
    assert np.array_equal(p2v[hit], faces[p2f[hit]])
    assert (p2v[~hit] == -1).all() and (bary[~hit] == -1).all()
    assert np.isfinite(bary[hit]).all()
    if tol is not None:
        assert np.abs(bary[hit].astype(np.float64).sum(-1) - 1).max() <= tol


def _to_world(view, R, T):
    """view-space points -> world (X_view = X_world.R + T with R orthonormal)"""
    return ((np.asarray(view, dtype=np.float64) - T.astype(np.float64)) @ R.astype(np.float64).T).astype(np.float32)


def _from_ndc(xyz):
    """(x_ndc, y_ndc, z_view) -> view-space points"""
    a = np.asarray(xyz, dtype=np.float64)
    return np.stack([a[:, 0] * a[:, 2] / S60, a[:, 1] * a[:, 2] / S60, a[:, 2]], 1)


# ---- banded reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.MESH_SCENES))
def test_mesh_every_pixel_in_its_allowed_set(hip_lib, cuda, name):
    v, f, cam, (H, W) = S.mesh_scene(name)
    allowed, decided, b64, bound = S.mesh_reference(name)
    print(f"{name}: undecided {int((~decided).sum())} of {int(allowed.covered.sum())} covered")
    assert allowed.undecided_share() <= S.UNDECIDED_CAP      # (from the reference alone, before the kernel is looked at)
    p2v, bary, p2f = _mesh(cuda, v, f, cam, (H, W))
    assert p2v.shape == (H, W, 3) and bary.shape == (H, W, 3) and p2f.shape == (H, W)
    inside = allowed.contains(p2f)
    w = allowed.winner
    hit = decided & (w >= 0)
    err = np.abs(bary.astype(np.float64) - b64).max(-1)
    ratio = float((err[hit] / bound[hit]).max())
    one = np.abs(bary.astype(np.float64).sum(-1) - 1)
    print(f"{name}: outside the set {int((~inside).sum())}, worst bary err / bound {ratio:.3f}, "
          f"worst |sum - 1| / bound {float((one[hit] / bound[hit]).max()):.3f}")
    assert inside.all(), (name, np.argwhere(~inside)[:8].tolist(), p2f[~inside][:8].tolist())
    assert np.array_equal(p2f[decided], w[decided])
    _well_formed(p2v, bary, p2f, f)
    assert (err[hit] <= bound[hit]).all(), (name, ratio, np.argwhere(hit & (err > bound))[:8].tolist())
    assert (one[hit] <= bound[hit]).all()
    assert _bit_equal(_mesh(cuda, v, f, cam, (H, W)), (p2v, bary, p2f))


@pytest.mark.parametrize("name", list(S.POINT_SCENES))
def test_points_every_pixel_in_its_allowed_set(hip_lib, cuda, name):
    p, cam, radius, (H, W) = S.point_scene(name)
    allowed = S.point_reference(name)
    print(f"{name}: undecided {int((~allowed.decided).sum())} of {int(allowed.covered.sum())} covered")
    assert allowed.undecided_share() <= S.UNDECIDED_CAP
    m = _points(cuda, p, cam, radius, (H, W))
    assert m.shape == (H, W) and m.dtype == np.int32
    inside = allowed.contains(m)
    print(f"{name}: outside the set {int((~inside).sum())}")
    assert inside.all(), (name, np.argwhere(~inside)[:8].tolist(), m[~inside][:8].tolist())
    assert np.array_equal(_points(cuda, p, cam, radius, (H, W)), m)


# ---- ties and order (no reference needed) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SMALL_MESH_SCENES)
def test_mesh_ties_order_and_winding(hip_lib, cuda, name):
    v, f, cam, size = S.mesh_scene(name)
    allowed, decided, _, _ = S.mesh_reference(name)
    nf = len(f)
    base = _mesh(cuda, v, f, cam, size)
    # F ++ F: every pixel is an exact depth tie between k and k + nf; the lower index wins it
    assert _bit_equal(_mesh(cuda, v, np.concatenate([f, f]), cam, size), base)
    # a permutation of the face order relabels the answer and changes nothing else
    perm = np.random.default_rng(5).permutation(nf)            # new face k is old face perm[k]
    p2v_p, bary_p, p2f_p = _mesh(cuda, v, f[perm], cam, size)
    back = np.where(p2f_p >= 0, perm[np.maximum(p2f_p, 0)], -1)
    assert np.array_equal(back[decided], base[2][decided]) and allowed.contains(back).all()
    assert _bit_equal((p2v_p[decided], bary_p[decided]), (base[0][decided], base[1][decided]))
    # reversed-winding copies: nothing is culled, nothing new is covered, and the same triangle wins
    _, _, p2f_r = _mesh(cuda, v, np.concatenate([f, f[:, ::-1]]), cam, size)
    assert np.array_equal(p2f_r >= 0, base[2] >= 0)
    assert np.array_equal(np.where(p2f_r >= 0, p2f_r % nf, -1)[decided], base[2][decided])
    # the reversed mesh alone gives the same face on every decided pixel
    assert np.array_equal(_mesh(cuda, v, np.ascontiguousarray(f[:, ::-1]), cam, size)[2][decided], base[2][decided])


@pytest.mark.parametrize("name", list(S.POINT_SCENES))
def test_point_ties_and_order(hip_lib, cuda, name):
    p, cam, radius, size = S.point_scene(name)
    allowed = S.point_reference(name)
    base = _points(cuda, p, cam, radius, size)
    assert np.array_equal(_points(cuda, np.concatenate([p, p]), cam, radius, size), base)
    perm = np.random.default_rng(6).permutation(len(p))
    m = _points(cuda, p[perm], cam, radius, size)
    back = np.where(m >= 0, perm[np.maximum(m, 0)], -1)
    assert np.array_equal(back[allowed.decided], base[allowed.decided]) and allowed.contains(back).all()


# ---- primitives that must draw nothing -------------------------------------------------------------------------------------------
def _tri_at(cx, cy, z):
    """a small triangle around (cx, cy) in NDC at view depth z (view-space points)"""
    return _from_ndc([[cx - 0.1, cy - 0.1, z], [cx + 0.1, cy - 0.1, z * 1.2], [cx, cy + 0.1, z * 0.9]])


@pytest.mark.parametrize("name", S.SMALL_MESH_SCENES)
def test_mesh_primitives_that_draw_nothing(hip_lib, cuda, name):
    v, f, cam, size = S.mesh_scene(name)
    R, T = S.camera(cam)
    nv = len(v)
    base = _mesh(cuda, v, f, cam, size)
    assert (base[2] >= 0).any() and (base[2] < 0).any()
    tri = np.arange(3, dtype=np.int32)[None] + nv
    extra = {
        "behind": (_tri_at(0.0, 0.0, -1.5), tri),                        # in the middle of the image, had it not been behind
        "behind-large": (_from_ndc([[-3, -3, -0.2], [3, -3, -0.2], [0, 3, -4.0]]), tri),
        "left": (_tri_at(1.25, 0.2, 2.0), tri),                           # +X is left: x_ndc > 1
        "right": (_tri_at(-1.25, -0.2, 2.0), tri),
        "above": (_tri_at(0.2, 1.25, 2.0), tri),
        "below": (_tri_at(-0.2, -1.25, 1.0), tri),
        "corner": (_tri_at(1.5, 1.5, 3.0), tri),
    }
    for what, (view, idx) in extra.items():
        v2 = np.concatenate([v, _to_world(view, R, T)])
        assert _bit_equal(_mesh(cuda, v2, np.concatenate([f, idx]), cam, size), base), what
        assert _bit_equal(_mesh(cuda, v2, np.concatenate([idx, f, idx[:, ::-1]]), cam, size)[:2], base[:2]), what
    # repeated-index faces over vertices in the middle of what is drawn: each of the three pairs, and a single vertex
    a, b = int(f[0, 0]), int(f[0, 1])
    rep = np.array([[a, a, b], [a, b, b], [a, b, a], [a, a, a]], dtype=np.int32)
    assert _bit_equal(_mesh(cuda, v, np.concatenate([f, rep]), cam, size), base)
    # all of them at once, in front of the list: the answer is the same up to the shift of the labels
    allv = np.concatenate([v] + [_to_world(view, R, T) for view, _ in extra.values()])
    allf = np.concatenate([rep] + [tri + 3 * k for k in range(len(extra))] + [f])
    p2v, bary, p2f = _mesh(cuda, allv, allf, cam, size)
    shift = len(allf) - len(f)
    assert _bit_equal((p2v, bary), base[:2]) and np.array_equal(np.where(p2f >= 0, p2f - shift, -1), base[2])


@pytest.mark.parametrize("name", list(S.POINT_SCENES))
def test_points_that_draw_nothing(hip_lib, cuda, name):
    p, cam, radius, size = S.point_scene(name)
    R, T = S.camera(cam, points=True)
    base = _points(cuda, p, cam, radius, size)
    e = 1.0 + radius + 0.01                                             # the disc ends 0.01 outside the image
    extra = {
        "behind": _from_ndc([[0.0, 0.0, -1.0], [0.3, -0.2, -0.05], [-0.5, 0.5, -6.0]]),
        "outside": _from_ndc([[e, 0.0, 1.0], [-e, 0.3, 2.0], [0.1, e, 1.5], [-0.4, -e, 0.7], [e, e, 1.0], [30.0, -40.0, 0.05]]),
    }
    for what, view in extra.items():
        w = _to_world(view, R, T)
        assert np.array_equal(_points(cuda, np.concatenate([p, w]), cam, radius, size), base), what
        m = _points(cuda, np.concatenate([w, p]), cam, radius, size)
        assert np.array_equal(np.where(m >= 0, m - len(w), -1), base), what


# ---- a face that straddles the camera plane --------------------------------------------------------------------------------------
def test_mesh_face_straddling_the_camera_plane_is_well_formed(hip_lib, cuda):
    """A ground quad that runs from in front of the camera to behind it, under a sphere.  Outside the banded reference: what a
    projected face with a corner behind the camera covers is an artefact (in pytorch3d as well).  Well-formedness only.
    This test found a fault: the two quad faces used to fill rows 0 .. 35 of this image - pixel (0, 0) first - with barycentrics like
    (1.4e8, -2.1e8, -1.2e8): the 1/z weights of corners on both sides of the plane cancel, and the clamp of their sum to 1e-8 took
    over.  The same formulas in oracle/raster.py gave the same.  Both now ask the corrected barycentrics to be positive too."""
    from oracle import raster as O

    sv, sf = O.icosphere(2)
    cam, size = (2.0, 20.0, 0.0, 0.0, 0.0), (88, 136)                    # eye at (0, 0.68, 1.88), looking at the origin
    quad = np.array([[-3, -0.6, -3], [3, -0.6, -3], [3, -0.6, 4], [-3, -0.6, 4]], dtype=np.float32)   # z = 4 is behind the eye
    v = np.concatenate([(sv * 0.5).astype(np.float32), quad])
    n = len(sv)
    f = np.concatenate([sf.astype(np.int32), np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], dtype=np.int32)])
    R, T = S.camera(cam)
    z = v.astype(np.float64) @ R.astype(np.float64) + T
    assert (z[f[-2:], 2].min(1) < -0.5).all() and (z[f[-2:], 2].max(1) > 0.5).all()   # both quad faces straddle the plane
    p2v, bary, p2f = _mesh(cuda, v, f, cam, size)
    _well_formed(p2v, bary, p2f, f, tol=1e-5)
    assert ((p2f >= 0) & (p2f < len(sf))).sum() > 1000                              # the sphere in front of it is drawn
    assert _bit_equal(_mesh(cuda, v, f, cam, size), (p2v, bary, p2f))


# ---- the C ABI, called directly --------------------------------------------------------------------------------------------------
PAD = 64            # sentinel entries on each side of an output
GUARD = 256         # sentinel bytes on each side of the workspace


def _sentinel(n, dtype, device):
    """NaN for fp32, 0x7fffffff for int32, 0xa5 for bytes"""
    fill = {F32: float("nan"), I32: 0x7FFFFFFF, U8: 0xA5}[dtype]
    return torch.full((n,), fill, dtype=dtype, device=device)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(I32) if t.dtype == F32 else t


def _is_sentinel(t):
    return bool((_bits(t) == _bits(_sentinel(1, t.dtype, "cpu"))).all())


class _Out:
    """an output of n entries embedded in a sentinel-filled buffer"""

    def __init__(self, n, dtype, device):
        self.n, self.buf = n, _sentinel(PAD + n + PAD, dtype, device)

    @property
    def ptr(self):
        return self.buf.data_ptr() + PAD * self.buf.element_size()

    def take(self):
        """-> the n entries, after checking that nothing around them changed"""
        assert _is_sentinel(self.buf[:PAD]) and _is_sentinel(self.buf[PAD + self.n:]), "wrote outside the output"
        return self.buf[PAD: PAD + self.n].cpu().numpy()

    def untouched(self):
        return _is_sentinel(self.buf)


def _cam12(cam, points=False):
    R, T = S.camera(cam, points)
    return (ctypes.c_float * 12)(*np.concatenate([R.reshape(-1), T.reshape(-1)]).astype(np.float32).tolist())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_abi_mesh_sentinels_workspace_and_refusals(hip_lib, cuda):
    lib = hip_lib
    names = ("sphere", "crossing")                                       # the second needs less workspace than the first
    scenes = [S.mesh_scene(n) for n in names]
    need = [lib.ivlm_raster_workspace_bytes(len(v), H, W) for v, _, _, (H, W) in scenes]
    assert need[0] > need[1] > 0
    assert need[0] >= 8 * 96 * 160 + 12 * len(scenes[0][0])              # a 64-bit key per pixel and the projected vertices
    ws = _sentinel(GUARD + need[0] + GUARD, U8, cuda)
    ws_ptr = ws.data_ptr() + GUARD
    for (v, f, cam, (H, W)), nbytes in zip(scenes, need):
        vt, ft = torch.from_numpy(v.copy()).to(cuda), torch.from_numpy(f.copy()).to(cuda)
        before = ws.clone()
        p2v, bary, p2f = _Out(3 * H * W, I32, cuda), _Out(3 * H * W, F32, cuda), _Out(H * W, I32, cuda)
        args = [vt.data_ptr(), len(v), ft.data_ptr(), len(f), _cam12(cam), 60.0, H, W, p2v.ptr, bary.ptr, p2f.ptr, ws_ptr, nbytes,
                _stream()]
        assert lib.ivlm_rasterize_mesh(*args) == IVLM_OK
        torch.cuda.synchronize()
        got = (p2v.take().reshape(H, W, 3), bary.take().reshape(H, W, 3), p2f.take().reshape(H, W))
        assert _bit_equal(got, _mesh(cuda, v, f, cam, (H, W)))           # (which the banded tests above hold to the reference)
        assert torch.equal(ws[:GUARD], before[:GUARD]) and torch.equal(ws[GUARD + nbytes:], before[GUARD + nbytes:]), \
            "wrote outside the workspace it was given"
        # a null pix_to_face is accepted and changes nothing else
        p2v2, bary2 = _Out(3 * H * W, I32, cuda), _Out(3 * H * W, F32, cuda)
        args2 = list(args)
        args2[8], args2[9], args2[10] = p2v2.ptr, bary2.ptr, 0
        assert lib.ivlm_rasterize_mesh(*args2) == IVLM_OK
        torch.cuda.synchronize()
        assert _bit_equal((p2v2.take().reshape(H, W, 3), bary2.take().reshape(H, W, 3)), got[:2])
        # refusals, before any launch: the outputs stay as they were
        outs = _Out(3 * H * W, I32, cuda), _Out(3 * H * W, F32, cuda), _Out(H * W, I32, cuda)

        def refused(**kw):
            a = list(args)
            a[8], a[9], a[10] = (o.ptr for o in outs)
            for k, val in kw.items():
                a[{"nv": 1, "nf": 3, "H": 6, "W": 7, "ws_bytes": 12}[k]] = val
            return lib.ivlm_rasterize_mesh(*a)

        assert refused(ws_bytes=nbytes - 1) == IVLM_ERR_WORKSPACE
        for k in ("nv", "nf", "H", "W"):
            for bad in (0, -1):
                assert refused(**{k: bad}) == IVLM_ERR_INVALID_ARG, (k, bad)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)


def test_abi_points_sentinels_workspace_and_refusals(hip_lib, cuda):
    lib = hip_lib
    names = ("sphere-r0.05", "box")
    scenes = [S.point_scene(n) for n in names]
    need = [lib.ivlm_raster_workspace_bytes(len(p), H, W) for p, _, _, (H, W) in scenes]
    assert need[0] > need[1] > 0
    ws = _sentinel(GUARD + need[0] + GUARD, U8, cuda)
    ws_ptr = ws.data_ptr() + GUARD
    for (p, cam, radius, (H, W)), nbytes in zip(scenes, need):
        pt = torch.from_numpy(p.copy()).to(cuda)
        before = ws.clone()
        out = _Out(H * W, I32, cuda)
        args = [pt.data_ptr(), len(p), _cam12(cam, points=True), 60.0, float(radius), H, W, out.ptr, ws_ptr, nbytes, _stream()]
        assert lib.ivlm_rasterize_points(*args) == IVLM_OK
        torch.cuda.synchronize()
        assert np.array_equal(out.take().reshape(H, W), _points(cuda, p, cam, radius, (H, W)))
        assert torch.equal(ws[:GUARD], before[:GUARD]) and torch.equal(ws[GUARD + nbytes:], before[GUARD + nbytes:]), \
            "wrote outside the workspace it was given"
        keep = _Out(H * W, I32, cuda)

        def refused(**kw):
            a = list(args)
            a[7] = keep.ptr
            for k, val in kw.items():
                a[{"np": 1, "radius": 4, "H": 5, "W": 6, "ws_bytes": 9}[k]] = val
            return lib.ivlm_rasterize_points(*a)

        assert refused(ws_bytes=nbytes - 1) == IVLM_ERR_WORKSPACE
        for k in ("np", "H", "W"):
            for bad in (0, -1):
                assert refused(**{k: bad}) == IVLM_ERR_INVALID_ARG, (k, bad)
        for bad in (0.0, -0.05, float("nan")):
            assert refused(radius=bad) == IVLM_ERR_INVALID_ARG, bad
        torch.cuda.synchronize()
        assert keep.untouched()
