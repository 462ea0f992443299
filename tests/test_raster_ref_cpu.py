"""Pins the banded fp64 rasteriser reference (tests/_raster_ref.py) before tests/test_raster_exact_gpu.py leans on it.  No GPU.

  * on decided pixels it names the face and the barycentrics that oracle/raycast.py finds by another algorithm (world-space rays);
  * the fp32 restatement oracle/raster.py answers inside the allowed set at every pixel of every scene and inside the barycentric
    bound (it uses < 0.2 of it);
  * undecided pixels are at most 0.5 % of the covered ones in every scene (the reference alone gives <= 0.16 %);
  * each planted mistake in a copy of oracle.raster.rasterize_mesh is flagged - the affine z test by the crossing scene, which is
    the only scene that can see it, and a swapped H / W by every scene, since every size is non-square.

Undecided / covered pixels: sphere 0 / 2360, overflow 0 / 8772, crossing 0 / 2910, body topfront 4 / 3808, topback 4 / 3808,
bottomfront 5 / 3341, bottomback 5 / 3341; points sphere r 0.05 0 / 2231, r 0.006 1 / 616, box 0 / 5178."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _raster_ref as ref  # noqa: E402
import _raster_scenes as S  # noqa: E402

from oracle import raster as O  # noqa: E402

F = np.float32


def _judge(name, p2f, bary, p2v=None):
    """-> (pixels outside the allowed set, worst barycentric err / bound over the decided hits)"""
    allowed, decided, b64, bound = S.mesh_reference(name)
    p2f = np.asarray(p2f)
    outside = int((~allowed.contains(p2f)).sum())
    hit = decided & (allowed.winner >= 0) & (p2f == allowed.winner)
    err = np.abs(np.asarray(bary, dtype=np.float64)[hit] - b64[hit]).max(-1)
    if p2v is not None:
        _, f, _, _ = S.mesh_scene(name)
        assert np.array_equal(np.asarray(p2v)[hit], f[p2f[hit]])
    return outside, float((err / bound[hit]).max()) if hit.any() else 0.0


@pytest.mark.parametrize("name", list(S.MESH_SCENES))
def test_undecided_share_and_shape_of_the_reference(name):
    allowed, decided, b64, bound = S.mesh_reference(name)
    _, f, _, (H, W) = S.mesh_scene(name)
    assert H != W and decided.shape == (H, W) and b64.shape == (H, W, 3) and bound.shape == (H, W)
    print(f"{name}: undecided {int((~decided).sum())} of {int(allowed.covered.sum())} covered")
    assert allowed.undecided_share() <= S.UNDECIDED_CAP
    if name in S.SMALL_MESH_SCENES:
        assert decided.all()
    w = allowed.winner
    assert ((w >= -1) == decided).all() and w.max() < len(f)
    hit = decided & (w >= 0)
    assert 0.05 < hit.mean() < 0.99                                      # something is drawn and something is empty
    assert np.abs(b64[hit].sum(-1) - 1).max() < 1e-12 and (b64[hit] > 0).all() and (bound[hit] > 0).all()
    assert (b64[decided & (w < 0)] == -1).all() and np.isnan(b64[~decided]).all()
    # the bound is a bound on fp32 work, not a tolerance that would pass a wrong formula: far below one barycentric unit
    assert bound[hit].max() < 5e-3


@pytest.mark.parametrize("name", list(S.POINT_SCENES))
def test_point_reference_and_fp32_restatement(name):
    allowed = S.point_reference(name)
    p, cam, r, (H, W) = S.point_scene(name)
    print(f"{name}: undecided {int((~allowed.decided).sum())} of {int(allowed.covered.sum())} covered")
    assert H != W and allowed.undecided_share() <= S.UNDECIDED_CAP
    assert allowed.covered.sum() > 500 and not allowed.covered.all()
    Rm, T = S.camera(cam, points=True)
    m = O.rasterize_points(p, Rm, T, r, H, W)
    assert allowed.contains(m).all()
    # a brute-force fp64 nearest-disc search (no bands, no boxes) names the decided winners
    x, y, z, _, _ = ref.project(p, Rm, T, 60.0)
    ys, xs = ref.pixel_centres(H), ref.pixel_centres(W)
    best, brute = np.full((H, W), np.inf), np.full((H, W), -1, dtype=np.int64)
    for q in np.nonzero(z > 0)[0]:
        win = ((xs[None, :] - x[q]) ** 2 + (ys[:, None] - y[q]) ** 2 < float(F(r)) ** 2) & (z[q] < best)
        best[win], brute[win] = z[q], q
    assert np.array_equal(brute[allowed.decided], allowed.winner[allowed.decided])
    if name == "box":
        assert (z < 0).sum() > 100                                        # (points behind the camera are in the scene)


@pytest.mark.parametrize("name", ["crossing"] + ["body-" + v for v in S.BODY_VIEWS])
def test_reference_agrees_with_the_ray_caster_on_decided_pixels(name):
    """oracle/raycast.py states its camera in fp64 from the angles; the reference takes the fp32 R, T.  That is one rounding of each
    entry, inside the 8u budget of the projection, so the barycentrics of the two agree within the reference's own bound."""
    from oracle import raycast as RC

    v, f, cam, (H, W) = S.mesh_scene(name)
    allowed, decided, b64, bound = S.mesh_reference(name)
    cf, cb, _ = RC.cast_mesh(v, f, RC.camera(*cam), H, W)
    assert np.array_equal(cf[decided], allowed.winner[decided])
    hit = decided & (cf >= 0)
    ratio = float((np.abs(cb[hit] - b64[hit]).max(-1) / bound[hit]).max())
    print(f"{name}: ray caster vs reference, worst bary err / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert allowed.contains(cf).all()


@pytest.mark.parametrize("name", list(S.MESH_SCENES))
def test_fp32_restatement_is_inside_the_allowed_sets(name):
    v, f, cam, (H, W) = S.mesh_scene(name)
    Rm, T = S.camera(cam)
    assert all(np.array_equal(a, b) for a, b in zip(O.look_at_view_transform(*cam), (Rm, T)))  # (oracle and package: one camera)
    p2v, bary, p2f = O.rasterize_mesh(v, f, Rm, T, H, W)
    outside, ratio = _judge(name, p2f, bary, p2v)
    print(f"{name}: oracle/raster.py outside the set {outside}, worst bary err / bound {ratio:.3f}")
    assert outside == 0 and ratio <= 1.0


# ---- planted mistakes -----------------------------------------------------------------------------------------------------------
MUTATIONS = ("box_short", "affine_bary", "affine_z", "farthest_wins", "x_not_mirrored", "hw_swapped")
MUTANT_SCENES = S.SMALL_MESH_SCENES + ("body-bottomfront",)  # (one body view: the other three see what it sees, at 0.4 s per edit each)


def _mutant(verts, faces, R, T, H, W, mut=None):
    """oracle.raster.rasterize_mesh, copied, with one edit switched on by ``mut`` (None: the copy itself, held bit-equal to the original
    by test_planted_mistakes_are_flagged)."""
    EPS = O.EPS
    sv = O.project(verts, R, T)
    far = mut == "farthest_wins"
    zbest = np.full((H, W), -np.inf if far else np.inf, dtype=F)
    fbest = np.full((H, W), -1, dtype=np.int64)
    bbest = np.full((H, W, 3), -1, dtype=F)
    if mut == "hw_swapped":
        ys, xs = O._ndc(np.arange(H), W), O._ndc(np.arange(W), H)
    else:
        ys, xs = O._ndc(np.arange(H), H), O._ndc(np.arange(W), W)
    if mut == "x_not_mirrored":
        xs = -xs
    for f, (i0, i1, i2) in enumerate(faces):
        (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = sv[i0], sv[i1], sv[i2]
        if max(z0, z1, z2) < EPS:
            continue
        area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
        if -EPS <= area <= EPS:
            continue
        xmn, xmx, ymn, ymx = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
        jj = np.nonzero((xs >= xmn) & (xs <= xmx))[0]
        ii = np.nonzero((ys >= ymn) & (ys <= ymx))[0]
        if mut == "box_short":
            jj = jj[:-1]
        if len(jj) == 0 or len(ii) == 0:
            continue
        px, py = xs[jj][None, :], ys[ii][:, None]
        inv = F(1.0) / (area + EPS)
        b0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) * inv
        b1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) * inv
        b2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) * inv
        inside = (b0 > 0) & (b1 > 0) & (b2 > 0)
        if not inside.any():
            continue
        t0, t1, t2 = b0 * z1 * z2, z0 * b1 * z2, z0 * z1 * b2
        inside &= (t0 > 0) & (t1 > 0) & (t2 > 0)
        den = np.maximum(t0 + t1 + t2, EPS)
        pz = (t0 * z0 + t1 * z1 + t2 * z2) / den
        if mut == "affine_z":
            pz = b0 * z0 + b1 * z1 + b2 * z2
        sub_z = zbest[np.ix_(ii, jj)]
        win = inside & (pz >= 0) & ((pz > sub_z) if far else (pz < sub_z))
        if not win.any():
            continue
        wi, wj = np.nonzero(win)
        gi, gj = ii[wi], jj[wj]
        zbest[gi, gj] = pz[wi, wj]
        fbest[gi, gj] = f
        out = (b0, b1, b2) if mut == "affine_bary" else (t0 / den, t1 / den, t2 / den)
        for k in range(3):
            bbest[gi, gj, k] = np.broadcast_to(out[k], win.shape)[wi, wj]
    return bbest, fbest


@pytest.fixture(scope="module")
def verdicts():
    """(mutation, scene) -> (pixels outside the set, worst bary err / bound); the unedited copy is bit-equal to the original"""
    out = {}
    for name in MUTANT_SCENES:
        v, f, cam, (H, W) = S.mesh_scene(name)
        Rm, T = S.camera(cam)
        _, bary, p2f = O.rasterize_mesh(v, f, Rm, T, H, W)
        cb, cf = _mutant(v, f, Rm, T, H, W)
        assert np.array_equal(cf, p2f) and np.array_equal(cb.view(np.int32), bary.view(np.int32)), name
        for mut in MUTATIONS:
            out[mut, name] = _judge(name, *_mutant(v, f, Rm, T, H, W, mut)[::-1])
    return out


@pytest.mark.parametrize("mut", MUTATIONS)
def test_planted_mistakes_are_flagged(verdicts, mut):
    flagged = {name: (o, r) for (m, name), (o, r) in verdicts.items() if m == mut and (o > 0 or r > 1.0)}
    print(mut, {n: (o, round(r, 1)) for (m, n), (o, r) in verdicts.items() if m == mut})
    assert flagged, mut
    if mut == "affine_z":
        assert verdicts[mut, "crossing"][0] > 0            # wrong faces, and only a scene with crossing faces can show them
    if mut == "hw_swapped":
        assert all(verdicts[mut, name][0] > 100 for name in MUTANT_SCENES)
    if mut in ("box_short", "farthest_wins", "x_not_mirrored"):
        assert all(verdicts[mut, name][0] > 0 for name in MUTANT_SCENES)
    if mut == "affine_bary":                                 # the ids are all right: only the barycentric bound can see this
        assert all(verdicts[mut, name] [0] == 0 and verdicts[mut, name][1] > 10 for name in MUTANT_SCENES)
