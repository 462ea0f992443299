"""Banded fp64 reference for the rasteriser (csrc/raster.hip), plain numpy.  Nothing here imports oracle/ or the package;
tests/test_raster_ref_cpu.py pins it against oracle/raycast.py (another algorithm) and oracle/raster.py (the fp32 restatement).

The reference does not name one winner per pixel.  It names the SET OF ANSWERS THAT FP32 ARITHMETIC MAY LEGITIMATELY GIVE, by carrying
a forward error bound through the formulas raster.hip states; the kernel must answer inside the set at every pixel, and where the
set has one element (a *decided* pixel) it must match exactly, with barycentrics inside a derived bound.

Conventions (raster.hip's header): row-vector cameras X_view = X_world.R + T, s = 1 / tan(fov / 2), x_ndc = s v_x / v_z (+X left),
y_ndc = s v_y / v_z (+Y up), pixel (i, j) centre at y = 1 - (2 i + 1) / H, x = 1 - (2 j + 1) / W: EACH AXIS RUNS OVER [-1, 1] ACROSS
ITS OWN SIZE.  pytorch3d scales the longer axis of a non-square image (its NDC range there is [-max(H, W) / min(H, W), ...]), so
non-square output here follows the project's convention only.  View-space z is the depth; the inside test is strict, on the
un-corrected barycentrics; no culling; output barycentrics are perspective-correct; nearest z wins.

Error model, u = 2^-24; the inputs are the fp32 values of verts, R, T (and s, and the point radius) widened to fp64:
  per vertex   v = X.R + T, magnitudes m = |X|.|R| + |T|
               e_z = 8u m_z             three products and three additions, each at most one rounding of a partial result <= m_z, contracted
                                        (fma) or not: <= 6 roundoffs, 8 allowed
               x = s v_x / v_z
               e_x = s (8u m_x + |v_x / v_z| e_z) / |v_z| + 3u |x|
                                        the first-order propagation of the errors of v_x and v_z through the quotient, plus the roundings
                                        of the product, of the quotient and of s itself; e_y likewise, e_xy = max(e_x, e_y)
  per face     distance band (NDC)  d = 2 max e_xy + 8u max(1, |x|, |y|)     over its three vertices: an edge line moves by at most
                                        the larger displacement of its two ends (<= max e_xy) and the pixel centre, the differences and
                                        the two products of the edge function each round once at magnitude <= max(1, |x|, |y|) (8u); the
                                        factor 2 covers a pixel beyond the ends of the edge, where a line through two displaced points
                                        moves further than either
               depth band        t_z = 64u max|z| + 2 max e_z                the perspective-correct depth is a weighted mean of the
                                        three z (moves by <= max e_z with them, 2 allowed for the weights moving too), evaluated in ~20
                                        fp32 operations on positive terms (64u max|z|)
               sliver margin       2 max e_xy * perimeter: how far the signed area can move; |area| <= max(1e-8 - margin, 0) is
                                        skipped like the kernel's degenerate test, |area| < 1e-8 + margin can never be a SURE hit
               max z < 1e-8 is skipped, as in the kernel
  per pixel and face  signed distance from the pixel centre to each edge line = the edge function, oriented by the sign of the area,
               over the edge length;  POSSIBLE if the smallest of the three > -d;  SURE if it is > d, the face is no sliver and its
               perspective-correct depth pz > t_z
  per pixel    zs = min over sure faces of (pz + t_z);  allowed = possible faces with pz - t_z <= zs, plus -1 (empty) if no face is sure
  barycentrics (decided pixel)  |err| <= (d / h_min) (z_max / z_min)^2, h_min = 2 |area| / longest edge: a screen-space barycentric
               moves by band / height, and the 1/z correction b_k / z_k / sum(b / z) stretches that by at most (z_max / z_min)^2
  points       band on the disc edge e_xy + 8u max(1, |x|, |y|, r), depth band e_z, the same allowed-set rule (the kernel draws z >= 0)

A face with a corner at or behind the camera plane while another is in front (it straddles the plane) is outside this reference -
the projection of such a face is an artefact in pytorch3d too - and classify_mesh refuses it.  A face whose fp64 area is exactly 0
(a repeated index) is skipped: the kernel's area and one of its edge functions are then exact zeros as well.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EPS = 1e-8


def _f32_as_f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def pixel_centres(S):
    return 1.0 - (2.0 * np.arange(S, dtype=np.float64) + 1.0) / S


def project(X, R, T, fov):
    """-> x, y, z, e_xy, e_z per vertex (fp64)"""
    X, R, T = _f32_as_f64(X), _f32_as_f64(R).reshape(3, 3), _f32_as_f64(T).reshape(3)
    s = float(np.float32(1.0 / np.tan(np.deg2rad(fov) / 2.0)))
    v = X @ R + T
    m = np.abs(X) @ np.abs(R) + np.abs(T)
    e_z = 8 * U * m[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = v[:, :2] / v[:, 2:3]
        xy = s * q
        e = s * (8 * U * m[:, :2] + np.abs(q) * e_z[:, None]) / np.abs(v[:, 2:3]) + 3 * U * np.abs(xy)
    return xy[:, 0], xy[:, 1], v[:, 2], e.max(1), e_z


class Allowed:
    """The per-pixel sets of answers: records (pixel, primitive) plus ``empty_ok`` [H, W] (-1 is allowed there)"""

    def __init__(self, H, W, n, pix, prim, empty_ok):
        self.H, self.W, self.n = H, W, n
        order = np.argsort(pix * n + prim, kind="stable")
        self.pix, self.prim = pix[order], prim[order]
        self.keys = self.pix * n + self.prim
        self.empty_ok = empty_ok
        self.n_prims = np.bincount(self.pix, minlength=H * W).reshape(H, W)

    @property
    def size(self):
        return self.n_prims + self.empty_ok

    @property
    def decided(self):
        return self.size == 1

    @property
    def covered(self):
        """pixels some primitive may cover"""
        return self.n_prims > 0

    @property
    def winner(self):
        """the one answer of a decided pixel (-1: empty); -2 on undecided pixels"""
        w = np.full(self.H * self.W, -2, dtype=np.int64)
        w[self.empty_ok.reshape(-1)] = -1
        w[self.pix] = self.prim
        w[~self.decided.reshape(-1)] = -2
        return w.reshape(self.H, self.W)

    def contains(self, ids):
        """ids int [H, W] -> bool [H, W]: is each pixel's answer in its set"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        assert ids.shape[0] == self.H * self.W
        inr = (ids >= 0) & (ids < self.n)
        ok = np.isin(np.arange(self.H * self.W) * self.n + np.where(inr, ids, 0), self.keys) & inr
        ok |= (ids == -1) & self.empty_ok.reshape(-1)
        return ok.reshape(self.H, self.W)

    def undecided_share(self):
        """undecided pixels / covered pixels"""
        return float((~self.decided).sum()) / max(int(self.covered.sum()), 1)


def _expand(lo_i, hi_i, lo_j, hi_j):
    """ragged boxes -> (box index, i, j) of every pixel of every box"""
    ni, nj = np.maximum(hi_i - lo_i + 1, 0), np.maximum(hi_j - lo_j + 1, 0)
    cnt = ni * nj
    box = np.repeat(np.arange(len(cnt)), cnt)
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return box, lo_i[box] + off // nj[box], lo_j[box] + off % nj[box]


def _pixel_box(lo, hi, S):
    """NDC interval [lo, hi] -> inclusive pixel index range that holds every centre inside it (larger ndc = smaller index)"""
    a = np.floor(((1.0 - hi) * S - 1.0) / 2.0)
    b = np.ceil(((1.0 - lo) * S - 1.0) / 2.0)
    return np.clip(a, 0, S).astype(np.int64), np.clip(b, -1, S - 1).astype(np.int64)


def _resolve(H, W, n, p, prim, possible, sure, z, tz):
    zs = np.full(H * W, np.inf)
    np.minimum.at(zs, p[sure], (z + tz)[sure])
    any_sure = np.zeros(H * W, dtype=bool)
    any_sure[p[sure]] = True
    keep = possible & (z - tz <= zs[p])
    return Allowed(H, W, n, p[keep], prim[keep], ~any_sure.reshape(H, W)), keep


def classify_mesh(verts, faces, R, T, H, W, fov=60.0):
    """-> (allowed: Allowed, decided bool [H, W], bary f64 [H, W, 3], bound f64 [H, W]).
    bary: the perspective-correct barycentrics of the decided winner (-1 on decided-empty pixels, NaN on undecided ones);
    bound: the per-pixel bound on them (0 on decided-empty pixels, NaN on undecided ones)."""
    faces = np.asarray(faces, dtype=np.int64)
    nf = faces.shape[0]
    x, y, z, exy, ez = project(verts, R, T, fov)
    fz = z[faces]
    live = ~(fz.max(1) < EPS)                                # (a face wholly behind the camera: skipped, as in the kernel)
    if (live & (fz.min(1) <= ez[faces].max(1))).any():
        raise ValueError("a face straddles the camera plane: outside the banded reference")
    fx, fy = np.where(live[:, None], x[faces], 0.0), np.where(live[:, None], y[faces], 0.0)
    fz = np.where(live[:, None], fz, 1.0)
    fe = np.where(live, exy[faces].max(1), 0.0)
    d = 2 * fe + 8 * U * np.maximum(1.0, np.maximum(np.abs(fx), np.abs(fy)).max(1))
    tz = 64 * U * np.abs(fz).max(1) + 2 * np.where(live, ez[faces].max(1), 0.0)
    area = (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]) - (fy[:, 2] - fy[:, 0]) * (fx[:, 1] - fx[:, 0])
    # edge k is opposite vertex k: from vertex k+1 to vertex k+2
    ex, ey = np.roll(fx, -2, 1) - np.roll(fx, -1, 1), np.roll(fy, -2, 1) - np.roll(fy, -1, 1)
    elen = np.hypot(ex, ey)
    margin = 2 * fe * elen.sum(1)
    live &= ~(np.abs(area) <= np.maximum(EPS - margin, 0.0))
    sliver = np.abs(area) < EPS + margin
    with np.errstate(divide="ignore", invalid="ignore"):
        hmin = 2 * np.abs(area) / elen.max(1)
        bbound = (d / hmin) * (fz.max(1) / fz.min(1)) ** 2
    ys, xs = pixel_centres(H), pixel_centres(W)
    lo_i, hi_i = _pixel_box(fy.min(1) - d, fy.max(1) + d, H)
    lo_j, hi_j = _pixel_box(fx.min(1) - d, fx.max(1) + d, W)
    hi_i = np.where(live, hi_i, lo_i - 1)
    f, ii, jj = _expand(lo_i, hi_i, lo_j, hi_j)
    px, py = xs[jj], ys[ii]
    sgn = np.sign(area)[f]
    E, dist = [], []
    for k in range(3):
        ax, ay = fx[f, (k + 1) % 3], fy[f, (k + 1) % 3]
        Ek = (px - ax) * ey[f, k] - (py - ay) * ex[f, k]
        E.append(Ek)
        dist.append(Ek * sgn / elen[f, k])
    dmin = np.minimum(np.minimum(dist[0], dist[1]), dist[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.stack(E, 1) / area[f][:, None]
        zf = fz[f]
        t = b * np.roll(zf, -1, 1) * np.roll(zf, -2, 1)
        den = t.sum(1)
        pz = (t * zf).sum(1) / den
        pb = t / den[:, None]
    possible = dmin > -d[f]
    sure = (dmin > d[f]) & ~sliver[f] & (pz > tz[f])
    pz = np.where(possible, pz, np.inf)
    p = ii * W + jj
    allowed, keep = _resolve(H, W, nf, p, f, possible, sure, pz, tz[f])
    decided = allowed.decided
    bary = np.full((H * W, 3), np.nan)
    bound = np.full(H * W, np.nan)
    dflat = decided.reshape(-1)
    empty = dflat & allowed.empty_ok.reshape(-1)
    bary[empty], bound[empty] = -1.0, 0.0
    one = keep & dflat[p]
    bary[p[one]], bound[p[one]] = pb[one], bbound[f[one]]
    return allowed, decided, bary.reshape(H, W, 3), bound.reshape(H, W)


def classify_points(pts, R, T, radius, H, W, fov=60.0):
    """-> allowed: Allowed (the per-pixel sets of point indices the map may hold; -1 where ``empty_ok``)"""
    x, y, z, exy, ez = project(pts, R, T, fov)
    n = x.shape[0]
    r = float(np.float32(radius))
    live = z > -ez                                           # (the kernel skips z < 0)
    live &= np.isfinite(x) & np.isfinite(y) & np.isfinite(exy)
    xx, yy = np.where(live, x, 0.0), np.where(live, y, 0.0)
    band = np.where(live, exy, 0.0) + 8 * U * np.maximum(np.maximum(1.0, r), np.maximum(np.abs(xx), np.abs(yy)))
    ys, xs = pixel_centres(H), pixel_centres(W)
    # (a point whose band swallows the image is a candidate everywhere; clip keeps the index arithmetic finite)
    reach = np.minimum(r + band, 1e6)
    xx, yy = np.clip(xx, -1e6, 1e6), np.clip(yy, -1e6, 1e6)
    lo_i, hi_i = _pixel_box(yy - reach, yy + reach, H)
    lo_j, hi_j = _pixel_box(xx - reach, xx + reach, W)
    hi_i = np.where(live, hi_i, lo_i - 1)
    q, ii, jj = _expand(lo_i, hi_i, lo_j, hi_j)
    dist = np.hypot(xs[jj] - x[q], ys[ii] - y[q])
    possible = dist < r + band[q]
    sure = (dist < r - band[q]) & (z[q] > ez[q])
    allowed, _ = _resolve(H, W, n, ii * W + jj, q, possible, sure, z[q], ez[q])
    return allowed
