"""fp64 reference for csrc/depth_order.hip (``occlusion.depth_image`` / ``depth_order``): plain numpy and torch on the CPU, dense
[H W, F].  It imports neither oracle/ nor the kernels; it restates the definition.

    u = fx X / Z + px, v = fy Y / Z + py;  pixel (row i, col j) has its centre q at (j + 0.5, i + 0.5)
    face (a, b, c):  e_a = cross(c - b, q - b), e_b = cross(a - c, q - c), e_c = cross(b - a, q - a); it covers the pixel when the three
    are all > 0 or all < 0;  z = s / (e_a / Z_a + e_b / Z_b + e_c / Z_c), s = e_a + e_b + e_c (= 1 / sum w_i / Z_i, w_i = e_i / s)
    a face is skipped whole when its screen area (b - a) x (c - a) is zero or any vertex has Z <= 1e-6
    depth = min z over the covering faces (+inf: none), face_id = the lowest index that attains it (-1: none)
    x = sign(c) (D_o - D_h) / tau where c != 0 and both depths are finite;  L = (tau / n) sum |c| softplus(x),  n = sum |c| (whole image)
    softplus(x) = max(x, 0) + log1p(exp(-|x|));  L = 0 exactly when n == 0
    the gradient holds the winner of every pixel fixed (torch autograd through z of that one face); nothing flows through D_h

Like tests/_raster_ref.py it also says which pixels fp32 arithmetic may answer differently, by a forward bound (u = 2^-24; the inputs are
the fp32 vertices widened to fp64, so Z is exact):

  projected point   each coordinate moves by at most e_pt = 12 u M, M = the largest of H, W, |u|, |v|, |u - px|, |v - py| over the
                    face's vertices: the silhouette's IVLM_SILHOUETTE_POS_ULPS for a projected point and the differences taken from
                    it (the projection itself is a division and an fma: 2 sqrt 2 u M of the 12)
  edge function     E = ex wy - ey wx with ex = Qx - Px (error <= 2 e_pt + u |ex|), wy = qy - Py (error <= e_pt + u |wy|; q is exact),
                    each product rounded once, the difference rounded once (no contraction: the file is built with -ffp-contract=off):
                    |dE| <= e_pt (2 |wx| + 2 |wy| + |ex| + |ey|) + 3 u (|ex wy| + |ey wx|) + u |E|, to first order.
                    band_E = 2 x that (the factor covers the second-order terms and the pixel grid's own rounding: q is exact up to
                    2^23, so it costs nothing here).  The same formula with w = c - a (error 2 e_pt: + e_pt (|ex| + |ey|)) bounds the area.
  coverage          a face is POSSIBLE at a pixel when E_i sgn(area) > -band_i for its three edges, SURE when E_i sgn(area) > +band_i and
                    |area| > its band
  depth             dz/de_i = n_i / t^2 with t = sum e_j / Z_j, n_i = sum_j e_j (1 / Z_j - 1 / Z_i); the three 1 / Z_i, the three products,
                    two additions each for s and t and the division round once each at positive magnitudes (<= 8 u z):
                    band_z = sum_i |n_i| band_i / t^2 + 8 u z
  per pixel         zs = min over sure faces of (z + band_z); allowed = the possible faces with z - band_z <= zs, plus "empty" when no
                    face is sure.  A pixel is DECIDED when that set has one element: the kernel must give it, with depth within band_z.
                    Otherwise it is UNDECIDED - for the coverage (a centre within the band of an edge) or for the gradient (the two
                    nearest depths within their bands of each other): the kernel must answer inside the set, and the tests of the term
                    give such pixels signed_weight = 0 on both sides of the comparison.
"""
import numpy as np
import torch

U = 2.0 ** -24
MIN_Z = 1e-6
POINT_ULPS = 12          # e_pt = POINT_ULPS u M
UNDECIDED_CAP = 0.02     # undecided pixels / covered pixels, asserted by every test that uses the rule


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, radius=0.5):
    """-> (vertices f64 [(n_lat - 1) n_lon + 2, 3], faces int64 [2 n_lon (n_lat - 1), 3]), outward"""
    v = [(0.0, radius, 0.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.cos(th), radius * np.sin(th) * np.sin(ph)))
    v.append((0.0, -radius, 0.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon  # noqa: E731
    last = len(v) - 1
    for j in range(n_lon):
        f.append((0, ring(1, j + 1), ring(1, j)))
        f.append((last, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i, j + 1), ring(i + 1, j)))
            f.append((ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)))
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def rotation(axis, angle):
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def tilted_sphere(n_lat, n_lon, centre=(0.07, -0.05, 3.0), radius=0.5):
    """the sphere turned by 0.4 about (1, 2, 3), so that no edge runs through a row of pixel centres by symmetry -> (f32 [N,3], int64)"""
    v, f = uv_sphere(n_lat, n_lon, radius)
    return (v @ rotation((1.0, 2.0, 3.0), 0.4).T + np.asarray(centre)).astype(np.float32), f


def camera(H, W, focal):
    """(fx, fy, px, py) with an off-centre principal point"""
    return float(focal), float(focal), W / 2 + 0.3, H / 2 - 0.2


# the two scenes of the z-buffer tests: (n_lat, n_lon, H, W, focal); 42 vertices / 80 faces and 738 vertices / 1472 faces
SMALL = (6, 8, 24, 40, 44.0)
LARGE = (24, 32, 48, 64, 75.0)


def scene(which):
    n_lat, n_lon, H, W, focal = which
    v, f = tilted_sphere(n_lat, n_lon)
    return v, f, camera(H, W, focal), H, W


def plane(z0, half=6.0):
    """a tilted occluder: two triangles of z = z0 + 0.1 x + 0.05 y, larger than any image here"""
    xy = np.array([(-half, -half), (half, -half), (half, half), (-half, half)], dtype=np.float64)
    v = np.concatenate([xy, (z0 + 0.1 * xy[:, :1] + 0.05 * xy[:, 1:])], 1).astype(np.float32)
    return v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int64)


def weight_image(H, W, seed=5):
    """a signed weight image that holds both signs, several magnitudes and zeros"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1.5, -1.0, 0.0, 0.5, 1.0, 2.0], dtype=np.float32), size=(H, W))


# ---- the dense definition ---------------------------------------------------------------------------------------------------------
def _edge(px_, py_, qx_, qy_, x, y):
    """cross(Q - P, q - P) for every (pixel, face): P, Q [F], x, y [P] -> [P,F]"""
    return (qx_ - px_)[None, :] * (y[:, None] - py_[None, :]) - (qy_ - py_)[None, :] * (x[:, None] - px_[None, :])


def dense(verts, faces, cam, H, W):
    """numpy fp64 of the fp32 vertices (an fp64 array is taken as it is: central differences step below fp32's spacing) -> dict of
    [H W, F] arrays (e [3], z, inside) and per-face arrays (live, area, uv [F,3,2], Z [F,3])"""
    fx, fy, px, py = cam
    V = np.asarray(verts)
    V = V if V.dtype == np.float64 else V.astype(np.float32).astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    okidx = ((faces >= 0) & (faces < V.shape[0])).all(1)
    fc = np.where(okidx[:, None], faces, 0)
    Z = V[fc, 2]
    live = okidx & (Z > MIN_Z).all(1)
    Zs = np.where(live[:, None], Z, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([fx * V[:, 0] / V[:, 2] + px, fy * V[:, 1] / V[:, 2] + py], 1)
    t = np.where(live[:, None, None], uv[fc], 0.0)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    live &= area != 0.0
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    x, y = jj.reshape(-1) + 0.5, ii.reshape(-1) + 0.5
    ea = _edge(b[:, 0], b[:, 1], c[:, 0], c[:, 1], x, y)
    eb = _edge(c[:, 0], c[:, 1], a[:, 0], a[:, 1], x, y)
    ec = _edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], x, y)
    inside = live[None, :] & (((ea > 0) & (eb > 0) & (ec > 0)) | ((ea < 0) & (eb < 0) & (ec < 0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = ea + eb + ec
        tt = ea / Zs[:, 0] + eb / Zs[:, 1] + ec / Zs[:, 2]
        z = s / tt
    return {"e": (ea, eb, ec), "z": z, "t": tt, "inside": inside, "live": live, "area": area, "uv": t, "Z": Zs, "x": x, "y": y}


def depth_image(verts, faces, cam, H, W):
    """-> (depth f64 [H,W] (+inf: empty), face_id int64 [H,W] (-1: empty; the lowest index among equal depths))"""
    d = dense(verts, faces, cam, H, W)
    z = np.where(d["inside"], d["z"], np.inf)
    depth = z.min(1)
    fid = np.where(np.isfinite(depth), np.argmin(z, 1), -1)  # argmin: the first of equal minima
    return depth.reshape(H, W), fid.reshape(H, W)


# ---- which pixels fp32 may answer differently -------------------------------------------------------------------------------------
class Classified:
    """allowed [H W, F] bool, empty_ok [H W] bool, decided [H,W] bool, winner int64 [H,W] (-2 on undecided pixels), depth f64 [H,W] and
    band f64 [H,W] (of the decided winner; +inf / 0 on decided-empty pixels, NaN on undecided ones), covered [H,W] (a face is possible)"""

    def __init__(self, H, W, allowed, empty_ok, z, band_z):
        self.H, self.W, self.allowed, self.empty_ok = H, W, allowed, empty_ok
        n = allowed.sum(1) + empty_ok
        dec = n == 1
        first = np.argmax(allowed, 1)
        win = np.where(allowed.any(1), first, -1)
        self.decided = dec.reshape(H, W)
        self.winner = np.where(dec, win, -2).reshape(H, W)
        rows = np.arange(H * W)
        has = dec & (win >= 0)
        self.depth = np.where(has, z[rows, first], np.where(dec, np.inf, np.nan)).reshape(H, W)
        self.band = np.where(has, band_z[rows, first], np.where(dec, 0.0, np.nan)).reshape(H, W)
        self.covered = allowed.any(1).reshape(H, W)

    def undecided_share(self):
        return float((~self.decided).sum()) / max(int(self.covered.sum()), 1)

    def contains(self, face_id):
        ids = np.asarray(face_id, dtype=np.int64).reshape(-1)
        ok = (ids == -1) & self.empty_ok
        inr = (ids >= 0) & (ids < self.allowed.shape[1])
        ok |= inr & self.allowed[np.arange(ids.shape[0]), np.where(inr, ids, 0)]
        return ok.reshape(self.H, self.W)


def _band(px_, py_, qx_, qy_, x, y, E, e_pt):
    ex, ey = np.abs(qx_ - px_)[None, :], np.abs(qy_ - py_)[None, :]
    wx, wy = np.abs(x[:, None] - px_[None, :]), np.abs(y[:, None] - py_[None, :])
    return 2.0 * (e_pt[None, :] * (2 * wx + 2 * wy + ex + ey) + 3 * U * (ex * wy + ey * wx) + U * np.abs(E))


def classify(verts, faces, cam, H, W, extra_px=0.0):
    """-> Classified; extra_px: a further displacement of every projected point that the caller knows of (a transform before it)"""
    fx, fy, px, py = cam
    d = dense(verts, faces, cam, H, W)
    t, live, area, Zs = d["uv"], d["live"], d["area"], d["Z"]
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    M = np.maximum(max(H, W), np.maximum(np.abs(t).max((1, 2)), np.abs(t - np.array([px, py])).max((1, 2))))
    e_pt = POINT_ULPS * U * M + extra_px
    x, y = d["x"], d["y"]
    ea, eb, ec = d["e"]
    ba = _band(b[:, 0], b[:, 1], c[:, 0], c[:, 1], x, y, ea, e_pt)
    bb = _band(c[:, 0], c[:, 1], a[:, 0], a[:, 1], x, y, eb, e_pt)
    bc = _band(a[:, 0], a[:, 1], b[:, 0], b[:, 1], x, y, ec, e_pt)
    ab, ac = np.abs(b - a), np.abs(c - a)
    band_area = 2.0 * (e_pt * (3 * ac[:, 0] + 3 * ac[:, 1] + ab[:, 0] + ab[:, 1]) + 3 * U * (ab[:, 0] * ac[:, 1] + ab[:, 1] * ac[:, 0])
                       + U * np.abs(area))
    sg = np.sign(area)[None, :]
    lo = np.minimum(np.minimum(ea * sg + ba, eb * sg + bb), ec * sg + bc)
    hi = np.minimum(np.minimum(ea * sg - ba, eb * sg - bb), ec * sg - bc)
    # (a live face whose fp64 area is within its band may be skipped by the kernel or not: possible, never sure)
    possible = live[None, :] & (lo > 0)
    sure = live[None, :] & (hi > 0) & (np.abs(area) > band_area)[None, :]
    iz = 1.0 / Zs
    na = eb * (iz[:, 1] - iz[:, 0]) + ec * (iz[:, 2] - iz[:, 0])
    nb = ea * (iz[:, 0] - iz[:, 1]) + ec * (iz[:, 2] - iz[:, 1])
    nc = ea * (iz[:, 0] - iz[:, 2]) + eb * (iz[:, 1] - iz[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        band_z = (np.abs(na) * ba + np.abs(nb) * bb + np.abs(nc) * bc) / (d["t"] * d["t"]) + 8 * U * np.abs(d["z"])
    z = d["z"]
    # a possible face that is not inside in fp64 (its centre is within the band outside an edge): its plane's depth there
    zs = np.where(sure, z + band_z, np.inf).min(1)
    good = possible & np.isfinite(z) & np.isfinite(band_z)
    allowed = good & (z - band_z <= zs[:, None])
    allowed |= possible & ~good  # (a degenerate evaluation: never excluded by depth)
    return Classified(H, W, allowed, ~sure.any(1), z, band_z)


# ---- the term, winner fixed, in torch (fp64: the yardstick; fp32: what measures the tolerance constants) ----------------------------
def winner_depth(verts, faces, winner, cam, H, W):
    """verts torch [N,3] (any float dtype, may require grad), winner int64 [H,W] (< 0: no face) -> z [H W] of that face at each pixel
    (0 where winner < 0), by the definition above, operation by operation"""
    fx, fy, px, py = cam
    w = torch.as_tensor(np.asarray(winner).reshape(-1), dtype=torch.int64)
    has = w >= 0
    fc = torch.as_tensor(np.asarray(faces, dtype=np.int64))[torch.where(has, w, torch.zeros_like(w))]
    u = fx * verts[:, 0] / verts[:, 2] + px
    v = fy * verts[:, 1] / verts[:, 2] + py
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    x = torch.as_tensor(jj.reshape(-1) + 0.5, dtype=verts.dtype)
    y = torch.as_tensor(ii.reshape(-1) + 0.5, dtype=verts.dtype)
    ax, ay, bx, by, cx, cy = u[fc[:, 0]], v[fc[:, 0]], u[fc[:, 1]], v[fc[:, 1]], u[fc[:, 2]], v[fc[:, 2]]
    Za, Zb, Zc = verts[fc[:, 0], 2], verts[fc[:, 1], 2], verts[fc[:, 2], 2]
    ea = (cx - bx) * (y - by) - (cy - by) * (x - bx)
    eb = (ax - cx) * (y - cy) - (ay - cy) * (x - cx)
    ec = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
    s = (ea + eb) + ec
    t = (ea * (1.0 / Za) + eb * (1.0 / Zb)) + ec * (1.0 / Zc)
    return torch.where(has, s / t, torch.zeros_like(s))


def order_terms(verts, faces, winner, cam, H, W, occluder_depth, signed_weight, tau):
    """-> the per-pixel terms (tau / n) |c| softplus(x) [H W] in verts' dtype (0 where the pixel does not count); their sum is L"""
    dt = verts.dtype
    z = winner_depth(verts, faces, winner, cam, H, W)
    c = torch.as_tensor(np.asarray(signed_weight, dtype=np.float32).reshape(-1)).to(dt)
    dh = torch.as_tensor(np.asarray(occluder_depth, dtype=np.float32).reshape(-1)).to(dt)
    n = c.abs().double().sum()
    if float(n) == 0.0:
        return z * 0.0  # (exact zeros that still hang on verts, so that autograd gives an exact zero gradient)
    counts = (c != 0) & torch.isfinite(dh) & torch.as_tensor(np.asarray(winner).reshape(-1) >= 0)
    x = torch.sign(c) * (z - torch.where(counts, dh, torch.zeros_like(dh))) / tau
    sp = torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    return torch.where(counts, (tau / n).to(dt) * (c.abs() * sp), torch.zeros_like(sp))


def depth_order(verts, faces, winner, cam, H, W, occluder_depth, signed_weight, tau, dtype=torch.float64, through=None):
    """One pose -> dict(L, g [N,3] (dL/dverts), A = sum |terms|, s [N,3] = sum_px |d term_px / d verts|; with ``through`` = (fn, params):
    verts = fn(*params) and g_p, s_p per parameter too).  dtype float64 is the yardstick; float32 the same operations in fp32, sums in
    fp64 (what the kernel promises), which is what the tests' K is measured with."""
    if through is None:
        leaf = [torch.as_tensor(np.asarray(verts, dtype=np.float32)).to(dtype).requires_grad_(True)]
        make = lambda v: v  # noqa: E731
    else:
        fn, params = through
        leaf = [torch.as_tensor(np.asarray(p, dtype=np.float32)).to(dtype).requires_grad_(True) for p in params]
        make = fn

    def terms(*xs):
        return order_terms(make(*xs), faces, winner, cam, H, W, occluder_depth, signed_weight, tau)

    with torch.enable_grad():  # (a test module elsewhere in the suite may have switched autograd off for the process)
        t = terms(*leaf)
        L = t.double().sum()
    grads = torch.autograd.grad(L, leaf, allow_unused=True, retain_graph=True)
    out = {"L": float(L.detach()), "A": float(t.detach().double().abs().sum()),
           "g": [np.zeros(tuple(x.shape)) if g is None else g.detach().double().numpy() for g, x in zip(grads, leaf)]}
    if dtype == torch.float64:  # the tolerance scales: sum over the pixels of |d term / d parameter|
        live = torch.nonzero(t.detach() != 0).reshape(-1)
        scales = [np.zeros(tuple(x.shape)) for x in leaf]
        for k in live.tolist():
            with torch.enable_grad():
                tk = t[k]
            gk = torch.autograd.grad(tk, leaf, allow_unused=True, retain_graph=True)
            for s, g in zip(scales, gk):
                if g is not None:
                    s += g.detach().abs().numpy()
        out["s"] = scales
    return out


def ratios(got_L, got_g, want):
    """the errors of a result against the fp64 ``want`` in units of 2^-24 x scale -> (ratio of L, largest ratio of a gradient entry);
    an entry whose scale is 0 must be an exact 0"""
    def ratio(err, scale):
        err, scale = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(scale, dtype=np.float64)
        zero = scale == 0
        if (err[zero] != 0).any():
            return float("inf")
        return float((err[~zero] / (U * scale[~zero])).max()) if (~zero).any() else 0.0

    rl = ratio([got_L - want["L"]], [want["A"]])
    rg = max(ratio(np.asarray(g, dtype=np.float64) - w, s) for g, w, s in zip(got_g, want["g"], want["s"]))
    return rl, rg


# ---- the inputs of tests/test_depth_order_gpu.py (and of the tolerance measurement below) -------------------------------------------
# the small sphere (front at z = 2.5, rim at z = 3) against the tilted plane: name -> (z0 of the plane, tau)
ORDER_CASES = {"front": (3.6, 0.01), "behind": (2.2, 0.01), "straddle": (2.75, 0.01), "straddle_soft": (2.75, 0.05)}
POSE_R6 = (0.9, 0.2, -0.1, 1.1, 0.3, -0.2)   # stretched and sheared: the Gram-Schmidt has work to do
POSE_T = (0.07, -0.05, 3.0)
POSE_FWD_ULPS = 6                            # IVLM_POSE_FWD_ULPS: what the fused transform may move a vertex coordinate by


def order_case(name):
    """-> dict(verts f32, faces, cam, H, W, occ f32 [H,W], c f32 [H,W] (0 at undecided pixels), tau, cls, winner, want (fp64))"""
    z0, tau = ORDER_CASES[name]
    v, f, cam, H, W = scene(SMALL)
    pv, pf = plane(z0)
    occ = depth_image(pv, pf, cam, H, W)[0].astype(np.float32)
    cls = classify(v, f, cam, H, W)
    c = np.where(cls.decided, weight_image(H, W), np.float32(0.0)).astype(np.float32)
    winner = np.where(cls.decided, cls.winner, -1)
    want = depth_order(v, f, winner, cam, H, W, occ, c, tau)
    return {"verts": v, "faces": f, "cam": cam, "H": H, "W": W, "occ": occ, "c": c, "tau": tau, "cls": cls, "winner": winner, "want": want}


def posed(r6, t):
    """the canonical small sphere under (r6, t, s = 1), y = v R + t with row vectors, in the dtype of r6: R's columns are the
    Gram-Schmidt of the two interleaved columns of r6 and their cross product (the fit's convention, restated)"""
    base = torch.as_tensor(uv_sphere(SMALL[0], SMALL[1])[0].astype(np.float32)).to(r6.dtype)
    a = r6.reshape(3, 2)
    b1 = a[:, 0] / a[:, 0].norm()
    u2 = a[:, 1] - (b1 * a[:, 1]).sum() * b1
    b2 = u2 / u2.norm()
    R = torch.stack((b1, b2, torch.linalg.cross(b1, b2)), dim=-1)
    return base[:, 0:1] * R[0] + base[:, 1:2] * R[1] + base[:, 2:3] * R[2] + t


def pose_case():
    """the straddle_soft case with the sphere placed by a 6-D rotation and a translation; the classification allows for the fused
    transform's documented forward error on top of the projection's"""
    z0, tau = ORDER_CASES["straddle_soft"]
    _, f, cam, H, W = scene(SMALL)
    r6, t = np.array(POSE_R6, dtype=np.float32), np.array(POSE_T, dtype=np.float32)
    v = posed(torch.as_tensor(r6).double(), torch.as_tensor(t).double()).numpy().astype(np.float32)
    pv, pf = plane(z0)
    occ = depth_image(pv, pf, cam, H, W)[0].astype(np.float32)
    extra = 2.0 * cam[0] / float(v[:, 2].min()) * POSE_FWD_ULPS * U * float(np.abs(v).max() + np.abs(t).max())
    cls = classify(v, f, cam, H, W, extra_px=extra)
    c = np.where(cls.decided, weight_image(H, W, seed=9), np.float32(0.0)).astype(np.float32)
    winner = np.where(cls.decided, cls.winner, -1)
    want = depth_order(None, f, winner, cam, H, W, occ, c, tau, through=(posed, (r6, t)))
    return {"r6": r6, "t": t, "faces": f, "cam": cam, "H": H, "W": W, "occ": occ, "c": c, "tau": tau, "cls": cls, "winner": winner,
            "want": want}


if __name__ == "__main__":  # measure K: python tests/_depth_order_ref.py
    worst = [0.0, 0.0]
    for which in (SMALL, LARGE):
        v, f, cam, H, W = scene(which)
        cls = classify(v, f, cam, H, W)
        d, fid = depth_image(v, f, cam, H, W)
        front = np.where(np.isfinite(d), d, np.nan)
        print(f"scene {which}: covered {int(cls.covered.sum())}, undecided {int((~cls.decided).sum())}, share {cls.undecided_share():.4f}, "
              f"largest depth band {np.nanmax(cls.band):.2e}, depth range {np.nanmin(front):.3f} .. {np.nanmax(front):.3f}")
    for name in ORDER_CASES:
        k = order_case(name)
        got = depth_order(k["verts"], k["faces"], k["winner"], k["cam"], k["H"], k["W"], k["occ"], k["c"], k["tau"], dtype=torch.float32)
        r = ratios(got["L"], got["g"], k["want"])
        worst = [max(a, b) for a, b in zip(worst, r)]
        print(f"{name}: L {k['want']['L']:.6e}, counted {int((k['c'] != 0).sum())}, fp32 / fp64 ratios: L {r[0]:.2f}, gradient {r[1]:.2f}")
    k = pose_case()
    got = depth_order(None, k["faces"], k["winner"], k["cam"], k["H"], k["W"], k["occ"], k["c"], k["tau"], dtype=torch.float32,
                      through=(posed, (k["r6"], k["t"])))
    r = ratios(got["L"], got["g"], k["want"])
    worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"pose: L {k['want']['L']:.6e}, undecided share {k['cls'].undecided_share():.4f}, ratios: L {r[0]:.2f}, gradient {r[1]:.2f}")
    print(f"worst ratios: L {worst[0]:.2f}, gradient {worst[1]:.2f}")
