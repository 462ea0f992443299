"""fp64 torch restatement of what interactvlm_amd.contact_icp computes, on the CPU and for ONE cloud pair (no batch axis):
the nearest neighbour, the alignment, both loop variants and the normal filter.  Row-vector convention: s x R + T ~ y.

Written from the definitions (pytorch3d's documented ``knn_points`` / Umeyama, and the loop as DESIGN 4.39 describes it), pinned
to the reference's own fp64 results by tests/test_contact_icp_cpu.py through tests/golden/contact_icp.npz.
"""
from __future__ import annotations

import torch

EPS = 1e-9


def f64(t):
    return t.detach().cpu().double()


def sqdist(q, t):
    """[N_o, N_h] direct sums of squared differences"""
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)


def nearest(q, t):
    """-> (idx int64 [N_o] lowest index of the minimum, d2 [N_o], relative gap [N_o] between best and second best: inf for one target)"""
    d = sqdist(f64(q), f64(t))
    best = d.min(1).values
    ar = torch.arange(d.shape[1]).expand_as(d)
    idx = torch.where(d == best[:, None], ar, torch.full_like(ar, d.shape[1])).min(1).values
    if d.shape[1] > 1:
        d_wo = d.clone()
        d_wo[torch.arange(d.shape[0]), idx] = float("inf")
        second = d_wo.min(1).values
        gap = (second - best) / second.clamp_min(1e-300)
    else:
        gap = torch.full_like(best, float("inf"))
    return idx, best, gap


def apply(X, R, T, s):
    return s * (X @ R) + T


def align(X, Y, w=None, estimate_scale=False, allow_reflection=False, with_singular=False):
    """Umeyama as the reference forms it: centroids by w, centred points multiplied by w (the covariance carries w^2), both
    divided by max(sum w, 1e-9).  -> (R [3,3], T [3], s []) (+ the singular values with_singular)"""
    X, Y = f64(X), f64(Y)
    w = torch.ones(X.shape[0], dtype=torch.float64) if w is None else f64(w)
    W = w.sum().clamp_min(EPS)
    mx = (w[:, None] * X).sum(0) / W
    my = (w[:, None] * Y).sum(0) / W
    Xc = (X - mx) * w[:, None]
    Yc = (Y - my) * w[:, None]
    C = Xc.T @ Yc / W
    U, S, Vh = torch.linalg.svd(C)
    E = torch.eye(3, dtype=torch.float64)
    if not allow_reflection:
        E[2, 2] = torch.det(U @ Vh)
    R = U @ E @ Vh
    s = torch.ones((), dtype=torch.float64)
    if estimate_scale:
        s = (torch.diagonal(E) * S).sum() / ((Xc * Xc).sum() / W).clamp_min(EPS)
    T = my - s * (mx @ R)
    return (R, T, s, S) if with_singular else (R, T, s)


def rmse(X, Ynn, R, T, s, w=None):
    X, Ynn = f64(X), f64(Ynn)
    w = torch.ones(X.shape[0], dtype=torch.float64) if w is None else f64(w)
    return (((apply(X, R, T, s) - Ynn) ** 2).sum(1) * w).sum().div(w.sum().clamp_min(EPS)).sqrt()


def _identity():
    return torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.ones((), dtype=torch.float64)


def icp_as_reference(X, Y, Xn=None, Yn=None, init=None, max_iterations=10, thr=1e-6, estimate_scale=False, allow_reflection=False):
    """The loop as the reference runs it: the query is built ONCE from init (normals not rotated) and never rebuilt, and the
    relative error is (combined - prev) / prev <= thr with combined = rmse + (1 - cos of the neighbour's normal with its rotated
    self) per point.  -> dict(converged, rmse, R, T, s, history [(R, T, s)], idx)"""
    X, Y = f64(X), f64(Y)
    R, T, s = _identity() if init is None else tuple(f64(t) for t in init)
    q = apply(X, R, T, s)
    t = Y
    if Xn is not None:
        q = torch.cat([q, f64(Xn)], -1)
        t = torch.cat([Y, -f64(Yn)], -1)
    history, prev, converged, err, idx = [], None, False, None, None
    for _ in range(max_iterations):
        idx = nearest(q, t)[0]
        nn = t[idx]
        nn_p, nn_n = nn[:, :3], -nn[:, 3:]
        R, T, s = align(X, nn_p, None, estimate_scale, allow_reflection)
        history.append((R, T, s))
        err = rmse(X, nn_p, R, T, s)
        combined = err + (1 - ((s * (nn_n @ R)) * nn_n).sum(1)) if Xn is not None else err.reshape(1)
        rel = torch.ones(1, dtype=torch.float64) if prev is None else (combined - prev) / prev
        if bool((rel <= thr).all()):
            converged = True
            break
        prev = combined
    return dict(converged=converged, rmse=err, R=R, T=T, s=s, history=history, idx=idx)


def icp_requery(X, Y, Xn=None, Yn=None, init=None, w=None, max_iterations=10, thr=1e-6, estimate_scale=False, allow_reflection=False):
    """The loop the name promises: queries [s x R + T, n R] rebuilt from the current transform at every iteration; ends when
    (prev - rmse) / prev <= thr (from the second iteration on) or rmse == 0.
    -> dict(converged, iterations, rmse, R, T, s, history, idx, rmse_history)"""
    X, Y = f64(X), f64(Y)
    R, T, s = _identity() if init is None else tuple(f64(t) for t in init)
    t = Y if Xn is None else torch.cat([Y, -f64(Yn)], -1)
    history, errs, prev, converged, idx = [], [], None, False, None
    for _ in range(max_iterations):
        q = apply(X, R, T, s)
        if Xn is not None:
            q = torch.cat([q, f64(Xn) @ R], -1)
        idx = nearest(q, t)[0]
        R, T, s = align(X, Y[idx], w, estimate_scale, allow_reflection)
        history.append((R, T, s))
        err = rmse(X, Y[idx], R, T, s, w)
        errs.append(err)
        if err == 0 or (prev is not None and (prev - err) / prev <= thr):
            converged = True
            break
        prev = err
    return dict(converged=converged, iterations=len(history), rmse=errs[-1], R=R, T=T, s=s, history=history, idx=idx, rmse_history=errs)


def normal_extremes(on, hn):
    """-> (max_j, min_j) over the human normals of dot(o_i / |o_i|, -h_j / |h_j|), norms clamped at 1e-12"""
    on, hn = f64(on), f64(hn)
    o = on / on.norm(dim=1, keepdim=True).clamp_min(1e-12)
    h = -hn / hn.norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = o @ h.T
    return d.max(1).values, d.min(1).values


def cos_threshold(angle_deg):
    """as the reference computes it, in fp32"""
    return float(torch.cos(torch.deg2rad(torch.tensor(angle_deg, dtype=torch.float32))))


def normal_filter(on, hn, angle_deg, angle_neg_deg=None):
    mx, mn = normal_extremes(on, hn)
    keep = mx > cos_threshold(angle_deg)
    if angle_neg_deg is not None:
        keep = keep | (mn < cos_threshold(angle_neg_deg))
    return keep
