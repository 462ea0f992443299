"""ICP between the object's and the human's contact points: the first thing the reference's joint fitting stage does with the
two contact vectors (optim/fit.py: threshold, filter by normals, then optim/icp/icp.py ``ICP`` for the starting R, T of the
optimiser), as HIP kernels (csrc/contact_icp.hip) with no [N_o, N_h] array and no host round trip inside the loop.

    contact_nearest        nearest target of every query (pytorch3d ``knn_points`` with K = 1)
    align_points           the reference's ``corresponding_points_alignment`` (Umeyama)
    contact_normal_filter  the ``filter_contacts`` step of optim/fit.py
    contact_icp            the loop, for B starts in one call

Row-vector convention as in the reference: s x R + T ~ y.  There is no CPU fallback.

What the reference's ``ICP`` computes (mirrored by ``requery=False``): its query ``obj_t_combined`` is built once
before the loop and never rebuilt, so every iteration finds the same neighbours and the same (R, T, s); and its relative rmse has
the sign of pytorch3d's flipped, so any non-increase counts as converged.  It therefore "converges" at its second iteration with
the transform of its first: ONE nearest-neighbour pass (object normals not rotated by the initial R) plus ONE alignment.
``requery=True`` is the ICP the name promises.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from ._args import batch_size, check_devices, check_points, check_vector, side
from ._lib import check

ESTIMATE_SCALE, ALLOW_REFLECTION, REQUERY = (_lib.header_constant(f"IVLM_ICP_{k}")
                                             for k in ("ESTIMATE_SCALE", "ALLOW_REFLECTION", "REQUERY"))


class ICPResult(NamedTuple):
    converged: torch.Tensor   # bool [B]
    rmse: torch.Tensor        # fp32 [B]
    Xt: torch.Tensor          # fp32 [B, N_o, 3]: s X R + T
    R: torch.Tensor           # fp32 [B, 3, 3]
    T: torch.Tensor           # fp32 [B, 3]
    s: torch.Tensor           # fp32 [B]
    iterations: torch.Tensor  # int32 [B]
    nn_idx: torch.Tensor      # int32 [B, N_o]: the correspondences the returned transform was aligned to
    history: tuple            # (R [max_iterations, B, 3, 3], T [max_iterations, B, 3], s [max_iterations, B])


def _check_weights(w, n, name="weights"):
    check_vector(w, n, name, batch=True)
    if bool((w < 0).any()):
        raise ValueError(f"{name}: expected non-negative weights")


def contact_nearest(queries, targets):
    """Nearest target of every query by squared L2 distance.

    queries [N_o,D] or [B,N_o,D], targets [N_h,D] or [B,N_h,D] (fp32, GPU, D = 3 or 6; an unbatched side is shared by the batch)
    -> (idx int32 [B,N_o], d2 fp32 [B,N_o]).  d^2 is the direct fp32 sum of squared differences, relative error <= 8 * 2^-24;
    the lowest index wins an exact tie, so the result does not depend on the kernel's tiling."""
    check_points(queries, "queries", (3, 6))
    check_points(targets, "targets", (3, 6))
    if queries.shape[-1] != targets.shape[-1]:
        raise ValueError(f"queries have D = {queries.shape[-1]}, targets D = {targets.shape[-1]}")
    named = [(queries, "queries", 2), (targets, "targets", 2)]
    B = batch_size(named)
    check_devices(named)
    lib = _lib.load()
    q, q_bs = side(queries, 2)
    t, t_bs = side(targets, 2)
    n_o, n_h, D = q.shape[1], t.shape[1], q.shape[2]
    with torch.cuda.device(q.device):
        idx = torch.empty(B, n_o, dtype=torch.int32, device=q.device)
        d2 = torch.empty(B, n_o, dtype=torch.float32, device=q.device)
        check(lib.ivlm_contact_nearest(q.data_ptr(), t.data_ptr(), D, B, n_o, n_h, q_bs, t_bs, idx.data_ptr(), d2.data_ptr(),
                                       _lib.stream()), "contact_nearest")
    return idx, d2


def align_points(X, Y, weights=None, estimate_scale=False, allow_reflection=False):
    """The similarity transform that takes X to Y in the weighted least-squares sense (Umeyama), as the reference's
    ``corresponding_points_alignment`` forms it:

        mu_x = sum w x / max(sum w, 1e-9),  Xc = w (x - mu_x),  Yc = w (y - mu_y)      (so the covariance carries w^2)
        C = Xc^T Yc / max(sum w, 1e-9) = U S V^T,  E = diag(1, 1, det(U V^T)) unless allow_reflection,  R = U E V^T
        s = trace(E S) / max(sum |Xc|^2 / max(sum w, 1e-9), 1e-9) if estimate_scale else 1,   T = mu_y - s mu_x R

    X, Y [N,3] or [B,N,3] (fp32, GPU), weights [N] or [B,N] >= 0 or None -> (R [B,3,3], T [B,3], s [B]).  Moments, the 3x3 Jacobi
    SVD and the solve are fp64, rounded once to fp32.  A degenerate covariance (collinear or coincident points, one point) still
    gives a finite orthonormal R, of determinant +1 unless allow_reflection."""
    check_points(X, "X")
    check_points(Y, "Y")
    if X.shape[-2] != Y.shape[-2]:
        raise ValueError(f"X has {X.shape[-2]} points, Y {Y.shape[-2]}")
    named = [(X, "X", 2), (Y, "Y", 2)]
    if weights is not None:
        _check_weights(weights, X.shape[-2])
        named.append((weights, "weights", 1))
    B = batch_size(named)
    check_devices(named)
    lib = _lib.load()
    x, x_bs = side(X, 2)
    y, y_bs = side(Y, 2)
    w, w_bs = side(weights, 1) if weights is not None else (None, 0)
    n = x.shape[1]
    dev = x.device
    with torch.cuda.device(dev):
        ws, nbytes = _lib.workspace(lib.ivlm_contact_icp_workspace_bytes, "align_points", dev, B=B, N=n)
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        T = torch.empty(B, 3, dtype=torch.float32, device=dev)
        s = torch.empty(B, dtype=torch.float32, device=dev)
        flags = (ESTIMATE_SCALE if estimate_scale else 0) | (ALLOW_REFLECTION if allow_reflection else 0)
        check(lib.ivlm_points_align(x.data_ptr(), y.data_ptr(), _lib.ptr(w), B, n, x_bs, y_bs, w_bs, flags, R.data_ptr(), T.data_ptr(),
                                    s.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "points_align")
    return R, T, s


def contact_normal_filter(obj_normals, human_normals, angle_deg, angle_neg_deg=None):
    """The ``filter_contacts`` step of the reference's optim/fit.py: which object contact points have a human contact normal
    facing them.  obj_normals [N_o,3], human_normals [N_h,3] (fp32, GPU, any length) -> bool [N_o]:

        d_ij = dot(o_i / |o_i|, -h_j / |h_j|),   keep_i = (max_j d_ij > cos(angle_deg)) or (min_j d_ij < cos(angle_neg_deg))

    The thresholds are computed as the reference computes them, in fp32: cos(deg2rad(90)) is -4.37e-8, not 0, so (90, -90) keeps
    every row that has any d_ij > -4.37e-8 or < -4.37e-8."""
    for v, name in ((obj_normals, "obj_normals"), (human_normals, "human_normals")):
        check_points(v, name, batch=False)
    check_devices([(obj_normals, "obj_normals", 2), (human_normals, "human_normals", 2)])

    def cosine(a):
        return float(torch.cos(torch.deg2rad(torch.tensor(a, dtype=torch.float32))))

    c_pos = cosine(angle_deg)
    c_neg = cosine(angle_neg_deg) if angle_neg_deg is not None else 0.0
    lib = _lib.load()
    o, h = obj_normals.contiguous(), human_normals.contiguous()
    with torch.cuda.device(o.device):
        keep = torch.empty(o.shape[0], dtype=torch.uint8, device=o.device)
        check(lib.ivlm_contact_normal_filter(o.data_ptr(), h.data_ptr(), o.shape[0], h.shape[0], c_pos, c_neg,
                                             int(angle_neg_deg is not None), keep.data_ptr(), _lib.stream()), "contact_normal_filter")
    return keep.bool()


def _validate_icp(obj_pts, human_pts, obj_normals, human_normals, init, weights, max_iterations):
    """-> B: raises before anything touches the library"""
    check_points(obj_pts, "obj_pts")
    check_points(human_pts, "human_pts")
    named = [(obj_pts, "obj_pts", 2), (human_pts, "human_pts", 2)]
    if (obj_normals is None) != (human_normals is None):
        raise ValueError("normals must be given for both sides or for neither")
    if obj_normals is not None:
        check_points(obj_normals, "obj_normals")
        check_points(human_normals, "human_normals")
        if obj_normals.shape[-2] != obj_pts.shape[-2] or human_normals.shape[-2] != human_pts.shape[-2]:
            raise ValueError("normals: expected one normal per point")
        named += [(obj_normals, "obj_normals", 2), (human_normals, "human_normals", 2)]
    if weights is not None:
        _check_weights(weights, obj_pts.shape[-2])
        named.append((weights, "weights", 1))
    if not isinstance(max_iterations, int) or max_iterations < 1:
        raise ValueError(f"max_iterations: expected an integer >= 1, got {max_iterations!r}")
    if init is not None:
        try:
            R, T, s = init
        except (TypeError, ValueError):
            raise ValueError("init: expected (R [B,3,3], T [B,3], s [B])") from None
        for t, name, tail in ((R, "init R", (3, 3)), (T, "init T", (3,)), (s, "init s", ())):
            if not isinstance(t, torch.Tensor) or t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tail or t.shape[0] < 1:
                raise ValueError(f"{name}: expected [B{''.join(',' + str(d) for d in tail)}], got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.dtype != torch.float32:
                raise ValueError(f"{name}: expected float32, got {t.dtype}")
        if not (R.shape[0] == T.shape[0] == s.shape[0]):
            raise ValueError(f"init: batch sizes {R.shape[0]}, {T.shape[0]}, {s.shape[0]} differ")
        named += [(R, "init R", 2), (T, "init T", 1), (s, "init s", 0)]
    B = batch_size(named)
    check_devices(named)
    return B


def contact_icp(obj_pts, human_pts, obj_normals=None, human_normals=None, init=None, weights=None, max_iterations=10,
                relative_rmse_thr=1e-6, estimate_scale=False, allow_reflection=False, requery=False) -> ICPResult:
    """Align the object's contact points to the human's: the reference's ``ICP`` (optim/icp/icp.py), for B starts in one call.

    obj_pts [N_o,3] or [B,N_o,3], human_pts [N_h,3] or [B,N_h,3], obj_normals / human_normals likewise (both or neither), weights
    [N_o] or [B,N_o] >= 0 (their sign is read on the host before the launch, the one host read of a call that passes weights) -
    all fp32 on one GPU; a side without a batch axis is shared by the batch.  init = (R [B,3,3], T [B,3], s [B]) gives B starts:
    ICP finds a local optimum, and multi-start is one launch sequence here, not B loops.  The query of a
    point is [s x R + T, n] against the targets [y, -m] (6-D with normals, else 3-D); the alignment is ``align_points`` of the
    ORIGINAL obj_pts with the neighbours found; rmse = sqrt(sum w |s x R + T - y_nn|^2 / max(sum w, 1e-9)).

    requery=False (default, the drop-in) returns what the reference returns.  The reference builds its query once before the
    loop and never rebuilds it, and it accepts any non-increase of the rmse as convergence, so its loop ends at the second
    iteration with the transform of the first: ONE nearest-neighbour pass (points moved by ``init``, object normals used as given,
    NOT rotated), ONE alignment and its rmse; iterations = min(2, max_iterations), converged = (max_iterations >= 2); s = 1
    without estimate_scale whatever scale went in.  All history rows hold that transform.

    requery=True is the ICP the name promises: every iteration rebuilds the queries [s x R + T, n R] from the current transform
    (normals rotated, by init's R at iteration 0) and a pose ends when (prev_rmse - rmse) / prev_rmse <= relative_rmse_thr
    (pytorch3d's criterion, on the position rmse, from the second iteration on) or when rmse == 0.  Finished poses cost an early
    exit; history rows after a pose's end repeat its final transform.

    The whole loop is enqueued on the current stream without host synchronisation (it can be captured in a HIP graph);
    converged, iterations and rmse are device tensors.  The same bits every call, and for a pose whatever the batch around it.
    Not supported (optim/fit.py passes neither): Pointclouds objects or per-cloud lengths, min_scale / scale_penalty."""
    B = _validate_icp(obj_pts, human_pts, obj_normals, human_normals, init, weights, max_iterations)
    lib = _lib.load()
    x, x_bs = side(obj_pts, 2)
    y, y_bs = side(human_pts, 2)
    xn, xn_bs = side(obj_normals, 2) if obj_normals is not None else (None, 0)
    yn, yn_bs = side(human_normals, 2) if human_normals is not None else (None, 0)
    w, w_bs = side(weights, 1) if weights is not None else (None, 0)
    n_o, n_h = x.shape[1], y.shape[1]
    dev = x.device
    iR = iT = i_s = None
    if init is not None:
        iR, iT, i_s = (t.contiguous().expand(B, *t.shape[1:]).contiguous() for t in init)
    flags = (ESTIMATE_SCALE if estimate_scale else 0) | (ALLOW_REFLECTION if allow_reflection else 0) | (REQUERY if requery else 0)
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        ws, nbytes = _lib.workspace(lib.ivlm_contact_icp_workspace_bytes, "contact_icp", dev, B=B, N_o=n_o)
        R, T, s, rmse = torch.empty(B, 3, 3, **f32), torch.empty(B, 3, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
        conv, iters, nn_idx = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, n_o, **i32)
        hR = torch.empty(max_iterations, B, 3, 3, **f32)
        hT = torch.empty(max_iterations, B, 3, **f32)
        hs = torch.empty(max_iterations, B, **f32)
        p = _lib.ptr
        check(lib.ivlm_contact_icp(x.data_ptr(), y.data_ptr(), p(xn), p(yn), p(w), p(iR), p(iT), p(i_s), B, n_o, n_h,
                                   x_bs, y_bs, xn_bs, yn_bs, w_bs, max_iterations, float(relative_rmse_thr), flags, R.data_ptr(),
                                   T.data_ptr(), s.data_ptr(), rmse.data_ptr(), conv.data_ptr(), iters.data_ptr(), nn_idx.data_ptr(),
                                   hR.data_ptr(), hT.data_ptr(), hs.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), "contact_icp")
        # s x R + T, elementwise and in place: no library GEMM whose summation could depend on the batch, no temporaries
        Xt = x[..., 0:1] * R[:, None, 0, :]
        Xt.addcmul_(x[..., 1:2], R[:, None, 1, :]).addcmul_(x[..., 2:3], R[:, None, 2, :])
        Xt.mul_(s[:, None, None]).add_(T[:, None, :])
    return ICPResult(conv.bool(), rmse, Xt, R, T, s, iters, nn_idx, (hR, hT, hs))
