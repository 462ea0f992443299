"""interactvlm_amd.contact_icp (csrc/contact_icp.hip) on the GPU against tests/_icp_ref.py (fp64, pinned to the reference by
test_contact_icp_cpu.py) and against the reference's own fp32 results in tests/golden/contact_icp.npz.

Bounds are derived, not tuned (u = 2^-24):
  * a d^2 is 6 rounded differences, 6 products and 5 additions: relative error <= 8u; an index may differ from the fp64 one only
    where the fp64 relative gap between best and second best is <= 16u, and every fixture asserts that NO query is in that band;
  * the alignment is computed in fp64 and rounded once: |R - R64| <= 4u, |T - T64|, |s - s64| <= 4u max(1, |value|), for
    fixtures whose singular values are a factor >= 1.5 apart with the smallest >= 1e-3 of the largest (asserted);
  * against an fp32 result of the reference: 2 x (that result's own fp32-minus-fp64 difference, stored in the npz) + 4u.

One property of the issue's list is restated: "the position rmse never rises along the history" is a theorem only without
normals (nearest neighbour and alignment then minimise the same 3-D error).  With normals the neighbour is the nearest in 6-D,
the position rmse may rise, and a rise is exactly what pytorch3d's criterion ends a pose on - the fp64 restatement shows it for
every seed tried.  So the 3-D run asserts the theorem over the whole history, and the run with normals asserts that every step
BEFORE the last fell by more than the threshold (what continuing means) and that the pose ended on the first step that did not.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _icp_ref as ref
from interactvlm_amd import _lib
from interactvlm_amd import contact_icp as ci

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_icp.npz"))
ALIGN_CASES = [str(c) for c in GOLDEN["align_cases"]]
ICP_CASES = [str(c) for c in GOLDEN["icp_cases"]]
SPREAD = 0.2 * torch.tensor([1.0, 0.6, 0.35])
CENTRE = torch.tensor([0.3, -0.2, 2.5])


def g(name):
    return torch.from_numpy(np.asarray(GOLDEN[name]))


def cloud(n, gen):
    return torch.randn(n, 3, generator=gen) * SPREAD + CENTRE


def unit(n, gen):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)


def rotation(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    t = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def assert_align(got, want, extra=(0.0, 0.0, 0.0), what=""):
    """got (R, T, s) fp32 against want in fp64 at 4u (+ extra per part)"""
    for k, a, b, e in zip("RTs", got, want, extra):
        a, b = ref.f64(a), ref.f64(b)
        scale = 1.0 if k == "R" else max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        assert err <= 4 * U * scale + e, f"{what} {k}: {err:.3e} > {4 * U * scale + e:.3e}"


# ---------------------------------------------------------------- contact_nearest

NEAREST_SHAPES = [(255, 511), (256, 512), (257, 513), (1, 1300), (300, 1), (700, 1300)]
NEAREST_SEED = {(700, 1300, 3): 1, (700, 1300, 6): 1}  # seed 0 has a near-tie at this shape (see make_golden_icp.py)


@functools.lru_cache(maxsize=None)
def nearest_case(n_o, n_h, D):
    gen = torch.Generator().manual_seed(NEAREST_SEED.get((n_o, n_h, D), 0) * 7919 + n_o * 31 + n_h + D)
    q, t = cloud(n_o, gen), cloud(n_h, gen)
    if D == 6:
        q, t = torch.cat([q, unit(n_o, gen)], -1), torch.cat([t, unit(n_h, gen)], -1)
    return q, t, ref.nearest(q, t)


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("n_o,n_h", NEAREST_SHAPES)
def test_nearest_against_fp64(n_o, n_h, D):
    q, t, (idx64, d64, gap) = nearest_case(n_o, n_h, D)
    assert float(gap.min()) > 16 * U, f"fixture has a near-tie (gap {float(gap.min()):.2e}): it could excuse a wrong index"
    idx, d2 = ci.contact_nearest(q.to(DEV), t.to(DEV))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1, n_o) and d2.dtype == torch.float32
    assert bool((idx[0].cpu().long() == idx64).all())
    err = (d2[0].cpu().double() - d64).abs()
    print("max relative d2 error / u:", float((err / d64.clamp_min(1e-300)).max() / U))
    assert bool((err <= 8 * U * d64).all())


def test_nearest_duplicates_return_lowest_index():
    gen = torch.Generator().manual_seed(5)
    q = cloud(300, gen)
    base = cloud(600, gen)
    t = torch.cat([base, base, base[:100]], 0)  # every target twice or three times, the copies in other tiles
    idx, _ = ci.contact_nearest(q.to(DEV), t.to(DEV))
    want = ref.nearest(q, t)[0]
    assert int(want.max()) < 600
    assert bool((idx[0].cpu().long() == want).all())


def test_nearest_batched_equals_unbatched():
    gen = torch.Generator().manual_seed(6)
    q = torch.stack([torch.cat([cloud(257, gen), unit(257, gen)], -1) for _ in range(3)]).to(DEV)
    t = torch.stack([torch.cat([cloud(513, gen), unit(513, gen)], -1) for _ in range(3)]).to(DEV)
    idx, d2 = ci.contact_nearest(q, t)
    for b in range(3):
        i1, d1 = ci.contact_nearest(q[b], t[b])
        assert torch.equal(idx[b], i1[0]) and torch.equal(d2[b], d1[0])
    idx_s, d2_s = ci.contact_nearest(q, t[1])  # a shared side
    i1, d1 = ci.contact_nearest(q[2], t[1])
    assert torch.equal(idx_s[2], i1[0]) and torch.equal(d2_s[2], d1[0])


# ---------------------------------------------------------------- align_points

@pytest.mark.parametrize("case", ALIGN_CASES)
def test_align_against_fp64_and_reference(case):
    src = str(GOLDEN["align_src"][ALIGN_CASES.index(case)])
    scale, refl = (bool(v) for v in GOLDEN[f"{case}_flags"])
    X, Y, w = g(f"{src}_X"), g(f"{src}_Y"), g(f"{src}_w")
    R64, T64, s64, S = ref.align(X, Y, w, scale, refl, with_singular=True)
    assert float(S[0] / S[1]) >= 1.5 and float(S[1] / S[2]) >= 1.5 and float(S[2] / S[0]) >= 1e-3, S
    R, T, s = ci.align_points(X.to(DEV), Y.to(DEV), w.to(DEV), estimate_scale=scale, allow_reflection=refl)
    got = (R[0], T[0], s[0])
    print(case, [float((ref.f64(a) - b).abs().max()) for a, b in zip(got, (R64, T64, s64))])
    assert_align(got, (R64, T64, s64), what="vs fp64")
    extra = tuple(2 * float(GOLDEN[f"{case}_d{k}"]) for k in "RTs")
    assert_align(got, tuple(g(f"{case}_{k}32") for k in "RTs"), extra, what="vs the reference's fp32")
    det = float(torch.det(ref.f64(R[0])))
    assert det == pytest.approx(-1.0 if (refl and src == "align_refl") else 1.0, abs=1e-6)
    if not scale:
        assert float(s[0]) == 1.0


def test_align_unweighted_and_batched():
    X, Y = g("align_n257_X"), g("align_n257_Y")
    Xb = torch.stack([X, X * 1.5, X + 0.25]).to(DEV)
    R, T, s = ci.align_points(Xb, Y.to(DEV), estimate_scale=True)
    for b in range(3):
        assert_align((R[b], T[b], s[b]), ref.align(Xb[b], Y, None, True), what=f"pose {b}")
        R1, T1, s1 = ci.align_points(Xb[b], Y.to(DEV), estimate_scale=True)
        assert torch.equal(R1[0], R[b]) and torch.equal(T1[0], T[b]) and torch.equal(s1[0], s[b])


@pytest.mark.parametrize("kind", ["collinear", "single", "one_weight", "coincident"])
@pytest.mark.parametrize("scale", [False, True])
def test_align_degenerate_is_finite_rotation(kind, scale):
    gen = torch.Generator().manual_seed(11)
    w = None
    if kind == "collinear":
        tpar = torch.randn(300, 1, generator=gen)
        X = tpar * torch.tensor([[0.3, -0.5, 0.8]]) + CENTRE
        Y = tpar * torch.tensor([[-0.6, 0.2, 0.4]]) + 1.0
    elif kind == "single":
        X, Y = cloud(1, gen), cloud(1, gen)
    elif kind == "one_weight":
        X, Y = cloud(300, gen), cloud(300, gen)
        w = torch.zeros(300)
        w[137] = 0.7
    else:
        X, Y = CENTRE.expand(300, 3).contiguous(), (CENTRE + 1).expand(300, 3).contiguous()
    R, T, s = ci.align_points(X.to(DEV), Y.to(DEV), None if w is None else w.to(DEV), estimate_scale=scale)
    for t in (R, T, s):
        assert bool(torch.isfinite(t).all())
    R = ref.f64(R[0])
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float(torch.det(R)) > 0


# ---------------------------------------------------------------- contact_icp, requery=False: the reference's result

def icp_inputs(case):
    fx = str(GOLDEN["icp_fixture"][ICP_CASES.index(case)])
    normals, use_init, scale, mi = (int(v) for v in GOLDEN[f"{case}_cfg"])
    X, Y, Xn, Yn = (g(f"{fx}_{k}") for k in ("X", "Y", "Xn", "Yn"))
    init = tuple(g(f"icp_init_{k}")[None] for k in "RTs") if use_init else None
    return X, Y, (Xn if normals else None), (Yn if normals else None), init, bool(scale), mi


def dev(t):
    return None if t is None else (tuple(v.to(DEV) for v in t) if isinstance(t, tuple) else t.to(DEV))


@pytest.mark.parametrize("case", ICP_CASES)
def test_icp_drop_in_against_reference(case):
    X, Y, Xn, Yn, init, scale, mi = icp_inputs(case)
    out = ci.contact_icp(dev(X), dev(Y), dev(Xn), dev(Yn), init=dev(init), max_iterations=mi, estimate_scale=scale)
    assert bool((out.nn_idx[0].cpu() == g(f"{case}_idx")).all())
    extra = tuple(2 * float(GOLDEN[f"{case}_d{k}"]) for k in "RTs")
    assert_align((out.R[0], out.T[0], out.s[0]), tuple(g(f"{case}_{k}32") for k in "RTs"), extra, what="vs the reference's fp32")
    r32, dr = float(g(f"{case}_rmse32")), float(GOLDEN[f"{case}_drmse"])
    assert abs(float(out.rmse[0]) - r32) <= 2 * dr + 4 * U * max(1.0, r32)
    assert out.converged.dtype == torch.bool and bool(out.converged[0]) == bool(GOLDEN[f"{case}_converged"])
    assert out.iterations.dtype == torch.int32 and int(out.iterations[0]) == int(GOLDEN[f"{case}_len_history"])
    hR, hT, hs = out.history
    assert tuple(hR.shape) == (mi, 1, 3, 3) and tuple(hT.shape) == (mi, 1, 3) and tuple(hs.shape) == (mi, 1)
    for row in range(mi):
        assert torch.equal(hR[row], out.R) and torch.equal(hT[row], out.T) and torch.equal(hs[row], out.s)
    Xt64 = ref.apply(ref.f64(X), ref.f64(out.R[0]), ref.f64(out.T[0]), ref.f64(out.s[0]))
    assert float((ref.f64(out.Xt[0]) - Xt64).abs().max()) <= 8 * U * float(Xt64.abs().max())


def test_icp_drop_in_without_normals_against_fp64():
    """the reference itself cannot run without normals (the npz records that it raises); the 3-D path against the restatement"""
    X, Y, _, _, init, _, _ = icp_inputs("icp_n1_i1_s1_m10")
    want = ref.icp_as_reference(X, Y, None, None, tuple(t[0] for t in init), max_iterations=10, estimate_scale=True)
    gap = ref.nearest(ref.apply(ref.f64(X), *(ref.f64(t[0]) for t in init)), Y)[2]
    assert float(gap.min()) > 16 * U
    out = ci.contact_icp(dev(X), dev(Y), init=dev(init), estimate_scale=True)
    assert bool((out.nn_idx[0].cpu().long() == want["idx"]).all())
    assert_align((out.R[0], out.T[0], out.s[0]), (want["R"], want["T"], want["s"]))
    assert abs(float(out.rmse[0]) - float(want["rmse"])) <= 4 * U
    assert bool(out.converged[0]) and int(out.iterations[0]) == 2


# ---------------------------------------------------------------- contact_icp, requery=True

@functools.lru_cache(maxsize=None)
def grid_case(s0, deg=0.5):
    """700 jittered grid points (10 x 10 x 7 about the origin, spacing 0.1, jitter 0.01) and a permutation of their image under a
    rotation by `deg` degrees, |T| = 0.02 and scale s0.  -> X, Y, Y in X's order, the inverse permutation, (R0, T0)"""
    gen = torch.Generator().manual_seed(3)
    ii = torch.arange(700)
    X = (torch.stack([ii % 10, (ii // 10) % 10, ii // 100], 1).float() - torch.tensor([4.5, 4.5, 3.0])) * 0.1
    X = X + 0.01 * (2 * torch.rand(700, 3, generator=gen) - 1)
    R0 = rotation([1.0, -2.0, 0.5], deg)
    T0 = 0.02 * torch.tensor([0.6, 0.0, -0.8], dtype=torch.float64)
    perm = torch.randperm(700, generator=gen)
    Ytrue = (s0 * (X.double() @ R0) + T0).float()
    inv = torch.empty(700, dtype=torch.long)
    inv[perm] = torch.arange(700)
    return X, Ytrue[perm], Ytrue, inv, (R0, T0)


@pytest.mark.parametrize("deg,s0", [(5.0, 1.0), (5.0, 1.1), (0.5, 1.0), (0.5, 1.01)])
def test_icp_requery_recovers_known_transform(deg, s0):
    """The issue's fixture (5 degrees, s in {1, 1.1}) and its statement that "the true correspondence is then the nearest one from
    the start" do not go together: the corners of 700 points at spacing 0.1 are 0.7 from the centre, 5 degrees move them by 0.06
    and a scale of 1.1 by 0.07, past the 0.04 that keeps a point inside its own cell.  The premise, and with it "<= 3 iterations"
    (two, in fact), holds for 0.5 degrees and s in {1, 1.01}; those cases assert it.  With the issue's numbers the loop still
    recovers the transform, in the number of iterations the fp64 restatement takes (3 for s = 1, 4 for s = 1.1): those cases
    assert that count instead, everything else alike.  Measured on an MI355X: 2, 3, 2 and 1 iterations for the four cases (each
    one less than fp64 where the closed-form rmse of the exact fit read 0), so the issue's "<= 3" is met by all of them there."""
    X, Y, Ymatched, inv, _ = grid_case(s0, deg)
    scale = s0 != 1.0
    want = ref.icp_requery(X, Y, estimate_scale=scale)
    assert want["converged"] and bool((want["idx"] == inv).all())
    if deg < 1.0:
        assert bool((ref.nearest(X, Y)[0] == inv).all()) and want["iterations"] <= 3  # the premise
    out = ci.contact_icp(dev(X), dev(Y), requery=True, estimate_scale=scale)
    print("iterations", int(out.iterations[0]), "fp64", want["iterations"])
    assert bool((out.nn_idx[0].cpu().long() == inv).all())
    assert_align((out.R[0], out.T[0], out.s[0]), ref.align(X, Ymatched, None, scale))
    # the kernel's rmse is a closed form of fp64 moments: an exact fit (true rmse ~1e-8 here, the fp32 rounding of Y) can read 0,
    # and rmse == 0 ends the pose one iteration before the one that would only have confirmed it
    n_it = int(out.iterations[0])
    assert bool(out.converged[0]) and (n_it == want["iterations"] or (n_it == want["iterations"] - 1 and float(out.rmse[0]) == 0.0))
    assert int(out.iterations[0]) <= (3 if deg < 1.0 or s0 == 1.0 else 4)


@functools.lru_cache(maxsize=None)
def random_case(seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    return cloud(257, gen), cloud(513, gen), unit(257, gen), unit(513, gen)


def replay_history(X, Y, Xn, Yn, out, b=0, init=None):
    """For every executed iteration: the fp64 neighbours of the queries rebuilt in fp64 from the previous history row, the band
    check of the docstring, and the fp64 position rmse of that row's transform.  -> (idx of the last iteration, [rmse])"""
    hR, hT, hs = (ref.f64(t)[:, b] for t in out.history)
    X64, Y64 = ref.f64(X), ref.f64(Y)
    t = Y64 if Xn is None else torch.cat([Y64, -ref.f64(Yn)], -1)
    R, T, s = ref._identity() if init is None else tuple(ref.f64(v) for v in init)
    errs, idx = [], None
    for it in range(int(out.iterations[b])):
        q = ref.apply(X64, R, T, s)
        if Xn is not None:
            q = torch.cat([q, ref.f64(Xn) @ R], -1)
        d = ref.sqdist(q, t)
        two = d.topk(min(2, d.shape[1]), dim=1, largest=False).values
        delta = 8 * U * (abs(float(s)) * float(X64.abs().sum(1).max()) + float(T.abs().max()))
        band = 16 * U * two[:, 1] + 2 * two[:, 1].sqrt() * delta
        assert bool((two[:, 1] - two[:, 0] > band).all()), f"iteration {it}: a query is inside the band"
        idx = ref.nearest(q, t)[0]
        R, T, s = hR[it], hT[it], hs[it]
        errs.append(float(ref.rmse(X64, Y64[idx], R, T, s)))
    return idx, errs


def test_icp_requery_self_consistent_with_normals():
    X, Y, Xn, Yn = random_case()
    thr = 1e-6
    out = ci.contact_icp(dev(X), dev(Y), dev(Xn), dev(Yn), requery=True, max_iterations=10, relative_rmse_thr=thr)
    n_it = int(out.iterations[0])
    idx, errs = replay_history(X, Y, Xn, Yn, out)
    print("iterations", n_it, "rmse history", errs)
    assert bool((out.nn_idx[0].cpu().long() == idx).all())
    assert_align((out.R[0], out.T[0], out.s[0]), ref.align(X, Y[idx]))
    assert abs(float(out.rmse[0]) - errs[-1]) <= 8 * U * errs[-1]
    # every step before the last fell by more than the threshold; the pose ended on the first that did not (or at the limit)
    for k in range(1, n_it - 1):
        assert errs[k] < errs[k - 1] * (1 - thr) * (1 + 8 * U)
    if bool(out.converged[0]):
        assert n_it >= 2 and errs[-1] >= errs[-2] * (1 - thr) * (1 - 8 * U)
    else:
        assert n_it == 10
    hR, hT, hs = out.history
    for row in range(n_it - 1, 10):
        assert torch.equal(hR[row], out.R) and torch.equal(hT[row], out.T) and torch.equal(hs[row], out.s)


@pytest.mark.parametrize("s0", [1.0, 1.1])
def test_icp_requery_issue_grid_is_self_consistent(s0):
    """the grid with the issue's own numbers (5 degrees, s in {1, 1.1}): every iteration's neighbours and the final alignment
    against fp64, and a position rmse that never rises (3-D)"""
    X, Y, _, _, _ = grid_case(s0, 5.0)
    scale = s0 != 1.0
    out = ci.contact_icp(dev(X), dev(Y), requery=True, max_iterations=6, estimate_scale=scale)
    idx, errs = replay_history(X, Y, None, None, out)
    assert bool((out.nn_idx[0].cpu().long() == idx).all())
    assert_align((out.R[0], out.T[0], out.s[0]), ref.align(X, Y[idx], None, scale))
    for k in range(1, len(errs)):
        assert errs[k] <= errs[k - 1] * (1 + 8 * U)


def test_icp_requery_rmse_never_rises_without_normals():
    X, Y, _, _ = random_case()
    out = ci.contact_icp(dev(X), dev(Y), requery=True, max_iterations=10)
    idx, errs = replay_history(X, Y, None, None, out)
    print("iterations", int(out.iterations[0]), "rmse history", errs)
    assert int(out.iterations[0]) >= 3
    assert bool((out.nn_idx[0].cpu().long() == idx).all())
    assert_align((out.R[0], out.T[0], out.s[0]), ref.align(X, Y[idx]))
    for k in range(1, len(errs)):
        assert errs[k] <= errs[k - 1] * (1 + 8 * U)


def batch_starts():
    _, _, _, _, (R0, T0) = grid_case(1.0)
    Rs = torch.stack([rotation([0.2, 1.0, 0.1], 25.0), R0, rotation([1.0, 0.3, -0.4], -18.0)]).float()
    Ts = torch.stack([torch.tensor([0.05, -0.02, 0.03], dtype=torch.float64), T0, torch.tensor([-0.04, 0.06, 0.0], dtype=torch.float64)]).float()
    return Rs, Ts, torch.ones(3)


def test_icp_requery_batch_of_starts():
    X, Y, _, inv, _ = grid_case(1.0)
    init = batch_starts()
    out = ci.contact_icp(dev(X), dev(Y), init=dev(init), requery=True, max_iterations=10)
    again = ci.contact_icp(dev(X), dev(Y), init=dev(init), requery=True, max_iterations=10)
    flat = lambda o: [o.converged, o.rmse, o.Xt, o.R, o.T, o.s, o.iterations, o.nn_idx, *o.history]
    assert all(torch.equal(a, b) for a, b in zip(flat(out), flat(again)))
    its = out.iterations.cpu().tolist()
    print("iterations per start", its)
    assert its[1] <= 2 and bool(out.converged[1]) and its[1] < max(its)  # the start at the solution ends first
    assert bool((out.nn_idx[1].cpu().long() == inv).all())
    hR, hT, hs = out.history
    for b in range(3):
        one = ci.contact_icp(dev(X), dev(Y), init=tuple(t[b:b + 1].to(DEV) for t in init), requery=True, max_iterations=10)
        for a, c in zip(flat(out)[:8], flat(one)[:8]):
            assert torch.equal(a[b], c[0])
        for h, h1 in zip(out.history, one.history):
            assert torch.equal(h[:, b], h1[:, 0])
        for row in range(its[b] - 1, 10):
            assert torch.equal(hR[row, b], out.R[b]) and torch.equal(hT[row, b], out.T[b]) and torch.equal(hs[row, b], out.s[b])


def test_icp_runs_without_host_round_trip():
    """the whole loop is a linear chain of launches: captured once, replayed twice, the same bits as the eager call"""
    X, Y, Xn, Yn = (t.to(DEV) for t in random_case())
    eager = ci.contact_icp(X, Y, Xn, Yn, requery=True, max_iterations=4)
    flat = lambda o: [o.converged, o.rmse, o.Xt, o.R, o.T, o.s, o.iterations, o.nn_idx, *o.history]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ci.contact_icp(X, Y, Xn, Yn, requery=True, max_iterations=4)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ci.contact_icp(X, Y, Xn, Yn, requery=True, max_iterations=4)
    for _ in range(2):
        for t in flat(captured):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(flat(captured), flat(eager)))


def test_icp_memory_is_linear():
    B, n_o, n_h = 8, 4096, 6890  # one dense [B, N_o, N_h] fp32 array would be 903 MB
    gen = torch.Generator().manual_seed(2)
    X, Y = cloud(n_o, gen).to(DEV), cloud(n_h, gen).to(DEV)
    Xn, Yn = unit(n_o, gen).to(DEV), unit(n_h, gen).to(DEV)
    Rs = torch.stack([rotation([0.1, 1.0, 0.3], 4.0 * b) for b in range(B)]).float().to(DEV)
    init = (Rs, torch.zeros(B, 3, device=DEV), torch.ones(B, device=DEV))
    ws = _lib.load().ivlm_contact_icp_workspace_bytes(B, n_o)
    assert 0 < ws <= B * n_o * 64
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ci.contact_icp(X, Y, Xn, Yn, init=init, requery=True, max_iterations=3)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    outputs = sum(t.numel() * t.element_size() for t in (out.converged, out.rmse, out.Xt, out.R, out.T, out.s, out.iterations,
                                                          out.nn_idx, *out.history))
    print("peak rise", rise, "workspace", ws, "outputs", outputs)
    assert rise <= ws + outputs + (1 << 20)
    assert bool(torch.isfinite(out.rmse).all())


# ---------------------------------------------------------------- contact_normal_filter

@functools.lru_cache(maxsize=None)
def normals_case(n_o, n_h):
    gen = torch.Generator().manual_seed(n_o * 13 + n_h)
    # lengths other than 1: the kernel normalises; human normals in a cone, so that some object normals face none of them
    hn = torch.nn.functional.normalize(torch.randn(n_h, 3, generator=gen) * 0.35 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    return unit(n_o, gen) * (0.5 + torch.rand(n_o, 1, generator=gen)), hn * (0.5 + torch.rand(n_h, 1, generator=gen))


@pytest.mark.parametrize("n_o,n_h", [(257, 513), (1, 1300)])
@pytest.mark.parametrize("angles", [(60.0, None), (90.0, -90.0)])
def test_normal_filter_against_fp64(n_o, n_h, angles):
    on, hn = normals_case(n_o, n_h)
    mx, mn = ref.normal_extremes(on, hn)
    keep = ci.contact_normal_filter(on.to(DEV), hn.to(DEV), *angles).cpu()
    assert keep.dtype == torch.bool and tuple(keep.shape) == (n_o,)
    c_pos = ref.cos_threshold(angles[0])
    sure = (mx - c_pos).abs() > 8 * U
    if angles[1] is not None:
        sure &= (mn - ref.cos_threshold(angles[1])).abs() > 8 * U
    else:
        assert bool(sure.all()), "fixture has an extreme inside the band"
        if n_o > 1:
            assert 0 < int(keep.sum()) < n_o  # the fixture exercises both outcomes
    want = ref.normal_filter(on, hn, *angles)
    assert bool((keep == want)[sure].all())
    if angles[1] is not None:
        # cos(deg2rad(90)) is -4.37e-8 in fp32 on both sides, so every row with any dot product away from it is kept
        assert c_pos == ref.cos_threshold(-90.0) and -5e-8 < c_pos < 0
        assert bool(keep.all())
