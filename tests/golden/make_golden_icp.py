"""Golden vectors for interactvlm_amd.contact_icp from the reference's own optim/icp/icp.py (``ICP`` and
``corresponding_points_alignment``), run on the CPU in fp32 and again on ``.double()`` inputs.

    python tests/golden/make_golden_icp.py        # writes tests/golden/contact_icp.npz

Run in the build container only (the reference is not on the GPU box).  The reference's two modules are imported by path; its
one outside dependency, pytorch3d's ``knn_points``, is stubbed with our own brute force (squared-L2 nearest neighbour on the
direct squared differences, in the dtype of its inputs).  pytorch3d itself is absent.

Every ICP fixture is checked to hold NO near-tie: for every query the fp64 relative gap between the best and the second-best
d^2 exceeds 16 * 2^-24, so an fp32 nearest-neighbour pass cannot legitimately return another index.  A seed that fails is rejected
(seed 0 at (700, 1300) has a gap of 9.1e-7).  All ICP cases carry normals: without them the reference's ``ICP`` raises (see icp_cases).
"""
from __future__ import annotations

import collections
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True  # never write __pycache__ into the reference
HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("IVLM_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(HERE, "contact_icp.npz")
U = 2.0 ** -24

_KNN = collections.namedtuple("KNN", "dists idx knn")


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, return_nn=False, **_):
    d = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)
    dists, idx = d.topk(K, dim=2, largest=False)
    knn = None
    if return_nn:
        knn = torch.gather(p2[:, None].expand(-1, p1.shape[1], -1, -1), 2, idx[..., None].expand(-1, -1, -1, p2.shape[2]))
    return _KNN(dists, idx, knn)


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    p3 = stub("pytorch3d")
    ops = stub("pytorch3d.ops", knn_points=knn_points)
    ops.knn = stub("pytorch3d.ops.knn", knn_points=knn_points)
    st = stub("pytorch3d.structures")
    st.utils = stub("pytorch3d.structures.utils")
    p3.ops, p3.structures = ops, st
    root = os.path.join(REFERENCE_ROOT, "optim", "icp")
    pkg = types.ModuleType("ref_icp")
    pkg.__path__ = [root]
    sys.modules["ref_icp"] = pkg
    mods = {}
    for name in ("utils", "icp"):
        spec = importlib.util.spec_from_file_location(f"ref_icp.{name}", os.path.join(root, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
        mods[name] = mod
    return mods["icp"]


def rotation(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    t = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


CENTRE = torch.tensor([0.3, -0.2, 2.5], dtype=torch.float64)
SPREAD = 0.2 * torch.tensor([1.0, 0.6, 0.35], dtype=torch.float64)  # anisotropic: the covariance's singular values stay well apart


def cloud(n, g):
    return torch.randn(n, 3, generator=g, dtype=torch.float64) * SPREAD + CENTRE


def align_cases(icp):
    out = {}
    names = []
    for n in (257, 2048):
        g = torch.Generator().manual_seed(100 + n)
        X = cloud(n, g)
        R0, s0, T0 = rotation([1.0, 2.0, -1.0], 35.0), 1.3, torch.tensor([0.1, -0.3, 0.2], dtype=torch.float64)
        Y = s0 * X @ R0 + T0 + 0.01 * 0.2 * torch.randn(n, 3, generator=g, dtype=torch.float64)
        w = 0.2 + 0.8 * torch.rand(n, generator=g, dtype=torch.float64)
        out[f"align_n{n}_X"], out[f"align_n{n}_Y"], out[f"align_n{n}_w"] = (t.float().numpy() for t in (X, Y, w))
        for scale in (False, True):
            names.append((f"align_n{n}_scale{int(scale)}", f"align_n{n}", scale, False))
    # a pair whose best orthogonal fit is a reflection
    n = 257
    g = torch.Generator().manual_seed(7)
    X = cloud(n, g)
    Rm = rotation([0.5, -1.0, 2.0], 50.0) @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    Y = 0.9 * X @ Rm + torch.tensor([-0.2, 0.1, 0.4], dtype=torch.float64) + 0.01 * 0.2 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    w = 0.2 + 0.8 * torch.rand(n, generator=g, dtype=torch.float64)
    out["align_refl_X"], out["align_refl_Y"], out["align_refl_w"] = (t.float().numpy() for t in (X, Y, w))
    for refl in (False, True):
        names.append((f"align_refl_allow{int(refl)}", "align_refl", True, refl))
    for name, src, scale, refl in names:
        X, Y, w = (torch.from_numpy(out[f"{src}_{k}"])[None] for k in "XYw")
        r32 = icp.corresponding_points_alignment(X.clone(), Y.clone(), w.clone(), estimate_scale=scale, allow_reflection=refl)
        r64 = icp.corresponding_points_alignment(X.double(), Y.double(), w.double(), estimate_scale=scale, allow_reflection=refl)
        for k, a32, a64 in zip("RTs", r32, r64):
            out[f"{name}_{k}32"] = a32[0].numpy()
            out[f"{name}_{k}64"] = a64[0].numpy()
            out[f"{name}_d{k}"] = np.abs(a32[0].double().numpy() - a64[0].numpy()).max()
        out[f"{name}_flags"] = np.array([int(scale), int(refl)])
        print(name, "dR %.2e dT %.2e ds %.2e" % tuple(float(out[f"{name}_d{k}"]) for k in "RTs"), "det", float(torch.det(r64.R[0])))
    out["align_cases"] = np.array([n[0] for n in names])
    out["align_src"] = np.array([n[1] for n in names])
    return out


INIT = (rotation([0.3, 1.0, 0.2], 20.0), torch.tensor([0.1, -0.05, 0.3], dtype=torch.float64), torch.tensor(1.2, dtype=torch.float64))


def icp_fixture(n_o, n_h, seed, moved):
    """human points Y and object points X; `moved`: X is given in a frame that INIT brings next to Y"""
    g = torch.Generator().manual_seed(seed)
    Y = cloud(n_h, g)
    X = cloud(n_o, g)
    if moved:
        R, T, s = INIT
        X = ((X - T) / s) @ R.T
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    return X.float(), Y.float(), unit(n_o).float(), unit(n_h).float()


def min_gap(X, Y, Xn, Yn, init, normals):
    R, T, s = init if init is not None else (torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    q = s * (X.double() @ R) + T
    t = Y.double()
    if normals:
        q, t = torch.cat([q, Xn.double()], -1), torch.cat([t, -Yn.double()], -1)
    d = ((q[:, None] - t[None]) ** 2).sum(-1)
    two = d.topk(2, dim=1, largest=False).values
    return float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())


def icp_cases(icp):
    out = {}
    fixtures = {"f257": (257, 513, 1), "f256": (256, 512, 2), "f255": (255, 511, 3)}
    cases = [  # name, fixture, normals, init, estimate_scale, max_iterations
        ("icp_n1_i1_s0_m10", "f257", True, True, False, 10),
        ("icp_n1_i1_s0_m2", "f257", True, True, False, 2),
        ("icp_n1_i1_s0_m1", "f257", True, True, False, 1),
        ("icp_n1_i1_s1_m10", "f257", True, True, True, 10),
        ("icp_n1_i0_s0_m10", "f256", True, False, False, 10),
        ("icp_n1_i0_s1_m10", "f256", True, False, True, 10),
        ("icp_n1_i0_s1_m2", "f255", True, False, True, 2),
        ("icp_n1_i0_s0_m1", "f255", True, False, False, 1),
    ]
    data = {}
    for fname, (n_o, n_h, seed) in fixtures.items():
        moved = fname == "f257"
        X, Y, Xn, Yn = icp_fixture(n_o, n_h, seed, moved)
        data[fname] = (X, Y, Xn, Yn)
        for k, t in zip(("X", "Y", "Xn", "Yn"), (X, Y, Xn, Yn)):
            out[f"{fname}_{k}"] = t.numpy()
    out["icp_init_R"], out["icp_init_T"], out["icp_init_s"] = (t.float().numpy() for t in INIT)
    init32 = tuple(torch.from_numpy(out[f"icp_init_{k}"]) for k in "RTs")
    for name, fname, normals, use_init, scale, mi in cases:
        X, Y, Xn, Yn = data[fname]
        gap = min_gap(X, Y, Xn, Yn, tuple(t.double() for t in init32) if use_init else None, normals)
        assert gap > 16 * U, f"{name}: near-tie in the fixture (relative gap {gap:.2e}): choose another seed"
        res = {}
        for tag, cast in (("32", lambda t: t.clone()), ("64", lambda t: t.double())):
            seen = []

            def spy(*a, **k):
                r = knn_points(*a, **k)
                seen.append(r.idx[0, :, 0].clone())
                return r

            icp.knn_points = spy
            kw = dict(max_iterations=mi, estimate_scale=scale)
            if use_init:
                kw["init_transform"] = icp.SimilarityTransform(cast(init32[0])[None], cast(init32[1])[None], cast(init32[2])[None])
            if normals:
                kw.update(obj_contact_normals=cast(Xn)[None], hum_contact_normals=cast(Yn)[None])
            sol = icp.ICP(cast(X)[None], cast(Y)[None], **kw)
            icp.knn_points = knn_points
            assert all(bool((s == seen[0]).all()) for s in seen), "the reference's query changed between iterations"
            res[tag] = (sol, seen[0])
        (s32, i32), (s64, i64) = res["32"], res["64"]
        assert bool((i32 == i64).all())
        out[f"{name}_idx"] = i32.numpy().astype(np.int32)
        out[f"{name}_converged"] = np.array(bool(s32.converged))
        out[f"{name}_len_history"] = np.array(len(s32.t_history))
        assert bool(s64.converged) == bool(s32.converged) and len(s64.t_history) == len(s32.t_history)
        for k, a32, a64 in (("R", s32.RTs.R, s64.RTs.R), ("T", s32.RTs.T, s64.RTs.T), ("s", s32.RTs.s, s64.RTs.s), ("rmse", s32.rmse, s64.rmse)):
            out[f"{name}_{k}32"] = a32[0].numpy()
            out[f"{name}_{k}64"] = a64[0].numpy()
            out[f"{name}_d{k}"] = np.abs(a32[0].double().numpy() - a64[0].numpy()).max()
        out[f"{name}_hist_same"] = np.array(all(bool((h.R == s32.t_history[0].R).all() and (h.T == s32.t_history[0].T).all())
                                                 for h in s32.t_history))
        out[f"{name}_cfg"] = np.array([int(normals), int(use_init), int(scale), mi])
        out[f"{name}_gap"] = np.array(gap)
        print(name, "converged", bool(s32.converged), "len", len(s32.t_history), "s", float(s32.RTs.s[0]), "rmse", float(s32.rmse[0]),
              "gap %.2e" % gap, "dR %.2e" % float(out[f"{name}_dR"]))
    # Without normals the reference cannot run at all: it slices the neighbours' normals out of the 3-D neighbours, gets an
    # [1, N, 0] array and multiplies it with R.  So there is no 3-D golden; record that the call raises.
    X, Y, _, _ = data["f255"]
    try:
        icp.ICP(X[None], Y[None], max_iterations=2)
        raised = False
    except RuntimeError:
        raised = True
    assert raised, "the reference ran without normals: add 3-D cases"
    out["icp_reference_raises_without_normals"] = np.array(raised)
    out["icp_cases"] = np.array([c[0] for c in cases])
    out["icp_fixture"] = np.array([c[1] for c in cases])
    return out


def main():
    icp = load_reference()
    out = {}
    with torch.no_grad():
        out.update(align_cases(icp))
        out.update(icp_cases(icp))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
