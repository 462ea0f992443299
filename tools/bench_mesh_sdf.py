"""Time MeshSDF.query and MeshSDF.penetration (value + gradient) against the obvious torch formulation of the distance on the same
GPU in one process: chunked fp32 point-to-face closest distance over [n, F] blocks (Ericson's regions with torch.where, min over
the faces), as a user without the kernel would write it.  The torch side computes the unsigned distance only - no winding number,
no gradient - so the ratio understates what the kernel saves.

    python tools/bench_mesh_sdf.py [--rounds 5] [--iters 20] [--out FILE.json]

Shapes: B in {1, 24} poses of N = 2048 object points against ``body_mesh()`` (F = 13 776, the SMPL topology's counts); the points
fill a box of edge 0.5 that overlaps the body (about a third of them inside), each pose shifted a little; and the same object moved
wholly outside the mesh's bounding box, where penetration sweeps no face.  Every variant is warmed up on every shape; kernel and
torch rounds alternate; times are device events around `iters` calls (the torch side: max(1, iters // 10), it is slow); the median
and the minimum of the rounds are reported.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from interactvlm_amd import mesh_sdf as ms  # noqa: E402
from interactvlm_amd.synthetic import body_mesh  # noqa: E402


def _dot(u, v):
    return (u * v).sum(-1)


def torch_distance(points, v0, v1, v2, block=256):
    """points [B,N,3] -> d [B,N]: the closest distance to any face, [block, F] at a time"""
    out = []
    flat = points.reshape(-1, 3)
    for lo in range(0, flat.shape[0], block):
        x = flat[lo:lo + block, None, :]
        a, b, c = v0 - x, v1 - x, v2 - x
        e1, e2 = b - a, c - a
        d1, d2, d3, d4, d5, d6 = -_dot(e1, a), -_dot(e2, a), -_dot(e1, b), -_dot(e2, b), -_dot(e1, c), -_dot(e2, c)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        d43, d56 = d4 - d3, d5 - d6
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        nv, nw, dn = vb, vc, va + vb + vc
        for cond, cv, cw, cd in (((va <= 0) & (d43 >= 0) & (d56 >= 0), d56, d43, d43 + d56), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                 ((d6 >= 0) & (d5 <= d6), zero, one, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                 ((d3 >= 0) & (d4 <= d3), one, zero, one), ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
            nv, nw, dn = torch.where(cond, cv, nv), torch.where(cond, cw, nw), torch.where(cond, cd, dn)
        q = a + e1 * (nv / dn)[..., None] + e2 * (nw / dn)[..., None]
        out.append(_dot(q, q).min(1).values.sqrt())
    return torch.cat(out).reshape(points.shape[:-1])


def timed(step, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sdf needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    verts, faces = (t.to(dev) for t in body_mesh())
    mesh = ms.MeshSDF(verts, faces)
    v0, v1, v2 = (verts[faces[:, k].long()][None] for k in range(3))
    g = torch.Generator().manual_seed(0)
    N = 2048
    results = []
    for B in (1, 24):
        box = (torch.rand(N, 3, generator=g) - 0.5) * 0.5 + torch.tensor([0.0, 0.4, 0.2])
        base = (box[None] + (torch.rand(B, 1, 3, generator=g) - 0.5) * 0.1).to(dev)
        for where, pts in (("overlapping", base), ("outside the bounding box", base + torch.tensor([5.0, 0.0, 0.0], device=dev))):
            x = pts.clone().requires_grad_(True)

            def query_step():
                mesh.query(pts)

            def pen_step():
                x.grad = None
                mesh.penetration(x).sum().backward()

            def torch_step():
                torch_distance(pts, v0, v1, v2)

            steps = {"query": (query_step, a.iters), "penetration": (pen_step, a.iters), "torch_distance": (torch_step, max(1, a.iters // 10))}
            for step, _ in steps.values():  # warm-up of this shape
                for _ in range(2):
                    step()
            sdf = mesh.query(pts)[0]
            agree = float((sdf.abs() - torch_distance(pts, v0, v1, v2)).abs().max())
            t = {k: [] for k in steps}
            for _ in range(a.rounds):
                for k, (step, iters) in steps.items():
                    t[k].append(timed(step, iters))
            r = {"B": B, "N": N, "F": int(faces.shape[0]), "object": where, "inside_fraction": float((sdf < 0).float().mean()),
                 "max_abs_distance_difference": agree}
            for k in steps:
                r[f"{k}_us_median"], r[f"{k}_us_min"] = statistics.median(t[k]), min(t[k])
            r["torch_over_query"] = r["torch_distance_us_median"] / r["query_us_median"]
            r["torch_over_penetration"] = r["torch_distance_us_median"] / r["penetration_us_median"]
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
