"""Time ``fit_start.reference_start`` and its stage functions next to the same steps written in torch operations on the same card.

    python tools/bench_fit_start.py [--rounds 5] [--iters 20] [--out FILE.json]

The scene has SMPL-X's counts: a stand-in body of 10475 vertices / 20908 faces (``synthetic.body_mesh(102, 102)``, 10406 / 20808, and
a second small component of 69 vertices / 100 faces, as SMPL-X's eyeballs are one), an object of 10002 vertices / 20000 faces (a UV
sphere), a 1024 x 1024 mask with an elliptic blob, contact vectors with a cap of each mesh above the thresholds.

"torch" is what a user without this module writes: normals as pytorch3d forms them (fp32 face crosses, three ``index_add``, normalise),
stage 1 as optim/fit.py:119-135 has it (``nonzero`` of the mask, a masked mean), the filter as optim/fit.py:142-167 has it (normalise,
``mm``, compare, ``any``).  The ICP is the same ``contact_icp`` call in both columns (it is the project's own, timed in
tools/bench_contact_icp.py), so the two columns differ by the stages of csrc/fit_start.hip and by the filter.  Both columns read the
device where their selections need it.  tools/bench_silhouette.py's method: device events around `iters` calls after a warm-up, the
median of `rounds` rounds, minimum and maximum stated.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_silhouette import timed, uv_sphere  # noqa: E402
from interactvlm_amd import fit_start as fs  # noqa: E402
from interactvlm_amd.contact_icp import contact_icp  # noqa: E402
from interactvlm_amd.synthetic import body_mesh  # noqa: E402


def smplx_sized_body():
    """-> (verts f32 [10475,3], faces int64 [20908,3])"""
    v, f = (torch.as_tensor(t) for t in body_mesh(102, 102))
    n = v.shape[0]
    i, j = torch.meshgrid(torch.arange(3), torch.arange(23), indexing="ij")
    patch = torch.stack([0.02 * j - 0.2, 0.6 + 0.02 * i, 0.3 + 0.001 * (i * j)], -1).reshape(-1, 3).float()
    a = (torch.arange(2)[:, None] * 23 + torch.arange(22)[None]).reshape(-1) + n
    pf = torch.cat([torch.stack([a, a + 1, a + 24], 1), torch.stack([a, a + 24, a + 23], 1)])
    pf = torch.cat([pf, pf[:12]])
    v, f = torch.cat([v, patch]), torch.cat([f.long(), pf])
    assert tuple(v.shape) == (10475, 3) and tuple(f.shape) == (20908, 3)
    return v, f


def torch_normals(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = torch.linalg.cross(b - a, c - a)
    out = torch.zeros_like(verts)
    for k in range(3):
        out.index_add_(0, faces[:, k], n)
    return out / out.norm(dim=1, keepdim=True)


def torch_centroid(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    return (area[:, None] * (a + b + c) / 3.0).sum(0) / area.sum()


def torch_stage1(mask, h_verts, h_probs, focal, principal):
    idx = torch.nonzero(mask).float()
    z = h_verts[h_probs > 0.5, 2].mean()
    cx = idx[1].mean() - principal[0]
    cy = idx[0].mean() - principal[1]
    return torch.stack([cx * z / focal[0], cy * z / focal[1], z])


def torch_start(o_v, o_f, h_v, h_f, o_p, h_p, mask, focal, principal):
    o_n, h_n = torch_normals(o_v, o_f), torch_normals(h_v, h_f)
    T1 = torch_stage1(mask, h_v, h_p, focal, principal)
    h_on, o_on = h_p > 0.5, o_p > 0.3
    hn = F.normalize(-h_n[h_on], p=2, dim=-1)
    on = F.normalize(o_n[o_on], p=2, dim=-1)
    dots = torch.mm(on, hn.T)
    c = torch.cos(torch.deg2rad(torch.tensor(90.0, device=dots.device)))
    c_neg = torch.cos(torch.deg2rad(torch.tensor(-90.0, device=dots.device)))
    best = ((dots > c) | (dots < c_neg)).any(dim=1)
    kept = o_on.clone()
    kept[o_on] = best
    probs = torch.where(kept, o_p, torch.zeros((), device=o_p.device))
    o_on = probs > 0.3
    eye = torch.eye(3, device=o_v.device)[None]
    return contact_icp(o_v[o_on], h_v[h_on], o_n[o_on], h_n[h_on], init=(eye, T1[None], torch.ones(1, device=o_v.device)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_start needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    h_v, h_f = (t.to(dev) for t in smplx_sized_body())
    o_v, o_f = uv_sphere(101, 100, 0.3)
    o_v, o_f = o_v.float().to(dev), o_f.to(dev)
    H = W = 1024
    i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = ((((i - 430.0) / 180.0) ** 2 + ((j - 610.0) / 140.0) ** 2) <= 1.0).to(torch.uint8).to(dev)
    focal, principal = (1.5 * W, 1.5 * W), (W / 2 + 1.3, H / 2 - 0.7)
    cam = (torch.tensor(focal, device=dev), torch.tensor(principal, device=dev))

    def cap(v, direction, cos):
        d = torch.tensor(direction, device=dev)
        inside = F.normalize(v, dim=1) @ (d / d.norm()) > cos
        r = torch.rand(v.shape[0], generator=gen).to(dev)
        return torch.where(inside, 0.55 + 0.45 * r, 0.25 * r)

    h_p, o_p = cap(h_v, [0.3, 0.2, 1.0], 0.9), cap(o_v, [0.1, -0.4, -1.0], 0.9)
    steps = {
        "reference_start": lambda: fs.reference_start(o_v, o_f, h_v, h_f, o_p, h_p, mask, focal, principal),
        "reference_start_torch": lambda: torch_start(o_v, o_f, h_v, h_f, o_p, h_p, mask, *cam),
        "vertex_normals_human": lambda: fs.vertex_normals(h_v, h_f),
        "vertex_normals_human_torch": lambda: torch_normals(h_v, h_f),
        "surface_centroid_human": lambda: fs.surface_centroid(h_v, h_f),
        "surface_centroid_human_torch": lambda: torch_centroid(h_v, h_f),
        "mask_stats": lambda: fs.mask_stats(mask),
        "centroid_start": lambda: fs.centroid_start(mask, h_v, h_p, focal, principal),
        "centroid_start_torch": lambda: torch_stage1(mask, h_v, h_p, *cam),
    }
    start = steps["reference_start"]()
    want = steps["reference_start_torch"]()
    info = dict(human=list(h_v.shape), human_faces=list(h_f.shape), obj=list(o_v.shape), obj_faces=list(o_f.shape), mask=[H, W],
                mask_pixels=int(mask.sum()), human_selected=int((h_p > 0.5).sum()), obj_selected=int((o_p > 0.3).sum()),
                obj_kept=int(start.kept.sum()),
                same_neighbours_as_torch=bool(torch.equal(start.icp.nn_idx, want.nn_idx)),
                max_abs_R_difference_from_torch=float((start.icp.R - want.R).abs().max()),
                max_abs_T_difference_from_torch=float((start.icp.T - want.T).abs().max()))
    print(json.dumps({"case": "scene", **info}), flush=True)
    results = [{"case": "scene", **info}]
    for name, step in steps.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        rounds = [timed(step, a.iters) for _ in range(a.rounds)]
        row = dict(case=name, us_median=round(statistics.median(rounds), 1), us_min=round(min(rounds), 1), us_max=round(max(rounds), 1),
                   rounds=a.rounds, iters=a.iters)
        print(json.dumps(row), flush=True)
        results.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
