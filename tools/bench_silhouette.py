"""Time soft_silhouette (forward + backward into the vertices) and one whole ObjectPoseFit step (silhouette, image terms, contact
term, backward into rotation and translation), and record the peak memory.

    python tools/bench_silhouette.py [--rounds 5] [--iters 20] [--out FILE.json]

Shapes: a UV sphere of radius 0.5 at Z = 3 seen with fx = fy = 1.5 W (it covers half the image width), sigma = 1e-4 and the default
blur_radius, as the reference's fit has them: (N, F, H, W) ~ (20 000, 40 000, 1024, 1024), the reference's scale, and (2048, 4096,
512, 512), at B = 1 and B = 8 poses.  A dense torch form cannot hold [H W, F] at these sizes and no earlier implementation exists,
so these are absolute numbers, not a speed-up.  Times are device events around `iters` calls; the median and the minimum of the
rounds are reported.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from interactvlm_amd import _lib, fit  # noqa: E402
from interactvlm_amd import silhouette as sil  # noqa: E402


def uv_sphere(nlat, nlon, radius=0.5):
    """-> verts fp32 [2 + (nlat - 1) nlon, 3], faces int64 [2 nlon (nlat - 1), 3]"""
    th = math.pi * torch.arange(1, nlat, dtype=torch.float64)[:, None] / nlat
    ph = 2 * math.pi * torch.arange(nlon, dtype=torch.float64)[None] / nlon
    ring = torch.stack((th.sin() * ph.cos(), th.sin() * ph.sin(), th.cos().expand(nlat - 1, nlon)), -1).reshape(-1, 3)
    verts = radius * torch.cat((torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64), ring, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64)))
    j = torch.arange(nlon)
    j1 = (j + 1) % nlon
    at = lambda i, jj: 1 + (i - 1) * nlon + jj  # noqa: E731
    faces = [torch.stack((torch.zeros_like(j), at(1, j), at(1, j1)), -1)]
    for i in range(1, nlat - 1):
        faces.append(torch.stack((at(i, j), at(i + 1, j), at(i + 1, j1)), -1))
        faces.append(torch.stack((at(i, j), at(i + 1, j1), at(i, j1)), -1))
    last = verts.shape[0] - 1
    faces.append(torch.stack((torch.full_like(j, last), at(nlat - 1, j1), at(nlat - 1, j)), -1))
    return verts.float(), torch.cat(faces)


def timed(step, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per call


def peak(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_silhouette needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(0)
    results = []
    for nlat, nlon, H, W in ((101, 200, 1024, 1024), (33, 64, 512, 512)):
        obj, faces = uv_sphere(nlat, nlon)
        N, F = obj.shape[0], faces.shape[0]
        faces = faces.to(dev)
        focal, principal = (1.5 * W, 1.5 * W), (W / 2 + 1.3, H / 2 - 0.7)
        human = (torch.randn(6890, 3, generator=gen) * 0.3 + torch.tensor([0.9, 0.0, 3.0])).to(dev)
        p_obj = (torch.rand(N, generator=gen) * (torch.rand(N, generator=gen) < 0.05)).to(dev)
        p_hum = (torch.rand(6890, generator=gen) * (torch.rand(6890, generator=gen) < 0.05)).to(dev)
        for B in (1, 8):
            shift = torch.stack([torch.tensor([0.1 + 0.01 * b, -0.05, 3.0 + 0.02 * b]) for b in range(B)])
            verts = (obj[None] + shift[:, None]).to(dev).requires_grad_(True)
            g = torch.randn(B, H, W, generator=gen).to(dev)
            target = (sil.soft_silhouette(verts[0].detach(), faces, focal, principal, (H, W)) > 0.5).float()

            def render_step():
                verts.grad = None
                sil.soft_silhouette(verts, faces, focal, principal, (H, W)).backward(g)

            model = fit.ObjectPoseFit(fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(dev), (shift + 0.03).to(dev), 1.0, obj.to(dev), faces,
                                      human, p_obj, p_hum, target, focal, principal)

            def fit_step():
                model.rotation.grad = model.translation.grad = None
                total, _ = model(step=0)
                total.sum().backward()

            for step in (render_step, fit_step):
                for _ in range(3):
                    step()
            mem = {"render": peak(render_step), "fit": peak(fit_step)}
            t = {"render": [], "fit": []}
            for _ in range(a.rounds):
                t["render"].append(timed(render_step, a.iters))
                t["fit"].append(timed(fit_step, a.iters))
            r = {"B": B, "N": N, "F": F, "H": H, "W": W, "sigma": 1e-4,
                 "render_fwd_bwd_us_median": statistics.median(t["render"]), "render_fwd_bwd_us_min": min(t["render"]),
                 "fit_step_us_median": statistics.median(t["fit"]), "fit_step_us_min": min(t["fit"]),
                 "render_peak_bytes": mem["render"], "fit_step_peak_bytes": mem["fit"],
                 "workspace_bytes": lib.ivlm_soft_silhouette_workspace_bytes(B, N, F, H, W)}
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
