"""Time one ObjectPoseFit step (forward and backward into rotation and translation) without and with the occlusion-aware terms, and the
depth-order term alone (``occlusion.depth_order`` forward + backward into the vertices).

    python tools/bench_occlusion.py [--rounds 5] [--iters 20] [--out FILE.json]

The scene: the 6890-vertex / 13776-face stand-in body (``synthetic.body_mesh``) three units in front of the camera and a UV sphere of
radius 0.5 (2050 vertices, 4096 faces) behind it, sticking out beside it, at 512 x 512 with fx = fy = 1.5 W, B = 1 and B = 8 poses.
The target mask is the sphere's visible pixels.  "plain" is ``ObjectPoseFit`` with occlusion=False and the default weights - the step
of the commit before the occlusion terms existed, bit for bit; "aware" adds the don't-care image (occlusion=True, default weights);
"aware_term" adds "depth_order_loss" as well.  There is no earlier implementation of the new kernels to compare against: "plain" is
the comparison.  tools/bench_silhouette.py's method: device events around `iters` calls, the median of `rounds` rounds, the minimum
and the maximum stated.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_silhouette import timed, uv_sphere  # noqa: E402
from interactvlm_amd import _lib, fit, occlusion  # noqa: E402
from interactvlm_amd.synthetic import body_mesh  # noqa: E402

DO = "depth_order_loss"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occlusion needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(0)
    H = W = 512
    focal, principal = (1.5 * W, 1.5 * W), (W / 2 + 1.3, H / 2 - 0.7)
    obj, faces = uv_sphere(33, 64)
    N, F = obj.shape[0], faces.shape[0]
    obj, faces = obj.to(dev), faces.to(dev)
    human, human_faces = (t.to(dev) for t in body_mesh())
    offset = torch.tensor([0.0, 0.0, 3.0], device=dev)
    p_obj = (torch.rand(N, generator=gen) * (torch.rand(N, generator=gen) < 0.05)).to(dev)
    p_hum = (torch.rand(human.shape[0], generator=gen) * (torch.rand(human.shape[0], generator=gen) < 0.05)).to(dev)
    centre = torch.tensor([0.35, 0.1, 0.8])
    d_h, _ = occlusion.depth_image(human + offset, human_faces, focal, principal, (H, W))
    d_o, _ = occlusion.depth_image(obj + centre.to(dev) + offset, faces, focal, principal, (H, W))
    target = (torch.isfinite(d_o[0]) & ~(d_h[0] < d_o[0])).float()
    weights = {**fit.DEFAULT_LOSS_WEIGHTS, DO: {"w": 1.0, "kick_in": 0}}
    results = []
    for B in (1, 8):
        shift = torch.stack([centre + torch.tensor([0.01 * b, -0.02, 0.02 * b]) for b in range(B)]).to(dev)
        r6 = fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(dev)
        scene_args = (obj, faces, human, p_obj, p_hum, target, focal, principal, offset)
        plain = fit.ObjectPoseFit(r6, shift, 1.0, *scene_args, human_faces=human_faces)
        aware = fit.ObjectPoseFit(r6, shift, 1.0, *scene_args, human_faces=human_faces, occlusion=True)
        verts = (obj[None] + shift[:, None] + offset).detach().requires_grad_(True)
        g = torch.ones(B, device=dev)

        def step_of(model, w):
            def step():
                model.rotation.grad = model.translation.grad = None
                total, _ = model(w, step=0)
                total.sum().backward()
            return step

        def term_step():
            verts.grad = None
            occlusion.depth_order(verts, faces, aware.scene.occluder_depth, aware.scene.signed_weight, focal, principal).backward(g)

        steps = {"plain": step_of(plain, None), "aware": step_of(aware, None), "aware_term": step_of(aware, weights), "term": term_step}
        for step in steps.values():
            for _ in range(3):
                step()
        t = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, step in steps.items():
                t[k].append(timed(step, a.iters))
        with torch.no_grad():
            _, terms = aware(weights, step=0)
        r = {"B": B, "N": N, "F": F, "H": H, "W": W, "N_h": int(human.shape[0]), "F_h": int(human_faces.shape[0]),
             "visible_pixels": int(target.sum()), "object_pixels": int(torch.isfinite(d_o).sum()),
             "weighted_pixels": int((aware.scene.signed_weight != 0).sum()), "depth_order_loss": [float(x) for x in terms[DO]],
             "workspace_bytes": lib.ivlm_depth_order_workspace_bytes(B, N, F, H, W)}
        for k, v in t.items():
            r[f"{k}_us_median"], r[f"{k}_us_min"], r[f"{k}_us_max"] = statistics.median(v), min(v), max(v)
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
