"""Time MeshSDF.intrusion next to MeshSDF.penetration on the same GPU in one process (value and gradients, through autograd).

    python tools/bench_intrusion.py [--rounds 5] [--iters 500] [--out FILE.json]

Shapes: the human is ``body_mesh()`` (N = 6890 vertices, F = 13 776), the object ``body_mesh(16, 16)`` (258 vertices, F = 512) shrunk
to a third and put where it overlaps the body, under B = 24 poses (small distinct rotations and shifts, s in [0.9, 1.1]).  Three calls:
  intrusion            object.intrusion(human vertices [N,3], the 24 poses): un-pose, two sweeps over 512 faces, 13 sums per pose
  penetration_same     object.penetration(x [24,N,3]) on the same un-posed points, made beforehand: the same sweeps, the gradient rows
  penetration_fit      human.penetration(posed object vertices [24,258,3]): the direction the fit's penetration term runs
Every call is warmed up; the rounds alternate between the calls; times are device events around `iters` calls; the median and the
minimum of the rounds are reported.  Prints one JSON line.  Needs a GPU: there is no CPU path.
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

from interactvlm_amd import mesh_sdf as ms  # noqa: E402
from interactvlm_amd.fit import matrix_to_rot6d  # noqa: E402
from interactvlm_amd.pose import axis_rotations, pose_transform  # noqa: E402
from interactvlm_amd.synthetic import body_mesh  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intrusion needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    B = 24
    hv, hf = (t.to(dev) for t in body_mesh())
    ov, of = body_mesh(16, 16)
    ov, of = (ov / 3.0).contiguous().to(dev), of.to(dev)
    ms.check_closed(ov, of)
    human, obj = ms.MeshSDF(hv, hf), ms.MeshSDF(ov, of)
    g = torch.Generator().manual_seed(0)
    R = axis_rotations(B * 15, axis=(0.3, 1.0, 0.2))[:B]  # 0 .. 23 x 1 degree
    r6 = matrix_to_rot6d(R).to(dev).requires_grad_(True)
    t = (torch.tensor([0.5, 0.3, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 0.1).to(dev).requires_grad_(True)
    s = (0.9 + 0.2 * torch.rand(B, generator=g)).to(dev).requires_grad_(True)
    with torch.no_grad():
        x = (((hv[None] - t[:, None]) @ R.to(dev).transpose(1, 2)) / s[:, None, None]).contiguous()
        inside = float((obj.query(x)[0] < 0).float().mean())
    xg = x.clone().requires_grad_(True)

    def intrusion_step():
        r6.grad = t.grad = s.grad = None
        obj.intrusion(hv, r6, t, s).sum().backward()

    def penetration_same_step():
        xg.grad = None
        obj.penetration(xg).sum().backward()

    def penetration_fit_step():
        r6.grad = t.grad = s.grad = None
        human.penetration(pose_transform(ov, r6, t, s)).sum().backward()

    steps = {"intrusion": intrusion_step, "penetration_same": penetration_same_step, "penetration_fit": penetration_fit_step}
    for step in steps.values():
        for _ in range(3):
            step()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, step in steps.items():
            times[k].append(timed(step, a.iters))
    with torch.no_grad():
        L = obj.intrusion(hv, r6, t, s)
    r = {"B": B, "N": int(hv.shape[0]), "F_object": int(of.shape[0]), "F_human": int(hf.shape[0]), "N_object": int(ov.shape[0]),
         "inside_fraction": inside, "intrusion_mean": float(L.mean()), "finite": bool(math.isfinite(float(L.sum()))),
         "rounds": a.rounds, "iters": a.iters}
    for k in steps:
        r[f"{k}_us_median"], r[f"{k}_us_min"] = statistics.median(times[k]), min(times[k])
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
