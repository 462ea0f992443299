"""Time contact_icp against a dense torch restatement of the same loop on the same GPU in one process, and record the peak
memory of both.

    python tools/bench_contact_icp.py [--rounds 5] [--iters 20] [--out FILE.json]

Variants: `requery` = contact_icp(requery=True, max_iterations=10, relative_rmse_thr=-1: every pose runs all 10 iterations),
`drop_in` = contact_icp(requery=False) (the reference's result: one pass), `dense` = broadcasted squared differences + argmin +
the alignment with torch.linalg.svd, 10 iterations, with the per-iteration `.all()` host read the reference's loop has, and
`dense_one` = one such iteration (what the reference's loop amounts to).  Shapes (B, N_o, N_h): (1, 4096, 2000), (1, 20000, 6890),
(64, 4096, 2000), with normals (6-D queries).  Each variant is warmed up on every shape; the rounds of the variants alternate;
times are device events around `iters` calls; median and minimum of the rounds.  Prints one JSON line per shape.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from interactvlm_amd import contact_icp as ci  # noqa: E402

ITERATIONS = 10


def dense_align(X, Y):
    mx, my = X.mean(1, keepdim=True), Y.mean(1, keepdim=True)
    Xc, Yc = X - mx, Y - my
    U, S, Vh = torch.linalg.svd(Xc.transpose(1, 2) @ Yc / X.shape[1])
    E = torch.eye(3, device=X.device).repeat(X.shape[0], 1, 1)
    E[:, 2, 2] = torch.det(U @ Vh)
    R = U @ E @ Vh
    return R, (my - mx @ R)[:, 0]


def dense_icp(X, Y, Xn, Yn, R, T, iterations):
    t = torch.cat([Y, -Yn], -1)
    prev = None
    for _ in range(iterations):
        q = torch.cat([X @ R + T[:, None], Xn @ R], -1)
        idx = ((q[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1).argmin(-1)
        nn = torch.gather(Y, 1, idx[..., None].expand(-1, -1, 3))
        R, T = dense_align(X, nn)
        rmse = ((X @ R + T[:, None] - nn) ** 2).sum(-1).mean(-1).sqrt()
        if prev is not None and bool((((prev - rmse) / prev) <= -1.0).all()):  # never true: the host read is what is timed
            break
        prev = rmse
    return R, T


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
        raise SystemExit("bench_contact_icp needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    results = []
    for B, n_o, n_h in ((1, 4096, 2000), (1, 20000, 6890), (64, 4096, 2000)):
        X = (torch.randn(n_o, 3, generator=g) * 0.2).to(dev)
        Y = (torch.randn(n_h, 3, generator=g) * 0.2).to(dev)
        Xn = torch.nn.functional.normalize(torch.randn(n_o, 3, generator=g), dim=-1).to(dev)
        Yn = torch.nn.functional.normalize(torch.randn(n_h, 3, generator=g), dim=-1).to(dev)
        ang = torch.linspace(0.0, 1.0, B)
        R0 = torch.eye(3).repeat(B, 1, 1)
        R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1] = ang.cos(), ang.sin(), -ang.sin(), ang.cos()
        R0, T0, s0 = R0.to(dev), torch.zeros(B, 3, device=dev), torch.ones(B, device=dev)
        dense_bytes = B * n_o * n_h * 4
        Xb, Yb, Xnb, Ynb = (t.unsqueeze(0).expand(B, -1, -1) for t in (X, Y, Xn, Yn))
        steps = {
            "requery": lambda: ci.contact_icp(X, Y, Xn, Yn, init=(R0, T0, s0), requery=True, max_iterations=ITERATIONS, relative_rmse_thr=-1.0),
            "drop_in": lambda: ci.contact_icp(X, Y, Xn, Yn, init=(R0, T0, s0), max_iterations=ITERATIONS),
        }
        if dense_bytes * 6 * 3 < 100e9:  # the [B, N_o, N_h, 6] difference array and its square
            steps["dense"] = lambda: dense_icp(Xb, Yb, Xnb, Ynb, R0, T0, ITERATIONS)
            steps["dense_one"] = lambda: dense_icp(Xb, Yb, Xnb, Ynb, R0, T0, 1)
        for step in steps.values():
            for _ in range(2):
                step()
        r = {"B": B, "n_o": n_o, "n_h": n_h, "iterations": ITERATIONS, "pairs_per_iteration": B * n_o * n_h}
        out = steps["requery"]()
        r["requery_iterations_run"] = out.iterations.cpu().tolist()[:4]
        if "dense" in steps:
            Rd, _ = steps["dense"]()
            r["max_abs_R_difference_requery_vs_dense"] = float((out.R - Rd).abs().max())
        for name, step in steps.items():
            r[f"{name}_peak_bytes"] = peak(step)
        t = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():
                t[name].append(timed(step, a.iters))
        for name in steps:
            r[f"{name}_us_median"] = statistics.median(t[name])
            r[f"{name}_us_min"] = min(t[name])
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
