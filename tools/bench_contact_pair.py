"""Time contact_distance (forward + backward into both vertex tensors) against the dense torch formulation of the same term
(cdist, outer product, autograd) on the same GPU in one process, and record the peak memory of both.

    python tools/bench_contact_pair.py [--rounds 5] [--iters 20] [--out FILE.json]

Shapes: (20000, 6890) an object mesh against the SMPL body, (2048, 6890) the 'oafford' cloud; contact probabilities 5 % non-zero
(what the predictors give) and all non-zero (the worst case for the fused path, which skips zeros).  Each variant is warmed up on
every shape; fused and dense rounds alternate; times are device events around `iters` calls; the median and the minimum of the
rounds are reported.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from interactvlm_amd import contact_pair as cp  # noqa: E402


def fused_step(o, h, p, q):
    o.grad = h.grad = None
    cp.contact_distance(o, h, p, q).backward()


def dense_step(o, h, p, q):
    o.grad = h.grad = None
    w = torch.outer(p, q)
    ((torch.cdist(o.unsqueeze(0), h.unsqueeze(0)).squeeze(0) * w).sum() / w.sum()).backward()


def timed(step, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per forward + backward


def peak(step, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(*args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contact_pair needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    results = []
    for n_o, n_h in ((20000, 6890), (2048, 6890)):
        for density in (0.05, 1.0):
            o = torch.randn(n_o, 3, generator=g).to(dev).requires_grad_(True)
            h = torch.randn(n_h, 3, generator=g).to(dev).requires_grad_(True)
            p = (torch.rand(n_o, generator=g) * (torch.rand(n_o, generator=g) < density)).to(dev)
            q = (torch.rand(n_h, generator=g) * (torch.rand(n_h, generator=g) < density)).to(dev)
            args = (o, h, p, q)
            for step in (fused_step, dense_step):  # warm-up of this shape
                for _ in range(3):
                    step(*args)
            fused_step(*args)
            gf = (o.grad.clone(), h.grad.clone())
            dense_step(*args)
            agree = max(float((o.grad - gf[0]).abs().max()), float((h.grad - gf[1]).abs().max()))
            mem = {"fused": peak(fused_step, args), "dense": peak(dense_step, args)}
            t = {"fused": [], "dense": []}
            for _ in range(a.rounds):
                t["fused"].append(timed(fused_step, args, a.iters))
                t["dense"].append(timed(dense_step, args, a.iters))
            r = {"n_o": n_o, "n_h": n_h, "nonzero": density, "pairs": n_o * n_h,
                 "fused_us_median": statistics.median(t["fused"]), "fused_us_min": min(t["fused"]),
                 "dense_us_median": statistics.median(t["dense"]), "dense_us_min": min(t["dense"]),
                 "fused_peak_bytes": mem["fused"], "dense_peak_bytes": mem["dense"], "max_abs_grad_difference": agree}
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
