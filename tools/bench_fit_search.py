"""Time one ObjectPoseFit step (forward, total.sum().backward()) with the pose-by-pose torch transform and with the fused
pose_transform, one whole iteration of the torch loop (that step plus torch.optim.Adam) and one of the device loop
(fit.DevicePoseFit.step, whose last total is checked against the torch loop's after the same iterations), at B = 1, 8, 24 starts,
and one whole search_object_pose (24 starts, 250 iterations) with the torch loop and with device_loop=True.

    python tools/bench_fit_search.py [--rounds 5] [--iters 20] [--out FILE.json] [--baseline PARENT.json] [--commit HASH]
    python tools/bench_fit_search.py --tree PATH --commit HASH --out PARENT.json    # the same steps with the package of another checkout

The method and the shapes are those of tools/bench_silhouette.py: a UV sphere of radius 0.5 at Z = 3 covering half the image width,
sigma 1e-4, (N, F, H, W) = (20002, 40000, 1024, 1024) and (2050, 4096, 512, 512), 6890 human vertices, 5 % contact on both sides;
device events around `iters` steps, the median of `rounds` rounds (all rounds are kept in the output).  The baseline of "fused off" is
the parent commit's step: run the tool with --tree on a checkout of the parent in the same session on the same machine (it times
only what that package has), then pass its output with --baseline; the merged file is what profiles/fit_search_bench.json holds
(profiles/fit_device_loop_bench.json for the run that added the device loop, whose parent column is the parent's torch iteration).
The whole search is wall time around a synchronised call, host reads included, beside the same 24 starts fitted by
fit_object_pose with the torch transform.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((101, 200, 1024, 1024), (33, 64, 512, 512))
BATCHES = (1, 8, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--search-rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=250)
    ap.add_argument("--tree", default=None, help="root of another checkout whose interactvlm_amd package is timed instead")
    ap.add_argument("--commit", default="unknown", help="the commit of the timed tree (a tree copied without .git cannot tell)")
    ap.add_argument("--baseline", default=None, help="output of a --tree run: merged into --out as the parent's side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(HERE)
    sys.path.insert(0, root)
    from interactvlm_amd import fit  # before bench_silhouette, which puts its own tree in front of the path
    from interactvlm_amd import silhouette as sil
    from bench_silhouette import timed, uv_sphere  # (this directory: the script's own)

    if os.path.dirname(os.path.dirname(os.path.abspath(fit.__file__))) != root:
        raise SystemExit(f"interactvlm_amd was imported from {fit.__file__}, not from {root}")

    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_search needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    has_fused = "fused_transform" in inspect.signature(fit.ObjectPoseFit.__init__).parameters
    has_device = hasattr(fit, "DevicePoseFit")
    modes = (("off", False), ("on", True)) if has_fused else (("off", False),)
    gen = torch.Generator().manual_seed(0)
    cases, scene_small = [], None
    for nlat, nlon, H, W in SHAPES:
        obj, faces = uv_sphere(nlat, nlon)
        N, F = obj.shape[0], faces.shape[0]
        faces = faces.to(dev)
        focal, principal = (1.5 * W, 1.5 * W), (W / 2 + 1.3, H / 2 - 0.7)
        human = (torch.randn(6890, 3, generator=gen) * 0.3 + torch.tensor([0.9, 0.0, 3.0])).to(dev)
        p_obj = (torch.rand(N, generator=gen) * (torch.rand(N, generator=gen) < 0.05)).to(dev)
        p_hum = (torch.rand(6890, generator=gen) * (torch.rand(6890, generator=gen) < 0.05)).to(dev)
        centre = torch.tensor([0.1, -0.05, 3.0])
        target = (sil.soft_silhouette((obj + centre).to(dev), faces, focal, principal, (H, W)) > 0.5).float()
        scene = (obj.to(dev), faces, human, p_obj, p_hum, target, focal, principal)
        if (H, W) == (512, 512):
            scene_small = scene
        for B in BATCHES:
            shift = torch.stack([centre + torch.tensor([0.01 * b, 0.0, 0.02 * b]) for b in range(B)])
            steps = {}
            for name, fused in modes:
                kw = {"fused_transform": True} if fused else {}
                model = fit.ObjectPoseFit(fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(dev), (shift + 0.03).to(dev), 1.0, *scene, **kw)

                def fit_step(model=model):
                    model.rotation.grad = model.translation.grad = None
                    total, _ = model(step=0)
                    total.sum().backward()

                for _ in range(3):
                    fit_step()
                steps[name] = fit_step
            if has_fused:  # a whole iteration of the torch loop: the fused step and torch.optim.Adam as fit_object_pose drives them
                model = fit.ObjectPoseFit(fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(dev), (shift + 0.03).to(dev), 1.0, *scene,
                                          fused_transform=True)
                opt = torch.optim.Adam([{"params": [model.rotation], "lr": 5e-2}, {"params": [model.translation], "lr": 1e-2}])

                last = {}

                def torch_iteration(model=model, opt=opt, last=last):
                    opt.zero_grad()
                    total, _ = model(step=0)
                    total.sum().backward()
                    opt.step()
                    last["total"] = total.detach()

                for _ in range(3):
                    torch_iteration()
                steps["torch_loop"] = torch_iteration
            if has_device:  # the same iteration as one C call
                dfit = fit.DevicePoseFit(fit.matrix_to_rot6d(torch.eye(3)).expand(B, 6).to(dev), (shift + 0.03).to(dev), 1.0, *scene,
                                         max_iter=3 + a.rounds * a.iters)
                for _ in range(3):
                    dfit.step()
                steps["device_loop"] = dfit.step
            t = {name: [] for name in steps}
            for _ in range(a.rounds):  # the modes alternate inside a round, so that a drift of the machine reaches both
                for name, step in steps.items():
                    t[name].append(timed(step, a.iters))
            r = {"B": B, "N": N, "F": F, "H": H, "W": W}
            for name in steps:
                r[f"step_{name}_us_rounds"] = t[name]
                r[f"step_{name}_us_median"] = statistics.median(t[name])
            if has_device:  # faster and different is not faster: both loops have run the same iterations from the same start
                theirs, mine = last["total"], dfit.history[dfit.iteration - 1]
                r["device_loop_iterations"] = dfit.iteration
                r["device_loop_last_total_max_rel_diff_to_torch"] = float(((mine - theirs).abs() / theirs.abs()).max())
                r["device_loop_last_total_finite"] = bool(torch.isfinite(mine).all())
            print(json.dumps(r), flush=True)
            cases.append(r)
    result = {"machine": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})", "torch": torch.__version__,
              "commit": a.commit, "fused_transform_available": has_fused, "rounds": a.rounds, "iters": a.iters, "cases": cases}
    if has_fused and a.search_rounds > 0:
        from interactvlm_amd import pose

        K = 24
        search = {"starts": K, "max_iter": a.max_iter, "N": scene_small[0].shape[0], "H": 512, "W": 512}
        init = (torch.eye(3), torch.tensor([0.13, -0.02, 3.03]), 1.0)
        r6, T, s = pose.pose_starts(pose.cube_rotations().to(dev), *init)

        def whole_search():
            return fit.search_object_pose(*scene_small, init=init, icp=True, max_iter=a.max_iter)

        def unfused_fit():
            return fit.fit_object_pose(*scene_small, init=(r6, T, s), max_iter=a.max_iter)

        fit.search_object_pose(*scene_small, init=init, icp=True, max_iter=3)  # warm: the topology cache, the allocator

        def device_search():
            return fit.search_object_pose(*scene_small, init=init, icp=True, max_iter=a.max_iter, device_loop=True)

        calls = [("search_ms_rounds", whole_search), ("unfused_fit_24_starts_ms_rounds", unfused_fit)]
        if has_device:
            fit.search_object_pose(*scene_small, init=init, icp=True, max_iter=3, device_loop=True)
            calls.insert(1, ("search_device_loop_ms_rounds", device_search))
        for name, call in calls:
            times = []
            for _ in range(a.search_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            search[name] = times
            search[name.replace("_rounds", "_median")] = statistics.median(times)
            if name.startswith("search"):  # (best_index: the torch loop's; the device loop's beside it)
                search["best_index" if name == "search_ms_rounds" else "device_loop_best_index"] = int(out["best_index"])
        print(json.dumps(search), flush=True)
        result["search"] = search
    if a.baseline:
        with open(a.baseline) as f:
            base = json.load(f)
        result["parent_commit"] = base["commit"]
        result["parent_machine"] = base["machine"]
        for r, p in zip(result["cases"], base["cases"]):
            assert all(r[k] == p[k] for k in ("B", "N", "F", "H", "W"))
            r["parent_step_us_rounds"] = p["step_off_us_rounds"]
            r["parent_step_us_median"] = p["step_off_us_median"]
            if "step_on_us_rounds" in p:  # the parent's step with the fused transform
                r["parent_step_on_us_rounds"] = p["step_on_us_rounds"]
                r["parent_step_on_us_median"] = p["step_on_us_median"]
            for mode in ("torch_loop", "device_loop"):  # the parent's whole iteration with the fused transform, in either loop
                if f"step_{mode}_us_rounds" in p:
                    r[f"parent_{mode}_us_rounds"] = p[f"step_{mode}_us_rounds"]
                    r[f"parent_{mode}_us_median"] = p[f"step_{mode}_us_median"]
        if "search" in base and "search" in result:
            for name in ("search", "search_device_loop"):
                if f"{name}_ms_rounds" in base["search"]:
                    result["search"][f"parent_{name}_ms_rounds"] = base["search"][f"{name}_ms_rounds"]
                    result["search"][f"parent_{name}_ms_median"] = base["search"][f"{name}_ms_median"]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
