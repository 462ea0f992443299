"""The fp64 yardstick of the multi-start search test: all 24 cube-rotation starts of tests/_pose_scene.py fitted on the CPU with the
project's own fp64 definitions (tests/_silhouette_ref.py render and terms, fit.apply_transformation in fp64, torch.optim.Adam).

    python tests/golden/make_golden_pose_search.py        # about a minute of CPU; writes tests/golden/pose_search_fp64.json

It refuses to write a fixture whose winner is not separated from the runner-up by 1e-3 of the winning total: the margin the GPU
test relies on must come from the fp64 definitions alone.
"""
from __future__ import annotations

import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _pose_scene as ps  # noqa: E402


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cam, obj, faces, hum, p_obj, p_hum, target, T_start = ps.search_scene()
    finals, first, last = [], [], []
    for k in range(24):
        history, final = ps.fit_fp64(k)
        finals.append(final)
        first.append(history[0])
        last.append(history[-1])
        print(f"start {k:2d}: total {history[0]:.4f} -> {final:.4f}", flush=True)
    order = sorted(range(24), key=lambda k: finals[k])
    gap = finals[order[1]] - finals[order[0]]
    print(f"winner {order[0]} ({finals[order[0]]:.4f}), runner-up {order[1]} (gap {gap:.3e}), identity {finals[0]:.4f}")
    assert order[0] == ps.TRUE_INDEX, "the fp64 winner is not the true rotation: change the scene"
    assert gap >= 1e-3 * finals[order[0]], "winner and runner-up are closer than 1e-3 of the winning total: change the scene"
    out = {"max_iter": ps.MAX_ITER, "vertices": obj.shape[0], "faces": faces.shape[0], "contact_obj": int((p_obj > 0).sum()),
           "contact_hum": int((p_hum > 0).sum()), "target_pixels": int(target.sum()), "final_total": finals, "first_total": first,
           "last_history": last, "winner": order[0], "runner_up": order[1]}
    with open(os.path.join(HERE, ps.GOLDEN), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
