"""Time the promptable-SAM path: ``ivlm_mask_dot_multi`` next to four ``ops.mask_dot`` calls, the two prompt kernels, and one
``SamPredictor.predict``.

    python tools/bench_sam_prompt.py [--rounds 7] [--iters 50] [--other-lib PATH] [--out FILE.json]

Shapes are the real ones: a 64 x 64 grid, C = 256, the upscaled embedding [1, 64, 64, 2, 2, 2, 2, 32] fp32 (8.4 MB), four mask tokens,
one positive point (N = 2 with the pad point) on synthetic weights.  ``--other-lib``: another build of libivlm_hip.so (the parent
commit's, say), whose ``ivlm_mask_dot`` is called four times in the same rounds, alternating with this build's, so that the two see the
same card at the same time.  tools/bench_silhouette.py's method: device events around `iters` calls after a warm-up, the median of
`rounds` rounds, minimum and maximum stated.  Prints one JSON line per case.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_silhouette import timed  # noqa: E402
from interactvlm_amd import ops, sam  # noqa: E402
from interactvlm_amd import weights as Wt  # noqa: E402
from interactvlm_amd.sam_predictor import SamPredictor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sam_prompt needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    g, C, M = 64, 32, 4
    up = torch.randn(g * g * 16, C, generator=gen).to(dev)
    hyper = torch.randn(1, M, C, generator=gen).to(dev)
    rows = [hyper[:, m].contiguous() for m in range(M)]
    steps = {
        "mask_dot_multi_M4": lambda: ops.mask_dot_multi(up, hyper, 1, g, g),
        "mask_dot_x4": lambda: [ops.mask_dot(up, r, 1, g, g) for r in rows],
    }
    same = all(torch.equal(ops.mask_dot_multi(up, hyper, 1, g, g)[:, m], ops.mask_dot(up, rows[m], 1, g, g)) for m in range(M))
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        other.ivlm_mask_dot.restype = ctypes.c_int
        other.ivlm_mask_dot.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        low = torch.empty(M, 4 * g, 4 * g, device=dev)

        def other_x4():
            for m in range(M):
                rc = other.ivlm_mask_dot(up.data_ptr(), rows[m].data_ptr(), 0, low[m].data_ptr(), 1, g, g, C, ops._stream())
                assert rc == 0, rc

        other_x4()
        same = same and torch.equal(low, ops.mask_dot_multi(up, hyper, 1, g, g)[0])
        steps["mask_dot_x4_other_lib"] = other_x4
    dec = sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), dev)
    emb = torch.randn(g * g, 256, generator=gen).to(torch.bfloat16).to(dev)
    pred = SamPredictor(None, dec)
    pred.set_embedding(emb, (1024, 683), (750, 500))
    point, label = torch.tensor([[250.0, 375.0]], device=dev), torch.tensor([1], device=dev)
    sparse, _ = dec.encode_prompts(point[None], label[None])
    mask_in = torch.randn(1, 1, 4 * g, 4 * g, generator=gen).to(dev)
    text = torch.randn(1, 1, 256, generator=gen).to(dev)
    steps.update({
        "predict_N2": lambda: pred.predict(point_coords=point, point_labels=label),
        "predict_masks_N2": lambda: dec.predict_masks(emb, sparse),
        "predict_masks_eager_N2": lambda: dec._predict_all(emb, sparse, None),
        "encode_prompts_point": lambda: dec.encode_prompts(point[None], label[None]),
        "encode_prompts_mask": lambda: dec.encode_prompts(mask_input=mask_in),
        "text_path_eager_T1": lambda: dec._forward(emb[None], text),
        "text_path_graph_T1": lambda: dec(emb[None], text),
    })
    info = dict(case="shapes", grid=g, up_bytes=up.numel() * 4, tokens=M, bits_equal_mask_dot=bool(same), rounds=a.rounds, iters=a.iters)
    print(json.dumps(info), flush=True)
    results = [info]
    for step in steps.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(a.rounds):  # the cases alternate inside every round
        for n, step in steps.items():
            times[n].append(timed(step, a.iters))
    for n, t in times.items():
        row = dict(case=n, us_median=round(statistics.median(t), 1), us_min=round(min(t), 1), us_max=round(max(t), 1))
        print(json.dumps(row), flush=True)
        results.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
