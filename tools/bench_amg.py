"""Time the filter stage of the automatic mask generator: ``SamAutomaticMaskGenerator.select`` (census on the fly, one host read)
next to the materialising route the reference takes, and one whole ``generate_on_set_image``.

    python tools/bench_amg.py [--rounds 5] [--iters 3] [--side 32] [--out profiles/amg_bench.json]

Sizes a user runs: a stored 64 x 64 embedding (synthetic weights), side^2 = 1024 point prompts x 3 masks = 3072 candidates, a
1500 x 1000 photo.  The candidates are computed once by the decoder; the thresholds are the medians of their predicted IoUs and
stabilities (synthetic weights predict no meaningful quality: about half of the candidates pass each filter, as a count it is stated
in the output).  The materialising route is written here from calls the library already had: per batch of 64 points
``ops.postprocess_masks`` of all 192 candidates, the IoU filter, the two threshold counts, the stability filter, the threshold and the
boxes with torch, in the reference's order; then the same sort and ``ops.box_nms``, and the survivors' masks.  tools/bench_silhouette.py's
method: device events around `iters` calls after a warm-up, the cases alternating inside every round, the median of `rounds` rounds
with minimum and maximum.  The bytes of full-resolution logits ``select`` does not write are computed from the shapes, not measured.
Needs a GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_silhouette import timed  # noqa: E402
from interactvlm_amd import ops, sam  # noqa: E402
from interactvlm_amd import weights as Wt  # noqa: E402
from interactvlm_amd.sam_amg import SamAutomaticMaskGenerator  # noqa: E402
from interactvlm_amd.sam_predictor import SamPredictor  # noqa: E402

PHOTO, BATCH = (1500, 1000), 64


def boxes_of(masks):
    """bool [n,H,W] -> int64 [n,4] XYXY inclusive, zeros for an empty mask"""
    n, H, W = masks.shape
    cols, rows = masks.any(1), masks.any(2)
    xs, ys = torch.arange(W, device=masks.device), torch.arange(H, device=masks.device)
    box = torch.stack([torch.where(cols, xs, W).min(1).values, torch.where(rows, ys, H).min(1).values,
                       torch.where(cols, xs, -1).max(1).values, torch.where(rows, ys, -1).max(1).values], 1)
    return box * cols.any(1, keepdim=True)


def materialising(gen, low, iou):
    """the reference's route on the same candidates -> (kept candidate indices in NMS order, their masks)"""
    pred = gen.predictor
    t, off = gen.mask_threshold, gen.stability_score_offset
    P, M = iou.shape
    index, boxes, scores = [], [], []
    for s in range(0, P, BATCH):
        e = min(P, s + BATCH)
        logits = ops.postprocess_masks(low[s:e], pred.input_size, pred.original_size, pred.img_size).flatten(0, 1)
        score = iou[s:e].flatten()
        idx = torch.arange(s * M, e * M, device=low.device)
        if gen.pred_iou_thresh > 0.0:
            keep = score > gen.pred_iou_thresh
            logits, score, idx = logits[keep], score[keep], idx[keep]
        above = (logits > t + off).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
        below = (logits > t - off).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
        if gen.stability_score_thresh > 0.0:
            keep = above / below >= gen.stability_score_thresh
            logits, score, idx = logits[keep], score[keep], idx[keep]
        boxes.append(boxes_of(logits > t))
        index.append(idx)
        scores.append(score)
    index, boxes, scores = torch.cat(index), torch.cat(boxes), torch.cat(scores)
    order = torch.sort(scores, descending=True, stable=True).indices
    keep = ops.box_nms(boxes[order].float().contiguous(), gen.box_nms_thresh)
    kept = index[order[keep.bool()]]
    masks = ops.postprocess_masks(low.flatten(0, 1)[kept], pred.input_size, pred.original_size, pred.img_size) > t
    return kept, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--side", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_amg needs a GPU (no CPU path)")
    dev = torch.device("cuda:0")
    g = 64
    dec = sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), dev)
    emb = torch.randn(g * g, 256, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(dev)
    pred = SamPredictor(None, dec)
    H, W = PHOTO
    pred.set_embedding(emb, (1024, 683), PHOTO)
    gen = SamAutomaticMaskGenerator(pred, points_per_side=a.side, points_per_batch=BATCH, pred_iou_thresh=0.0, stability_score_thresh=0.0)

    # the candidates, once: the decoder phase of generate_on_set_image
    points = torch.from_numpy(gen.point_grid * np.array([[W, H]], dtype=np.float64)).to(dev)
    P = points.shape[0]
    low, iou = torch.empty(P, 3, 4 * g, 4 * g, device=dev), torch.empty(P, 3, device=dev)
    for s in range(0, P, BATCH):
        sparse, dense = dec.encode_prompts(pred.scale_coords(points[s: s + BATCH].unsqueeze(1)),
                                           torch.ones(min(BATCH, P - s), 1, dtype=torch.int32, device=dev))
        lb, ib = dec.predict_masks(emb, sparse, dense)
        low[s: s + BATCH].copy_(lb)
        iou[s: s + BATCH].copy_(ib)
    # thresholds: the medians, measured with the census itself (an offset on both sides of which the candidates have pixels)
    off = float(low.abs().median())
    cen = ops.mask_census(low.flatten(0, 1), pred.input_size, PHOTO, pred.img_size, (off, 0.0, -off))
    stab = cen[:, 0].float() / cen[:, 2].float()
    gen.stability_score_offset = off
    gen.pred_iou_thresh = max(float(iou.median()), 0.0)
    active = iou.flatten() > gen.pred_iou_thresh if gen.pred_iou_thresh > 0 else torch.ones(P * 3, dtype=torch.bool, device=dev)
    finite = active & torch.isfinite(stab)
    gen.stability_score_thresh = max(float(stab[finite].median()), 0.0) if bool(finite.any()) else 0.0
    valid = active & (stab >= gen.stability_score_thresh) if gen.stability_score_thresh > 0 else active

    found = gen.select(low, iou, points)
    kept, masks = materialising(gen, low, iou)
    same = found.index.tolist() == kept.tolist() and torch.equal(found.masks, masks)
    n = P * 3
    info = dict(case="shapes", photo=list(PHOTO), points=P, candidates=n, pass_iou=int(active.sum()), pass_stability=int(valid.sum()),
                kept=len(found), same_result_as_materialising=bool(same), thresholds=dict(
                    pred_iou=gen.pred_iou_thresh, stability=gen.stability_score_thresh, offset=off, box_nms=gen.box_nms_thresh),
                full_resolution_logit_bytes_not_written_computed=(n - len(found)) * H * W * 4,
                materialising_logit_bytes_written_computed=(n + len(found)) * H * W * 4, rounds=a.rounds, iters=a.iters)
    print(json.dumps(info), flush=True)
    steps = {
        "select": lambda: gen.select(low, iou, points),
        "materialising_route": lambda: materialising(gen, low, iou),
        "mask_census_alone": lambda: ops.mask_census(low.flatten(0, 1), pred.input_size, PHOTO, pred.img_size, (off, 0.0, -off),
                                                     active.to(torch.int32)),
        "generate_on_set_image": lambda: gen.generate_on_set_image(),
    }
    for step in steps.values():
        step()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):  # the cases alternate inside every round
        for k, step in steps.items():
            times[k].append(timed(step, a.iters))
    results = [info]
    for k, t in times.items():
        row = dict(case=k, ms_median=round(statistics.median(t) / 1e3, 3), ms_min=round(min(t) / 1e3, 3), ms_max=round(max(t) / 1e3, 3))
        print(json.dumps(row), flush=True)
        results.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
