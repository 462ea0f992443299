#!/usr/bin/env python3
"""Generate tests/golden/amg_select.npz by RUNNING THE REFERENCE's SamAutomaticMaskGenerator.generate on the CPU (build container
only: it needs the reference through _ref_shims; the GPU box never runs this):

    python tests/golden/make_amg_golden.py

The generator's model is replaced by seeded logits: its ``SamPredictor`` name by a stub whose ``predict_torch`` returns the
reference's own ``Sam.postprocess_masks`` of tests/_amg_ref.py's ``candidates()`` and their seeded IoUs, batch by batch; its
``batched_nms`` (torchvision is not installed) by the restated NMS with the tie rule, the way make_golden_icp.py replaces
``knn_points``.  Everything behind them - IoU filter, stability, threshold, boxes, run lengths, records - is the reference's code.

Stored (data only; the logits are regenerated from the seed): per record its candidate index, bbox (XYWH), area, predicted_iou,
stability_score, point_coords and run lengths (concatenated, with offsets); the numbers of candidates behind every filter.

The script asserts what makes the kept set well defined; if another seed breaks a condition, change the seed or the blob parameters,
never the condition."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import _amg_ref as A  # noqa: E402
import _ref_shims  # noqa: E402
import _resample_ref as RR  # noqa: E402


def main():
    import torch

    _ref_shims.install()
    from model.segment_anything import automatic_mask_generator as G
    from model.segment_anything.modeling.sam import Sam
    from interactvlm_amd import preprocess

    assert preprocess.get_preprocess_shape(A.PHOTO[0], A.PHOTO[1], A.IMG) == A.INPUT
    low, iou = A.candidates()
    margins = []
    G.batched_nms = lambda boxes, scores, categories, iou_threshold: torch.from_numpy(
        A.nms(boxes.numpy(), scores.numpy(), iou_threshold, margins=margins))

    class _Enc:  # postprocess_masks only reads image_encoder.img_size
        img_size = A.IMG

    post = lambda m: Sam.postprocess_masks(type("S", (), {"image_encoder": _Enc})(), m, A.INPUT, A.PHOTO)

    class _Transform:
        @staticmethod
        def apply_coords(coords, size):
            nh, nw = preprocess.get_preprocess_shape(size[0], size[1], A.IMG)
            out = coords.astype(float).copy()
            out[..., 0] *= nw / size[1]
            out[..., 1] *= nh / size[0]
            return out

    class _Predictor:
        def __init__(self, model):
            self.model = type("M", (), {"mask_threshold": A.MASK_THRESH})()
            self.device, self.transform, self.at = torch.device("cpu"), _Transform, 0

        def set_image(self, image):
            self.at = 0

        def reset_image(self):
            pass

        def predict_torch(self, points, labels, multimask_output=True, return_logits=True):
            rows = slice(self.at, self.at + points.shape[0])
            self.at += points.shape[0]
            return post(torch.from_numpy(low[rows].copy())), torch.from_numpy(iou[rows].copy()), None

    G.SamPredictor = _Predictor
    gen = G.SamAutomaticMaskGenerator(None, points_per_side=A.SIDE, points_per_batch=A.BATCH, pred_iou_thresh=A.IOU_THRESH,
                                      stability_score_thresh=A.STABILITY_THRESH, stability_score_offset=A.OFFSET,
                                      box_nms_thresh=A.NMS_THRESH, output_mode="uncompressed_rle")
    recs = gen.generate(np.zeros(A.PHOTO + (3,), np.uint8))

    # ---- the conditions that make the kept set well defined -----------------------------------------------------------------------
    flat_low, flat_iou = low.reshape(-1, A.LOW, A.LOW), iou.reshape(-1)
    n = len(flat_iou)
    assert len(set(flat_iou.tolist())) == n  # a record's candidate is found by its predicted IoU
    index = np.array([int(np.flatnonzero(flat_iou == np.float32(r["predicted_iou"]))[0]) for r in recs], dtype=np.int64)
    few, many, in_band = A.golden_band()
    active = flat_iou > np.float32(A.IOU_THRESH)
    with np.errstate(divide="ignore", invalid="ignore"):
        ends = [many[:, 0] / few[:, 2], few[:, 0] / many[:, 2]]  # the largest and the smallest stability inside the band
        sides = [np.where(np.isfinite(s), s, -1.0) >= A.STABILITY_THRESH for s in ends]
    stable = sides[0] & sides[1]
    n_iou, n_stab, n_kept = int(active.sum()), int((active & stable).sum()), len(recs)
    print(f"  {n} candidates -> {n_iou} pass the IoU filter -> {n_stab} pass stability -> {n_kept} after NMS")
    assert n > n_iou > n_stab > n_kept >= 3, "every filter removes at least one candidate and at least 3 survive"
    m_iou = float(np.abs(flat_iou.astype(np.float64) - A.IOU_THRESH).min())
    assert m_iou >= A.MARGIN, m_iou
    assert bool((sides[0][active] == sides[1][active]).all()), "a stability changes side of the threshold inside its band"
    m_stab = float(min(np.abs(s[active & np.isfinite(s)] - A.STABILITY_THRESH).min() for s in ends))
    survivors = active & stable
    assert bool((few[survivors, 3:7] == many[survivors, 3:7]).all()), "a survivor's box differs between the ends of its band"
    assert margins and min(margins) >= A.MARGIN, min(margins)
    assert in_band.sum() <= 0.2 * n, int(in_band.sum())
    print(f"  margins: IoU {m_iou:.4f}, stability {m_stab:.4f}, NMS {min(margins):.4f}; {int(in_band.sum())} of {n} candidates have a "
          f"pixel inside the band (bound up to {float(RR.bound(flat_low, A.IMG, A.INPUT, A.PHOTO).max()):.2e})")

    counts = [np.asarray(r["segmentation"]["counts"], dtype=np.int32) for r in recs]
    assert all(r["segmentation"]["size"] == list(A.PHOTO) and r["crop_box"] == [0, 0, A.PHOTO[1], A.PHOTO[0]] for r in recs)
    path = os.path.join(HERE, "amg_select.npz")
    np.savez_compressed(
        path, seed=np.int64(A.SEED), index=index, bbox=np.array([r["bbox"] for r in recs], dtype=np.int64),
        area=np.array([r["area"] for r in recs], dtype=np.int64),
        predicted_iou=np.array([r["predicted_iou"] for r in recs], dtype=np.float32),
        stability_score=np.array([r["stability_score"] for r in recs], dtype=np.float32),
        point_coords=np.array([r["point_coords"][0] for r in recs], dtype=np.float64),
        rle_counts=np.concatenate(counts), rle_offsets=np.cumsum([0] + [len(c) for c in counts]).astype(np.int64),
        n_filters=np.array([n, n_iou, n_stab, n_kept], dtype=np.int64))
    print(f"  wrote amg_select.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
