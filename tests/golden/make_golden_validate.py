"""Golden vectors for the validate() metrics, produced by the REFERENCE's own functions on the CPU:

    python tests/golden/make_golden_validate.py        ->  tests/golden/validate_metrics.npz

utils/eval_utils.py get_segmentation_metrics / intersectionAndUnionGPU and get_o_affordance_metrics (sklearn's roc_auc_score
inside), and utils/utils.py AverageMeter driven by the update order of evaluate.py:122-176.  Only the arrays are committed;
the reference is needed to regenerate them, never to run the tests.  (torch.histc has no integer CPU kernel - the reference
only ever ran it on a GPU - so it is given float copies of the same integers; the counts are far below 2^24.)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402

N_POINTS = 2048
SIDE = 64
VIEWS = 4
IGNORE = -1


def _import_eval_utils():
    import torch

    _ref_shims.install()
    real_load = np.load

    def fake_load(path, *a, **k):  # eval_utils.py:15 loads the geodesic matrix at import time
        return np.zeros((4, 4), np.float32) if "geodesic" in str(path) else real_load(path, *a, **k)

    np.load = fake_load
    try:
        import utils.eval_utils as E
    finally:
        np.load = real_load
    real_histc = torch.histc

    def histc(x, *a, **k):
        return real_histc(x.float() if not x.is_floating_point() else x, *a, **k)

    torch.histc = histc
    return E


def seg_cases(rng):
    """[C,V,S,S] predictions and labels: ignore-label pixels, a view with empty gt AND empty prediction (union == 0 -> the +1
    rule), gt values other than 0 / 1 / 255, an all-positive probability map with an ignore band (the 'HM' views of oafford)."""
    C = 3
    pred = rng.normal(size=(C, VIEWS, SIDE, SIDE)).astype(np.float32)
    gt = (rng.random((C, VIEWS, SIDE, SIDE)) < 0.35).astype(np.int32)
    gt[0, 0, :9] = IGNORE                   # ignore band (the reference's IGNORE_LABEL is -1: utils/utils.py:19)
    gt[0, 1][rng.random((SIDE, SIDE)) < 0.1] = IGNORE
    pred[0, 2] = -np.abs(pred[0, 2])        # nothing predicted ...
    gt[0, 2] = 0                            # ... and nothing labelled: class 1 has union 0
    other = rng.random((SIDE, SIDE))
    gt[0, 3][other < 0.05] = 2              # values outside {0, 1, ignore}: in no target bin, still in the output area
    gt[0, 3][(other >= 0.05) & (other < 0.08)] = 7
    gt[0, 3][(other >= 0.08) & (other < 0.10)] = 255
    pred[0, 3, 5, :7] = 0.0                 # exactly 0 is class 0 (pred > 0)
    pred[1] = rng.random((VIEWS, SIDE, SIDE)).astype(np.float32) * 0.98 + 0.01   # probabilities: > 0 everywhere
    gt[1, :, :, :13] = IGNORE
    gt[1, 3] = IGNORE                       # a view that is ignored altogether: every count 0, both classes get +1
    gt[2, 1] = 1                            # a view that is all foreground
    gt[2, 2, 40:, :] = 255                  # (no negative label in this case: it can be held as uint8)
    return pred, gt


def afford_rows(rng):
    thr = np.linspace(0, 1, 20).astype(np.float32)
    R = 12
    gt = np.clip(rng.normal(0.35, 0.3, size=(R, N_POINTS)), 0, 1).astype(np.float32)
    pred = rng.random((R, N_POINTS)).astype(np.float32)
    pred[0] = np.clip(0.6 * gt[0] + 0.4 * pred[0], 0, 1)        # a prediction correlated with the ground truth
    gt[1] = (gt[1] >= 0.5).astype(np.float32)                    # binary ground truth
    gt[2] = 0.0                                                  # all zero: single class -> invalid
    gt[3] = 1.0                                                  # all one: invalid
    pred[4, 17] = np.nan                                         # NaN prediction: sklearn raises -> invalid
    pred[5] = np.floor(pred[5] * 8) / 8                          # heavy ties: 8 levels
    cyc = np.arange(N_POINTS) % 20
    pred[6] = thr[cyc]                                           # exactly on every fp32 threshold
    pred[7] = np.nextafter(thr[cyc], np.float32(-np.inf))        # one ulp below (below 0: the negative denormal)
    pred[8] = np.nextafter(thr[cyc], np.float32(np.inf))         # one ulp above
    pred[9, 5] = np.inf                                          # infinite prediction: invalid as well
    pred[10] = 0.25                                              # constant prediction: AUC 0.5 from ties alone
    gt[11, ::3] = 0.5                                            # ground truth exactly on its own 0.5 split
    gt[11, 1::3] = np.nextafter(np.float32(0.5), np.float32(0))
    return gt, pred


def main():
    import torch

    E = _import_eval_utils()
    from utils.utils import AverageMeter, Summary

    rng = np.random.default_rng(11)
    out = {}
    # ---- segmentation -------------------------------------------------------------------------------------------------
    spred, sgt = seg_cases(rng)
    C = spred.shape[0]
    inter, union, acc = (np.zeros((C, 2), np.float64) for _ in range(3))
    counts = np.zeros((C, VIEWS, 3, 2), np.int64)
    for c in range(C):
        od = {"pred_masks": [torch.from_numpy(spred[c])], "gt_masks": [torch.from_numpy(sgt[c])]}
        i, u, a = E.get_segmentation_metrics(od)
        inter[c], union[c], acc[c] = i, u, a
        for v in range(VIEWS):
            o = (torch.from_numpy(spred[c, v]) > 0).int()
            ai, au, at = E.intersectionAndUnionGPU(o.contiguous().clone(), torch.from_numpy(sgt[c, v]).int().contiguous(), 2)
            counts[c, v, 0], counts[c, v, 2] = ai.numpy(), at.numpy()
            counts[c, v, 1] = (au - at + ai).numpy()  # area_output
    out.update(seg_pred=spred, seg_gt=sgt, seg_inter=inter, seg_union=union, seg_acc=acc, seg_counts=counts.astype(np.int32))
    # the same function with its ignore constant set to 255 (the usual label of segmentation sets): the kernel takes the label as an argument
    counts255 = np.zeros_like(counts)
    E.IGNORE_LABEL = 255
    try:
        for c in range(C):
            for v in range(VIEWS):
                o = (torch.from_numpy(spred[c, v]) > 0).int()
                ai, au, at = E.intersectionAndUnionGPU(o.contiguous().clone(), torch.from_numpy(sgt[c, v]).int().contiguous(), 2)
                counts255[c, v, 0], counts255[c, v, 2] = ai.numpy(), at.numpy()
                counts255[c, v, 1] = (au - at + ai).numpy()
    finally:
        E.IGNORE_LABEL = IGNORE
    out.update(seg_counts_ign255=counts255.astype(np.int32))
    # ---- affordance ---------------------------------------------------------------------------------------------------
    agt, apred = afford_rows(rng)
    ref = np.zeros((agt.shape[0], 5), np.float64)
    for b in range(agt.shape[0]):
        ref[b] = E.get_o_affordance_metrics(torch.from_numpy(agt[b: b + 1]), torch.from_numpy(apred[b: b + 1]))
    out.update(aff_gt=agt, aff_pred=apred, aff_ref=ref, aff_thresholds=np.linspace(0, 1, 20).astype(np.float32))
    # ---- a three-sample oafford meter run, the middle sample invalid (evaluate.py:122-176) ------------------------------------
    seg_idx, aff_idx = [0, 1, 2], [0, 3, 5]
    names = ["intersection", "union", "acc_iou", "sim", "mae", "auc", "iou"]
    meters = {n: AverageMeter(n, ":6.3f", Summary.SUM) for n in names}
    for s, a in zip(seg_idx, aff_idx):
        od = {"pred_masks": [torch.from_numpy(spred[s])], "gt_masks": [torch.from_numpy(sgt[s])]}
        i, u, ac = E.get_segmentation_metrics(od)
        sim, mae, auc, iou, valid = E.get_o_affordance_metrics(torch.from_numpy(agt[a: a + 1]), torch.from_numpy(apred[a: a + 1]))
        if valid == 0:
            continue  # :153-155: the segmentation meters below are skipped too
        for n, v in (("sim", sim), ("mae", mae), ("auc", auc), ("iou", iou), ("intersection", i), ("union", u), ("acc_iou", ac)):
            meters[n].update(v)
    msum = np.concatenate([np.atleast_1d(np.asarray(meters[n].sum, np.float64)) for n in names])
    mcnt = np.concatenate([np.full(np.atleast_1d(np.asarray(meters[n].sum)).shape, meters[n].count, np.float64) for n in names])
    mavg = np.concatenate([np.atleast_1d(np.asarray(meters[n].avg, np.float64)) for n in names])
    iou_class = meters["intersection"].sum / (meters["union"].sum + 1e-10)
    out.update(meter_seg_idx=np.asarray(seg_idx), meter_aff_idx=np.asarray(aff_idx), meter_sum=msum, meter_count=mcnt,
               meter_avg=mavg, meter_ciou=np.float64(iou_class[1]), meter_giou=np.float64(meters["acc_iou"].avg[1]))
    path = os.path.join(HERE, "validate_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    print("aff_ref (sim, mae, auc, iou, valid):\n", ref)
    print("meter avg:", mavg, "giou", out["meter_giou"], "ciou", out["meter_ciou"])


if __name__ == "__main__":
    main()
