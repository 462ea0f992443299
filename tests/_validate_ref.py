"""Torch-CPU restatement of the validate() metrics and meter rules (TEST INFRASTRUCTURE ONLY), pinned to the reference's own
functions by tests/golden/validate_metrics.npz (tests/golden/make_golden_validate.py) in tests/test_validate_cpu.py:

    seg_iou_counts        intersectionAndUnionGPU with K = 2 per view      (utils/eval_utils.py:27-39)
    seg_metrics           get_segmentation_metrics                          (:41-61)
    affordance_metrics    get_o_affordance_metrics, per sample              (:153-213)
    afford_batch          its batch means and valid_samples
    run_meters            AverageMeter(Summary.SUM) under the update order of evaluate.py:122-176

It offers the function names validate() asks of its metric provider, so validate(metrics=<this module>) runs on the CPU.
"""
import numpy as np
import torch

from oracle import metrics as OM


def seg_iou_counts(pred, gt, ignore_label=-1):
    """pred f32 [V,H,W], gt [V,H,W] any dtype -> i32 [V,3,2] = (intersection, output area, target area) of classes 0 / 1."""
    out = torch.zeros(pred.shape[0], 3, 2, dtype=torch.int32)
    for v in range(pred.shape[0]):
        o = (pred[v] > 0).int().reshape(-1)
        t = gt[v].int().reshape(-1)
        keep = t != ignore_label
        for c in (0, 1):
            out[v, 0, c] = int((keep & (o == c) & (t == c)).sum())
            out[v, 1, c] = int((keep & (o == c)).sum())
            out[v, 2, c] = int((keep & (t == c)).sum())
    return out


def seg_metrics(counts):
    c = counts.to(torch.float64)
    inter = c[:, 0]
    union = c[:, 1] + c[:, 2] - c[:, 0]
    acc = inter / (union + 1e-5) + (union == 0).to(torch.float64)
    return inter.mean(0), union.mean(0), acc.mean(0)


THRESHOLDS = torch.from_numpy(np.linspace(0, 1, 20).astype(np.float32))


def affordance_metrics(gt, pred, thresholds=None):
    """gt, pred f32 [B,n] -> (f32 [B,4] = (sim, mae, auc, aiou), i32 [B] valid): fp64 sums, AUC as an exact pair count."""
    thr = THRESHOLDS if thresholds is None else thresholds.cpu()
    B = gt.shape[0]
    out = torch.zeros(B, 4, dtype=torch.float64)
    valid = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        g, p = gt[b].float(), pred[b].float()
        gd, pd = g.double(), p.double()
        out[b, 0] = torch.min(gd / (gd.sum() + 1e-12), pd / (pd.sum() + 1e-12)).sum()
        out[b, 1] = (gd - pd).abs().sum() / 2048
        lab = g >= 0.5
        P, N = int(lab.sum()), int((~lab).sum())
        if P == 0 or N == 0 or not bool(torch.isfinite(p).all()):
            out[b, 2] = out[b, 3] = float("nan")
            continue
        pos, neg = p[lab], p[~lab]
        gt_pairs = int((pos[:, None] > neg[None, :]).sum())
        eq_pairs = int((pos[:, None] == neg[None, :]).sum())
        out[b, 2] = (gt_pairs + 0.5 * eq_pairs) / (P * N)
        iou = 0.0
        for t in thr:
            pb = p >= t  # fp32 tensor against an fp32 scalar
            iou += float((pb & lab).sum()) / float((pb | lab).sum())
        out[b, 3] = iou / len(thr)
        valid[b] = 1
    return out.float(), valid


def afford_batch(per_sample, valid):
    p = per_sample.to(torch.float64)
    ok = valid > 0
    nv = int(ok.sum())
    den = max(1, nv)
    return (float(p[:, 0].mean()), float(p[:, 1].mean()), float(p[ok, 2].sum()) / den, float(p[ok, 3].sum()) / den, nv)


def contact_prf(gt, pred, threshold=0.5):
    return OM.h_contact_metrics(gt, pred, threshold)


o_contact_prf = contact_prf


def h_geo_metric_per_sample(pred, gt, dist):
    return OM.h_geo_metric(pred, gt, dist)[2]


def run_meters(samples):
    """samples: (values {name: scalar or vector}, valid) in order -> {name: (sum, count)} with the reference's rule that an
    invalid sample updates nothing."""
    acc = {}
    for values, valid in samples:
        if not valid:
            continue
        for name, v in values.items():
            v = np.atleast_1d(np.asarray(v, np.float64))
            s, c = acc.get(name, (np.zeros_like(v), 0))
            acc[name] = (s + v, c + 1)
    return acc
