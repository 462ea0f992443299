"""The reference's validate() loop (evaluate.py:37-260) with every metric and every meter kept on the device.

Per sample: inference ('generate': input_ids trimmed at the first labelled position + model.evaluate; 'forward':
model(**input_dict)), the 2-D segmentation counts, the task's 3-D metrics, the meter updates - all as launches on device
tensors, nothing is read back.  At the end: one cross-rank SUM of the meter buffer (dist.reduce_meters) and ONE
device-to-host copy that carries the meters, the per-sample metric lists and the saved predictions.

Kept from the reference: the hcontact fallback (pred_contact_3d None -> zeros, :111-113); a sample without valid affordance
statistics adds nothing to ANY meter (the `continue` of :153-155 also skips the segmentation meters below it) but is still
saved; get_h_geo_metric is called with (gt, pred) in its (pred, gt) parameters (:128); the segmentation ignore label is the
reference's IGNORE_LABEL = -1 (utils/utils.py:19), so a label map held as uint8 has no ignored pixel, as after its .int().  Logging, image dumps and pickling are
out of scope.
"""
from __future__ import annotations

import torch

from . import dist as _dist
from .constants import IGNORE_LABEL

TASKS = ("hcontact", "oafford", "ocontact")
_TASK_METERS = {
    "hcontact": ("f1", "precision", "recall", "geo"),
    "oafford": ("sim", "mae", "auc", "iou"),
    "ocontact": ("f1", "precision", "recall"),
}
_SEG_METERS = (("intersection", 2), ("union", 2), ("acc_iou", 2))


class Meters:
    """The reference's AverageMeter(Summary.SUM) set (utils/utils.py:147-198) as ONE device-resident fp64 [k,2] buffer of
    (sum, count) rows: update(name, v) adds v and 1, avg = sum / count.  A vector-valued meter (intersection, union,
    acc_iou) owns one row per component.  Updates are a few small torch ops on device tensors and never synchronise;
    ``gate`` (a 0 / 1 device scalar) makes an update a no-op without a branch on the host."""

    def __init__(self, spec, device):
        self.spec = [(name, int(width)) for name, width in spec]
        self.rows, k = {}, 0
        for name, width in self.spec:
            self.rows[name] = slice(k, k + width)
            k += width
        self.buf = torch.zeros(k, 2, dtype=torch.float64, device=device)

    def update(self, name, value, gate=None):
        row = self.buf[self.rows[name]]
        v = torch.as_tensor(value, device=self.buf.device).to(torch.float64).reshape(-1)
        if gate is None:
            row[:, 0] += v
            row[:, 1] += 1.0
        else:
            g = gate.to(torch.float64)
            row[:, 0] += torch.where(g > 0, v, torch.zeros_like(v))  # (a gated-off value may be NaN: it must not reach the sum)
            row[:, 1] += g

    def reduce(self, group=None):
        """AverageMeter.all_reduce: SUM of sums and counts over the ranks, one collective for the whole set."""
        flat = self.buf.view(-1)
        _dist.reduce_meters(flat, group=group)
        return self

    @staticmethod
    def read(buf, rows, name):
        """(sum, count, avg) of a meter from a host copy of the buffer."""
        r = buf[rows[name]]
        return r[:, 0], r[:, 1], r[:, 0] / r[:, 1]


def task_of(ds_name, model):
    """Which 3-D metric set the reference switches on for this dataset name (evaluate.py:52-73)."""
    hw, ow = float(getattr(model, "hC_loss_weight", 0.0)), float(getattr(model, "oC_loss_weight", 0.0))
    if "hcontact" in ds_name and hw > 0:
        return "hcontact"
    if "oafford" in ds_name and ow > 0:
        return "oafford"
    if "ocontact" in ds_name and ow > 0:
        return "ocontact"
    return None


def _answer_start(labels_row):
    """First labelled position of the sequence (evaluate.py:88-91), None when nothing is labelled."""
    pos = (labels_row != -100).nonzero(as_tuple=False)
    return int(pos[0]) if pos.numel() > 0 else None


def _seg_inputs(output_dict):
    """get_segmentation_metrics' operands: pred_masks[0] f32 [V,H,W] and gt_masks[0] as [V,H,W] of a dtype the kernel reads."""
    assert len(output_dict["pred_masks"]) == 1  # eval_utils.py:46
    pred = output_dict["pred_masks"][0]
    gt = output_dict["gt_masks"][0]
    if pred.dim() == 4:
        pred = pred[:, 0]
    if gt.dim() == 4:
        gt = gt[:, 0]
    gt = gt.to(pred.device)
    if gt.dtype not in (torch.uint8, torch.int32, torch.float32):
        gt = gt.to(torch.int32)
    return pred.float().contiguous(), gt.contiguous()


def seg_metrics(counts):
    """i32 [V,3,2] counts -> (intersection, union, acc_iou), each fp64 [2]: the per-view means get_segmentation_metrics returns
    (eval_utils.py:48-61), with its `union == 0 -> +1` rule for a class absent from both masks."""
    c = counts.to(torch.float64)
    inter = c[:, 0]
    union = c[:, 1] + c[:, 2] - c[:, 0]
    acc = inter / (union + 1e-5) + (union == 0).to(torch.float64)
    return inter.mean(0), union.mean(0), acc.mean(0)


def afford_batch(per_sample, valid):
    """[B,4] / [B] of ops.affordance_metrics -> (sim, mae, auc, iou, valid_samples) as get_o_affordance_metrics returns them for
    the batch (eval_utils.py:199-213): sim / mae means over B, auc / iou means over the valid samples (0 if there is none)."""
    p = per_sample.to(torch.float64)
    ok = valid > 0
    nv = ok.sum()
    den = nv.clamp(min=1).to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    auc = torch.where(ok, p[:, 2], zero).sum() / den
    iou = torch.where(ok, p[:, 3], zero).sum() / den
    return p[:, 0].mean(), p[:, 1].mean(), auc, iou, nv


def _to_device(input_dict, device):
    out = dict(input_dict)
    for k, v in input_dict.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(device)
        elif isinstance(v, (list, tuple)) and v and all(isinstance(t, torch.Tensor) for t in v):
            out[k] = [t.to(device) for t in v]
    for k in ("images", "images_clip"):
        if isinstance(out.get(k), torch.Tensor) and out[k].is_floating_point():
            out[k] = out[k].to(torch.bfloat16)  # the model's input dtype (evaluate.py:81-82 casts to args.precision)
    return out


def validate(model, samples, ds_name, inference_type="generate", dist_matrix=None, group=None, evaluate_kwargs=None, metrics=None,
             exact_sets=None):
    """Score ``samples`` (an iterable of collate_fn-shaped dicts, batch 1 as in the reference's val loader) for dataset
    ``ds_name``.  -> {"giou", "ciou", "avg_*" of the task, "saved_results", "count", "task", "meters": the reduced sums and counts}.

    dist_matrix: the f32 [Nv,Nv] geodesic matrix on the device, required for 'hcontact' (the reference loads it from a data
    file at import time).  evaluate_kwargs: extra arguments of model.evaluate in 'generate' mode (e.g. forced_new_tokens for
    weights that never emit [SEG]).  metrics: the provider of seg_iou_counts / affordance_metrics / contact_prf /
    o_contact_prf / h_geo_metric_per_sample; the HIP kernels of ``ops`` unless another is given.
    exact_sets ('generate' mode; None: off, nothing changes): forwarded to model.evaluate, which certifies each sample's
    vertex-id sets or re-runs the sample in the parity mode; saved_results gains "escalated" (one bool per sample) and the
    result "rerun_rate" (their mean).  No metric is added or changed."""
    if inference_type not in ("generate", "forward"):
        raise ValueError(f"inference_type must be 'generate' or 'forward', got {inference_type!r}")
    if exact_sets is not None and inference_type != "generate":
        raise ValueError("exact_sets is an option of model.evaluate: inference_type must be 'generate'")
    if metrics is None:
        from . import ops as metrics
    task = task_of(ds_name, model)
    if task == "hcontact" and dist_matrix is None:
        raise ValueError("hcontact validation needs dist_matrix (the geodesic distance matrix of the body mesh)")
    device = torch.device(getattr(model, "device", "cpu"))
    meters = Meters(_SEG_METERS + tuple((m, 1) for m in _TASK_METERS.get(task, ())), device)
    names = _TASK_METERS.get(task, ())
    saved = {"imgnames": [], "pred": [], "gt": []}
    if task == "hcontact":
        saved["objnames"] = []
    escalated = []
    per_sample = []  # one fp64 [len(names)] device tensor per sample: what the reference appends to its lists
    one = torch.ones((), dtype=torch.float64, device=device)

    for raw in samples:
        input_dict = _to_device(raw, device)
        gt3d = torch.vstack([t.float() for t in input_dict["gt_contact_3d_list"]]).contiguous()
        input_dict["gt_contact_3d"] = gt3d
        if inference_type == "generate":
            ids = input_dict["input_ids"]
            start = _answer_start(raw["labels"][0]) if "labels" in raw and raw["labels"] is not None else None
            if start is not None:
                ids = ids[:, :start]
            mask_path = input_dict["mask_paths_list"][0] if "mask_paths_list" in input_dict else None
            kw = dict(max_new_tokens=512)
            kw.update(evaluate_kwargs or {})
            if exact_sets is not None:
                kw["exact_sets"] = exact_sets
            ev = model.evaluate(images_clip=input_dict["images_clip"], images=input_dict["images"], input_ids=ids,
                                cam_params=input_dict["cam_params"], resize_list=input_dict["resize_list"],
                                original_size_list=input_dict["resize_list"], lift2d_dict_path=mask_path,
                                contact_type=input_dict["ds_name_list"][0], **kw)
            output_dict = {"pred_masks": ev["pred_masks"], "gt_masks": input_dict["masks_list"]}
            if exact_sets is not None:
                escalated.append(bool(ev["exact_sets"]["escalated"]))
            pred3d = ev.get("pred_contact_3d", None)
            if task == "hcontact":
                output_dict["pred_human_3d_contact"] = torch.zeros_like(gt3d) if pred3d is None else pred3d
            elif task == "ocontact":
                output_dict["pred_object_3d_contact"] = pred3d
            elif task == "oafford":
                output_dict["pred_object_3d_afford"] = pred3d
        else:
            input_dict.setdefault("inference", True)  # (collate_fn sets it for the val loader)
            output_dict = model(**input_dict)

        pm, gm = _seg_inputs(output_dict)
        inter, union, acc = seg_metrics(metrics.seg_iou_counts(pm, gm, ignore_label=IGNORE_LABEL))
        gate = one
        if task is not None:
            key = {"hcontact": "pred_human_3d_contact", "oafford": "pred_object_3d_afford",
                   "ocontact": "pred_object_3d_contact"}[task]
            pred3d = output_dict.get(key)
            if pred3d is None:
                raise ValueError(f"{task}: the model returned no 3-D prediction for this sample (no mask was decoded)")
            pred3d = pred3d.float().contiguous()
            if task == "hcontact":
                prf = metrics.contact_prf(gt3d, pred3d).to(torch.float64).mean(0)
                geo = metrics.h_geo_metric_per_sample(gt3d, pred3d, dist_matrix).to(torch.float64).mean(0)[0]  # (sic: evaluate.py:128)
                vals = torch.stack([prf[0], prf[1], prf[2], geo])
                saved["objnames"].append(raw.get("sampled_classes_list"))
                saved["imgnames"].append(raw.get("image_paths"))
            elif task == "oafford":
                sim, mae, auc, iou, nv = afford_batch(*metrics.affordance_metrics(gt3d, pred3d))
                vals = torch.stack([sim, mae, auc, iou])
                gate = (nv > 0).to(torch.float64)
                paths = raw.get("image_paths")
                saved["imgnames"].append(paths[0].rsplit("/", 1)[-1] if paths else None)
            else:
                vals = metrics.o_contact_prf(gt3d, pred3d).to(torch.float64).mean(0)
                saved["imgnames"].append(raw.get("image_paths"))
            for j, name in enumerate(names):
                meters.update(name, vals[j], gate)
            per_sample.append(vals)
            saved["pred"].append(pred3d)
            saved["gt"].append(gt3d)
        meters.update("intersection", inter, gate)
        meters.update("union", union, gate)
        meters.update("acc_iou", acc, gate)

    meters.reduce(group)
    # ONE device-to-host copy: meters | per-sample metrics | saved predictions | saved ground truth (fp32 values are exact in fp64)
    parts = [meters.buf.reshape(-1)] + [v.reshape(-1) for v in per_sample]
    rows_pred = [int(t.shape[0]) for t in saved["pred"]]
    width = int(saved["pred"][0].shape[1]) if saved["pred"] else 0
    if any(int(t.shape[1]) != width for t in saved["pred"] + saved["gt"]):
        raise ValueError("saved predictions of one dataset must have one width (np.vstack in the reference)")
    parts += [t.to(torch.float64).reshape(-1) for t in saved["pred"]] + [t.to(torch.float64).reshape(-1) for t in saved["gt"]]
    host = torch.cat(parts).cpu()

    k = meters.buf.numel()
    buf = host[:k].view(-1, 2)
    inter_sum = Meters.read(buf, meters.rows, "intersection")[0]
    union_sum = Meters.read(buf, meters.rows, "union")[0]
    acc_sum, acc_cnt, acc_avg = Meters.read(buf, meters.rows, "acc_iou")
    result = {"ciou": float(inter_sum[1] / (union_sum[1] + 1e-10)), "giou": float(acc_avg[1]), "count": float(acc_cnt[1]),
              "task": task}
    for name in names:
        result["avg_" + name] = float(Meters.read(buf, meters.rows, name)[2][0])
    result["meters"] = {name: {"sum": [float(x) for x in Meters.read(buf, meters.rows, name)[0]],
                               "count": float(Meters.read(buf, meters.rows, name)[1][0])} for name, _ in meters.spec}
    n = len(per_sample)
    ps = host[k: k + n * len(names)].view(n, len(names)) if n else host[:0].view(0, max(len(names), 1))
    for j, name in enumerate(names):
        if task != "oafford" and name in ("precision", "recall"):
            continue  # the reference saves f1 (and geo) only for the contact tasks
        saved[name] = [float(x) for x in ps[:, j]] if n else []
    off = k + n * len(names)
    total = sum(rows_pred)
    saved["pred"] = host[off: off + total * width].view(total, width).to(torch.float32).numpy() if total else []
    saved["gt"] = host[off + total * width: off + 2 * total * width].view(total, width).to(torch.float32).numpy() if total else []
    for name in names:
        saved["avg_" + name] = result["avg_" + name]
    if exact_sets is not None:
        saved["escalated"] = escalated
        result["rerun_rate"] = sum(escalated) / len(escalated) if escalated else 0.0
    result["saved_results"] = saved
    return result
