"""Segment everything: masks of one photo from a grid of point prompts, filtered by predicted IoU and stability and de-duplicated by
box NMS (segment_anything/automatic_mask_generator.py: SamAutomaticMaskGenerator, utils/amg.py), on the predictor of
``sam_predictor``.

    gen = SamAutomaticMaskGenerator.from_model(model)
    found = gen.generate(photo_u8)                        # AutoMasks: device tensors, best predicted IoU first
    human_mask = found.masks[found.match(silhouette)].float()   # FitScene(human_mask=...)
    records = found.records()                             # the reference's list of dicts

Host-side orchestration only.  The reference upsamples every candidate to the photo's size to count and box it; here the counts and
boxes come from ``ops.mask_census``, which evaluates the post-processed value at every pixel without storing it, the duplicates go
in ``ops.box_nms``, and only the survivors are upsampled.  ``select`` reads one number back (how many survived).  Every argument
error is raised before the library loads.  Not built: crops (``crop_n_layers``), small-region removal (``min_mask_region_area``)
and COCO run-length strings.
"""
from __future__ import annotations

import numpy as np
import torch

F32, I32 = torch.float32, torch.int32
OUTPUT_MODES = ("binary_mask", "uncompressed_rle")
# Prompts per decoder call.  The bits ``SamMaskDecoder.predict_masks`` gives a prompt depend on how many prompts share its call (the
# linears choose their kernel and their split of K by the row count: 4e-5 on the low-res logits between 5 and 16 per call), not on
# which ones.  The generator's result must not depend on points_per_batch, so every call has this many; 16 divides the default batch
# of 64 and the default grid of 1024, and one graph serves every call.
DECODER_PROMPTS = 16


def build_point_grid(n_per_side):
    """[n*n, 2] fp64 (x, y) in the unit square: n evenly spaced values per axis, half a step inside the border, x fastest"""
    n = int(n_per_side)
    if n < 1:
        raise ValueError(f"n_per_side: expected >= 1, got {n_per_side}")
    half = 1 / (2 * n)
    side = np.linspace(half, 1 - half, n)
    xs, ys = np.meshgrid(side, side)  # xs[i, j] = side[j], ys[i, j] = side[i]
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def _check_mode(output_mode):
    if output_mode == "coco_rle":
        raise ValueError("output_mode: 'coco_rle' needs pycocotools, which this build does without; use 'uncompressed_rle'")
    if output_mode not in OUTPUT_MODES:
        raise ValueError(f"output_mode: expected one of {OUTPUT_MODES}, got {output_mode!r}")
    return output_mode


def run_lengths(masks):
    """masks bool [K,H,W] -> K lists of run lengths over the column-major pixels, alternating unset / set and starting with the unset
    run (so a mask whose first pixel is set starts with 0): the uncompressed RLE of pycocotools.  Torch operations on the masks'
    device, one transfer of the change positions."""
    K, H, W = masks.shape
    if K == 0:
        return []
    flat = masks.permute(0, 2, 1).reshape(K, H * W)
    where = (flat[:, 1:] != flat[:, :-1]).nonzero()  # (mask, position of the last pixel of a run), sorted by mask, then position
    per_mask = torch.bincount(where[:, 0], minlength=K).cpu().tolist()
    ends = (where[:, 1] + 1).cpu()
    first = flat[:, 0].cpu().tolist()
    out, at = [], 0
    for k in range(K):
        edges = torch.cat([torch.zeros(1, dtype=ends.dtype), ends[at: at + per_mask[k]], torch.tensor([H * W], dtype=ends.dtype)])
        at += per_mask[k]
        out.append(([0] if first[k] else []) + (edges[1:] - edges[:-1]).tolist())
    return out


class AutoMasks:
    """The K masks ``select`` kept, as device tensors in NMS order (descending predicted IoU): masks bool [K,H,W], boxes int32 [K,4]
    XYXY (inclusive pixel indices), areas int32 [K], predicted_iou fp32 [K], stability_score fp32 [K], point_coords fp64 [K,2] (the
    prompt, in the photo's pixels), index int64 [K] (candidate = point * masks per point + token), low_res fp32 [K,4g,4g]."""

    def __init__(self, masks, boxes, areas, predicted_iou, stability_score, point_coords, index, low_res, output_mode="binary_mask"):
        self.masks, self.boxes, self.areas, self.predicted_iou = masks, boxes, areas, predicted_iou
        self.stability_score, self.point_coords, self.index, self.low_res = stability_score, point_coords, index, low_res
        self.output_mode = output_mode

    def __len__(self):
        return self.masks.shape[0]

    def records(self, output_mode=None):
        """-> the reference's list of dicts, one per mask: segmentation (bool array [H,W], or {"size": [H, W], "counts": [...]} with
        output_mode="uncompressed_rle"), area (int), bbox ([x, y, w, h] of the inclusive corner indices), predicted_iou (float),
        point_coords ([[x, y]]), stability_score (float), crop_box ([0, 0, W, H])."""
        mode = _check_mode(self.output_mode if output_mode is None else output_mode)
        K, H, W = self.masks.shape
        if mode == "binary_mask":
            host = self.masks.cpu().numpy()
            seg = [host[k] for k in range(K)]
        else:
            seg = [{"size": [H, W], "counts": c} for c in run_lengths(self.masks)]
        boxes, areas = self.boxes.cpu().tolist(), self.areas.cpu().tolist()
        iou, stab, pts = self.predicted_iou.cpu().tolist(), self.stability_score.cpu().tolist(), self.point_coords.cpu().tolist()
        return [{"segmentation": seg[k], "area": areas[k],
                 "bbox": [boxes[k][0], boxes[k][1], boxes[k][2] - boxes[k][0], boxes[k][3] - boxes[k][1]],
                 "predicted_iou": iou[k], "point_coords": [pts[k]], "stability_score": stab[k], "crop_box": [0, 0, W, H]}
                for k in range(K)]

    def match(self, reference_mask):
        """reference_mask [H,W] (bool, or numbers with > 0.5 set) -> the index of the kept mask with the largest IoU against it, a
        0-dim int64 tensor on the device (lowest index on ties; no host read)"""
        from .sam_predictor import select_largest

        K, H, W = self.masks.shape
        if not isinstance(reference_mask, torch.Tensor) or tuple(reference_mask.shape) != (H, W):
            raise ValueError(f"reference_mask: expected a tensor [{H},{W}], got "
                             f"{tuple(reference_mask.shape) if isinstance(reference_mask, torch.Tensor) else type(reference_mask).__name__}")
        if K == 0:
            raise ValueError("match: no mask was kept")
        ref = reference_mask.to(self.masks.device)
        ref = ref if ref.dtype == torch.bool else ref > 0.5
        inter = (self.masks & ref).sum((1, 2))
        union = self.masks.sum((1, 2)) + ref.sum() - inter
        return select_largest(inter.to(F32) / union.to(F32))


class SamAutomaticMaskGenerator:
    """predictor: a ``sam_predictor.SamPredictor``.  The arguments and defaults of the reference's class; point_grid: an explicit
    [P,2] array of (x, y) in the unit square instead of points_per_side (exactly one of the two)."""

    def __init__(self, predictor, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                 stability_score_offset=1.0, box_nms_thresh=0.7, point_grid=None, mask_threshold=0.0, crop_n_layers=0,
                 min_mask_region_area=0, output_mode="binary_mask"):
        if crop_n_layers != 0:
            raise ValueError(f"crop_n_layers: only 0 is built (every crop is another full encoder pass), got {crop_n_layers}")
        if min_mask_region_area > 0:
            raise ValueError(f"min_mask_region_area: only 0 is built (region removal needs OpenCV's connected components), got "
                             f"{min_mask_region_area}")
        self.output_mode = _check_mode(output_mode)
        if (points_per_side is None) == (point_grid is None):
            raise ValueError("points_per_side / point_grid: give exactly one of the two (points_per_side=None with a point_grid)")
        if points_per_side is not None:
            if int(points_per_side) != points_per_side or points_per_side < 1:
                raise ValueError(f"points_per_side: expected an integer >= 1, got {points_per_side}")
            self.point_grid = build_point_grid(int(points_per_side))
        else:
            grid = np.asarray(point_grid, dtype=np.float64)
            if grid.ndim != 2 or grid.shape[1] != 2 or grid.shape[0] < 1:
                raise ValueError(f"point_grid: expected [P,2] with P >= 1, got {grid.shape}")
            self.point_grid = grid
        if int(points_per_batch) != points_per_batch or points_per_batch < 1:
            raise ValueError(f"points_per_batch: expected an integer >= 1, got {points_per_batch}")
        self.predictor, self.points_per_batch = predictor, int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = float(pred_iou_thresh), float(stability_score_thresh)
        self.stability_score_offset, self.box_nms_thresh = float(stability_score_offset), float(box_nms_thresh)
        self.mask_threshold = float(mask_threshold)

    @classmethod
    def from_model(cls, model, **kwargs):
        """model: an ``InteractVLMForCausalLM`` - a predictor on its visual model's encoder and mask decoder"""
        from .sam_predictor import SamPredictor

        return cls(SamPredictor.from_model(model), **kwargs)

    def generate(self, image_u8):
        """image_u8: uint8 RGB [H,W,3] (NumPy) -> AutoMasks"""
        self.predictor.set_image(image_u8)
        return self.generate_on_set_image()

    def generate_on_set_image(self):
        """the grid of prompts on the predictor's current image (``set_image`` / ``set_embedding``) -> AutoMasks.  Every batch of
        points_per_batch prompts is scaled at once and goes through ``encode_prompts`` / ``predict_masks`` in calls of exactly
        DECODER_PROMPTS prompts; their low-res logits and predicted IoUs are collected, nothing is post-processed here.  The result
        does not depend on points_per_batch."""
        pred = self.predictor
        if not pred.is_image_set:
            raise RuntimeError("an image must be set with set_image(...) or set_embedding(...) before generating")
        d = pred.mask_decoder
        H, W = pred.original_size
        points = torch.from_numpy(self.point_grid * np.array([[W, H]], dtype=np.float64)).to(d.device)  # fp64, the photo's pixels
        P, S = points.shape[0], 4 * d.grid
        low = torch.empty(P, 3, S, S, dtype=F32, device=d.device)
        iou = torch.empty(P, 3, dtype=F32, device=d.device)
        C = DECODER_PROMPTS
        labels = torch.ones(C, 1, dtype=I32, device=d.device)
        for s in range(0, P, self.points_per_batch):
            e = min(P, s + self.points_per_batch)
            coords = pred.scale_coords(points[s:e].unsqueeze(1))
            for c in range(0, e - s, C):  # decoder calls of exactly C prompts: a short one is filled up with its last prompt
                n = min(C, e - s - c)
                chunk = coords[c: c + n]
                if n < C:
                    chunk = torch.cat([chunk, chunk[-1:].expand(C - n, -1, -1)])
                sparse, dense = d.encode_prompts(chunk.contiguous(), labels)
                low_b, iou_b = d.predict_masks(pred.embedding, sparse, dense, multimask_output=True)
                low[s + c: s + c + n].copy_(low_b[:n])
                iou[s + c: s + c + n].copy_(iou_b[:n])
        return self.select(low, iou, points)

    def select(self, low, iou, points):
        """The filter stage: low fp32 [P,M,4g,4g] low-res logits, iou fp32 [P,M] predicted IoUs, points [P,2] (x, y) in the photo's
        pixels, all for the predictor's current image sizes -> AutoMasks.  Kept: predicted IoU above pred_iou_thresh (a threshold
        <= 0 keeps all), stability #(v > t + offset) / #(v > t - offset) at least stability_score_thresh (the same), and not
        suppressed by box NMS in descending predicted IoU, ties to the lower candidate index."""
        from . import ops

        pred = self.predictor
        if pred.input_size is None:
            raise RuntimeError("an image must be set with set_image(...) or set_embedding(...) before selecting")
        if not isinstance(low, torch.Tensor) or low.dim() != 4 or low.dtype != F32 or low.numel() == 0:
            raise ValueError("low: expected a float32 tensor [P,M,h,w]")
        P, M, h, w = low.shape
        if not isinstance(iou, torch.Tensor) or tuple(iou.shape) != (P, M) or iou.dtype != F32:
            raise ValueError(f"iou: expected a float32 tensor [{P},{M}]")
        points = torch.as_tensor(points)
        if tuple(points.shape) != (P, 2):
            raise ValueError(f"points: expected [{P},2], got {tuple(points.shape)}")
        dev = low.device
        low, iou, n = low.reshape(P * M, h, w).contiguous(), iou.reshape(P * M).contiguous(), P * M
        points = points.to(dev, torch.float64)
        t, off = self.mask_threshold, self.stability_score_offset
        active = iou > self.pred_iou_thresh if self.pred_iou_thresh > 0.0 else torch.ones(n, dtype=torch.bool, device=dev)
        census = ops.mask_census(low, pred.input_size, pred.original_size, pred.img_size, (t + off, t, t - off), active.to(I32))
        stability = census[:, 0].float() / census[:, 2].float()  # 0 / 0 is NaN, which is not >= anything
        valid = active & (stability >= self.stability_score_thresh) if self.stability_score_thresh > 0.0 else active
        order = torch.sort(torch.where(valid, iou, torch.full_like(iou, float("-inf"))), descending=True, stable=True).indices
        keep = ops.box_nms(census[order, 3:7].float().contiguous(), self.box_nms_thresh, valid[order].to(I32))
        K = int(keep.sum())  # the one host read
        sel = order[torch.sort(keep, descending=True, stable=True).indices[:K]]  # the kept candidates, still in score order
        kept_low = low[sel]
        H, W = pred.original_size
        if K:
            masks = ops.postprocess_masks(kept_low, pred.input_size, pred.original_size, pred.img_size) > t
        else:
            masks = torch.zeros(0, H, W, dtype=torch.bool, device=dev)
        return AutoMasks(masks, census[sel, 3:7].contiguous(), census[sel, 1].contiguous(), iou[sel], stability[sel],
                         points[torch.div(sel, M, rounding_mode="floor")], sel, kept_low, self.output_mode)
