"""Promptable SAM: masks of one photo from point, box and mask prompts (segment_anything/predictor.py: SamPredictor.set_image /
predict / predict_torch), on the image encoder and mask decoder the contact path already holds.

    pred = SamPredictor.from_model(model)
    pred.set_image(photo_u8)                                            # HxWx3 RGB
    target_mask = pred.best_mask(box=torch.tensor([x0, y0, x1, y1]))   # float {0, 1} [H,W]: FitScene(target_mask=...)

Host-side orchestration only: coordinates are scaled with torch operations on the device (no host read), everything else runs in
libivlm_hip.so (``SamMaskDecoder.encode_prompts`` / ``predict_masks``, ``ops.postprocess_masks``).  Every argument error is raised
before the library loads (``sam.check_prompts``).  Results are device tensors.
"""
from __future__ import annotations

import numpy as np
import torch

from . import preprocess
from .sam import check_prompts, postprocess_masks

F32 = torch.float32


def select_largest(scores):
    """scores [M] -> the index of the largest finite score, a 0-dim int64 tensor on the scores' device: ``fit.select_best`` on the
    negated scores (non-finite ranks last, ties go to the lowest index, all non-finite gives 0; no host read; CPU tensors too)."""
    from .fit import select_best

    return select_best(-scores)


class SamPredictor:
    """image_encoder: sam.SamImageEncoder, mask_decoder: sam.SamMaskDecoder of one model; img_size: the encoder's square input."""

    def __init__(self, image_encoder, mask_decoder, img_size=1024):
        if int(img_size) != mask_decoder.input_size[0]:
            raise ValueError(f"img_size {img_size}: the mask decoder's grid of {mask_decoder.grid} cells covers {mask_decoder.input_size[0]} pixels")
        self.image_encoder, self.mask_decoder, self.img_size = image_encoder, mask_decoder, int(img_size)
        self.reset_image()

    @classmethod
    def from_model(cls, model):
        """model: an ``InteractVLMForCausalLM`` - its visual model's encoder and mask decoder"""
        vm = model.model.visual_model
        return cls(vm.image_encoder, vm.mask_decoder, img_size=vm.image_encoder.cfg.img_size)

    # ---- the image ------------------------------------------------------------------------------------------------------------------
    def reset_image(self):
        self.embedding, self.input_size, self.original_size = None, None, None

    @property
    def is_image_set(self):
        return self.embedding is not None

    def set_image(self, image_u8):
        """image_u8: uint8 RGB [H,W,3] (NumPy) -> resized and normalised as the reference does (``preprocess.sam_preprocess``), encoded
        as one view"""
        if not isinstance(image_u8, np.ndarray) or image_u8.ndim != 3 or image_u8.shape[2] != 3 or image_u8.dtype != np.uint8 \
                or image_u8.shape[0] < 1 or image_u8.shape[1] < 1:
            raise ValueError(f"image_u8: expected a uint8 RGB array [H,W,3], got "
                             f"{(image_u8.dtype, image_u8.shape) if isinstance(image_u8, np.ndarray) else type(image_u8).__name__}")
        if self.image_encoder is None:
            raise ValueError("set_image needs an image encoder (this predictor was built without one: use set_embedding)")
        self.reset_image()
        x, input_size = preprocess.sam_preprocess(image_u8, self.mask_decoder.device, self.img_size)
        emb = self.image_encoder(x.unsqueeze(0))  # [1, g*g, C]
        self.set_embedding(emb[0], input_size, image_u8.shape[:2])

    def set_embedding(self, embedding, input_size, original_size):
        """embedding: one image's encoder output [g*g, C] (channels last, fp32 or bf16) on the device; input_size: (h, w) of the
        resized image inside the padded square; original_size: (H, W) of the photo"""
        d = self.mask_decoder
        if not isinstance(embedding, torch.Tensor) or tuple(embedding.shape) != (d.grid * d.grid, d.C) \
                or embedding.dtype not in (F32, torch.bfloat16):
            raise ValueError(f"embedding: expected a float32 or bfloat16 tensor [{d.grid * d.grid},{d.C}], got "
                             f"{(embedding.dtype, tuple(embedding.shape)) if isinstance(embedding, torch.Tensor) else type(embedding).__name__}")
        sizes = []
        for s, name in ((input_size, "input_size"), (original_size, "original_size")):
            if len(s) != 2 or int(s[0]) < 1 or int(s[1]) < 1:
                raise ValueError(f"{name}: expected (height, width) >= 1, got {tuple(s)}")
            sizes.append((int(s[0]), int(s[1])))
        if max(sizes[0]) > self.img_size:
            raise ValueError(f"input_size {sizes[0]} exceeds the padded input of {self.img_size}")
        self.embedding, self.input_size, self.original_size = embedding.contiguous(), sizes[0], sizes[1]

    # ---- prompts --------------------------------------------------------------------------------------------------------------------
    def scale_coords(self, coords):
        """ResizeLongestSide.apply_coords / apply_boxes: (x, y) pairs in ORIGINAL image pixels [..., 2] -> the padded input frame, fp32
        on the decoder's device.  The product is taken in fp64 as the reference takes it (NumPy floats), then rounded to fp32."""
        old_h, old_w = self.original_size
        new_h, new_w = preprocess.get_preprocess_shape(old_h, old_w, self.img_size)
        scale = torch.tensor([new_w / old_w, new_h / old_h], dtype=torch.float64, device=self.mask_decoder.device)
        return (coords.to(self.mask_decoder.device, torch.float64) * scale).to(F32)

    def predict_batch(self, point_coords=None, point_labels=None, boxes=None, mask_input=None, multimask_output=True,
                      return_logits=False):
        """B prompt sets on the one image (predict_torch, but with coordinates in ORIGINAL image pixels): point_coords [B,N,2],
        point_labels [B,N], boxes [B,4], mask_input [B,1,4g,4g] -> (masks [B,M,H,W] bool, or fp32 logits with return_logits; iou fp32
        [B,M]; low_res fp32 [B,M,4g,4g]), M = 3 with multimask_output, else 1."""
        d = self.mask_decoder
        check_prompts(point_coords, point_labels, boxes, mask_input, 4 * d.grid)
        if not self.is_image_set:
            raise RuntimeError("an image must be set with set_image(...) or set_embedding(...) before predicting")
        pts = None if point_coords is None else self.scale_coords(point_coords)
        bxs = None if boxes is None else self.scale_coords(boxes.reshape(-1, 2, 2)).reshape(-1, 4)
        sparse, dense = d.encode_prompts(pts, point_labels, bxs, mask_input)
        low, iou = d.predict_masks(self.embedding, sparse, dense, multimask_output=multimask_output)
        low = low.contiguous()
        logits = postprocess_masks(low, self.input_size, self.original_size, self.img_size)
        return (logits if return_logits else logits > 0.0), iou.contiguous(), low

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True, return_logits=False):
        """One prompt set: point_coords [N,2] as (x, y) in ORIGINAL image pixels, point_labels [N] (1 foreground, 0 background), box
        [4] = (x0, y0, x1, y1), mask_input [1,4g,4g] (the low_res logits of an earlier call) -> (masks [M,H,W], iou [M], low_res
        [M,4g,4g]) as device tensors."""
        check_prompts(point_coords, point_labels, box, mask_input, 4 * self.mask_decoder.grid, batch=False)
        one = lambda t: None if t is None else t.unsqueeze(0)
        masks, iou, low = self.predict_batch(one(point_coords), one(point_labels), one(box), one(mask_input), multimask_output,
                                             return_logits)
        return masks[0], iou[0], low[0]

    def best_mask(self, point_coords=None, point_labels=None, box=None, mask_input=None):
        """``predict(..., multimask_output=True)``, then the mask of the largest predicted IoU, picked on the device (lowest index on
        ties) -> float32 {0, 1} [H,W]: what ``FitScene(target_mask=...)`` and ``human_mask=`` take."""
        masks, iou, _ = self.predict(point_coords, point_labels, box, mask_input, multimask_output=True)
        return masks.index_select(0, select_largest(iou).reshape(1))[0].to(F32)

