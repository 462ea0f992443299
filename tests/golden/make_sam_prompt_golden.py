#!/usr/bin/env python3
"""Generate tests/golden/sam_prompts.npz and sam_prompts_post.npz by RUNNING THE REFERENCE's PromptEncoder, MaskDecoder,
Sam.postprocess_masks and ResizeLongestSide on point, box and mask prompts (build container only: it needs the reference through
_ref_shims; the GPU box never runs this):

    python tests/golden/make_sam_prompt_golden.py

The modules are built as make_golden.py's gen_sam_decoder builds them (synth.fill_state_dict, seed 0); then EVERY PARAMETER IS ROUNDED
TO BF16 and held as fp32 (the Gaussian matrix stays unrounded) and the synthetic image embedding is rounded to bf16 - the operands the
device path holds.  The reference's output is then the fp32 computation on identical operands: no weight-rounding term enters a
tolerance.  The prompt cases are tests/_sam_prompt_ref.py's (one definition for this file and the tests).  Fixtures are data only.

Stored per case X in (a, b, c, d, e): X/sparse whole, X/low_res = [token 0 of the multimask_output=False run | tokens 1..3 of the
True run] every 4th pixel, X/low_sum its fp64 sums per (prompt, token), X/iou whole in the same token order; e/dense every 8th cell;
and, in sam_prompts_post.npz (a file of its own: with it the first would pass the size limit of a committed file), X/post = the
post-processed logits of the same tokens at a non-identity size ((1024, 683) -> (750, 500)) every 10th pixel.  Beside them
photo_coords / photo_coords_scaled: ResizeLongestSide(1024).apply_coords for a 750 x 500 photo.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import _ref_shims  # noqa: E402
import _sam_prompt_ref as R  # noqa: E402
from interactvlm_amd import synth  # noqa: E402


def main():
    import torch

    _ref_shims.install()
    from model.segment_anything.modeling import MaskDecoder, PromptEncoder, TwoWayTransformer
    from model.segment_anything.modeling.sam import Sam
    from model.segment_anything.utils.transforms import ResizeLongestSide
    from interactvlm_amd.weights import SAM_PREFIX

    torch.manual_seed(0)
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(R.GRID, R.GRID), input_image_size=(R.IMG, R.IMG), mask_in_chans=16)
    md = MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048,
                     num_heads=8), transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    synth.fill_state_dict(pe, 0, SAM_PREFIX + ".prompt_encoder.")
    synth.fill_state_dict(md, 0, SAM_PREFIX + ".mask_decoder.")
    with torch.no_grad():
        for mod in (pe, md):
            for name, t in mod.state_dict().items():
                if t.dtype.is_floating_point and "gaussian" not in name:
                    t.copy_(t.to(torch.bfloat16).float())
    pe.eval(), md.eval()

    class _Enc:  # postprocess_masks only reads image_encoder.img_size
        img_size = R.IMG

    post = lambda m: Sam.postprocess_masks(type("S", (), {"image_encoder": _Enc})(), m, R.PHOTO_INPUT, R.PHOTO)
    emb = torch.from_numpy(R.image_embedding())
    t = lambda x: None if x is None else torch.from_numpy(x)
    main_, post_ = {}, {}
    for name in R.CASES:
        c = R.case(name)
        with torch.no_grad():
            points = None if c["points"] is None else (t(c["points"]), t(c["labels"]))
            sparse, dense = pe(points=points, boxes=t(c["boxes"]), masks=t(c["mask_input"]), text_embeds=None)
            runs = [md(image_embeddings=emb, image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=sparse,
                       dense_prompt_embeddings=dense, multimask_output=mm) for mm in (False, True)]
            low = torch.cat([runs[0][0], runs[1][0]], 1)  # [B, 4, 256, 256]: token 0 | tokens 1..3
            iou = torch.cat([runs[0][1], runs[1][1]], 1)
            full = post(low)
        assert low.shape[1:] == (4, 256, 256) and tuple(full.shape[-2:]) == R.PHOTO
        main_[name + "/sparse"] = sparse.numpy()
        main_[name + "/low_res"] = np.ascontiguousarray(low.numpy()[..., ::4, ::4])
        main_[name + "/low_sum"] = low.double().sum((-2, -1)).numpy()
        main_[name + "/iou"] = iou.numpy()
        if c["mask_input"] is not None:
            main_[name + "/dense"] = np.ascontiguousarray(dense.numpy()[..., ::8, ::8])  # [B, C, 8, 8]
        post_[name + "/post"] = np.ascontiguousarray(full.numpy()[..., ::10, ::10])
    pc = R.photo_coords()
    main_["photo_coords"] = pc
    main_["photo_coords_scaled"] = ResizeLongestSide(R.IMG).apply_coords(pc, R.PHOTO)
    for fn, arrays in (("sam_prompts.npz", main_), ("sam_prompts_post.npz", post_)):
        path = os.path.join(HERE, fn)
        np.savez_compressed(path, **arrays)
        print(f"  wrote {fn}  ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
