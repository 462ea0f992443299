"""Promptable SAM on the GPU: the three kernels (ivlm_prompt_embed, ivlm_mask_downscale, ivlm_mask_dot_multi) against the fp64
restatement of tests/_sam_prompt_ref.py and the reference's own outputs (tests/golden/sam_prompts*.npz, identical operands), the
decoder path SamMaskDecoder.encode_prompts / predict_masks end to end, the untouched text path, and SamPredictor.

Bounds (none of them measured on the code under test): the point / box encoding 1e-4 absolute, the bound
test_sam_decoder_vs_reference_golden holds dense_pe to for the same encoding over the same argument range; the mask downscaling, the
low-resolution logits and the post-processed logits 2e-4 of max |reference| and the IoU head 2e-4 absolute, the bounds that test holds
the fp32-activation decoder chain to against the fp32 oracle on identical weights."""
import os

import numpy as np
import pytest
import torch

import _sam_prompt_ref as R

pytestmark = pytest.mark.gpu

EMBED_ABS, CHAIN_REL, IOU_ABS = 1e-4, 2e-4, 2e-4


@pytest.fixture(scope="module")
def golden(golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "sam_prompts.npz")))
    d.update(np.load(os.path.join(golden_dir, "sam_prompts_post.npz")))
    return d


@pytest.fixture(scope="module")
def dec(hip_lib, cuda):
    from interactvlm_amd import sam
    from interactvlm_amd import weights as Wt

    return sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), cuda)


@pytest.fixture(scope="module")
def emb(cuda):
    """the golden's image embedding, channels last [4096, 256] fp32 (bf16 values)"""
    return torch.from_numpy(R.image_embedding())[0].permute(1, 2, 0).reshape(R.GRID * R.GRID, 256).contiguous().to(cuda)


def _case_tensors(name, cuda):
    c = R.case(name)
    return {k: (None if v is None else torch.from_numpy(v).to(cuda)) for k, v in c.items()}


@pytest.fixture(scope="module")
def runs(dec, emb, cuda):
    """every golden case through encode_prompts and the decoder ONCE, all four mask tokens: name -> (sparse, dense, low, iou)"""
    out = {}
    for name in R.CASES:
        t = _case_tensors(name, cuda)
        sparse, dense = dec.encode_prompts(t["points"], t["labels"], t["boxes"], t["mask_input"])
        low, iou = dec._predict_all(emb, sparse, dense)
        out[name] = (sparse, dense, low, iou)
    torch.cuda.synchronize()
    return out


def _rng(*key):
    return np.random.default_rng([ord(c) for c in "samprompt"] + [int(k) for k in key])


# ---- ivlm_prompt_embed ------------------------------------------------------------------------------------------------------------
def _embed_operands(Rr, F, size, seed=0):
    g = _rng(Rr, F, seed)
    coords = (g.random((Rr, 2)) * np.array([size[1], size[0]])).astype(np.float32)  # inside [0, size]: the range of dense_pe's bound
    coords[0] = (0.0, 0.0)
    coords[-1] = (size[1], size[0])
    labels = np.array([(-1, 0, 1, 2, 3)[(r + 1) % 5] for r in range(Rr)], np.int32)  # R = 1: a point; R >= 5: all five labels
    gauss = g.standard_normal((2, F)).astype(np.float32)
    table = (0.5 * g.standard_normal((5, 2 * F))).astype(np.float32)
    return coords, labels, gauss, table


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("Rr", [1, 2, 5, 67])
def test_prompt_embed_vs_restatement(hip_lib, cuda, Rr, F):
    from interactvlm_amd import ops

    for size in ((1024, 1024), (480, 768)):  # (H, W): x is divided by W, y by H
        coords, labels, gauss, table = _embed_operands(Rr, F, size)
        if Rr >= 5:
            assert set(labels.tolist()) == {-1, 0, 1, 2, 3}
        dv = lambda a: torch.from_numpy(a).to(cuda)
        got = ops.prompt_embed(dv(coords), dv(labels), dv(gauss), dv(table), size).cpu().numpy()
        ref = R.embed_rows_ref(coords, labels, gauss, table, size)
        err = float(np.abs(got - ref).max())
        print(f"prompt_embed R={Rr} F={F} size={size}: max |err| {err:.2e}")
        assert got.shape == (Rr, 2 * F) and err < EMBED_ABS
        for r in np.nonzero(labels == -1)[0]:
            assert np.array_equal(got[r], table[4])


def test_prompt_embed_label_rules(hip_lib, cuda):
    from interactvlm_amd import ops

    coords, labels, gauss, table = _embed_operands(67, 128, (1024, 1024))
    dv = lambda a: torch.from_numpy(a).to(cuda)
    base = ops.prompt_embed(dv(coords), dv(labels), dv(gauss), dv(table), (1024, 1024)).cpu()
    # a not-a-point row is the table row bit for bit, whatever its coordinates
    c2 = coords.copy()
    nap = np.nonzero(labels == -1)[0]
    c2[nap[0]] = (np.nan, np.inf)
    c2[nap[1]] = (-1e30, 3e38)
    c2[nap[2:]] = 123456.75
    got = ops.prompt_embed(dv(c2), dv(labels), dv(gauss), dv(table), (1024, 1024)).cpu()
    assert torch.equal(got, base) and all(torch.equal(got[r], torch.from_numpy(table[4])) for r in nap)
    # a label outside -1..3: NaN in its own row only (and no read outside the 5-row table)
    l2 = labels.copy()
    bad = {3: 4, 17: -2, 40: 1000000, 66: -2 ** 31, 5: 5, 64: 2 ** 31 - 1}
    for r, v in bad.items():
        l2[r] = v
    got = ops.prompt_embed(dv(coords), dv(l2), dv(gauss), dv(table), (1024, 1024)).cpu()
    for r in range(67):
        if r in bad:
            assert bool(torch.isnan(got[r]).all()), r
        else:
            assert torch.equal(got[r], base[r]), r


@pytest.mark.parametrize("F", [16, 48, 136, 160, 256])
def test_prompt_embed_refuses_other_widths(hip_lib, cuda, F):
    from interactvlm_amd import _lib, ops

    coords, labels, gauss, table = _embed_operands(5, F, (1024, 1024))
    dv = lambda a: torch.from_numpy(a).to(cuda)
    out = torch.full((5, 2 * F), -7.0, device=cuda)
    args = [dv(a) for a in (coords, labels, gauss, table)]
    rc = hip_lib.ivlm_prompt_embed(*[a.data_ptr() for a in args], out.data_ptr(), 5, F, 1024, 1024, ops._stream())
    torch.cuda.synchronize()
    assert rc == -4 and b"unsupported" in hip_lib.ivlm_error_string(rc).lower()
    with pytest.raises(_lib.IvlmError):
        ops.prompt_embed(*args, (1024, 1024), out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_encode_prompts_vs_reference_sparse(runs, golden):
    worst = 0.0
    for name in R.CASES:
        ref = torch.from_numpy(golden[name + "/sparse"])
        got = runs[name][0].cpu()
        assert got.shape == ref.shape and got.dtype == torch.float32
        worst = max(worst, float((got - ref).abs().max()))
    print(f"encode_prompts vs the reference's sparse embeddings: max |err| {worst:.2e}")
    assert worst < EMBED_ABS


# ---- ivlm_mask_downscale ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def down_weights():
    return {C: R.mask_down_weights(R.prompt_weights(embed_dim=C)) for C in (64, 256)}


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grid", [(1, 1), (2, 2), (3, 5), (64, 64)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_mask_downscale_vs_restatement(hip_lib, cuda, down_weights, grid, B, C):
    from interactvlm_amd import ops

    gh, gw = grid
    ws = down_weights[C]
    mask = (5.0 * _rng(gh, gw, B, C).standard_normal((B, 4 * gh, 4 * gw))).astype(np.float32)
    if B == 3:
        mask[1] = 2.5  # an all-constant mask: eps keeps the 4-channel norm finite
    wd = [torch.from_numpy(w).to(cuda) for w in ws]
    got = ops.mask_downscale(torch.from_numpy(mask).to(cuda), wd)
    ref = R.mask_downscale_ref(mask, ws)
    assert got.shape == (B, gh * gw, C) and bool(torch.isfinite(got).all())
    rel = float(np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"mask_downscale {gh}x{gw} B={B} C={C}: max err {rel:.2e} of max |ref|")
    assert rel < CHAIN_REL
    # prompt b does not depend on the batch: alone and inside the batch, the same bits
    for b in range(B):
        alone = ops.mask_downscale(torch.from_numpy(mask[b: b + 1]).to(cuda), wd)
        assert torch.equal(alone[0], got[b])
    zeros = ops.mask_downscale(torch.zeros(1, 4 * gh, 4 * gw, device=cuda), wd)
    assert bool(torch.isfinite(zeros).all())


def test_mask_downscale_vs_reference_dense(runs, golden):
    ref = torch.from_numpy(golden["e/dense"])  # [2, 256, 8, 8]
    got = runs["e"][1].cpu().view(2, R.GRID, R.GRID, 256)[:, ::8, ::8].permute(0, 3, 1, 2)
    rel = float((got - ref).abs().max() / ref.abs().max())
    print(f"mask_downscale vs the reference's dense embedding: max err {rel:.2e} of max |ref|")
    assert rel < CHAIN_REL


@pytest.mark.parametrize("C, mid", [(32, 16), (96, 16), (320, 16), (256, 8)])
def test_mask_downscale_refuses_other_shapes(hip_lib, cuda, C, mid):
    from interactvlm_amd import ops

    buf = torch.zeros(8192, device=cuda)
    out = torch.full((4 * 320,), -7.0, device=cuda)
    rc = hip_lib.ivlm_mask_downscale(*[buf.data_ptr()] * 11, out.data_ptr(), 1, 2, 2, C, mid, 1e-6, ops._stream())
    torch.cuda.synchronize()
    assert rc == -4 and bool((out == -7.0).all())


# ---- ivlm_mask_dot_multi --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("grid", [(1, 1), (3, 5), (64, 64)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [1, 3, 4])
def test_mask_dot_multi_gives_mask_dot_bits(hip_lib, cuda, M, B, grid, dtype):
    _check_mask_dot_multi(cuda, M, B, grid, 32, dtype)


@pytest.mark.parametrize("C", [8, 40, 72])  # a short chunk, one chunk and a tail, two chunks and a tail of the 32-channel LDS tile
def test_mask_dot_multi_other_channel_counts(hip_lib, cuda, C):
    _check_mask_dot_multi(cuda, 4, 2, (3, 5), C, torch.float32)
    _check_mask_dot_multi(cuda, 2, 2, (3, 5), C, torch.bfloat16)


def _check_mask_dot_multi(cuda, M, B, grid, C, dtype):
    from interactvlm_amd import ops

    gh, gw = grid
    g = torch.Generator().manual_seed(1000 * M + 100 * B + gh + C)
    up = torch.randn(B * gh * gw * 16, C, generator=g).to(dtype).to(cuda)
    hyper = torch.randn(B, M, C, generator=g).to(dtype).to(cuda)
    out = torch.full((B, M, 4 * gh, 4 * gw), float("nan"), device=cuda)  # every element has to be written
    got = ops.mask_dot_multi(up, hyper, B, gh, gw, out=out)
    assert got.shape == (B, M, 4 * gh, 4 * gw) and not bool(torch.isnan(got).any())
    for m in range(M):
        assert torch.equal(got[:, m], ops.mask_dot(up, hyper[:, m].contiguous(), B, gh, gw)), m


def test_mask_dot_multi_refuses_five_tokens(hip_lib, cuda):
    from interactvlm_amd import _lib, ops

    out = torch.full((1, 5, 4, 4), -7.0, device=cuda)
    with pytest.raises(_lib.IvlmError):
        ops.mask_dot_multi(torch.zeros(16, 32, device=cuda), torch.zeros(1, 5, 32, device=cuda), 1, 1, 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- predict_masks end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_predict_masks_vs_reference(dec, emb, runs, golden, cuda, name):
    from interactvlm_amd import sam

    sparse, dense, low, iou = runs[name]
    ref_low, ref_iou = torch.from_numpy(golden[name + "/low_res"]), torch.from_numpy(golden[name + "/iou"])
    B = sparse.shape[0]
    assert low.shape == (B, 4, 256, 256) and iou.shape == (B, 4) and low.dtype == iou.dtype == torch.float32
    scale = float(ref_low.abs().max())
    e_low = float((low.cpu()[..., ::4, ::4] - ref_low).abs().max()) / scale
    e_iou = float((iou.cpu() - ref_iou).abs().max())
    e_sum = float((low.double().sum((-2, -1)).cpu() - torch.from_numpy(golden[name + "/low_sum"])).abs().max()) / (256 * 256 * scale)
    post = sam.postprocess_masks(low, R.PHOTO_INPUT, R.PHOTO)
    ref_post = torch.from_numpy(golden[name + "/post"])
    assert post.shape == (B, 4) + R.PHOTO
    e_post = float((post.cpu()[..., ::10, ::10] - ref_post).abs().max() / ref_post.abs().max())
    print(f"predict_masks case {name}: low_res {e_low:.2e} of max |ref| = {scale:.3f}, mean {e_sum:.2e}, iou {e_iou:.2e}, "
          f"post-processed {e_post:.2e}")
    assert e_low < CHAIN_REL and e_sum < CHAIN_REL and e_post < CHAIN_REL
    assert e_iou < IOU_ABS
    # multimask_output picks slices of one and the same result: tokens 1..3, or token 0
    low3, iou3 = dec.predict_masks(emb, sparse, dense, multimask_output=True)
    low1, iou1 = dec.predict_masks(emb, sparse, dense, multimask_output=False)
    assert low3.shape == (B, 3, 256, 256) and iou3.shape == (B, 3) and low1.shape == (B, 1, 256, 256) and iou1.shape == (B, 1)
    assert torch.equal(low3, low[:, 1:]) and torch.equal(iou3, iou[:, 1:])
    assert torch.equal(low1, low[:, 0:1]) and torch.equal(iou1, iou[:, 0:1])


def test_a_prompt_alone_gives_its_bits_in_the_batch(dec, emb, runs):
    sparse, _, low, iou = runs["d"]
    for b in range(3):
        low_b, iou_b = dec._predict_all(emb, sparse[b: b + 1].contiguous(), None)
        assert torch.equal(low_b[0], low[b]) and torch.equal(iou_b[0], iou[b]), b


def test_graph_replay_equals_the_eager_chain(dec, emb, runs):
    """as test_sam_decoder_vs_reference_golden asserts it of the text path: the replay, the eager chain and a second replay after a
    call with other inputs give the same bits"""
    assert dec.use_graph
    for name in ("a", "e"):
        sparse, dense, low, iou = runs[name]  # (the eager chain)
        low_g, iou_g = dec._predict_all(emb, sparse, dense, graph=True)
        assert len(dec._graphs) >= 1
        dec._predict_all(emb.flip(0).contiguous(), sparse * 0.5, None if dense is None else dense.flip(1).contiguous(), graph=True)
        low_r, iou_r = dec._predict_all(emb, sparse, dense, graph=True)
        assert torch.equal(low_g, low) and torch.equal(iou_g, iou) and torch.equal(low_r, low) and torch.equal(iou_r, iou)
    n = len(dec._graphs)
    dec.predict_masks(emb, *runs["a"][:2], multimask_output=False)  # multimask_output selects a slice, not another graph
    assert len(dec._graphs) == n


def test_bf16_embedding_and_the_text_path_is_undisturbed(dec, emb, runs, cuda):
    from interactvlm_amd import synth

    sparse, dense, low, iou = runs["a"]
    low_h, iou_h = dec._predict_all(emb.to(torch.bfloat16), sparse, dense)  # the embedding holds bf16 values: same numbers
    assert torch.equal(low_h, low) and torch.equal(iou_h, iou)
    # a fresh decoder's text path before and after predict_masks on the same object: identical bits, eager and replayed
    from interactvlm_amd import sam
    from interactvlm_amd import weights as Wt

    fresh = sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), cuda)
    text = torch.from_numpy(synth.synth_normal("samdec/text/1", (1, 1, 256), 1.0, 0)).to(torch.bfloat16).float().to(cuda)
    emb1 = emb.to(torch.bfloat16)[None].contiguous()
    before, before_e = fresh(emb1, text), fresh._forward(emb1, text)
    fresh.predict_masks(emb, sparse, dense)
    after, after_e = fresh(emb1, text), fresh._forward(emb1, text)
    for x, y in zip(before + before_e, after + after_e):
        assert torch.equal(x, y)
    for x, y in zip(before, dec(emb1, text)):  # ... and of the module's decoder after all of its prompt runs
        assert torch.equal(x, y)


# ---- SamPredictor ---------------------------------------------------------------------------------------------------------------------
def test_predictor_on_a_stored_embedding(dec, emb, cuda):
    from interactvlm_amd.sam_predictor import SamPredictor

    pred = SamPredictor(None, dec)
    pred.set_embedding(emb.to(torch.bfloat16), R.PHOTO_INPUT, R.PHOTO)
    box = torch.tensor([60.5, 100.0, 420.25, 700.75])  # (x0, y0, x1, y1) in the 750 x 500 photo's pixels
    masks, iou, low = pred.predict(box=box)
    logits, iou_l, low_l = pred.predict(box=box, return_logits=True)
    assert masks.shape == (3,) + R.PHOTO and masks.dtype == torch.bool and masks.is_cuda
    assert logits.shape == masks.shape and logits.dtype == torch.float32
    assert iou.shape == (3,) and low.shape == (3, 256, 256) and torch.equal(iou, iou_l) and torch.equal(low, low_l)
    assert torch.equal(masks, logits > 0)
    one, iou1, low1 = pred.predict(box=box, multimask_output=False)
    assert one.shape == (1,) + R.PHOTO and iou1.shape == (1,) and low1.shape == (1, 256, 256)
    best = pred.best_mask(box=box)
    assert best.shape == R.PHOTO and best.dtype == torch.float32 and best.is_cuda
    assert torch.equal(best, masks[int(torch.argmax(iou))].float())
    # the batch form: the same prompt twice and a point prompt, coordinates scaled on the device
    bm, bi, bl = pred.predict_batch(boxes=torch.stack([box, box]))
    assert bm.shape == (2, 3) + R.PHOTO and bi.shape == (2, 3) and bl.shape == (2, 3, 256, 256)
    assert torch.equal(bm[0], bm[1]) and torch.equal(bl[0], bl[1])
    pm, pi, pl = pred.predict(point_coords=torch.tensor([[250.0, 375.0]]), point_labels=torch.tensor([1]), mask_input=low1)
    assert pm.shape == (3,) + R.PHOTO and bool(torch.isfinite(pl).all()) and bool(torch.isfinite(pi).all())
    mm, mi, ml = pred.predict(mask_input=low1)  # a mask alone: no sparse token at all
    assert mm.shape == (3,) + R.PHOTO and bool(torch.isfinite(ml).all()) and bool(torch.isfinite(mi).all())


def test_set_image_smoke(hip_lib, cuda):
    """a 64 x 48 photo through the small encoder configuration of test_sam_encoder_small_vs_reference_golden: shapes, finiteness"""
    from interactvlm_amd import sam
    from interactvlm_amd import weights as Wt
    from interactvlm_amd.sam_predictor import SamPredictor

    c = Wt.SamEncCfg(embed_dim=160, depth=2, num_heads=2, global_attn_indexes=(1,), img_size=480)
    enc = sam.SamImageEncoder(Wt.synth_weights(Wt.sam_encoder_spec(c)), c, cuda)
    small = sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), cuda, grid=c.grid)
    pred = SamPredictor(enc, small, img_size=480)
    photo = _rng(64, 48).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    pred.set_image(photo)
    assert pred.is_image_set and pred.original_size == (48, 64) and pred.input_size == (360, 480)
    assert pred.embedding.shape == (c.grid * c.grid, 256)
    masks, iou, low = pred.predict(point_coords=torch.tensor([[31.5, 20.0], [2.0, 3.0]]), point_labels=torch.tensor([1, 0]))
    assert masks.shape == (3, 48, 64) and masks.dtype == torch.bool and iou.shape == (3,) and low.shape == (3, 4 * c.grid, 4 * c.grid)
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(iou).all())
    best = pred.best_mask(box=torch.tensor([4.0, 4.0, 60.0, 40.0]))
    assert best.shape == (48, 64) and bool(((best == 0) | (best == 1)).all())
