"""The automatic mask generator on the GPU: ivlm_mask_census against the integers torch takes from ivlm_postprocess_masks' own output
(exact) and against the float64 bracket of tests/_resample_ref.py, ivlm_box_nms against the restated NMS (exact), ``select`` on the
seeded candidates of tests/golden/amg_select.npz against the reference's records, and ``generate_on_set_image`` on the stored
embedding of tests/_sam_prompt_ref.py against the materialising route (post-process every candidate, count with torch).

No tolerance in this file: every comparison is of integers or of bits, or a bracket whose ends are ``_resample_ref.bound`` away from
the float64 value."""
import os
import types

import numpy as np
import pytest
import torch

import _amg_ref as A
import _resample_ref as RR
import _sam_prompt_ref as R

pytestmark = pytest.mark.gpu

THRESHOLDS = (1.0, 0.0, -1.0)
SMALL_CASES = [
    (8, 8, 32, (32, 32), (32, 32)),
    (8, 8, 32, (32, 21), (47, 31)),
    (16, 12, 64, (64, 43), (5, 1027)),
    (16, 16, 64, (48, 64), (3, 2049)),
    (1, 1, 8, (8, 8), (5, 6)),
    (4, 4, 16, (16, 16), (1, 1)),
    (256, 256, 1024, (1024, 683), (7, 1367)),
]
REAL_CASE = (256, 256, 1024, (1024, 683), (750, 500))
CASES = [(c, 3) for c in SMALL_CASES] + [(REAL_CASE, 6)]


def torch_census(logits, thresholds=THRESHOLDS):
    """logits [n,H,W] on the device -> int32 [n,8]: the census as torch takes it from the materialised values"""
    n, H, W = logits.shape
    hi, mid, lo = thresholds
    inside = logits > mid
    out = torch.zeros(n, 8, dtype=torch.int32, device=logits.device)
    out[:, 0], out[:, 1], out[:, 2] = (logits > hi).sum((1, 2)), inside.sum((1, 2)), (logits > lo).sum((1, 2))
    cols, rows = inside.any(1), inside.any(2)  # [n,W], [n,H]
    xs, ys = torch.arange(W, device=logits.device), torch.arange(H, device=logits.device)
    some = out[:, 1] > 0
    out[:, 3] = torch.where(some, torch.where(cols, xs, W).min(1).values, 0)
    out[:, 4] = torch.where(some, torch.where(rows, ys, H).min(1).values, 0)
    out[:, 5] = torch.where(some, torch.where(cols, xs, -1).max(1).values, 0)
    out[:, 6] = torch.where(some, torch.where(rows, ys, -1).max(1).values, 0)
    return out


def _both(low, case, thresholds=THRESHOLDS, **kw):
    from interactvlm_amd import ops

    h, w, img, ins, orig = case
    got = ops.mask_census(low, ins, orig, img, thresholds, **kw)
    want = torch_census(ops.postprocess_masks(low, ins, orig, img), thresholds)
    return got, want


# ---- census, exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, n", CASES, ids=[RR.case_id(c) for c, _ in CASES])
def test_census_equals_torch_on_the_materialised_values(hip_lib, cuda, case, n):
    h, w = case[:2]
    low = torch.from_numpy(RR.smooth(n, h, w)).to(cuda)
    got, want = _both(low, case)
    assert got.shape == (n, 8) and got.dtype == torch.int32
    print(f"census {RR.case_id(case)}: counts {got[:, :3].tolist()}")
    assert torch.equal(got, want)
    assert bool((got[:, 7] == 0).all())


def test_census_of_constant_and_impulse_images(hip_lib, cuda):
    from interactvlm_amd import ops

    for case in (SMALL_CASES[1], SMALL_CASES[2]):
        h, w, img, ins, (oh, ow) = case
        below = ops.mask_census(torch.full((2, h, w), -5.0, device=cuda), ins, (oh, ow), img)
        assert bool((below == 0).all())
        above = ops.mask_census(torch.full((2, h, w), 5.0, device=cuda), ins, (oh, ow), img)
        assert above.tolist() == [[oh * ow] * 3 + [0, 0, ow - 1, oh - 1, 0]] * 2
        only_lo = ops.mask_census(torch.full((1, h, w), -0.5, device=cuda), ins, (oh, ow), img)  # above t_lo alone: no box
        assert only_lo.tolist() == [[0, 0, oh * ow, 0, 0, 0, 0, 0]]
        r, c = RR.visible_impulse(case)
        sites = [(r, c), (0, 0), (h - 1, w - 1)]
        low = torch.from_numpy(np.stack([4.0 * RR.impulse(h, w, *s) - 2.0 for s in sites])).to(cuda)
        got, want = _both(low, case)
        assert torch.equal(got, want)
        assert int(got[0, 2]) > 0  # the visible impulse is seen


def test_census_active_rows_garbage_and_repeat(hip_lib, cuda):
    from interactvlm_amd import ops

    h, w, img, ins, orig = REAL_CASE
    low = torch.from_numpy(RR.smooth(6, h, w)).to(cuda)
    full = ops.mask_census(low, ins, orig, img)
    active = torch.tensor([1, 0, 0, 1, 7, 0], dtype=torch.int32, device=cuda)
    out = torch.full((6, 8), 0x5A5A5A5A, dtype=torch.int32, device=cuda)  # the call initialises its output itself
    got = ops.mask_census(low, ins, orig, img, active=active, out=out)
    assert got.data_ptr() == out.data_ptr()
    for i in range(6):
        assert torch.equal(got[i], full[i] if int(active[i]) else torch.zeros_like(full[i])), i
    assert int(full[:, 1].min()) > 0  # (no row is zero by itself)
    again = ops.mask_census(low, ins, orig, img, active=active, out=torch.full_like(out, -1))
    assert torch.equal(again, got) and torch.equal(ops.mask_census(low, ins, orig, img), full)
    # other thresholds than the defaults, NaN pixels count nowhere
    ths = (0.75, 0.25, -2.5)
    g, wnt = _both(low, REAL_CASE, ths)
    assert torch.equal(g, wnt)
    nan = low[:1].clone()
    nan[0, 100:140, 60:90] = float("nan")
    g, wnt = _both(nan, REAL_CASE)
    assert torch.equal(g, wnt)


def test_census_sizes_accepted_and_refused(hip_lib, cuda):
    from interactvlm_amd import _lib, ops

    n = 64 * 64 * 3
    low = torch.full((n, 4, 4), -3.0, device=cuda)
    low[n - 1] = 3.0
    got = ops.mask_census(low, (16, 16), (5, 3), 16)
    assert got.shape == (n, 8) and bool((got[: n - 1] == 0).all()) and got[n - 1].tolist() == [15, 15, 15, 0, 0, 2, 4, 0]
    out = torch.full((1, 8), -7, dtype=torch.int32, device=cuda)
    small = torch.zeros(1, 4, 4, device=cuda)
    rc = hip_lib.ivlm_mask_census(small.data_ptr(), 1, 4, 4, 16, 16, 16, 65536, 32768, 1.0, 0.0, -1.0, None, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == -4 and bool((out == -7).all())
    with pytest.raises(_lib.IvlmError):
        ops.mask_census(small, (16, 16), (46341, 46341), 16, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7).all())


# ---- census against float64 -----------------------------------------------------------------------------------------------------------
def _inside_bracket(got, few, many):
    """got, few, many: census rows [n,8] (few: thresholds raised by the bound, many: lowered) -> None or what is outside"""
    for i in range(len(got)):
        for c in range(3):
            if not few[i, c] <= got[i, c] <= many[i, c]:
                return f"row {i} count {c}: {got[i, c]} outside [{few[i, c]}, {many[i, c]}]"
        if got[i, 1] == 0:
            if few[i, 1] != 0 or tuple(got[i, 3:7]) != (0, 0, 0, 0):
                return f"row {i}: empty with box {got[i, 3:7]}, at least {few[i, 1]} pixels expected"
            continue
        x0, y0, x1, y1 = got[i, 3:7]
        mx0, my0, mx1, my1 = many[i, 3:7]
        if not (mx0 <= x0 and my0 <= y0 and x1 <= mx1 and y1 <= my1):
            return f"row {i}: box {got[i, 3:7]} outside the widest {many[i, 3:7]}"
        if few[i, 1] > 0:
            fx0, fy0, fx1, fy1 = few[i, 3:7]
            if not (x0 <= fx0 and y0 <= fy0 and fx1 <= x1 and fy1 <= y1):
                return f"row {i}: box {got[i, 3:7]} does not hold the narrowest {few[i, 3:7]}"
    return None


@pytest.mark.parametrize("case", SMALL_CASES, ids=[RR.case_id(c) for c in SMALL_CASES])
def test_census_inside_the_float64_bracket(hip_lib, cuda, case):
    from interactvlm_amd import ops

    h, w, img, ins, orig = case
    low = RR.smooth(3, h, w)
    ref, e = RR.post64(low, img, ins, orig), RR.bound(low, img, ins, orig)
    few, many = A.census_of(ref, THRESHOLDS, e), A.census_of(ref, THRESHOLDS, -e)
    got = ops.mask_census(torch.from_numpy(low).to(cuda), ins, orig, img).cpu().numpy()
    print(f"census {RR.case_id(case)}: {int((few[:, :3] != many[:, :3]).sum())} of 9 counts have a pixel inside the band")
    assert _inside_bracket(got, few, many) is None


# ---- NMS ------------------------------------------------------------------------------------------------------------------------------
def _device_nms(boxes, scores, thr, cuda, valid=None):
    """the ordering ``select`` uses (stable descending sort) + ops.box_nms -> kept indices in score order"""
    from interactvlm_amd import ops

    b, s = torch.from_numpy(np.asarray(boxes, np.float32)).to(cuda), torch.from_numpy(np.asarray(scores, np.float32)).to(cuda)
    order = torch.sort(s, descending=True, stable=True).indices
    v = None if valid is None else torch.from_numpy(np.asarray(valid, np.int32)).to(cuda)[order].contiguous()
    keep = ops.box_nms(b[order].contiguous(), thr, v)
    assert keep.dtype == torch.int32 and bool(((keep == 0) | (keep == 1)).all())
    return order[keep.bool()].cpu().numpy(), order.cpu().numpy()


def _random_boxes(n, seed):
    """integer boxes with corners on about n / 10 lattice sites and sides from a few lengths, so that many pairs overlap heavily and
    some are equal"""
    g = np.random.default_rng(seed)
    site = g.integers(0, max(1, n // 10), n)
    x0, y0 = (site % 12) * 16, (site // 12) * 16
    return np.stack([x0, y0, x0 + g.choice([24, 28, 32, 44], n), y0 + g.choice([24, 28, 32, 44], n)], 1).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 3072])
def test_box_nms_equals_the_restatement(hip_lib, cuda, n):
    boxes = _random_boxes(n, n)
    g = np.random.default_rng(1000 + n)
    for scores, valid, what in (
            (g.random(n).astype(np.float32), None, "distinct scores"),
            (g.integers(0, 4, n).astype(np.float32), None, "tied scores"),
            (g.random(n).astype(np.float32), (g.random(n) < 0.6).astype(np.int32), "valid holes")):
        for thr in (0.7, 0.3):
            kept, order = _device_nms(boxes, scores, thr, cuda, valid)
            assert order.tolist() == A.score_order(scores), what
            flags = A.nms_ordered(boxes[order], thr, None if valid is None else valid[order])
            want = order[flags.astype(bool)]
            assert kept.tolist() == want.tolist(), (what, thr)
            if n >= 63 and valid is None:
                assert 1 < len(want) < n  # the case suppresses something and keeps something
        if valid is not None:
            assert not set(kept.tolist()) & set(np.flatnonzero(valid == 0).tolist())


def test_box_nms_rules(hip_lib, cuda):
    from interactvlm_amd import ops

    def run(rows, thr, valid=None):
        b = torch.tensor(rows, dtype=torch.float32, device=cuda)
        v = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=cuda)
        got = ops.box_nms(b, thr, v).tolist()
        assert got == A.nms_ordered(np.array(rows, np.float32), thr, valid).tolist()
        return got

    assert run([[0, 0, 100, 100], [0, 0, 100, 80], [0, 0, 100, 60]], 0.7) == [1, 0, 1]  # B is suppressed: it does not suppress C
    assert run([[0, 0, 10, 10], [0, 0, 10, 5]], 0.5) == [1, 1]                              # IoU == threshold: kept
    assert run([[0, 0, 10, 10], [0, 0, 10, 5]], 0.4999) == [1, 0]
    assert run([[0, 0, 0, 0]] * 3, 0.7) == [1, 1, 1]                                        # 0 / 0 suppresses nothing
    assert run([[0, 0, 10, 10]] * 3, 0.7) == [1, 0, 0]
    assert run([[0, 0, 10, 10]] * 3, 0.7, [0, 1, 1]) == [0, 1, 0]                           # invalid: neither kept nor suppressing
    assert run([[0, 0, 10, 10]] * 3, 0.7, [0, 0, 0]) == [0, 0, 0]
    # a suppression across words of the bit matrix: row 0 and row 200 are the same box
    rows = [[1000.0 * i, 0.0, 1000.0 * i + 10.0, 10.0] for i in range(300)]
    rows[200] = rows[0]
    rows[299] = rows[70]
    assert run(rows, 0.7) == [0 if i in (200, 299) else 1 for i in range(300)]


def test_box_nms_refuses_more_than_16384(hip_lib, cuda):
    from interactvlm_amd import _lib, ops

    n = 16385
    boxes = torch.zeros(n, 4, device=cuda)
    keep = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    ws = torch.zeros(1024, dtype=torch.uint8, device=cuda)
    rc = hip_lib.ivlm_box_nms(boxes.data_ptr(), None, n, 0.7, keep.data_ptr(), ws.data_ptr(), 1 << 40, ops._stream())
    torch.cuda.synchronize()
    assert rc == -4 and bool((keep == -7).all())
    with pytest.raises(_lib.IvlmError):
        ops.box_nms(boxes, 0.7)
    assert hip_lib.ivlm_box_nms_workspace_bytes(16384) == 16384 * 256 * 8
    kept = ops.box_nms(torch.zeros(16384, 4, device=cuda), 0.7)  # the largest size: degenerate boxes, all kept
    assert bool((kept == 1).all())


# ---- select on the golden's seeded candidates -------------------------------------------------------------------------------------------
def _golden_generator(**kw):
    from interactvlm_amd.sam_amg import SamAutomaticMaskGenerator

    pred = types.SimpleNamespace(input_size=A.INPUT, original_size=A.PHOTO, img_size=A.IMG)
    return SamAutomaticMaskGenerator(pred, points_per_side=A.SIDE, points_per_batch=A.BATCH, pred_iou_thresh=A.IOU_THRESH,
                                     stability_score_thresh=A.STABILITY_THRESH, stability_score_offset=A.OFFSET,
                                     box_nms_thresh=A.NMS_THRESH, **kw)


def test_select_gives_the_reference_records(hip_lib, cuda, golden_dir):
    golden = np.load(os.path.join(golden_dir, "amg_select.npz"))
    low, iou = A.candidates()
    few, many, in_band = A.golden_band()
    got = _golden_generator().select(torch.from_numpy(low).to(cuda), torch.from_numpy(iou).to(cuda), A.golden_points())
    index = got.index.cpu().numpy()
    assert got.index.dtype == torch.int64 and index.tolist() == golden["index"].tolist()  # the kept set and its order
    K = len(index)
    assert got.masks.shape == (K,) + A.PHOTO and got.masks.dtype == torch.bool and got.low_res.shape == (K, A.LOW, A.LOW)
    assert got.boxes.dtype == got.areas.dtype == torch.int32 and got.point_coords.dtype == torch.float64
    assert np.array_equal(got.predicted_iou.cpu().numpy().view(np.uint32), golden["predicted_iou"].view(np.uint32))
    assert np.array_equal(got.point_coords.cpu().numpy(), golden["point_coords"])
    assert torch.equal(got.low_res.cpu(), torch.from_numpy(low.reshape(-1, A.LOW, A.LOW)[index]))
    boxes, areas, stab = got.boxes.cpu().numpy().astype(np.int64), got.areas.cpu().numpy(), got.stability_score.cpu().numpy()
    gb = golden["bbox"]
    ref_boxes = np.stack([gb[:, 0], gb[:, 1], gb[:, 0] + gb[:, 2], gb[:, 1] + gb[:, 3]], 1)
    ref_masks = RR.post64(low.reshape(-1, A.LOW, A.LOW)[index], A.IMG, A.INPUT, A.PHOTO) > A.MASK_THRESH
    masks = got.masks.cpu().numpy()
    print(f"select: {K} kept, {int(in_band[index].sum())} of them with a pixel inside the band")
    for k, i in enumerate(index):
        if not in_band[i]:
            assert areas[k] == golden["area"][k] and boxes[k].tolist() == ref_boxes[k].tolist(), k
            assert stab[k].view(np.uint32) == golden["stability_score"][k].view(np.uint32), k
            assert np.array_equal(masks[k], ref_masks[k]), k
        else:
            assert few[i, 1] <= areas[k] <= many[i, 1] and boxes[k].tolist() == ref_boxes[k].tolist(), k  # (the golden asserts
            lo_s, hi_s = few[i, 0] / many[i, 2], many[i, 0] / few[i, 2]                                  # equal boxes at both ends)
            assert np.float32(lo_s) <= stab[k] <= np.float32(hi_s), k
        assert areas[k] == int(masks[k].sum()) and tuple(boxes[k]) == A.box_of(masks[k]), k
    # the records of the two modes
    off = golden["rle_offsets"]
    for mode in ("binary_mask", "uncompressed_rle"):
        recs = got.records(mode)
        assert len(recs) == K
        for k, r in enumerate(recs):
            assert r["bbox"] == gb[k].tolist() and r["crop_box"] == [0, 0, A.PHOTO[1], A.PHOTO[0]]
            assert r["point_coords"] == [golden["point_coords"][k].tolist()]
            assert np.float32(r["predicted_iou"]) == golden["predicted_iou"][k]
            if mode == "binary_mask":
                assert np.array_equal(r["segmentation"], masks[k])
            else:
                assert np.array_equal(A.rle_decode(r["segmentation"]["counts"], A.PHOTO), masks[k])
                if not in_band[index[k]]:
                    assert r["segmentation"]["counts"] == golden["rle_counts"][off[k]: off[k + 1]].tolist()


def test_select_with_filters_off_and_nothing_kept(hip_lib, cuda):
    low, iou = A.candidates()
    dl, di = torch.from_numpy(low).to(cuda), torch.from_numpy(iou).to(cuda)
    gen = _golden_generator()
    gen.pred_iou_thresh, gen.stability_score_thresh = 0.0, 0.0  # both filters off: NMS alone, over all 48
    got = gen.select(dl, di, A.golden_points())
    want = A.select_ref(low, iou, A.golden_points(), A.IMG, A.INPUT, A.PHOTO, iou_thresh=0.0, stability_thresh=0.0)
    few, many, _ = A.golden_band()
    if np.array_equal(few[:, 3:7], many[:, 3:7]):  # (no box inside its band: the kept set is pinned)
        assert got.index.cpu().tolist() == want["index"].tolist()
    gen.pred_iou_thresh = 2.0  # nothing passes
    none = gen.select(dl, di, A.golden_points())
    assert len(none) == 0 and none.masks.shape == (0,) + A.PHOTO and none.records() == [] and none.boxes.shape == (0, 4)


# ---- end to end on the stored embedding -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predictor(hip_lib, cuda):
    from interactvlm_amd import sam
    from interactvlm_amd import weights as Wt
    from interactvlm_amd.sam_predictor import SamPredictor

    dec = sam.SamMaskDecoder(Wt.synth_weights({**Wt.prompt_encoder_spec(), **Wt.mask_decoder_spec()}), cuda)
    emb = torch.from_numpy(R.image_embedding())[0].permute(1, 2, 0).reshape(R.GRID * R.GRID, 256).contiguous().to(cuda)
    pred = SamPredictor(None, dec)
    pred.set_embedding(emb.to(torch.bfloat16), R.PHOTO_INPUT, R.PHOTO)
    return pred


BATCHES = (5, 7, 16)  # the 16 prompts of the test in decoder calls of 5 + 11 fill, 7 + 9 fill, or all 16 real


def _route(predictor, pts, cuda):
    """the route the reference takes, from existing calls: ``predict_batch`` of the 16 points with the logits post-processed to the
    photo's size -> (logits [n,H,W], iou [n], low [n,4g,4g])"""
    p = torch.from_numpy(pts).to(cuda).unsqueeze(1)
    got = predictor.predict_batch(p, torch.ones(p.shape[0], 1, dtype=torch.int32, device=cuda), multimask_output=True, return_logits=True)
    return tuple(t.flatten(0, 1).clone() for t in got)


def _route_select(logits, iou, kw):
    """the filters on the materialised logits, counted and boxed with torch, the restated NMS -> (kept indices in NMS order, census,
    stability, numbers of candidates that pass the first and the first two filters)"""
    t, off = kw["mask_threshold"], kw["stability_score_offset"]
    cen = torch_census(logits, (t + off, t, t - off))
    stab = cen[:, 0].float() / cen[:, 2].float()
    active = iou > kw["pred_iou_thresh"] if kw["pred_iou_thresh"] > 0.0 else torch.ones_like(iou, dtype=torch.bool)
    valid = active & (stab >= kw["stability_score_thresh"]) if kw["stability_score_thresh"] > 0.0 else active
    idx = np.flatnonzero(valid.cpu().numpy())
    boxes = cen[:, 3:7].cpu().numpy().astype(np.float32)
    kept = idx[A.nms(boxes[idx], iou.cpu().numpy()[idx], kw["box_nms_thresh"])] if len(idx) else idx
    return kept, cen, stab, int(active.sum()), len(idx)


@pytest.fixture(scope="module")
def materialised(predictor, cuda):
    """the materialising route's result; the thresholds of the test are measured on it (synthetic weights predict no meaningful
    quality: only the machinery is under test): the medians of the predicted IoUs, of the stabilities and of the pairwise box IoUs
    below 1; the mask threshold is the 90th percentile of all logits and the stability offset its distance to the 85th or 95th (with
    the reference's 0 and 1 every synthetic mask spans the photo and all boxes are equal)"""
    from interactvlm_amd.sam_amg import DECODER_PROMPTS, build_point_grid

    H, W = R.PHOTO
    pts = build_point_grid(4) * np.array([[W, H]], dtype=np.float64)
    assert len(pts) == DECODER_PROMPTS  # one predict_batch of all points is one decoder call of the generator's size
    logits, iou, low = _route(predictor, pts, cuda)
    q85, q90, q95 = torch.quantile(logits[:, ::4, ::4].flatten(), torch.tensor([0.85, 0.90, 0.95], device=cuda)).tolist()
    kw = dict(mask_threshold=q90, stability_score_offset=min(q95 - q90, q90 - q85), pred_iou_thresh=max(float(iou.median()), 0.0),
              stability_score_thresh=0.0, box_nms_thresh=2.0)
    _, cen, stab, _, _ = _route_select(logits, iou, kw)
    finite = (iou > kw["pred_iou_thresh"]) & torch.isfinite(stab)
    kw["stability_score_thresh"] = max(float(stab[finite].median()), 0.0) if bool(finite.any()) else 0.0
    order, _, _, _, _ = _route_select(logits, iou, kw)  # (NMS threshold 2: nothing suppressed) the valid candidates in score order
    boxes = cen[:, 3:7].cpu().numpy()
    pair = [float(A.box_iou32(boxes[a], boxes[b])) for k, a in enumerate(order) for b in order[k + 1:]]
    kw["box_nms_thresh"] = float(np.float32(np.median([v for v in pair if v < 1.0] or [0.7])))
    kept, cen, stab, n_iou, n_valid = _route_select(logits, iou, kw)
    print(f"end to end: {n_iou} of {len(iou)} pass the IoU filter, {n_valid} stability, {len(kept)} kept; {kw}")
    assert 1 <= len(kept) <= n_valid <= n_iou <= len(iou)
    return dict(points=pts, kw=kw, logits=logits, iou=iou, low=low, census=cen, stability=stab, kept=kept)


@pytest.fixture(scope="module")
def generated(predictor, materialised):
    from interactvlm_amd.sam_amg import SamAutomaticMaskGenerator

    return {b: SamAutomaticMaskGenerator(predictor, points_per_side=4, points_per_batch=b, **materialised["kw"]).generate_on_set_image()
            for b in BATCHES}


@pytest.mark.parametrize("batch", BATCHES)
def test_generate_equals_the_materialising_route(materialised, generated, batch):
    m, got = materialised, generated[batch]
    kept = torch.from_numpy(m["kept"]).to(got.index.device)
    assert got.index.tolist() == m["kept"].tolist()  # the set and its order
    assert torch.equal(got.boxes, m["census"][kept, 3:7]) and torch.equal(got.areas, m["census"][kept, 1])
    assert torch.equal(got.stability_score.view(torch.int32), m["stability"][kept].view(torch.int32))
    assert torch.equal(got.predicted_iou, m["iou"][kept]) and torch.equal(got.low_res, m["low"][kept])
    assert torch.equal(got.masks, m["logits"][kept] > m["kw"]["mask_threshold"])
    assert np.array_equal(got.point_coords.cpu().numpy(), m["points"][m["kept"] // 3])
    assert bool((got.predicted_iou[1:] <= got.predicted_iou[:-1]).all())


def test_points_per_batch_does_not_change_the_result(generated):
    """``SamMaskDecoder.predict_masks`` is not bit-invariant to the number of prompts per call (measured for these 16 prompts: 5
    per call against 16 moves the low-res logits by up to 3.9e-5 and the predicted IoUs by 5.7e-6), so the generator makes every
    decoder call with ``DECODER_PROMPTS`` prompts, filling a short one up; a prompt's bits do not depend on its companions"""
    a = generated[16]
    for batch in BATCHES:
        b = generated[batch]
        for name in ("index", "boxes", "areas", "predicted_iou", "stability_score", "point_coords", "low_res", "masks"):
            assert getattr(a, name).shape == getattr(b, name).shape and torch.equal(getattr(a, name), getattr(b, name)), (batch, name)


def test_records_decode_to_the_masks_and_match_finds_a_mask(generated):
    got = generated[16]
    masks = got.masks.cpu().numpy()
    H, W = R.PHOTO
    for mode in ("binary_mask", "uncompressed_rle"):
        recs = got.records(mode)
        assert len(recs) == len(got)
        for k, r in enumerate(recs):
            seg = r["segmentation"] if mode == "binary_mask" else A.rle_decode(r["segmentation"]["counts"], (H, W))
            assert np.array_equal(seg, masks[k]), (mode, k)
            assert r["area"] == int(masks[k].sum()) and r["crop_box"] == [0, 0, W, H]
            x0, y0, x1, y1 = A.box_of(masks[k])
            assert r["bbox"] == [x0, y0, x1 - x0, y1 - y0]
    for j in range(len(got)):
        if int(got.areas[j]) > 0:
            found = got.match(got.masks[j])
            assert found.is_cuda and found.dtype == torch.int64 and int(found) == j
            assert int(got.match(got.masks[j].float())) == j
