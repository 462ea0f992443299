"""validate() without a GPU: the CPU restatement of its metrics (tests/_validate_ref.py) against the numbers the reference's own
functions returned (tests/golden/validate_metrics.npz), the device-meter arithmetic and its cross-rank reduction on gloo, and
the loop's bookkeeping with a stub model.  Tolerances: counts and flags exact; AUC 1e-6; SIM / MAE / aIoU / giou / ciou 1e-5."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _validate_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "validate_metrics.npz"))


def test_restated_segmentation_metrics_match_the_reference(gold):
    for c in range(gold["seg_pred"].shape[0]):
        pred, gt = torch.from_numpy(gold["seg_pred"][c]), torch.from_numpy(gold["seg_gt"][c])
        counts = R.seg_iou_counts(pred, gt)
        assert np.array_equal(counts.numpy(), gold["seg_counts"][c])
        assert np.array_equal(R.seg_iou_counts(pred, gt, ignore_label=255).numpy(), gold["seg_counts_ign255"][c])
        for dtype in (torch.uint8, torch.float32):  # the other label dtypes read the same classes
            if dtype == torch.uint8 and bool((gt < 0).any()):
                continue  # (a negative label does not survive uint8)
            assert torch.equal(R.seg_iou_counts(pred, gt.to(dtype)), counts)
        inter, union, acc = R.seg_metrics(counts)
        assert np.array_equal(inter.numpy(), gold["seg_inter"][c]) and np.array_equal(union.numpy(), gold["seg_union"][c])
        print(f"[seg case {c}] acc_iou {acc.numpy()} ref {gold['seg_acc'][c]}")
        np.testing.assert_allclose(acc.numpy(), gold["seg_acc"][c], rtol=0, atol=1e-5)
    # the cases the fixture is there for
    assert (gold["seg_gt"] == -1).any() and gold["seg_counts"][0, 2, :, 1].sum() == 0 and (gold["seg_gt"] == 7).any()
    assert (gold["seg_gt"] == 255).any() and not (gold["seg_gt"][2] < 0).any()


def test_restated_affordance_metrics_match_the_reference(gold):
    gt, pred, ref = torch.from_numpy(gold["aff_gt"]), torch.from_numpy(gold["aff_pred"]), gold["aff_ref"]
    assert np.array_equal(gold["aff_thresholds"], R.THRESHOLDS.numpy())
    per, valid = R.affordance_metrics(gt, pred)
    per = per.double().numpy()
    assert np.array_equal(valid.numpy(), ref[:, 4].astype(np.int32))
    assert list(valid.numpy()) == [1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1]
    for b in range(len(ref)):
        print(f"[afford row {b}] got {per[b]} ref {ref[b]}")
        for j in (0, 1):  # SIM, MAE: NaN / inf where the reference's are
            if np.isfinite(ref[b, j]):
                assert abs(per[b, j] - ref[b, j]) <= 1e-5
            else:
                assert np.isnan(per[b, j]) if np.isnan(ref[b, j]) else per[b, j] == ref[b, j]
        if valid[b]:
            assert abs(per[b, 2] - ref[b, 2]) <= 1e-6 and abs(per[b, 3] - ref[b, 3]) <= 1e-5
        else:
            assert np.isnan(per[b, 2]) and np.isnan(per[b, 3])
        # the batch form the loop consumes: invalid -> auc = iou = 0, valid_samples = 0
        one = R.afford_batch(torch.from_numpy(per[b: b + 1]), valid[b: b + 1])
        assert one[4] == int(ref[b, 4]) and abs(one[2] - ref[b, 2]) <= 1e-6 and abs(one[3] - ref[b, 3]) <= 1e-5


def _meter_inputs(gold, device="cpu"):
    """(pred masks, label maps, affordance gt, affordance pred) of the fixture's three-sample run, on the device."""
    return [(torch.from_numpy(gold["seg_pred"][s]).to(device), torch.from_numpy(gold["seg_gt"][s]).to(device),
             torch.from_numpy(gold["aff_gt"][a: a + 1]).to(device), torch.from_numpy(gold["aff_pred"][a: a + 1]).to(device))
            for s, a in zip(gold["meter_seg_idx"], gold["meter_aff_idx"])]


def _meter_run(inputs, provider, device="cpu"):
    from interactvlm_amd import validate as V

    m = V.Meters(V._SEG_METERS + tuple((n, 1) for n in V._TASK_METERS["oafford"]), device)
    for pred, gt, agt, apred in inputs:
        inter, union, acc = V.seg_metrics(provider.seg_iou_counts(pred, gt, ignore_label=-1))
        per, valid = provider.affordance_metrics(agt, apred)
        sim, mae, auc, iou, nv = V.afford_batch(per, valid)
        gate = (nv > 0).to(torch.float64)
        for name, v in (("sim", sim), ("mae", mae), ("auc", auc), ("iou", iou), ("intersection", inter), ("union", union),
                        ("acc_iou", acc)):
            m.update(name, v, gate)
    return m


def check_meter_run(gold, m):
    """The meter buffer against the reference's AverageMeter run (used by the GPU test as well)."""
    from interactvlm_amd import validate as V

    buf = m.buf.cpu()
    got_sum = torch.cat([V.Meters.read(buf, m.rows, n)[0] for n in ("intersection", "union", "acc_iou", "sim", "mae", "auc", "iou")])
    got_cnt = torch.cat([V.Meters.read(buf, m.rows, n)[1] for n in ("intersection", "union", "acc_iou", "sim", "mae", "auc", "iou")])
    got_avg = got_sum / got_cnt
    print(f"[meters] avg {got_avg.numpy()} ref {gold['meter_avg']}")
    assert np.array_equal(got_cnt.numpy(), gold["meter_count"]) and set(gold["meter_count"]) == {2.0}  # the middle sample is skipped
    assert np.array_equal(got_sum.numpy()[:4], gold["meter_sum"][:4])  # intersection / union: integers over 4 views, exact
    np.testing.assert_allclose(got_avg.numpy()[4:], gold["meter_avg"][4:], rtol=0, atol=1e-5)
    inter, union = V.Meters.read(buf, m.rows, "intersection")[0], V.Meters.read(buf, m.rows, "union")[0]
    assert abs(float(inter[1] / (union[1] + 1e-10)) - float(gold["meter_ciou"])) <= 1e-5
    assert abs(float(got_avg[5]) - float(gold["meter_giou"])) <= 1e-5


def test_meters_follow_the_reference_average_meter_run(gold):
    check_meter_run(gold, _meter_run(_meter_inputs(gold), R))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_values(rank, i):
    return torch.tensor([0.25 * (rank + 1) + i, 1000.0 * rank + i], dtype=torch.float64), float(rank * 10 + i) + 0.5


def _reduce_worker(rank, world, port, counts, q):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from interactvlm_amd.validate import Meters

    m = Meters((("vec", 2), ("x", 1)), "cpu")
    for i in range(counts[rank]):  # unequal sample counts per rank; one gated-off update that must leave no trace
        vec, x = _rank_values(rank, i)
        m.update("vec", vec)
        m.update("x", torch.tensor(x))
    m.update("x", torch.tensor(float("nan")), gate=torch.zeros(()))
    m.reduce()
    if rank == 0:
        q.put(m.buf.tolist())
    dist.destroy_process_group()


@pytest.mark.parametrize("world,counts", [(2, (3, 1)), (3, (2, 0, 5))])
def test_meters_reduce_on_gloo_with_unequal_sample_counts(world, counts):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, counts, q)) for r in range(world)]
    for p in procs:
        p.start()
    buf = torch.tensor(q.get(timeout=120))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    vec = sum((_rank_values(r, i)[0] for r in range(world) for i in range(counts[r])), torch.zeros(2, dtype=torch.float64))
    x = sum(_rank_values(r, i)[1] for r in range(world) for i in range(counts[r]))
    n = float(sum(counts))
    assert torch.equal(buf[:, 1], torch.tensor([n, n, n], dtype=torch.float64))
    assert torch.equal(buf[:2, 0], vec) and float(buf[2, 0]) == x


# ---- validate(): the loop's bookkeeping with a stub model on the CPU ------------------------------------------------------------
class _StubModel:
    """Returns prepared masks / 3-D predictions sample by sample and records what it was called with."""
    device = "cpu"

    def __init__(self, masks, pred3d, hC=0.0, oC=0.0, forward_key=None):
        self.masks, self.pred3d, self.hC_loss_weight, self.oC_loss_weight = masks, pred3d, hC, oC
        self.forward_key, self.calls = forward_key, []

    def evaluate(self, **kw):
        i = len(self.calls)
        self.calls.append(("evaluate", kw))
        return {"output_ids": None, "pred_masks": [self.masks[i]], "pred_contact_3d": self.pred3d[i]}

    def __call__(self, **kw):
        i = len(self.calls)
        self.calls.append(("forward", kw))
        return {"pred_masks": [self.masks[i]], "gt_masks": [kw["masks_list"][0][:, 0]], self.forward_key: self.pred3d[i]}


def _sample(gold, s, gt3d, ds_name, name, answer_at=7, L=12):
    labels = torch.full((1, L), -100)
    labels[0, answer_at:] = 5
    return {"image_paths": [f"/data/img/{name}.jpg"], "images": torch.zeros(1, 4, 3, 8, 8), "images_clip": torch.zeros(1, 3, 8, 8),
            "input_ids": torch.arange(L)[None], "labels": labels, "attention_masks": torch.ones(1, L),
            "masks_list": [torch.from_numpy(gold["seg_gt"][s])[:, None]], "label_list": [torch.zeros(64, 64)],
            "gt_contact_3d_list": [gt3d], "cam_params": torch.zeros(1, 4, 5), "resize_list": [(64, 64)],
            "offset": torch.tensor([0, 1]), "sampled_classes_list": [["chair"]], "ds_name_list": [ds_name],
            "mask_paths_list": [None], "inference": True}


def test_validate_oafford_bookkeeping_generate_mode(gold):
    from interactvlm_amd import validate as V

    idx = list(zip(gold["meter_seg_idx"], gold["meter_aff_idx"]))
    masks = [torch.from_numpy(gold["seg_pred"][s]) for s, _ in idx]
    pred3d = [torch.from_numpy(gold["aff_pred"][a: a + 1]) for _, a in idx]
    samples = [_sample(gold, s, torch.from_numpy(gold["aff_gt"][a: a + 1]), "oafford_piad", f"im{k}", answer_at=5 + k)
               for k, (s, a) in enumerate(idx)]
    m = _StubModel(masks, pred3d, oC=1.0)
    out = V.validate(m, samples, "oafford_piad", "generate", metrics=R, evaluate_kwargs={"forced_new_tokens": [1, 2]})
    # inference calls: ids trimmed at the first labelled position, original sizes = resize_list, reference max_new_tokens
    for k, (kind, kw) in enumerate(m.calls):
        assert kind == "evaluate" and kw["input_ids"].shape == (1, 5 + k) and kw["original_size_list"] == [(64, 64)]
        assert kw["max_new_tokens"] == 512 and kw["forced_new_tokens"] == [1, 2] and kw["contact_type"] == "oafford_piad"
        assert kw["images"].dtype == torch.bfloat16 and kw["lift2d_dict_path"] is None
    # the middle sample is invalid: no meter saw it (count 2), but it is saved
    assert out["task"] == "oafford" and out["count"] == 2.0
    assert abs(out["giou"] - float(gold["meter_giou"])) <= 1e-5 and abs(out["ciou"] - float(gold["meter_ciou"])) <= 1e-5
    for j, name in enumerate(("sim", "mae", "auc", "iou")):
        assert abs(out["avg_" + name] - gold["meter_avg"][6 + j]) <= 1e-5
    sr = out["saved_results"]
    assert set(sr) == {"imgnames", "pred", "gt", "sim", "mae", "auc", "iou", "avg_sim", "avg_mae", "avg_auc", "avg_iou"}
    assert sr["imgnames"] == ["im0.jpg", "im1.jpg", "im2.jpg"] and sr["pred"].shape == (3, 2048) and sr["pred"].dtype == np.float32
    assert np.array_equal(sr["pred"], gold["aff_pred"][gold["meter_aff_idx"]]) and np.array_equal(sr["gt"], gold["aff_gt"][gold["meter_aff_idx"]])
    ref = gold["aff_ref"][gold["meter_aff_idx"]]
    for j, name in enumerate(("sim", "mae", "auc", "iou")):
        np.testing.assert_allclose(sr[name], ref[:, j], rtol=0, atol=1e-5)
    assert sr["auc"][1] == 0.0 and sr["iou"][1] == 0.0  # what the reference appends for the invalid sample


def test_validate_hcontact_fallback_and_forward_mode(gold):
    from interactvlm_amd import validate as V

    g = torch.Generator().manual_seed(3)
    n = 97
    pts = torch.randn(n, 3, generator=g)
    dmat = torch.cdist(pts, pts).contiguous()
    gts = [(torch.rand(1, n, generator=g) < 0.3).float() for _ in range(2)]
    preds = [torch.rand(1, n, generator=g), None]  # no [SEG] mask decoded for the second sample: zeros (evaluate.py:111-113)
    masks = [torch.from_numpy(gold["seg_pred"][s]) for s in (0, 2)]
    samples = [_sample(gold, s, gts[k], "hcontact_damon", f"h{k}") for k, s in enumerate((0, 2))]
    with pytest.raises(ValueError):
        V.validate(_StubModel(masks, preds, hC=1.0), samples, "hcontact_damon", metrics=R)
    out = V.validate(_StubModel(masks, preds, hC=1.0), samples, "hcontact_damon", "generate", dist_matrix=dmat, metrics=R)
    filled = [preds[0], torch.zeros(1, n)]
    prf = torch.stack([R.contact_prf(gts[k], filled[k])[0] for k in range(2)]).double()
    geo = [float(R.h_geo_metric_per_sample(gts[k], filled[k], dmat)[0, 0]) for k in range(2)]  # (gt, pred): evaluate.py:128
    assert out["task"] == "hcontact" and out["count"] == 2.0
    for j, name in enumerate(("f1", "precision", "recall")):
        assert abs(out["avg_" + name] - float(prf[:, j].mean())) <= 1e-6
    assert abs(out["avg_geo"] - sum(geo) / 2) <= 1e-6
    sr = out["saved_results"]
    assert set(sr) == {"imgnames", "objnames", "pred", "gt", "f1", "geo", "avg_f1", "avg_precision", "avg_recall", "avg_geo"}
    assert np.array_equal(sr["pred"][1], np.zeros(n, np.float32)) and sr["objnames"] == [[["chair"]], [["chair"]]]
    counts = [R.seg_iou_counts(masks[k], torch.from_numpy(gold["seg_gt"][s])) for k, s in enumerate((0, 2))]
    acc = torch.stack([R.seg_metrics(c)[2] for c in counts]).mean(0)
    assert abs(out["giou"] - float(acc[1])) <= 1e-9

    # 'forward' mode: model(**input_dict) with the stacked ground truth added, its own gt_masks, the task's output key
    m = _StubModel(masks, [preds[0], preds[0]], oC=1.0, forward_key="pred_object_3d_contact")
    out = V.validate(m, samples, "ocontact_x", "forward", metrics=R)
    assert [k for k, _ in m.calls] == ["forward", "forward"] and m.calls[0][1]["input_ids"].shape == (1, 12)
    assert torch.equal(m.calls[1][1]["gt_contact_3d"], gts[1]) and m.calls[0][1]["inference"] is True
    prf = torch.stack([R.o_contact_prf(gts[k], preds[0])[0] for k in range(2)]).double().mean(0)
    assert out["task"] == "ocontact" and abs(out["avg_f1"] - float(prf[0])) <= 1e-6 and abs(out["avg_recall"] - float(prf[2])) <= 1e-6
    assert set(out["saved_results"]) == {"imgnames", "pred", "gt", "f1", "avg_f1", "avg_precision", "avg_recall"}
    # a dataset name without a 3-D task still gets giou / ciou
    out = V.validate(_StubModel(masks, preds), samples, "refer_seg", "generate", metrics=R)
    assert out["task"] is None and out["count"] == 2.0 and abs(out["giou"] - float(acc[1])) <= 1e-9
