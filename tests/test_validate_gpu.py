"""validate() on the device: the two metric kernels against the reference's numbers (tests/golden/validate_metrics.npz) and against
the CPU restatement (tests/_validate_ref.py) at real sizes, bit-reproducibility, the loop end to end on the tiny synthetic model.
Tolerances: counts and valid flags exact; AUC 1e-6 (an integer ratio, only the fp32 output rounds); SIM / MAE / aIoU / giou / ciou
1e-5 absolute (the bound tests/test_metrics_gpu.py uses for fp32 sums of this length)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "validate_metrics.npz"))


def _check_afford(per, valid, ref_per, ref_valid, tag):
    """per [B,4] / valid [B] from the kernel against a reference of the same layout (NaN / inf where the reference's are)."""
    per, ref_per = np.asarray(per, np.float64), np.asarray(ref_per, np.float64)
    assert np.array_equal(np.asarray(valid), np.asarray(ref_valid)), tag
    for b in range(per.shape[0]):
        print(f"[{tag} row {b}] got {per[b]} ref {ref_per[b]}")
        for j, tol in ((0, 1e-5), (1, 1e-5), (2, 1e-6), (3, 1e-5)):
            r, g = ref_per[b, j], per[b, j]
            if np.isfinite(r):
                assert abs(g - r) <= tol, (tag, b, j, g, r)
            else:
                assert (np.isnan(g) if np.isnan(r) else g == r), (tag, b, j, g, r)


def test_kernels_vs_reference_golden(hip_lib, cuda, gold):
    import torch

    from interactvlm_amd import ops

    for c in range(gold["seg_pred"].shape[0]):
        pred, gt = torch.from_numpy(gold["seg_pred"][c]).to(cuda), torch.from_numpy(gold["seg_gt"][c])
        assert np.array_equal(ops.seg_iou_counts(pred, gt.to(cuda), ignore_label=-1).cpu().numpy(), gold["seg_counts"][c])
        assert np.array_equal(ops.seg_iou_counts(pred, gt.to(cuda)).cpu().numpy(), gold["seg_counts_ign255"][c])  # default label 255
        assert np.array_equal(ops.seg_iou_counts(pred, gt.float().to(cuda), ignore_label=-1).cpu().numpy(), gold["seg_counts"][c])
        if not bool((gt < 0).any()):
            assert np.array_equal(ops.seg_iou_counts(pred, gt.to(torch.uint8).to(cuda)).cpu().numpy(), gold["seg_counts_ign255"][c])
    gt, pred, ref = torch.from_numpy(gold["aff_gt"]).to(cuda), torch.from_numpy(gold["aff_pred"]).to(cuda), gold["aff_ref"]
    per, valid = ops.affordance_metrics(gt, pred)
    per, valid = per.cpu().numpy(), valid.cpu().numpy()
    exp = ref[:, :4].copy()
    exp[ref[:, 4] == 0, 2:] = np.nan  # the kernel reports NaN where the reference's batch mean reports 0 of 0 valid samples
    _check_afford(per, valid, exp, ref[:, 4].astype(np.int32), "golden")
    assert ops.o_contact_prf is ops.contact_prf


@pytest.mark.parametrize("shape", [(4, 1024, 1024), (3, 480, 640), (2, 33, 61)])
def test_seg_iou_counts_real_size_every_label_dtype(hip_lib, cuda, shape):
    import torch

    import _validate_ref as R
    from interactvlm_amd import ops

    g = torch.Generator().manual_seed(shape[1])
    pred = torch.randn(shape, generator=g)
    gt = (torch.rand(shape, generator=g) < 0.3).to(torch.int32)
    sel = torch.rand(shape, generator=g)
    gt[sel < 0.07] = 255
    gt[(sel >= 0.07) & (sel < 0.09)] = 3
    gt[0, : shape[1] // 5] = 255
    exp = R.seg_iou_counts(pred, gt, ignore_label=255)
    assert int(exp.sum()) > 0
    for dtype in (torch.uint8, torch.int32, torch.float32):
        a = ops.seg_iou_counts(pred.to(cuda), gt.to(dtype).to(cuda))
        b = ops.seg_iou_counts(pred.to(cuda), gt.to(dtype).to(cuda))
        assert torch.equal(a.cpu(), exp), dtype
        assert torch.equal(a, b)  # the same bits from run to run
    # a view of a larger buffer that starts off a 16-byte boundary takes the element-wise path: same counts
    flat = torch.zeros(pred.numel() + 1, device=cuda)
    flat[1:] = pred.reshape(-1).to(cuda)
    assert torch.equal(ops.seg_iou_counts(flat[1:].view(shape), gt.to(cuda)).cpu(), exp)


def test_affordance_metrics_real_size_and_limits(hip_lib, cuda):
    import torch

    import _validate_ref as R
    from interactvlm_amd import _lib, ops

    g = torch.Generator().manual_seed(7)
    B, n = 16, 2048
    gt = torch.rand(B, n, generator=g)
    pred = (0.5 * gt + 0.5 * torch.rand(B, n, generator=g)).clamp(0, 1)
    pred[3] = torch.floor(pred[3] * 4) / 4  # ties
    gt[5] = 0.2                             # single class
    pred[9, 100] = float("nan")
    exp, exp_valid = R.affordance_metrics(gt, pred)
    per, valid = ops.affordance_metrics(gt.to(cuda), pred.to(cuda))
    per2, valid2 = ops.affordance_metrics(gt.to(cuda), pred.to(cuda))
    _check_afford(per.cpu().numpy(), valid.cpu().numpy(), exp.numpy(), exp_valid.numpy(), "B16")
    assert torch.equal(per.view(torch.int32), per2.view(torch.int32)) and torch.equal(valid, valid2)  # bit-identical runs
    # other row lengths up to the limit of the header; beyond it the error code, before any launch
    for n2 in (1, 5, 777, 4096):
        gt2, pred2 = torch.rand(2, n2, generator=g), torch.rand(2, n2, generator=g)
        e, ev = R.affordance_metrics(gt2, pred2)
        p, v = ops.affordance_metrics(gt2.to(cuda), pred2.to(cuda))
        _check_afford(p.cpu().numpy(), v.cpu().numpy(), e.numpy(), ev.numpy(), f"n{n2}")
    big = torch.rand(1, 4097, device=cuda)
    out, vflag = torch.empty(1, 4, device=cuda), torch.empty(1, dtype=torch.int32, device=cuda)
    thr = ops.afford_thresholds(cuda)
    rc = hip_lib.ivlm_afford_metrics(big.data_ptr(), big.data_ptr(), 1, 4097, thr.data_ptr(), 20, 2048.0, out.data_ptr(),
                                     vflag.data_ptr(), 0)
    assert rc == -4  # IVLM_ERR_UNSUPPORTED
    with pytest.raises(_lib.IvlmError):
        ops.affordance_metrics(big, big)


def test_meters_on_device_follow_the_reference_run_without_synchronising(hip_lib, cuda, gold):
    import torch

    from interactvlm_amd import ops
    from test_validate_cpu import _meter_inputs, _meter_run, check_meter_run

    inputs = _meter_inputs(gold, cuda)
    check_meter_run(gold, _meter_run(inputs, ops, cuda))  # (also warms every launch and the threshold upload)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device=cuda).item()  # a synchronisation: the mode must refuse it
        except RuntimeError:
            honoured = True
        assert honoured, "this torch build does not honour set_sync_debug_mode('error')"
        m = _meter_run(inputs, ops, cuda)  # kernels + seg_metrics + afford_batch + every meter update: nothing may synchronise
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    check_meter_run(gold, m)


# ---- validate() end to end on the tiny synthetic model ------------------------------------------------------------------------------
def _cpu(x):
    import torch

    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_cpu(v) for v in x]
    return x


class _Recorder:
    """The model, keeping what it returned."""

    def __init__(self, m):
        self.m, self.outs, self.device = m, [], m.device
        self.hC_loss_weight, self.oC_loss_weight = m.hC_loss_weight, m.oC_loss_weight

    def evaluate(self, **kw):
        self.outs.append(self.m.evaluate(**kw))
        return self.outs[-1]

    def __call__(self, **kw):
        self.outs.append(self.m(**kw))
        return self.outs[-1]


class _Replay:
    """A CPU stand-in that returns the recorded outputs: validate(metrics=<restatement>) over it is the expected result."""
    device = "cpu"

    def __init__(self, rec):
        self.outs, self.i = [_cpu(o) for o in rec.outs], 0
        self.hC_loss_weight, self.oC_loss_weight = rec.hC_loss_weight, rec.oC_loss_weight

    def evaluate(self, **kw):
        self.i += 1
        return self.outs[self.i - 1]

    __call__ = evaluate


@pytest.fixture(scope="module")
def tiny(hip_lib, cuda, tmp_path_factory):
    import torch

    from interactvlm_amd import model as M
    from interactvlm_amd import render, synth, synthetic
    from interactvlm_amd import weights as Wt

    tmp = tmp_path_factory.mktemp("validate")
    cfg = synthetic.config_tiny()
    cfg.oC_loss_weight = 1.0
    w = Wt.synth_weights(Wt.ivlm_spec(cfg))
    tables = synth.synth_mesh_tables(4, 1024, 1024, 6890, fg=0.4, seed=0, patch=8)
    m = M.InteractVLMForCausalLM(cfg, w, cuda, lift_tables=tables)
    # object tables: a 642-vertex mesh lift (lift2d_dict.pkl for 'generate', p2vmap_*.npz for 'forward') and 2048-point maps
    nv = 642
    vid, bary = synth.synth_mesh_tables(4, 1024, 1024, nv, fg=0.4, seed=3, patch=8)
    pkl = str(tmp / "lift2d_dict.pkl")
    render.save_lift2d_dict(pkl, torch.from_numpy(vid), torch.from_numpy(bary), nv)
    pid = synth.synth_point_maps(1, 4, 1024, 1024, 2048, fg=0.3, seed=5)[0]
    mask_paths = []
    for v in range(4):
        mp = str(tmp / f"chair_mask_{v}.png")
        np.savez(mp.replace("mask", "p2vmap").replace(".png", ".npz"), pixel_to_vertices_map=vid[v], bary_coords_map=bary[v],
                 num_vertices=nv)
        np.savez(mp.replace("mask", "p2pmap")[:-4] + ".npz", mapping=pid[v])
        mask_paths.append(mp)
    g = torch.Generator().manual_seed(1)
    pts = torch.randn(6890, 3, generator=g).to(cuda)
    dmat = torch.cdist(pts, pts).contiguous()
    return dict(cfg=cfg, model=m, nv=nv, pkl=pkl, mask_paths=mask_paths, dist=dmat)


def _samples(tiny, ds_name, mode, n_samples=3):
    """collate_fn-shaped dicts (batch 1): prompt + forced answer as input_ids, the answer positions labelled."""
    import torch

    from interactvlm_amd import synthetic

    cfg = tiny["cfg"]
    task = "hcontact" if "hcontact" in ds_name else ("oafford" if "oafford" in ds_name else "ocontact")
    n3d = 6890 if task == "hcontact" else (2048 if (task == "oafford" and mode == "forward") else tiny["nv"])
    out, forced = [], None
    for k in range(n_samples):
        ids, forced_k = synthetic.prompt_ids(cfg, n_prompt=40, n_answer=6, seed=k)
        forced = forced if forced is not None else forced_k  # one answer for every sample (evaluate_kwargs is per run)
        full = torch.cat([ids, torch.tensor(forced)[None]], 1)
        labels = torch.full_like(full, -100)
        labels[0, ids.shape[1]:] = full[0, ids.shape[1]:]
        ic, im = synthetic.images(cfg, "cpu", seed=k)
        g = torch.Generator().manual_seed(100 + k)
        gt_mask = (torch.rand(4, 1, 1024, 1024, generator=g) < 0.4).float()
        gt_mask[:, :, :100] = -1.0  # the ignore band of the reference's label maps
        gt3d = torch.rand(1, n3d, generator=g)
        if task != "oafford":
            gt3d = (gt3d < 0.3).float()
        elif k == 1:
            gt3d = torch.zeros(1, n3d)  # no valid affordance statistics: the sample must not reach any meter
        paths = None
        if task != "hcontact":
            paths = tiny["pkl"] if mode == "generate" else tiny["mask_paths"]
        out.append({"image_paths": [f"/data/{ds_name}/{k}.jpg"], "images": im.float(), "images_clip": ic.float(),
                    "input_ids": full, "labels": labels, "attention_masks": torch.ones_like(full),
                    "masks_list": [gt_mask], "label_list": [torch.zeros(1024, 1024)], "gt_contact_3d_list": [gt3d],
                    "cam_params": synthetic.human_cam_params(), "resize_list": [(1024, 1024)], "offset": torch.tensor([0, 1]),
                    "sampled_classes_list": [["chair"]], "ds_name_list": [ds_name], "mask_paths_list": [paths], "inference": True})
    return out, forced


@pytest.mark.parametrize("mode", ["generate", "forward"])
@pytest.mark.parametrize("ds_name", ["hcontact_damon", "oafford_piad", "ocontact_pico"])
def test_validate_end_to_end_vs_restatement_on_the_models_own_outputs(tiny, ds_name, mode):
    import _validate_ref as R
    from interactvlm_amd import validate as V

    samples, forced = _samples(tiny, ds_name, mode)
    rec = _Recorder(tiny["model"])
    kw = dict(evaluate_kwargs={"forced_new_tokens": forced, "max_new_tokens": 32}) if mode == "generate" else {}
    got = V.validate(rec, samples, ds_name, mode, dist_matrix=tiny["dist"], **kw)
    assert len(rec.outs) == len(samples)
    exp = V.validate(_Replay(rec), samples, ds_name, mode, dist_matrix=tiny["dist"].cpu(), metrics=R, **kw)
    print(f"[validate {ds_name} {mode}] got { {k: v for k, v in got.items() if k != 'saved_results'} }")
    print(f"[validate {ds_name} {mode}] exp { {k: v for k, v in exp.items() if k != 'saved_results'} }")
    assert got["task"] == exp["task"] == ds_name.split("_")[0] and got["count"] == exp["count"]
    assert got["count"] == (2.0 if got["task"] == "oafford" else 3.0)
    for k in exp:
        if k in ("giou", "ciou") or k.startswith("avg_"):
            tol = 1e-6 if k == "avg_auc" else 1e-5
            assert abs(got[k] - exp[k]) <= tol, (k, got[k], exp[k])
    for name, m in exp["meters"].items():  # intersection / union are integer counts over 4 views: exact
        if name in ("intersection", "union"):
            assert got["meters"][name] == m
    sg, se = got["saved_results"], exp["saved_results"]
    assert set(sg) == set(se) and np.array_equal(sg["pred"], se["pred"]) and np.array_equal(sg["gt"], se["gt"])
    assert sg["imgnames"] == se["imgnames"]


def test_sharded_validation_gives_the_meters_of_one_rank(tiny):
    """Two ranks' contiguous shards (dist.evaluate_sharded), each scored by validate(), then summed as Meters.reduce does: the
    meters of one rank over all samples."""
    import torch

    from interactvlm_amd import dist as D
    from interactvlm_amd import validate as V

    samples, forced = _samples(tiny, "hcontact_damon", "generate", n_samples=3)
    kw = dict(dist_matrix=tiny["dist"], evaluate_kwargs={"forced_new_tokens": forced, "max_new_tokens": 32})
    whole = V.validate(tiny["model"], samples, "hcontact_damon", "generate", **kw)
    total, rows = {}, []
    for rank in range(2):
        def chunk(idx):
            if not idx:
                return torch.zeros(0, 6890)
            r = V.validate(tiny["model"], [samples[i] for i in idx], "hcontact_damon", "generate", **kw)
            for name, m in r["meters"].items():
                t = total.setdefault(name, {"sum": [0.0] * len(m["sum"]), "count": 0.0})
                t["sum"] = [a + b for a, b in zip(t["sum"], m["sum"])]
                t["count"] += m["count"]
            return torch.from_numpy(r["saved_results"]["pred"])
        rows.append(D.evaluate_sharded(len(samples), 2, chunk, rank=rank, world=2))
    assert np.array_equal(torch.cat(rows).numpy(), whole["saved_results"]["pred"])
    for name, m in whole["meters"].items():
        assert total[name]["count"] == m["count"] == 3.0
        np.testing.assert_allclose(total[name]["sum"], m["sum"], rtol=1e-12, atol=0)
