"""Host-side bookkeeping of evaluate(exact_sets=...) with the census ops replaced by a torch stand-in: the option's defaults, the
one-read layout, which images are re-run, how an evaluate_batch call is cut down to them and spliced back, and the report."""
import inspect
import math

import pytest
import torch

from interactvlm_amd import exact_sets as ES
from interactvlm_amd import model as M


class _FakePlan:
    pass


class _FakeOps:
    """contact_band_census / mask_band_census of ops.py on CPU tensors (same outputs, same dtypes)"""

    IvlmError = RuntimeError

    def __init__(self):
        self.calls = []

    def contact_band_census(self, p, thresholds, margin):
        self.calls.append(("contact", tuple(p.shape), tuple(thresholds), margin))
        thr = torch.tensor(thresholds, dtype=torch.float32)
        fin = torch.isfinite(p)
        d = (p[:, :, None] - thr[None, None, :]).abs()
        counts = torch.cat([((d <= margin) & fin[:, :, None]).sum(1), (~fin).sum(1, keepdim=True)], 1).to(torch.int32)
        mind = torch.where(fin[:, :, None], d, torch.full_like(d, math.inf)).min(1).values
        return counts, mind

    def mask_band_census(self, logits, plan, threshold, margin):
        self.calls.append(("mask", threshold, margin))
        d = (torch.sigmoid(logits) - threshold).abs()
        return torch.tensor([int((d <= margin).sum()), int((~torch.isfinite(logits)).sum())], dtype=torch.int32)


def test_option_defaults_and_validation():
    assert ES.config(None) is None and ES.config(False) is None
    assert ES.config(True) == {"thresholds": (0.5, 0.3), "margin": 1e-3, "mask_margin": 1e-3}
    c = ES.config(dict(margin=2e-3))
    assert c["margin"] == 2e-3 and c["mask_margin"] == 2e-3 and c["thresholds"] == (0.5, 0.3)
    c = ES.config(dict(thresholds=[0.5], mask_margin=5e-3))
    assert c == {"thresholds": (0.5,), "margin": 1e-3, "mask_margin": 5e-3}
    with pytest.raises(ValueError):
        ES.config(dict(marign=1e-3))
    with pytest.raises(ValueError):
        ES.config(dict(margin=-1.0))
    with pytest.raises(ValueError):
        ES.config(dict(thresholds=()))
    assert ES.PARITY_MARGIN == 1e-5
    for fn in (M.InteractVLMForCausalLM.evaluate, M.InteractVLMForCausalLM.evaluate_batch):
        assert inspect.signature(fn).parameters["exact_sets"].default is None


def _outs():
    a = torch.full((1, 50), 0.9)
    a[0, 3] = 0.5004  # in the band of 0.5 at 1e-3
    b = torch.full((1, 7), 0.1)  # nothing near a threshold: min distance 0.2 to 0.3
    c = torch.full((1, 9), 0.7)
    c[0, 0] = float("nan")
    e = torch.full((1, 5), 0.8)
    return [{"pred_contact_3d": a}, {"pred_contact_3d": b}, {"pred_contact_3d": None}, {"pred_contact_3d": c},
            {"pred_contact_3d": e}, {"pred_contact_3d": e.clone()}]


def test_layout_of_the_one_read_and_the_selection():
    ops = _FakeOps()
    logit03 = math.log(0.3 / 0.7)
    lifts = {4: ("dense", None, None), 5: ("plan", _FakePlan(), torch.tensor([[[3.0, logit03], [float("inf"), -3.0]]]))}
    parts, layout = ES.launch(_outs(), lifts, (0.5, 0.3), 1e-3, 2e-3, 0.3, ops)
    assert all(p.dtype == torch.int32 and p.dim() == 1 for p in parts)
    assert layout[2] is None and layout[4][1] == "uncensused" and layout[5][1] == "census" and layout[0][1] is None
    assert ("mask", 0.3, 2e-3) in ops.calls and sum(c[0] == "contact" for c in ops.calls) == 5
    ok, recs = ES.read([torch.tensor(True), torch.tensor(True)], parts, layout)
    assert ok is True and recs[2] is None
    assert recs[0]["in_band"] == [1, 0] and recs[0]["nonfinite"] == 0
    assert recs[0]["min_distance"][0] == pytest.approx(4e-4, rel=1e-3) and recs[0]["min_distance"][1] == pytest.approx(0.2004, rel=1e-4)
    assert recs[1]["in_band"] == [0, 0] and recs[1]["min_distance"] == [pytest.approx(0.4), pytest.approx(0.2)]
    assert recs[3]["nonfinite"] == 1 and recs[3]["in_band"] == [0, 0]
    assert recs[4]["mask_band"] == "uncensused" and recs[5]["mask_band"] == 1 and recs[5]["mask_nonfinite"] == 1
    assert [ES.undecided(r) for r in recs] == ["band", None, None, "nonfinite", "uncensused", "nonfinite"]
    assert ES.select(True, recs) == {0: "band", 3: "nonfinite", 4: "uncensused", 5: "nonfinite"}
    # a failed finite flag (tower outputs included) belongs to the call: every image is re-run, also one without contacts
    ok, recs2 = ES.read([torch.tensor(True), torch.tensor(False)], parts, layout)
    assert ok is False
    assert ES.select(ok, recs2) == {0: "band", 1: "nonfinite", 2: "nonfinite", 3: "nonfinite", 4: "uncensused", 5: "nonfinite"}
    # no flags (the guard does not apply): the census alone
    ok, recs3 = ES.read([], parts, layout)
    assert ok is True and recs3 == recs
    assert ES.read([], [], [None]) == (True, [None])


def test_report():
    rec = {"in_band": [0, 0], "nonfinite": 0, "min_distance": [0.25, 0.125], "mask_band": None, "mask_nonfinite": 0}
    assert ES.report(rec, 1e-3, 2) == {"certified": True, "escalated": False, "margin": 1e-3, "in_band": [0, 0],
                                       "min_distance": [0.25, 0.125], "mask_band": None}
    hot = dict(rec, in_band=[2, 0], min_distance=[1e-4, 0.125])
    r = ES.report(hot, 1e-3, 2, parity_rec=rec, reason="band")
    assert r["escalated"] is True and r["certified"] is True and r["reason"] == "band" and r["in_band"] == [2, 0]
    assert r["parity"] == {"in_band": [0, 0], "min_distance": [0.25, 0.125], "mask_band": None, "margin": 1e-5}
    r = ES.report(hot, 1e-3, 2, parity_rec=dict(rec, in_band=[1, 0]), reason="band")
    assert r["escalated"] is True and r["certified"] is False  # even the parity pass sits within its error of a threshold
    none = ES.report(None, 1e-3, 2)  # no mask decoded: no sets
    assert none["certified"] is True and none["in_band"] == [0, 0] and none["min_distance"] == [math.inf, math.inf]


def test_subset_of_an_evaluate_batch_call():
    B = 4
    ic, im = torch.arange(B).float().view(B, 1), torch.arange(B).float().view(B, 1, 1)
    ids = [torch.tensor([b]) for b in range(B)]
    cams = torch.arange(B).float().view(B, 1)
    sizes = [(b, b) for b in range(B)]
    args = (ic, im, ids, cams, sizes, sizes, "hcontact", 32, [5, 6, 7], 2, None, None)
    s = ES.subset_batch_args(args, [1, 3])
    assert s[0].flatten().tolist() == [1.0, 3.0] and s[1].flatten().tolist() == [1.0, 3.0]
    assert [int(t) for t in s[2]] == [1, 3] and [float(c) for c in s[3]] == [1.0, 3.0] and s[4] == [(1, 1), (3, 3)] == s[5]
    assert s[6] == "hcontact" and s[7] == 32 and s[8] == [5, 6, 7] and s[9] == 2 and s[10] is None and s[11] is None
    # one picture for all prompts, per-prompt contact types / forced answers / table paths / embeddings
    emb = [torch.full((1,), float(b)) for b in range(B)]
    args = (ic[:1], im, ids, [cams[b] for b in range(B)], sizes, sizes, ["hcontact", "ocontact"] * 2, 32,
            [[b] for b in range(B)], 2, [None, "a.pkl", None, "b.pkl"], emb)
    s = ES.subset_batch_args(args, [3, 1])
    assert s[0].shape[0] == 1 and s[1].flatten().tolist() == [3.0, 1.0] and s[6] == ["ocontact", "ocontact"]
    assert s[8] == [[3], [1]] and s[10] == ["b.pkl", "a.pkl"] and [float(e) for e in s[11]] == [3.0, 1.0]
    shared = ES.subset_batch_args(args[:11] + (emb[0],), [2])
    assert shared[11] is emb[0] and shared[1].flatten().tolist() == [2.0]
    assert ES.splice(["a", "b", "c", "d"], [1, 3], ["B", "D"]) == ["a", "B", "c", "D"]


def _bare_model(monkeypatch, precision="default"):
    m = object.__new__(M.InteractVLMForCausalLM)
    m.fp8, m.precision, m.nonfinite_guard = False, precision, False
    m.object_3d_contact_predictor = None
    m.log = []

    def recompute(target, fn, unpacked_decode=True):
        m.log.append((target, unpacked_decode))
        return fn()

    m._recompute_in = recompute
    monkeypatch.setattr(M, "ops", _FakeOps())
    return m


def test_pass_reruns_only_the_undecided_images_and_splices_them_back(monkeypatch):
    m = _bare_model(monkeypatch)
    first = _outs()[:2] + [{"pred_contact_3d": torch.full((1, 5), 0.8)}]
    asked = []

    def rerun(idx):
        asked.append(list(idx))
        return [{"pred_contact_3d": torch.full((1, 50), 0.9), "rerun_of": i} for i in idx]

    outs = m._exact_sets_pass(ES.config(True), lambda: first, rerun)
    assert asked == [[0]] and m.log == [("parity", False)]
    assert outs[0]["rerun_of"] == 0 and outs[1] is first[1] and outs[2] is first[2]
    assert outs[0]["exact_sets"]["escalated"] and outs[0]["exact_sets"]["certified"] and outs[0]["exact_sets"]["reason"] == "band"
    assert outs[0]["exact_sets"]["in_band"] == [1, 0] and outs[0]["exact_sets"]["parity"]["in_band"] == [0, 0]
    for o in outs[1:]:
        assert o["exact_sets"] == dict(o["exact_sets"], certified=True, escalated=False, margin=1e-3, in_band=[0, 0])
    assert M.ops.calls[-1] == ("contact", (1, 50), (0.5, 0.3), 1e-5)  # the re-run's own census, at the parity margin
    assert m._lift_log is None and getattr(m, "_in_guard", False) is False
    # band empty everywhere (margin 0): nothing is re-run
    m.log.clear()
    outs = m._exact_sets_pass(ES.config(dict(margin=0.0)), lambda: _outs()[:2], lambda idx: pytest.fail("re-run"))
    assert m.log == [] and [o["exact_sets"]["escalated"] for o in outs] == [False, False]


def test_pass_of_a_model_already_in_parity_and_unsupported_modes(monkeypatch):
    m = _bare_model(monkeypatch, precision="parity")
    outs = m._exact_sets_pass(ES.config(True), lambda: _outs()[:1], lambda idx: pytest.fail("a parity model is never re-run"))
    assert outs[0]["exact_sets"]["margin"] == 1e-5 and outs[0]["exact_sets"]["escalated"] is False
    assert outs[0]["exact_sets"]["certified"] is True  # 0.5004 is outside the parity mode's own band
    m = _bare_model(monkeypatch, precision="bf16")
    with pytest.raises(Exception, match="no error bound"):
        m._exact_sets_pass(ES.config(True), lambda: _outs()[:1], lambda idx: [])


def test_census_ops_raise_on_cpu_tensors():
    from interactvlm_amd import _lib, ops

    with pytest.raises(_lib.IvlmError):
        ops.contact_band_census(torch.zeros(1, 8), (0.5, 0.3), 1e-3)
    m = object.__new__(M.InteractVLMForCausalLM)
    m.fp8, m.precision, m.nonfinite_guard, m.object_3d_contact_predictor = False, "default", False, None
    with pytest.raises(_lib.IvlmError):  # evaluate(exact_sets=...) on CPU results: no fallback, as everywhere else
        m._exact_sets_pass(ES.config(True), lambda: [{"pred_contact_3d": torch.zeros(1, 8)}], lambda idx: [])


def test_rows_of_one_buffer_share_a_census_launch():
    """the batched body lift returns views of ONE [n, Nv] tensor: one launch with B = n, the same records as per-image launches"""
    ops = _FakeOps()
    buf = torch.full((3, 20), 0.9)
    buf[1, 4] = 0.5004
    buf[2, 0] = float("nan")
    outs = [{"pred_contact_3d": buf[i: i + 1]} for i in range(3)] + [{"pred_contact_3d": torch.full((1, 20), 0.2)}]
    parts, layout = ES.launch(outs, {}, (0.5, 0.3), 1e-3, 1e-3, 0.3, ops)
    assert [c[1] for c in ops.calls] == [(3, 20), (1, 20)]
    _, recs = ES.read([], parts, layout)
    ops2 = _FakeOps()
    parts2, layout2 = ES.launch([{"pred_contact_3d": o["pred_contact_3d"].clone()} for o in outs], {}, (0.5, 0.3), 1e-3, 1e-3, 0.3, ops2)
    assert len(ops2.calls) == 4 and ES.read([], parts2, layout2)[1] == recs
    assert [ES.undecided(r) for r in recs] == [None, "band", "nonfinite", None]


def test_nonfinite_fallback_keyword_is_validated():
    with pytest.raises(ValueError, match="nonfinite_fallback"):
        M.InteractVLMForCausalLM(None, {}, "cpu", nonfinite_fallback="fp32")


class _StubModel:
    """what validate() needs of a model: evaluate() returning canned results with an exact_sets report"""
    device = "cpu"
    hC_loss_weight, oC_loss_weight = 0.0, 0.0

    def __init__(self, escalated):
        self.escalated, self.seen = list(escalated), []

    def evaluate(self, **kw):
        self.seen.append(kw.get("exact_sets", "absent"))
        out = {"pred_masks": [torch.ones(2, 4, 4)], "pred_contact_3d": torch.zeros(1, 8)}
        if "exact_sets" in kw:
            out["exact_sets"] = {"escalated": self.escalated[len(self.seen) - 1], "certified": True}
        return out


class _StubMetrics:
    @staticmethod
    def seg_iou_counts(pred, gt, ignore_label=255):
        return torch.ones(pred.shape[0], 3, 2, dtype=torch.int32)


def _sample():
    return {"images_clip": torch.zeros(1, 3, 2, 2), "images": torch.zeros(1, 2, 3, 4, 4), "input_ids": torch.ones(1, 6, dtype=torch.long),
            "cam_params": torch.zeros(1, 2, 5), "resize_list": [(4, 4)], "ds_name_list": ["seg"],
            "masks_list": [torch.ones(2, 4, 4)], "gt_contact_3d_list": [torch.zeros(1, 8)]}


def test_validate_forwards_exact_sets_and_reports_the_rerun_rate():
    from interactvlm_amd.validate import validate

    m = _StubModel([True, False, False, True])
    res = validate(m, [_sample() for _ in range(4)], "seg", metrics=_StubMetrics, exact_sets=dict(margin=2e-3))
    assert m.seen == [dict(margin=2e-3)] * 4
    assert res["saved_results"]["escalated"] == [True, False, False, True] and res["rerun_rate"] == 0.5
    m = _StubModel([])
    res = validate(m, [_sample()], "seg", metrics=_StubMetrics)  # option off: not forwarded, nothing added
    assert m.seen == ["absent"] and "rerun_rate" not in res and "escalated" not in res["saved_results"]
    with pytest.raises(ValueError, match="generate"):
        validate(m, [_sample()], "seg", inference_type="forward", metrics=_StubMetrics, exact_sets=True)
