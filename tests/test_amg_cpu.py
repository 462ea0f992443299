"""The automatic mask generator without a GPU: the float64 restatement of tests/_amg_ref.py against the records of the reference's own
SamAutomaticMaskGenerator.generate (tests/golden/amg_select.npz), the point grid, the run-length encoding, the NMS restatement's
rules, every Python refusal before the library loads, and the two new C entry points' prototypes."""
import os

import numpy as np
import pytest
import torch

import _amg_ref as A
from interactvlm_amd import _lib, sam_amg
from interactvlm_amd.sam_amg import AutoMasks, SamAutomaticMaskGenerator, build_point_grid


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "amg_select.npz"))


@pytest.fixture(scope="module")
def restated():
    low, iou = A.candidates()
    return A.select_ref(low, iou, A.golden_points(), A.IMG, A.INPUT, A.PHOTO)


# ---- the restatement against the reference's records ---------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_records(golden, restated):
    assert int(golden["seed"]) == A.SEED
    n, n_iou, n_stab, n_kept = golden["n_filters"].tolist()
    assert (n, n_iou, n_kept) == (A.SIDE * A.SIDE * 3, restated["n_iou"], len(restated["index"])) and n_stab == restated["n_stability"]
    assert n > n_iou > n_stab > n_kept >= 3
    assert np.array_equal(restated["index"], golden["index"])  # the set and its order
    b = restated["boxes"]
    assert np.array_equal(np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1), golden["bbox"])
    assert np.array_equal(restated["areas"], golden["area"])
    assert np.array_equal(restated["points"], golden["point_coords"])
    assert restated["stability"].dtype == np.float32
    assert np.array_equal(restated["stability"].view(np.uint32), golden["stability_score"].view(np.uint32))
    assert np.array_equal(restated["predicted_iou"].view(np.uint32), golden["predicted_iou"].view(np.uint32))
    assert bool((np.diff(restated["predicted_iou"]) <= 0).all())


def test_restated_run_lengths_are_the_reference_s(golden, restated):
    off = golden["rle_offsets"]
    for k, mask in enumerate(restated["masks"]):
        want = golden["rle_counts"][off[k]: off[k + 1]].tolist()
        assert A.rle_encode(mask) == want, k
        assert np.array_equal(A.rle_decode(want, A.PHOTO), mask) and sum(want[1::2]) == int(golden["area"][k])


def test_golden_decisions_keep_their_distance(golden):
    """what the golden script asserted, read back from the data: no decision of the kept set sits at its threshold"""
    low, iou = A.candidates()
    assert float(np.abs(iou.astype(np.float64) - A.IOU_THRESH).min()) >= A.MARGIN
    few, many, in_band = A.golden_band()
    assert in_band.sum() <= 0.2 * in_band.size
    kept = golden["index"]
    assert np.array_equal(few[kept, 3:7], many[kept, 3:7])
    margins = []
    A.select_ref(low, iou, A.golden_points(), A.IMG, A.INPUT, A.PHOTO, margins=margins)
    assert min(margins) >= A.MARGIN


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 32])
def test_point_grid(n):
    g = build_point_grid(n)
    assert g.shape == (n * n, 2) and g.dtype == np.float64
    assert float(np.abs(g - A.grid(n)).max()) <= 2.0 ** -52  # linspace against (k + 0.5) / n: one rounding
    if n == 1:
        assert g.tolist() == [[0.5, 0.5]]
    if n == 2:
        assert g.tolist() == [[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]]  # x fastest


def test_grid_scaled_to_the_photo_is_the_reference_s_points(golden):
    pts = build_point_grid(A.SIDE) * np.array([[A.PHOTO[1], A.PHOTO[0]]], dtype=np.float64)
    assert np.array_equal(pts[golden["index"] // 3], golden["point_coords"])


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------
def _rle_masks():
    rng = np.random.default_rng(11)
    m = rng.random((6, 7, 5)) < 0.5
    m[0, 0, 0] = True    # the first pixel set: the counts start with 0
    m[1, 0, 0] = False
    m[2] = False         # empty
    m[3] = True          # full
    m[4] = False
    m[4, -1, -1] = True  # only the last pixel
    return m


def test_run_length_round_trip():
    masks = _rle_masks()
    for k, m in enumerate(masks):
        counts = A.rle_encode(m)
        assert sum(counts) == m.size and np.array_equal(A.rle_decode(counts, m.shape), m), k
        assert all(c > 0 for c in counts[1:]) and sum(counts[1::2]) == int(m.sum())
    assert A.rle_encode(masks[0])[0] == 0 and A.rle_encode(masks[1])[0] > 0
    assert A.rle_encode(masks[2]) == [35] and A.rle_encode(masks[3]) == [0, 35] and A.rle_encode(masks[4]) == [34, 1]
    assert A.rle_encode(np.array([[0, 1], [1, 1]], bool)) == [1, 3]
    assert A.rle_encode(np.array([[0, 1], [1, 0]], bool)) == [1, 2, 1]  # column-major: (0,0) (1,0) (0,1) (1,1)


def test_run_lengths_of_the_module_on_cpu_tensors():
    masks = _rle_masks()
    got = sam_amg.run_lengths(torch.from_numpy(masks))
    assert got == [A.rle_encode(m) for m in masks]
    assert sam_amg.run_lengths(torch.zeros(0, 4, 4, dtype=torch.bool)) == []


def test_records_of_cpu_tensors_have_the_reference_s_keys_and_types():
    masks = torch.from_numpy(_rle_masks()[:2])
    am = AutoMasks(masks, torch.tensor([[0, 0, 4, 6], [1, 0, 4, 6]], dtype=torch.int32), masks.sum((1, 2)).to(torch.int32),
                   torch.tensor([0.9, 0.8]), torch.tensor([0.99, 0.97]), torch.tensor([[1.5, 2.5], [3.5, 4.5]], dtype=torch.float64),
                   torch.tensor([4, 1]), torch.zeros(2, 4, 4))
    for mode in ("binary_mask", "uncompressed_rle"):
        recs = am.records(mode)
        assert len(recs) == 2
        for k, r in enumerate(recs):
            assert set(r) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
            assert type(r["area"]) is int and r["area"] == int(masks[k].sum()) and r["crop_box"] == [0, 0, 5, 7]
            assert all(type(v) is int for v in r["bbox"]) and type(r["predicted_iou"]) is float and type(r["stability_score"]) is float
            assert r["point_coords"] == [[1.5, 2.5], [3.5, 4.5]][k: k + 1]
            if mode == "binary_mask":
                assert r["segmentation"].dtype == np.bool_ and np.array_equal(r["segmentation"], masks[k].numpy())
            else:
                assert r["segmentation"]["size"] == [7, 5]
                assert np.array_equal(A.rle_decode(r["segmentation"]["counts"], (7, 5)), masks[k].numpy())
    assert recs[1]["bbox"] == [1, 0, 3, 6]
    with pytest.raises(ValueError, match="output_mode"):
        am.records("coco_rle")
    assert int(am.match(masks[1])) == 1 and int(am.match(masks[0].float())) == 0


# ---- the NMS restatement --------------------------------------------------------------------------------------------------------------
def test_nms_restatement_rules():
    f = lambda rows: np.array(rows, dtype=np.float32)
    # the chain A > B > C: B is suppressed by A and therefore does not suppress C
    chain = f([[0, 0, 100, 100], [0, 0, 100, 80], [0, 0, 100, 60]])
    assert A.box_iou32(chain[0], chain[1]) > 0.7 and A.box_iou32(chain[1], chain[2]) > 0.7 and A.box_iou32(chain[0], chain[2]) < 0.7
    assert A.nms_ordered(chain, 0.7).tolist() == [1, 0, 1]
    # an IoU equal to the threshold is kept: 50 / 100 == 0.5 exactly
    assert A.box_iou32([0, 0, 10, 10], [0, 0, 10, 5]) == np.float32(0.5)
    assert A.nms_ordered(f([[0, 0, 10, 10], [0, 0, 10, 5]]), 0.5).tolist() == [1, 1]
    assert A.nms_ordered(f([[0, 0, 10, 10], [0, 0, 10, 5]]), 0.4999).tolist() == [1, 0]
    # degenerate boxes: 0 / 0 suppresses nothing
    assert A.nms_ordered(f([[0, 0, 0, 0]] * 3), 0.7).tolist() == [1, 1, 1]
    # an invalid row neither keeps nor suppresses
    same = f([[0, 0, 10, 10]] * 3)
    assert A.nms_ordered(same, 0.7).tolist() == [1, 0, 0]
    assert A.nms_ordered(same, 0.7, valid=[0, 1, 1]).tolist() == [0, 1, 0]
    # tied scores go to the lower index
    assert A.score_order([0.5, 0.9, 0.9, 0.5]) == [1, 2, 0, 3]
    assert A.nms(same, [0.5, 0.9, 0.9], 0.7).tolist() == [1]
    assert A.nms(f([[0, 0, 10, 10], [20, 20, 30, 30], [0, 0, 10, 10]]), [0.5, 0.9, 0.5], 0.7).tolist() == [1, 0]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load the library fails the test: a refusal has to come before it"""
    def boom():
        raise AssertionError("the library was loaded before the argument check")

    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("kw, msg", [
    (dict(crop_n_layers=1), "crop_n_layers"),
    (dict(min_mask_region_area=100), "min_mask_region_area"),
    (dict(output_mode="coco_rle"), "output_mode"),
    (dict(output_mode="polygons"), "output_mode"),
    (dict(point_grid=np.zeros((4, 2))), "points_per_side / point_grid"),
    (dict(points_per_side=None), "points_per_side / point_grid"),
    (dict(points_per_side=0), "points_per_side"),
    (dict(points_per_side=-3), "points_per_side"),
    (dict(points_per_batch=0), "points_per_batch"),
    (dict(points_per_batch=-1), "points_per_batch"),
    (dict(points_per_side=None, point_grid=np.zeros((4, 3))), "point_grid"),
])
def test_constructor_refuses_before_the_library_loads(no_library, kw, msg):
    with pytest.raises(ValueError, match=msg):
        SamAutomaticMaskGenerator(object(), **kw)


def test_constructor_accepts_the_reference_s_defaults_and_an_explicit_grid(no_library):
    g = SamAutomaticMaskGenerator(object())
    assert g.point_grid.shape == (1024, 2) and g.points_per_batch == 64
    assert (g.pred_iou_thresh, g.stability_score_thresh, g.stability_score_offset, g.box_nms_thresh, g.mask_threshold) == \
        (0.88, 0.95, 1.0, 0.7, 0.0)
    g = SamAutomaticMaskGenerator(object(), points_per_side=None, point_grid=[[0.5, 0.5], [0.25, 0.75]], output_mode="uncompressed_rle")
    assert g.point_grid.dtype == np.float64 and g.point_grid.shape == (2, 2)
    with pytest.raises(ValueError, match="n_per_side"):
        build_point_grid(0)


def test_ops_fail_loudly_on_cpu_tensors():
    from interactvlm_amd import ops

    with pytest.raises(_lib.IvlmError):
        ops.mask_census(torch.zeros(1, 8, 8), (32, 32), (32, 32), img_size=32)
    with pytest.raises(_lib.IvlmError):
        ops.box_nms(torch.zeros(2, 4), 0.7)


def test_abi_of_the_new_calls():
    protos = _lib.header_prototypes()
    C = _lib.C
    want = {
        "ivlm_mask_census": [C.c_void_p] + [C.c_int] * 8 + [C.c_float] * 3 + [C.c_void_p] * 3,
        "ivlm_box_nms_workspace_bytes": [C.c_int],
        "ivlm_box_nms": [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    }
    for name, args in want.items():
        assert [_lib._to_ctype(a) for a in protos[name][1]] == args, name
    lib = _lib.load()
    assert lib.ivlm_abi_version() == 5
    assert lib.ivlm_box_nms_workspace_bytes(16384) == 16384 * 256 * 8 and lib.ivlm_box_nms_workspace_bytes(16385) == 0
    assert lib.ivlm_box_nms_workspace_bytes(65) == 65 * 2 * 8 and lib.ivlm_box_nms_workspace_bytes(0) == 0
    # refusals come before any launch (no GPU here)
    assert lib.ivlm_mask_census(None, 1, 4, 4, 16, 16, 16, 16, 16, 1.0, 0.0, -1.0, None, None, None) == -1
    assert lib.ivlm_mask_census(1 << 12, 1, 4, 4, 16, 16, 16, 65536, 32768, 1.0, 0.0, -1.0, None, 1 << 12, None) == -4
    assert lib.ivlm_mask_census(1 << 12, 70000, 4, 4, 16, 16, 16, 16, 16, 1.0, 0.0, -1.0, None, 1 << 12, None) == -4
    assert lib.ivlm_box_nms(1 << 12, None, 16385, 0.7, 1 << 12, 1 << 12, 1 << 30, None) == -4
    assert lib.ivlm_box_nms(1 << 12, None, 128, 0.7, 1 << 12, 1 << 12, 8, None) == -2
    assert lib.ivlm_box_nms(None, None, 128, 0.7, None, None, 0, None) == -1
