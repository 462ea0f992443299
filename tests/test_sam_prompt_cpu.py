"""Promptable SAM without a GPU: the fp64 restatement of the prompt encodings against the reference's own outputs, every Python
refusal before the library loads, the coordinate scaling, the three new C entry points, and the tie rule of best_mask."""
import os
import types

import numpy as np
import pytest
import torch

import _sam_prompt_ref as R
from interactvlm_amd import _lib, sam
from interactvlm_amd.sam_predictor import SamPredictor, select_largest

# The reference computes its encodings in fp32; the restatement is fp64 on the same operands, so their difference is the reference's
# own fp32 noise.  Measured here (printed by the test): sparse 2.20e-6 absolute (the phase 2 pi (c @ gauss) reaches tens of radians,
# where one fp32 unit is 1.9e-6), dense 2.38e-7 of max |dense| = 2.88.  Asserted with a 4x margin.
SPARSE_NOISE, DENSE_NOISE_REL = 4 * 2.20e-6, 4 * 2.38e-7


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam_prompts.npz"))


def test_restatement_matches_the_reference(golden):
    pw = R.prompt_weights()
    gauss, table = pw["pe_layer.positional_encoding_gaussian_matrix"], R.point_table(pw)
    worst = 0.0
    for name in R.CASES:
        c = R.case(name)
        ref = golden[name + "/sparse"]
        got = R.sparse_ref(c["points"], c["labels"], c["boxes"], gauss, table, (R.IMG, R.IMG))
        assert got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"\n[restatement vs reference] sparse: max abs difference {worst:.2e}")
    assert worst < SPARSE_NOISE
    # token order: points, the pad point only when there is no box, then the two corners
    assert golden["a/sparse"].shape[1] == 2 and golden["b/sparse"].shape[1] == 4 and golden["c/sparse"].shape[1] == 2
    assert golden["d/sparse"].shape == (3, 4, 256) and golden["e/sparse"].shape == (2, 2, 256)
    assert np.array_equal(golden["a/sparse"][0, 1], table[4])  # the pad row is the not-a-point embedding alone
    dense = R.mask_downscale_ref(R.case("e")["mask_input"][:, 0], R.mask_down_weights(pw))  # [2, 4096, 256]
    sub = dense.reshape(2, R.GRID, R.GRID, 256)[:, ::8, ::8].transpose(0, 3, 1, 2)
    ref = golden["e/dense"]
    rel = float(np.abs(sub - ref).max() / np.abs(ref).max())
    print(f"[restatement vs reference] dense: max difference {rel:.2e} of max |dense| = {float(np.abs(ref).max()):.2f}")
    assert rel < DENSE_NOISE_REL


def _stub_decoder():
    return types.SimpleNamespace(grid=R.GRID, C=256, input_size=(R.IMG, R.IMG), device=torch.device("cpu"))


@pytest.fixture()
def no_library(monkeypatch):
    """any attempt to load the library fails the test: a refusal has to come before it"""
    def boom():
        raise AssertionError("the library was loaded before the argument check")

    monkeypatch.setattr(_lib, "load", boom)


_P, _L = torch.zeros(2, 3, 2), torch.zeros(2, 3, dtype=torch.int64)
BAD_BATCH = [
    (dict(), "no prompt"),
    (dict(labels=_L), "without point_coords"),
    (dict(points=_P), "without point_labels"),
    (dict(points=_P[0], labels=_L[0]), "point_coords"),
    (dict(points=torch.zeros(2, 3, 3), labels=_L), "point_coords"),
    (dict(points=_P.long(), labels=_L), "point_coords"),
    (dict(points=_P, labels=_L[:, :2]), "point_labels"),
    (dict(points=_P, labels=_L.float()), "point_labels"),
    (dict(points=_P.numpy(), labels=_L), "expected a tensor"),
    (dict(boxes=torch.zeros(2, 5)), "boxes"),
    (dict(boxes=torch.zeros(4)), "boxes"),
    (dict(points=_P, labels=_L, boxes=torch.zeros(3, 4)), "prompt sets"),
    (dict(mask_input=torch.zeros(2, 256, 256)), "mask_input"),
    (dict(mask_input=torch.zeros(2, 1, 128, 256)), "mask_input"),
    (dict(points=_P, labels=_L, mask_input=torch.zeros(1, 1, 256, 256)), "prompt sets"),
]


@pytest.mark.parametrize("kw, msg", BAD_BATCH, ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(BAD_BATCH)])
def test_encode_prompts_and_predict_batch_refuse_before_the_library_loads(no_library, kw, msg):
    with pytest.raises(ValueError, match=msg):
        sam.SamMaskDecoder.encode_prompts(_stub_decoder(), **kw)
    pred = SamPredictor(None, _stub_decoder())
    pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256), R.PHOTO_INPUT, R.PHOTO)
    kw = {{"points": "point_coords", "labels": "point_labels"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError, match=msg):
        pred.predict_batch(**kw)


def test_predictor_refusals_before_the_library_loads(no_library):
    dec = _stub_decoder()
    with pytest.raises(ValueError, match="img_size"):
        SamPredictor(None, dec, img_size=512)
    pred = SamPredictor(None, dec)
    box = torch.tensor([1.0, 2.0, 30.0, 40.0])
    with pytest.raises(RuntimeError, match="image must be set"):
        pred.predict(box=box)
    with pytest.raises(RuntimeError, match="image must be set"):
        pred.best_mask(box=box)
    with pytest.raises(ValueError, match="image_u8"):
        pred.set_image(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="image_u8"):
        pred.set_image(np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError, match="needs an image encoder"):
        pred.set_image(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="embedding"):
        pred.set_embedding(torch.zeros(1, R.GRID * R.GRID, 256), R.PHOTO_INPUT, R.PHOTO)
    with pytest.raises(ValueError, match="embedding"):
        pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256, dtype=torch.float64), R.PHOTO_INPUT, R.PHOTO)
    with pytest.raises(ValueError, match="input_size"):
        pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256), (2048, 100), R.PHOTO)
    with pytest.raises(ValueError, match="original_size"):
        pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256), R.PHOTO_INPUT, (0, 10))
    pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256), R.PHOTO_INPUT, R.PHOTO)
    assert pred.is_image_set
    for kw, msg in ((dict(), "no prompt"), (dict(point_labels=torch.zeros(1, dtype=torch.int64)), "without point_coords"),
                    (dict(point_coords=torch.zeros(1, 2)), "without point_labels"),
                    (dict(point_coords=torch.zeros(1, 1, 2), point_labels=torch.zeros(1, 1, dtype=torch.int64)), "point_coords"),
                    (dict(box=torch.zeros(1, 4)), "box"), (dict(mask_input=torch.zeros(256, 256)), "mask_input")):
        with pytest.raises(ValueError, match=msg):
            pred.predict(**kw)
        with pytest.raises(ValueError, match=msg):
            pred.best_mask(**{k: v for k, v in kw.items()})
    pred.reset_image()
    assert not pred.is_image_set and pred.input_size is None and pred.original_size is None
    # predict_masks: shapes are refused before the library loads too
    full = types.SimpleNamespace(grid=R.GRID, C=256, n_mask=4)
    emb, sp = torch.zeros(R.GRID * R.GRID, 256), torch.zeros(2, 3, 256)
    for args, msg in (((emb[None], sp, None), "image_embedding"), ((emb, sp[0], None), "sparse"), ((emb, sp.double(), None), "sparse"),
                      ((emb, sp, torch.zeros(1, R.GRID * R.GRID, 256)), "dense")):
        with pytest.raises(ValueError, match=msg):
            sam.SamMaskDecoder._predict_all(full, *args)


def test_coordinate_scaling_is_the_reference_apply_coords(golden):
    pred = SamPredictor(None, _stub_decoder())
    pred.set_embedding(torch.zeros(R.GRID * R.GRID, 256), R.PHOTO_INPUT, R.PHOTO)
    pc, ref = golden["photo_coords"], golden["photo_coords_scaled"]
    assert np.array_equal(pc, R.photo_coords()) and ref.dtype == np.float64
    got = pred.scale_coords(torch.from_numpy(pc))
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(ref).float())  # the fp64 product, rounded once
    boxes = torch.from_numpy(pc[:4].reshape(2, 4))
    assert torch.equal(pred.scale_coords(boxes.reshape(-1, 2, 2)).reshape(-1, 4), torch.from_numpy(ref[:4].reshape(2, 4)).float())
    assert float(ref[1, 0]) == 499.0 * (683 / 500) and float(ref[1, 1]) == 749.0 * (1024 / 750)  # (1024, 683) is the resized photo


def test_abi_of_the_three_new_calls():
    protos = _lib.header_prototypes()
    C = _lib.C
    want = {
        "ivlm_prompt_embed": [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p],
        "ivlm_mask_downscale": [C.c_void_p] * 12 + [C.c_int] * 5 + [C.c_float, C.c_void_p],
        "ivlm_mask_dot_multi": [C.c_void_p] * 2 + [C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p],
    }
    for name, args in want.items():
        assert name in protos, f"{name} is not declared in ivlm_hip.h"
        ret, decl = protos[name]
        assert ret == "int" and [_lib._to_ctype(a) for a in decl] == args, (name, decl)
    lib = _lib.load()  # (no GPU needed: loading types every declared symbol, a missing one raises)
    for name, args in want.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is C.c_int
    # refusals that come before any launch need no GPU: NULL pointers, the unsupported widths and token counts
    assert lib.ivlm_prompt_embed(None, None, None, None, None, 1, 128, 1024, 1024, None) == -1
    assert lib.ivlm_mask_downscale(*[None] * 12, 1, 2, 2, 256, 16, 1e-6, None) == -1
    assert lib.ivlm_mask_dot_multi(None, None, 0, None, 1, 4, 2, 2, 32, None) == -1
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.ivlm_mask_dot_multi(p, p, 0, p, 1, 5, 1, 1, 32, None) == -4  # IVLM_ERR_UNSUPPORTED
    for F in (0, 16, 48, 160, 256):
        assert lib.ivlm_prompt_embed(p, p, p, p, p, 1, F, 1024, 1024, None) == -4
    for Cc, mid in ((32, 16), (320, 16), (96, 16), (256, 8), (256, 32)):
        assert lib.ivlm_mask_downscale(*[p] * 12, 1, 1, 1, Cc, mid, 1e-6, None) == -4


def test_best_mask_tie_rule_on_cpu_tensors():
    pick = lambda *v: int(select_largest(torch.tensor(v, dtype=torch.float32)))
    assert pick(0.1, 0.9, 0.5) == 1
    assert pick(0.7, 0.7, 0.2) == 0 and pick(0.2, 0.7, 0.7) == 1  # ties: the lowest index
    assert pick(float("nan"), 0.3, 0.3) == 1 and pick(float("inf"), 0.1, 0.2) == 2  # non-finite ranks last
    assert pick(float("nan"), float("nan"), float("nan")) == 0
    assert pick(-0.5, -0.25, -0.75) == 1

    class _Fixed(SamPredictor):  # best_mask on a fixed prediction: the device argmax picks the mask
        def predict(self, *a, **k):
            return torch.stack([torch.zeros(4, 5), torch.ones(4, 5), torch.ones(4, 5)]) > 0, torch.tensor([0.2, 0.8, 0.8]), None

    best = _Fixed(None, _stub_decoder()).best_mask(box=torch.zeros(4))
    assert best.dtype == torch.float32 and best.shape == (4, 5) and bool((best == 1).all())
