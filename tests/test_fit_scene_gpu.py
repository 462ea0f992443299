"""``fit.FitScene``: the constants of a fit are prepared once per search, not once per model.  The scene of
tests/test_fit_intrusion_gpu.py; 3 starts in chunks of 1 are 3 loops and 3 scoring models, which before the scene existed prepared
every mesh 6 times (12 ``MeshSDF``)."""
import pytest
import torch

from interactvlm_amd import fit, mesh_sdf
from interactvlm_amd import silhouette as sil
from interactvlm_amd.pose import cube_rotations
from test_fit_intrusion_gpu import scene

pytestmark = pytest.mark.gpu


def test_search_prepares_the_scene_once(hip_lib, cuda, monkeypatch):
    args, offset, hf = scene(cuda)
    calls = {"MeshSDF": 0, "check_closed": 0, "mask_bbox_centre": 0}

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(mesh_sdf.MeshSDF, "__init__", counted("MeshSDF", mesh_sdf.MeshSDF.__init__))
    monkeypatch.setattr(fit, "check_closed", counted("check_closed", fit.check_closed))
    monkeypatch.setattr(fit, "mask_bbox_centre", counted("mask_bbox_centre", fit.mask_bbox_centre))
    monkeypatch.setattr(sil, "_topology", {})
    weights = {**fit.DEFAULT_LOSS_WEIGHTS, "penetration_loss": {"w": 2.0, "kick_in": 0}, "intrusion_loss": {"w": 3.0, "kick_in": 1}}
    with torch.enable_grad():
        out = fit.search_object_pose(*args, rotations=cube_rotations()[:3], init=(None, torch.tensor([0.05, 0.78, 0.03], device=cuda), 1.0),
                                     icp=False, chunk=1, intrusion=True, human_faces=hf, hum_centroid_offset=offset, loss_weights=weights,
                                     max_iter=2)
    assert out["scores"].shape == (3,) and out["history"].shape == (2, 3)
    print(calls, "topology entries:", len(sil._topology))
    assert calls == {"MeshSDF": 2, "check_closed": 1, "mask_bbox_centre": 1}
    assert len(sil._topology) == 1
