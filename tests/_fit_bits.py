"""The cases of tests/test_fit_bits_gpu.py and tests/golden/make_golden_fit_bits.py: every input form of the object-pose fit family's
Python side (contact_pair, silhouette, pose, mesh_sdf, contact_icp, fit) on the scene of tests/test_fit_intrusion_gpu.py - the 8-vertex
cube, the 134-vertex body, a 32 x 32 mask.  A case is a function of the prepared inputs that returns a list of tensors; ``record``
turns it into strings that compare equal exactly when every bit does.

The inputs are built from exact fp32 operations only (a product and a sum per element, ``torch.rand``'s scaled integers), so that
they are the same numbers wherever the cases run.
"""
import functools
import hashlib
import types

import torch

import _intrusion_ref as ir
from interactvlm_amd import contact_icp as icp
from interactvlm_amd import fit
from interactvlm_amd.contact_pair import contact_distance
from interactvlm_amd.mesh_sdf import MeshSDF
from interactvlm_amd.pose import cube_rotations, pose_transform
from interactvlm_amd.silhouette import silhouette_terms, soft_silhouette
from test_fit_intrusion_gpu import scene

B = 3
FIVE = {"mask_loss": {"w": 5.0, "kick_in": 0}, "centroid_loss": {"w": 1e-4, "kick_in": 2}, "contact_loss": {"w": 10.0, "kick_in": 0},
        "penetration_loss": {"w": 2.0, "kick_in": 1}, "intrusion_loss": {"w": 3.0, "kick_in": 3}}
THREE = {"mask_loss": {"w": 5.0, "kick_in": 0}, "centroid_loss": {"w": 1e-4, "kick_in": 2}, "contact_loss": {"w": 10.0, "kick_in": 4}}
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def encode(t):
    """a tensor -> the hex of its int32 (fp32, int32, int64 values) or uint8 (bool, uint8) view; the sha256 of those bytes when they
    are more than 64, so that the golden file stays a few KB"""
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.bool, torch.uint8):
        raw = t.to(torch.uint8).numpy().tobytes()
    else:
        assert t.dtype in (torch.float32, torch.int32, torch.int64), t.dtype
        raw = (t.to(torch.int32) if t.dtype == torch.int64 else t.view(torch.int32)).numpy().tobytes()
    return raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


def record(name, dev):
    return [f"{tuple(t.shape)} {encode(t)}" for t in CASES[name](inputs(dev))]


def ramp(t):
    """a fixed incoming gradient that is not all ones: 1, 1.25, 1.5, ... in the shape of t"""
    return (torch.arange(t.numel(), dtype=torch.float32, device=t.device) * 0.25 + 1.0).reshape(t.shape)


def graded(fn, *leaves):
    """-> [the outputs of fn(*leaves), the gradient of sum(ramp * output) to every leaf that is a tensor requiring grad]"""
    leaves = [x.detach().clone().requires_grad_() if isinstance(x, torch.Tensor) and x.requires_grad else x for x in leaves]
    out = fn(*leaves)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    with torch.enable_grad():
        sum((o * ramp(o)).sum() for o in outs).backward()
    return [o.detach() for o in outs] + [x.grad for x in leaves if isinstance(x, torch.Tensor) and x.requires_grad]


def g(x):
    return x.detach().clone().requires_grad_()


@functools.lru_cache(maxsize=None)
def inputs(dev):
    args, offset, hf = scene(dev)
    cv, cf, hv, p_obj, p_hum, target = args[:6]
    S = types.SimpleNamespace(args=args, offset=offset, hf=hf, cv=cv, cf=cf, hv=hv, p_obj=p_obj, p_hum=p_hum, target=target, dev=dev)
    gen = torch.Generator().manual_seed(0)
    centre = torch.tensor(ir.CUBE_CENTRE)
    S.t3 = (centre + (torch.rand(B, 3, generator=gen) - 0.5) * 0.125).to(dev)
    S.r3 = (torch.tensor(ir.IDENTITY6) + (torch.rand(B, 6, generator=gen) - 0.5) * 0.25).to(dev)
    S.s3 = torch.tensor([1.0, 0.875, 1.125], device=dev)
    S.o = cv + S.t3[0]                       # the cube at the scene's place, [8,3]
    S.oB = cv * S.s3[:, None, None] + S.t3[:, None, :]  # [B,8,3]
    S.pts = torch.stack([hv[:40] * 0.875 + d for d in S.t3 - S.t3[0]])  # [B,40,3]: most of them inside the body
    S.start = (torch.tensor(ir.IDENTITY6, device=dev).repeat(B, 1), S.t3, S.s3)
    S.human, S.cube = MeshSDF(hv, hf), MeshSDF(cv, cf)
    with torch.no_grad():
        S.alpha = soft_silhouette(S.oB + offset, cf, *args[6:], (32, 32))
    S.targets = torch.stack([target, target.roll(2, 0), target.roll(-3, 1)])
    S.rot4, S.T0 = cube_rotations()[:4], centre.to(dev)
    return S


# ---- contact_distance ---------------------------------------------------------------------------------------------------------------
@case
def contact_distance_forms(S):
    out = []
    for o, h in ((S.o, S.hv), (S.oB, S.hv), (S.oB[:1], S.hv), (S.oB, S.hv[None]), (S.o, S.hv[None].repeat(B, 1, 1) + S.t3[:, None] * 0.0625)):
        for p, q in ((S.p_obj, S.p_hum), (S.p_obj.bfloat16(), S.p_hum.bfloat16()), (S.p_obj.bfloat16(), S.p_hum), (S.p_obj, S.p_hum.bfloat16())):
            out.append(contact_distance(o, h, p, q))
    return out


@case
def contact_distance_gradients(S):
    out = []
    for o, h in ((S.o, S.hv), (S.oB, S.hv), (S.oB, S.hv[None]), (S.oB[:1], S.hv[None].repeat(B, 1, 1))):
        for go, gh in ((1, 0), (0, 1), (1, 1)):
            out += graded(lambda a, b: contact_distance(a, b, S.p_obj, S.p_hum.bfloat16()), g(o) if go else o, g(h) if gh else h)
    return out


# ---- silhouette ---------------------------------------------------------------------------------------------------------------------
@case
def soft_silhouette_forms(S):
    out = []
    for v in (S.o + S.offset, S.oB + S.offset):
        for faces in (S.cf, S.cf.long()):
            out += graded(lambda x: soft_silhouette(x, faces, *S.args[6:], (32, 32)), g(v))
    return out


@case
def silhouette_terms_forms(S):
    out = []
    for alpha in (S.alpha[1], S.alpha):
        for t in (S.target, S.target.bool(), S.target.to(torch.uint8), S.targets, S.targets.bool()):
            if alpha.dim() == 2 and t.dim() == 3:
                t = t[:1]
            out += graded(lambda a: silhouette_terms(a, t), g(alpha))
    return out


# ---- pose_transform -----------------------------------------------------------------------------------------------------------------
@case
def pose_transform_forms(S):
    out = graded(lambda r, t: pose_transform(S.cv, r, t, 1.125), g(S.r3[1]), g(S.t3[1]))
    out += graded(lambda r, t, s: pose_transform(S.cv, r, t, s), g(S.r3[1]), g(S.t3[1]), g(S.s3[1]))
    for s in (0.875, S.s3, S.s3[:, None], S.s3[:1]):
        out.append(pose_transform(S.cv, S.r3, S.t3, s))
    for need in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)):
        for s in (S.s3, S.s3[:, None]):
            leaves = [g(x) if n else x for x, n in zip((S.r3, S.t3, s), need)]
            out += graded(lambda r, t, s: pose_transform(S.cv, r, t, s), *leaves)
    return out


# ---- mesh_sdf -----------------------------------------------------------------------------------------------------------------------
@case
def mesh_sdf_query_and_penetration(S):
    out = [*S.human.query(S.pts[0]), *S.human.query(S.pts), *S.human.query(S.oB), *S.cube.query(S.hv)]
    for p in (S.pts[0], S.pts, S.oB):
        out.append(S.human.penetration(p))
        out += graded(S.human.penetration, g(p))
    return out


@case
def mesh_sdf_intrusion_forms(S):
    out = [S.cube.intrusion(S.hv, S.r3[0], S.t3[0]), S.cube.intrusion(S.hv, S.r3[1], S.t3[1], 1.125)]
    out += graded(lambda r, t, s: S.cube.intrusion(S.hv, r, t, s), g(S.r3[2]), g(S.t3[2]), g(S.s3[2]))
    for s in (1.0, 0.875, S.s3, S.s3[:, None]):
        out.append(S.cube.intrusion(S.hv, S.r3, S.t3, s))
        out += graded(lambda r, t: S.cube.intrusion(S.hv, r, t, s), g(S.r3), g(S.t3))
    for s in (S.s3, S.s3[:, None]):
        out += graded(lambda r, t, s: S.cube.intrusion(S.hv, r, t, s), S.r3, g(S.t3), g(s))
        out += graded(lambda r, t, s: S.cube.intrusion(S.hv, r, t, s), g(S.r3), g(S.t3), g(s))
    return out


# ---- contact_icp --------------------------------------------------------------------------------------------------------------------
def _flat(result):
    return [*result[:8], *result.history]


@case
def contact_nearest_and_align(S):
    six = lambda x: torch.cat((x, x * 0.5), dim=-1)  # noqa: E731
    out = [*icp.contact_nearest(S.o, S.hv), *icp.contact_nearest(S.oB, S.hv), *icp.contact_nearest(S.o, S.hv[None].repeat(B, 1, 1)),
           *icp.contact_nearest(six(S.oB), six(S.hv))]
    Y, w = S.hv[20:28], ramp(S.p_obj)
    for X, W in ((S.o, None), (S.oB, None), (S.oB, w), (S.o, torch.stack((w, w * 0.5, w.flip(0))))):
        out += icp.align_points(X, Y, W)
        out += icp.align_points(X, Y, W, estimate_scale=True, allow_reflection=True)
    return out


@case
def contact_icp_forms(S):
    init = (cube_rotations()[:B].to(S.dev), S.t3 - S.t3[0], S.s3)
    w = ramp(S.p_obj)
    out = _flat(icp.contact_icp(S.o, S.hv, max_iterations=4))
    out += _flat(icp.contact_icp(S.oB, S.hv, max_iterations=4, requery=True, estimate_scale=True))
    out += _flat(icp.contact_icp(S.o, S.hv, init=init, max_iterations=4))
    out += _flat(icp.contact_icp(S.o, S.hv, init=init, weights=w, max_iterations=4, requery=True))
    out += _flat(icp.contact_icp(S.o, S.hv, S.cv * 2.5, S.hv, max_iterations=4))
    out += _flat(icp.contact_icp(S.o, S.hv, S.cv * 2.5, S.hv, init=init, weights=w, max_iterations=4, requery=True))
    return out


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
@case
def object_pose_fit_step0(S):
    out = []
    every = {k: {"w": v["w"], "kick_in": 0} for k, v in FIVE.items()}
    for fused in (False, True):
        model = fit.ObjectPoseFit(S.r3, S.t3, S.s3, *S.args, S.offset, vars=("pose", "scale"), fused_transform=fused, intrusion=True,
                                  human_faces=S.hf)
        with torch.enable_grad():
            total, terms = model(every, step=0)
            (total * ramp(total)).sum().backward()
        assert list(terms) == list(FIVE)
        out += [total.detach(), *(t.detach() for t in terms.values()), model.rotation.grad, model.translation.grad, model.scale.grad]
    return out


def _fitted(out):
    return [out[k] for k in ("history", "term_history", "rotation", "translation", "scale", "object_vertices") if k in out]


@case
def fit_object_pose_torch_loop(S):
    out = []
    for fused in (False, True):
        out += _fitted(fit.fit_object_pose(*S.args, init=S.start, hum_centroid_offset=S.offset, vars=("pose", "scale"), loss_weights=FIVE,
                                           max_iter=6, fused_transform=fused, intrusion=True, human_faces=S.hf))
    return out


@case
def fit_object_pose_device_loop(S):
    return _fitted(fit.fit_object_pose(*S.args, init=S.start, hum_centroid_offset=S.offset, vars=("pose", "scale"), loss_weights=THREE,
                                       max_iter=6, device_loop=True))


def _search(S, chunk, device_loop):
    extra = {"device_loop": True, "loss_weights": THREE} if device_loop else {"intrusion": True, "human_faces": S.hf, "loss_weights": FIVE}
    out = fit.search_object_pose(*S.args, rotations=S.rot4, init=(None, S.T0, 1.0), icp=True, chunk=chunk, hum_centroid_offset=S.offset,
                                 max_iter=4, **extra)
    return [out["scores"], out["best_index"], *_fitted(out), *out["best"].values()]


@case
def search_object_pose_torch_loop(S):
    return [t for chunk in (None, 1, 3) for t in _search(S, chunk, False)]


@case
def search_object_pose_device_loop(S):
    return [t for chunk in (None, 1, 3) for t in _search(S, chunk, True)]
