"""interactvlm_amd.fit_start (csrc/fit_start.hip) on the GPU against tests/_fit_start_ref.py (fp64, written from the definitions).

Bounds are derived, not tuned (U = 2^-24):
  * normals: both sides compute in fp64 from the same fp32 coordinates and round once: one U for the rounding (components are <= 1 in
    magnitude), a second for an fp64 order difference that lands on a rounding boundary: |n - n64| <= 2U;
  * centroid: the same argument per axis, relative to the value: <= 2U max(1, |c|);
  * mask statistics: integers, exact;
  * the mirrored stage 1: the mean z is an fp64 sum rounded once and the four fp32 operations are IEEE, so z and T are bit-equal to
    the restatement; the intent mode is fp64 rounded once from an fp32 z that both sides share: <= 4U max(1, |T|);
  * the chain: the tolerances of tests/test_contact_icp_gpu.py (|R - R64| <= 4U, |T - T64| <= 4U max(1, |T|)) under its conditions
    (no near-tie inside its band, singular values apart), with the restatement fed the device's own normals and stage-1 translation.
"""
import functools

import pytest
import torch

import _fit_start_ref as ref
from interactvlm_amd import fit_start as fs
from interactvlm_amd.fit import ObjectPoseFit, fit_object_pose, matrix_to_rot6d

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(autouse=True)
def grad_enabled():
    """the chain test runs ``fit_object_pose``, which differentiates; a whole-suite run reaches this file with autograd switched off
    for the process (tests/test_contact_pair_gpu.py's fixture of the same name says by whom)"""
    with torch.enable_grad():
        yield


# ---------------------------------------------------------------- normals

def _with_zero_area_face():
    v, f = ref.tetrahedron()
    v = torch.cat([v, torch.tensor([[0.5, 0.5, 0.5]], dtype=torch.float64)])
    # (0, 1, 1) has no area and changes nothing; vertex 4 has ONLY faces without area: its sum is zero
    return v, torch.cat([f, torch.tensor([[0, 1, 1], [4, 4, 0], [4, 2, 4]])])


def _with_unreferenced_vertex():
    v, f = ref.icosphere(1)
    return torch.cat([v[:20], torch.tensor([[3.0, -2.0, 1.0]], dtype=torch.float64), v[20:]]), torch.where(f >= 20, f + 1, f)


NORMAL_CASES = {
    "tetrahedron": ref.tetrahedron,
    "icosphere2": lambda: ref.icosphere(2),
    "fan63": lambda: ref.fan(63), "fan64": lambda: ref.fan(64), "fan65": lambda: ref.fan(65), "fan257": lambda: ref.fan(257),
    "grid1023": lambda: ref.grid(33, 31), "grid1025": lambda: ref.grid(25, 41),
    "zero_area_face": _with_zero_area_face,
    "unreferenced_vertex": _with_unreferenced_vertex,
}


@functools.lru_cache(maxsize=None)
def normal_case(name):
    v, f = NORMAL_CASES[name]()
    v = v.float()
    return v, f, ref.normals(v, f)


def assert_normals(n, n64, what=""):
    err = float((n.cpu().double() - n64).abs().max())
    print(what, "max |n - n64| / U:", err / U)
    assert err <= 2 * U, f"{what}: {err:.3e} > {2 * U:.3e}"


@pytest.mark.parametrize("name", list(NORMAL_CASES))
def test_normals_against_fp64(cuda, name):
    v, f, n64 = normal_case(name)
    assert f.dtype == torch.int64
    n = fs.vertex_normals(v.to(cuda), f.to(cuda))
    assert n.dtype == torch.float32 and tuple(n.shape) == tuple(v.shape)
    assert bool(torch.isfinite(n).all())
    assert_normals(n, n64, name)
    assert torch.equal(n, fs.vertex_normals(v.to(cuda), f.to(cuda)))  # the same bits every call
    if name == "grid1023":
        assert v.shape[0] == 1023
    if name == "grid1025":
        assert v.shape[0] == 1025
    if name.startswith("fan"):
        assert int((f == 0).sum()) == int(name[3:])  # the hub's valence
    if name == "zero_area_face":
        assert torch.equal(n[4].cpu(), torch.zeros(3))
        assert torch.equal(n[:4], fs.vertex_normals(v[:4].to(cuda), f[:4].to(cuda)))  # faces without area change no bit
    if name == "unreferenced_vertex":
        assert torch.equal(n[20].cpu(), torch.zeros(3)) and float(n64[20].abs().max()) == 0.0


def test_normals_int32_faces_and_strided_verts(cuda):
    v, f, n64 = normal_case("icosphere2")
    want = fs.vertex_normals(v.to(cuda), f.to(cuda))
    assert torch.equal(fs.vertex_normals(v.to(cuda), f.to(cuda).to(torch.int32)), want)
    wide = torch.full((v.shape[0], 5), 7.0, device=cuda)
    wide[:, 1:4] = v.to(cuda)
    strided = wide[:, 1:4]
    assert not strided.is_contiguous()
    got = fs.vertex_normals(strided, f.to(cuda))
    assert torch.equal(got, want)
    assert_normals(got, n64, "strided")
    with pytest.raises(ValueError, match="faces"):
        fs.vertex_normals(v.to(cuda), (f + 1).to(cuda))  # an index out of range


# ---------------------------------------------------------------- centroid

@functools.lru_cache(maxsize=None)
def soup(F):
    """the first F faces of a bumpy grid, moved off the origin"""
    v, f = ref.grid(92, 92)
    assert f.shape[0] >= F
    v = (v + torch.tensor([-3.0, 1.5, 0.7], dtype=torch.float64)).float()
    f = f[:F].contiguous()
    return v, f, ref.centroid(v, f)


@pytest.mark.parametrize("F", [1, 255, 256, 257, 16385])
def test_centroid_against_fp64(cuda, F):
    v, f, c64 = soup(F)
    c = fs.surface_centroid(v.to(cuda), f.to(cuda))
    assert c.dtype == torch.float32 and tuple(c.shape) == (3,)
    err = (c.cpu().double() - c64).abs()
    bound = 2 * U * c64.abs().clamp_min(1.0)
    print(F, "err / U per axis:", (err / U).tolist())
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    assert torch.equal(c, fs.surface_centroid(v.to(cuda), f.to(cuda)))


def test_centroid_of_a_closed_box_and_degenerate_meshes(cuda):
    v, f = ref.box(4, (0.5, 0.3, 0.2))
    centre = torch.tensor([0.25, -1.5, 3.0], dtype=torch.float64)
    v = (v + centre).float()
    c = fs.surface_centroid(v.to(cuda), f.to(cuda).to(torch.int32))
    assert bool(((c.cpu().double() - ref.centroid(v, f)).abs() <= 2 * U * centre.abs().clamp_min(1.0)).all())
    flat = torch.tensor([[0, 0, 1], [2, 2, 2], [3, 1, 3]])
    with pytest.raises(ValueError, match="area"):
        fs.surface_centroid(v.to(cuda), flat.to(cuda))
    # one face with an area among degenerate ones: its own centroid
    mixed = torch.cat([flat, f[:1]])
    c1 = fs.surface_centroid(v.to(cuda), mixed.to(cuda))
    assert bool(((c1.cpu().double() - v[f[0]].double().mean(0)).abs() <= 2 * U * centre.abs().clamp_min(1.0)).all())


def test_centre_meshes(cuda):
    sc = ref.chain_scene()
    hv = sc["human_vertices"] + torch.tensor([0.2, -0.4, 3.1])
    ov = sc["obj_vertices"] * 2.0 + torch.tensor([1.0, 2.0, -0.5])
    out = fs.centre_meshes(hv.to(cuda), sc["human_faces"].to(cuda), ov.to(cuda), sc["obj_faces"].to(cuda))
    ch, co = ref.centroid(hv, sc["human_faces"]), ref.centroid(ov, sc["obj_faces"])
    tol = lambda c, v: 2 * U * max(1.0, float(c.abs().max())) + U * float((v.double() - c).abs().max())  # noqa: E731
    assert float((out.hum_centroid_offset.cpu().double() - ch).abs().max()) <= 2 * U * max(1.0, float(ch.abs().max()))
    assert float((out.human_vertices.cpu().double() - (hv.double() - ch)).abs().max()) <= tol(ch, hv)
    flip = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)
    assert float((out.obj_vertices.cpu().double() - (ov.double() - co) * flip).abs().max()) <= tol(co, ov)
    # the normals are those of the centred meshes (after the flip of y and z)
    assert torch.equal(out.human_normals, fs.vertex_normals(out.human_vertices, sc["human_faces"].to(cuda)))
    assert_normals(out.obj_normals, ref.normals(out.obj_vertices.cpu(), sc["obj_faces"]), "object")
    assert_normals(out.human_normals, ref.normals(out.human_vertices.cpu(), sc["human_faces"]), "human")


# ---------------------------------------------------------------- mask statistics

def _sparse(H, W, seed, p):
    return (torch.rand(H, W, generator=torch.Generator().manual_seed(seed)) < p)


def _at(H, W, *pixels):
    m = torch.zeros(H, W, dtype=torch.bool)
    for r, c in pixels:
        m[r, c] = True
    return m


MASK_CASES = {
    "1x2_both": lambda: torch.ones(1, 2, dtype=torch.bool),
    "3x5_sparse": lambda: _sparse(3, 5, 1, 0.4),
    "3x5_same_row": lambda: _at(3, 5, (1, 1), (1, 3), (2, 0)),
    "3x5_other_rows": lambda: _at(3, 5, (0, 4), (2, 0), (2, 3)),
    "3x5_corners": lambda: _at(3, 5, (0, 0), (2, 4)),
    "3x5_full": lambda: torch.ones(3, 5, dtype=torch.bool),
    "3x5_one": lambda: _at(3, 5, (1, 2)),
    "3x5_empty": lambda: torch.zeros(3, 5, dtype=torch.bool),
    "64x64_sparse": lambda: _sparse(64, 64, 2, 0.05),
    "64x64_corners": lambda: _at(64, 64, (0, 0), (63, 63)),
    "64x64_blob": lambda: ref.blob_mask(64, 64, (20.5, 40.0), (9.0, 13.0)).bool(),
    "65x257_sparse": lambda: _sparse(65, 257, 3, 0.01),
    "65x257_corners": lambda: _at(65, 257, (0, 0), (64, 256)),
    "65x257_full": lambda: torch.ones(65, 257, dtype=torch.bool),
    "65x257_late": lambda: _at(65, 257, (15, 240), (16, 3), (64, 100)),  # the first two in different blocks of the walk
    "1024x1024_sparse": lambda: _sparse(1024, 1024, 4, 0.003),
}
MASK_VALUES = {"uint8": lambda m: m.to(torch.uint8) * 255, "float": lambda m: m.float() * 0.5, "bool": lambda m: m}


def assert_stats(st, want):
    got = dict(count=int(st.count), row_min=int(st.row_min), row_max=int(st.row_max), col_min=int(st.col_min), col_max=int(st.col_max),
               row_sum=int(st.row_sum), col_sum=int(st.col_sum), first=tuple(st.first.tolist()), second=tuple(st.second.tolist()))
    assert got == want


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_mask_stats_exact(cuda, name):
    m = MASK_CASES[name]()
    want = ref.mask_stats(m)
    kinds = ["uint8"] if name.startswith("1024") else list(MASK_VALUES)
    for kind in kinds:
        st = fs.mask_stats(MASK_VALUES[kind](m).to(cuda))
        assert all(t.dtype == torch.int64 and t.is_cuda for t in st)
        assert_stats(st, want)
    if name == "3x5_same_row":
        assert want["first"][0] == want["second"][0]
    if name in ("3x5_other_rows", "65x257_late"):
        assert want["first"][0] != want["second"][0]
    if name.endswith("corners"):
        H, W = m.shape
        assert want["first"] == (0, 0) and want["second"] == (H - 1, W - 1) and want["count"] == 2
    if name.endswith("full"):
        assert want["count"] == m.numel()
    if name == "3x5_empty":
        assert want["count"] == 0 and want["first"] == (-1, -1) and want["row_min"] == -1


def test_mask_stats_strided_view(cuda):
    big = _sparse(70, 300, 5, 0.02).to(cuda)
    view = big[3:68, 20:277]
    assert not view.is_contiguous()
    assert_stats(fs.mask_stats(view), ref.mask_stats(view.cpu()))


# ---------------------------------------------------------------- contact depth and the stage-1 translation

FOCAL, PRINCIPAL = (613.0, 601.5), (322.25, 241.75)


@functools.lru_cache(maxsize=None)
def depth_case(n):
    gen = torch.Generator().manual_seed(50 + n)
    v = torch.randn(n, 3, generator=gen) * torch.tensor([0.3, 0.8, 0.2]) + torch.tensor([0.0, 0.0, -0.05])
    p = torch.rand(n, generator=gen)
    p[0] = 0.875
    if n > 1:
        p[n // 2] = 0.5   # exactly at the threshold: excluded - and if it were not, the mean would move by about 1000 / n
        v[n // 2, 2] = 1000.0
    return v, p


@pytest.mark.parametrize("n", [1, 255, 257, 10475])
def test_contact_depth_bits(cuda, n):
    v, p = depth_case(n)
    count, z = ref.contact_z(v, p, 0.5)
    assert n == 1 or not bool((p > 0.5)[n // 2])
    for probs in (p, p.bfloat16()):
        if probs.dtype == torch.bfloat16:
            count, z = ref.contact_z(v, probs, 0.5)
        out = fs.contact_depth(v.to(cuda), probs.to(cuda), 0.5)
        assert int(out.count) == count
        assert out.z.dtype == torch.float32 and out.z_sum.dtype == torch.float64
        assert float(out.z) == float(z), (float(out.z), float(z))
        assert abs(float(out.z_sum) - float(z.double()) * count) <= 2 * U * abs(float(z)) * count
        again = fs.contact_depth(v.to(cuda), probs.to(cuda), 0.5)
        assert torch.equal(again.z, out.z) and torch.equal(again.z_sum, out.z_sum)


def test_contact_depth_compares_in_fp32_and_counts_none(cuda):
    v = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [0.0, 0.0, 4.0]])
    p = torch.tensor([0.3, 0.30000004, 0.2])  # fp32(0.3) is not above the threshold 0.3 as torch's probs.float() > 0.3 sees it
    assert (p > 0.3).tolist() == [False, True, False]
    out = fs.contact_depth(v.to(cuda), p.to(cuda), 0.3)
    assert int(out.count) == 1 and float(out.z) == 2.0
    none = fs.contact_depth(v.to(cuda), p.to(cuda), 0.9)
    assert int(none.count) == 0 and float(none.z) == 0.0 and float(none.z_sum) == 0.0  # a zero, never a NaN


@pytest.mark.parametrize("n", [1, 255, 257, 10475])
def test_centroid_start_mirror_bits(cuda, n):
    v, p = depth_case(n)
    for name in ("3x5_same_row", "3x5_other_rows", "65x257_late", "64x64_blob"):
        m = MASK_CASES[name]()
        want = ref.stage1_mirror(m, v, p, FOCAL, PRINCIPAL, 0.5)
        T = fs.centroid_start(m.to(cuda), v.to(cuda), p.to(cuda), FOCAL, PRINCIPAL, threshold=0.5)
        assert T.dtype == torch.float32 and tuple(T.shape) == (3,)
        assert torch.equal(T.cpu(), want), (name, T.cpu().tolist(), want.tolist())
    # the camera as device tensors, and an offset that the mirrored mode does not use
    T2 = fs.centroid_start(m.to(cuda), v.to(cuda), p.to(cuda), torch.tensor(FOCAL, device=cuda), torch.tensor(PRINCIPAL, device=cuda),
                           hum_centroid_offset=torch.tensor([0.3, 0.1, 2.5], device=cuda))
    assert torch.equal(T2, T)


@pytest.mark.parametrize("n", [1, 255, 257, 10475])
def test_centroid_start_intent(cuda, n):
    v, p = depth_case(n)
    _, z = ref.contact_z(v, p, 0.5)
    for name, offset in (("64x64_blob", torch.tensor([0.1, -0.05, 3.0])), ("65x257_sparse", torch.tensor([-0.4, 0.3, 2.2])),
                         ("3x5_one", None)):
        m = MASK_CASES[name]()
        want = ref.stage1_intent(m, z, FOCAL, PRINCIPAL, torch.zeros(3) if offset is None else offset)
        T = fs.centroid_start(m.to(cuda), v.to(cuda), p.to(cuda), FOCAL, PRINCIPAL, None if offset is None else offset.to(cuda),
                              mirror_reference=False)
        err = (T.cpu().double() - want).abs()
        print(name, "err / U:", (err / U).tolist())
        assert bool((err <= 4 * U * want.abs().clamp_min(1.0)).all())
        assert float(T[2]) == float(z)


def test_centroid_start_raises_by_name(cuda):
    v, p = depth_case(255)
    args = (v.to(cuda), p.to(cuda), FOCAL, PRINCIPAL)
    for name in ("3x5_one", "3x5_empty"):  # count 1 and count 0
        with pytest.raises(ValueError, match="mask.*fewer than two"):
            fs.centroid_start(MASK_CASES[name]().to(cuda), *args)
    with pytest.raises(ValueError, match="mask.*no non-zero"):
        fs.centroid_start(MASK_CASES["3x5_empty"]().to(cuda), *args, mirror_reference=False)
    m = MASK_CASES["3x5_full"]().to(cuda)
    with pytest.raises(ValueError, match="human_contact_probs"):
        fs.centroid_start(m, v.to(cuda), torch.full((255,), 0.5, device=cuda), FOCAL, PRINCIPAL)  # at the threshold: none above
    with pytest.raises(ValueError, match="human_contact_probs"):
        fs.centroid_start(m, v[:1].to(cuda), torch.full((1,), 0.5, device=cuda), FOCAL, PRINCIPAL, mirror_reference=False)


# ---------------------------------------------------------------- the chain

FILTERS = [(True, 90, -90), (True, 60), (False,)]


def chain_inputs(cuda):
    sc = ref.chain_scene()
    d = lambda k: sc[k].to(cuda)  # noqa: E731
    return sc, dict(obj_vertices=d("obj_vertices"), obj_faces=d("obj_faces"), human_vertices=d("human_vertices"),
                    human_faces=d("human_faces"), obj_contact_probs=d("obj_probs"), human_contact_probs=d("human_probs"),
                    target_mask=d("mask"), focal=sc["focal"], principal=sc["principal"], hum_centroid_offset=d("offset"))


@pytest.mark.parametrize("filter_contacts", FILTERS, ids=["90_-90", "60", "off"])
def test_reference_start_chain(cuda, filter_contacts):
    sc, kw = chain_inputs(cuda)
    start = fs.reference_start(**kw, filter_contacts=filter_contacts)
    # the stages are the stage functions' results, bit for bit (they are held to fp64 above)
    assert torch.equal(start.obj_normals, fs.vertex_normals(kw["obj_vertices"], kw["obj_faces"]))
    assert torch.equal(start.human_normals, fs.vertex_normals(kw["human_vertices"], kw["human_faces"]))
    T1 = fs.centroid_start(kw["target_mask"], kw["human_vertices"], kw["human_contact_probs"], kw["focal"], kw["principal"])
    assert torch.equal(start.stage1_translation, T1)
    assert torch.equal(T1.cpu(), ref.stage1_mirror(sc["mask"], sc["human_vertices"], sc["human_probs"], sc["focal"], sc["principal"]))

    # the restatement, fed the device's own normals and stage-1 translation; the fixture conditions on it, in fp64
    on, hn = start.obj_normals.cpu(), start.human_normals.cpu()
    want = ref.chain(sc["obj_vertices"], sc["human_vertices"], on, hn, sc["obj_probs"], sc["human_probs"], T1.cpu(),
                     filter_contacts=filter_contacts)
    if filter_contacts[0]:
        margin = ref.filter_margin(on, hn, sc["obj_probs"] > 0.3, want["h_on"], filter_contacts)
        print("smallest distance of a dot product from a threshold cosine:", margin)
        assert margin > 1e-5
    assert ref.chain_conditions(want) == []
    assert int(want["kept"].sum()) >= 8 and int(want["h_on"].sum()) >= 8

    assert start.kept.dtype == torch.bool and torch.equal(start.kept.cpu(), want["kept"])
    assert torch.equal(start.obj_contact_probs.cpu(), want["probs"])
    assert bool((start.obj_contact_probs[~start.kept] == 0).all()) == bool(filter_contacts[0])
    assert bool((start.icp.nn_idx[0].cpu().long() == want["idx"]).all())
    R, T = start.icp.R[0].cpu().double(), start.icp.T[0].cpu().double()
    eR, eT = float((R - want["R"]).abs().max()), float((T - want["T"]).abs().max())
    print("|R - R64| / U:", eR / U, " |T - T64| / U:", eT / U)
    assert eR <= 4 * U
    assert eT <= 4 * U * max(1.0, float(want["T"].abs().max()))
    R6, Ti, s = start.init
    assert tuple(R6.shape) == (1, 6) and tuple(Ti.shape) == (1, 3) and s == 1.0
    assert torch.equal(R6, matrix_to_rot6d(start.icp.R)) and torch.equal(Ti, start.icp.T)

    # the fit continues from it: the first history row is one forward of the model at the start
    scene = (kw["obj_vertices"], kw["obj_faces"], kw["human_vertices"], start.obj_contact_probs, kw["human_contact_probs"],
             kw["target_mask"], kw["focal"], kw["principal"])
    out = fit_object_pose(*scene, init=start.init, hum_centroid_offset=kw["hum_centroid_offset"], max_iter=2)
    assert tuple(out["history"].shape) == (2, 1) and bool(torch.isfinite(out["history"]).all())
    model = ObjectPoseFit(*start.init, *scene, hum_centroid_offset=kw["hum_centroid_offset"])
    with torch.no_grad():
        total, _ = model(None, step=0)
    assert torch.equal(out["history"][0], total)


def test_reference_start_options(cuda):
    sc, kw = chain_inputs(cuda)
    start = fs.reference_start(**kw)
    again = fs.reference_start(**kw)
    assert all(torch.equal(a, b) for a, b in zip(start.init[:2] + (start.obj_contact_probs, start.kept),
                                                 again.init[:2] + (again.obj_contact_probs, again.kept)))
    # normals that the caller has: the same start, and human_faces is then not needed
    given = fs.reference_start(**{**kw, "human_faces": None}, obj_normals=start.obj_normals, human_normals=start.human_normals)
    assert torch.equal(given.init[0], start.init[0]) and torch.equal(given.init[1], start.init[1])
    # icp=False: the stage-1 translation with the identity, and no filter (the reference filters inside its ICP branch)
    plain = fs.reference_start(**kw, icp=False)
    assert plain.icp is None and torch.equal(plain.init[1][0], start.stage1_translation)
    assert torch.equal(plain.init[0], matrix_to_rot6d(torch.eye(3, device=cuda)))
    assert torch.equal(plain.obj_contact_probs, kw["obj_contact_probs"])
    # translation_hum_centroid=False: ICP starts from 0; the scale goes through unchanged
    zero = fs.reference_start(**kw, translation_hum_centroid=False, scale=1.25)
    assert float(zero.stage1_translation.abs().max()) == 0.0 and zero.init[2] == 1.25
    # the intent mode goes through to stage 1
    intent = fs.reference_start(**kw, mirror_reference=False)
    assert torch.equal(intent.stage1_translation,
                       fs.centroid_start(kw["target_mask"], kw["human_vertices"], kw["human_contact_probs"], kw["focal"], kw["principal"],
                                         kw["hum_centroid_offset"], mirror_reference=False))


def test_reference_start_raises_by_name(cuda):
    sc, kw = chain_inputs(cuda)
    with pytest.raises(ValueError, match="target_mask"):
        fs.reference_start(**{**kw, "target_mask": torch.zeros(48, 64, device=cuda)})
    with pytest.raises(ValueError, match="human_contact_probs"):
        fs.reference_start(**{**kw, "human_contact_probs": torch.zeros(162, device=cuda)})
    with pytest.raises(ValueError, match="obj_contact_probs"):
        fs.reference_start(**{**kw, "obj_contact_probs": torch.zeros(98, device=cuda)})
    # a filter nothing passes: cos(0) = 1 and no dot product of this scene comes near it (asserted on the restatement)
    on, hn = ref.normals(sc["obj_vertices"], sc["obj_faces"]), ref.normals(sc["human_vertices"], sc["human_faces"])
    o = on[sc["obj_probs"] > 0.3]
    h = -hn[sc["human_probs"] > 0.5]
    assert float((o @ h.T).max()) < 1 - 1e-5
    with pytest.raises(ValueError, match="obj_contact_probs.*filter_contacts"):
        fs.reference_start(**kw, filter_contacts=(True, 0.0))
