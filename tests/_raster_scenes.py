"""The scenes of the banded rasteriser tests (tests/test_raster_ref_cpu.py, tests/test_raster_exact_gpu.py), and the cached fp64
classification of each (tests/_raster_ref.py).  Every image is non-square and both orientations occur, so a swapped H / W cannot pass;
the meshes include one that overflows all four image borders, faces that span a large depth range and cross each other, two layers
1e-3 apart listed far-then-near, and a repeated-index face; the point sets include sub-pixel discs and points behind the camera."""
from __future__ import annotations

import functools

import numpy as np

import _raster_ref as ref

F = np.float32


def camera(cam, points=False):
    """R, T of a (dist, elev, azim, tx, ty) camera as render.rasterize_mesh / rasterize_points build them (the point path drops tx)"""
    from interactvlm_amd import render

    d, e, a, tx, ty = cam
    return render.look_at_view_transform(d, e, a, 0.0 if points else tx, ty)


def _icosphere(scale):
    from oracle import raster as O

    v, f = O.icosphere(2)
    return (v * F(scale)).astype(F), f.astype(np.int32)


def _crossing():
    """Two large triangles that cross along a line near x = 0 (each spans view depths ~1.4 .. 2.6), two quads 1e-3 apart with the FAR
    one listed first, and one repeated-index face."""
    v = np.array([
        [-0.9, -0.5, -0.6], [0.9, -0.5, 0.6], [0.0, 0.8, 0.0],          # A: near on the right
        [-0.9, -0.3, 0.6], [0.9, -0.3, -0.6], [0.0, 0.9, 0.0],          # B: near on the left
        [0.5, -0.9, -0.101], [0.9, -0.9, -0.101], [0.9, -0.6, -0.101], [0.5, -0.6, -0.101],   # far quad
        [0.5, -0.9, -0.100], [0.9, -0.9, -0.100], [0.9, -0.6, -0.100], [0.5, -0.6, -0.100],   # near quad
    ], dtype=F)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 8, 9], [10, 11, 12], [10, 12, 13], [0, 0, 1]], dtype=np.int32)
    return v, f


def _body():
    from interactvlm_amd import synthetic

    v, f = synthetic.body_mesh()
    return v.numpy().astype(F), f.numpy().astype(np.int32)


def _body_cams():
    from interactvlm_amd import constants

    return constants.HUMAN_VIEW_DICT["4MV-Z_Vitru"]["cam_params"]


# name -> (mesh builder, camera, (H, W))
MESH_SCENES = {
    "sphere": (lambda: _icosphere(0.5), (2.0, 45.0, 315.0, 0.0, 0.0), (96, 160)),
    "overflow": (lambda: _icosphere(1.3), (2.0, 20.0, 30.0, 0.1, -0.2), (112, 80)),
    "crossing": (_crossing, (2.0, 5.0, 8.0, 0.0, 0.0), (80, 112)),
}
BODY_VIEWS = ("topfront", "topback", "bottomfront", "bottomback")
for _name in BODY_VIEWS:
    MESH_SCENES["body-" + _name] = (_body, _name, (120, 168))
SMALL_MESH_SCENES = ("sphere", "overflow", "crossing")  # (no undecided pixel in any of them: test_raster_ref_cpu pins that)


def _sphere_points():
    rng = np.random.default_rng(0)
    p = rng.standard_normal((2048, 3)).astype(F)
    return (p / (np.linalg.norm(p, axis=1, keepdims=True) * 2.2)).astype(F)


def _box_points():
    rng = np.random.default_rng(1)
    return (rng.uniform(-1.0, 1.0, (1500, 3)) * np.array([1.5, 1.5, 3.0])).astype(F)


# name -> (points builder, camera, radius, (H, W))
POINT_SCENES = {
    "sphere-r0.05": (_sphere_points, (2.0, 45.0, 45.0, 0.0, 0.0), 0.05, (96, 144)),
    "sphere-r0.006": (_sphere_points, (2.0, 45.0, 45.0, 0.0, 0.0), 0.006, (96, 144)),
    "box": (_box_points, (2.0, 20.0, 200.0, 0.0, 0.2), 0.03, (144, 96)),
}

UNDECIDED_CAP = 0.005  # of covered pixels, in every banded scene


@functools.lru_cache(maxsize=None)
def mesh_scene(name):
    """-> (verts f32, faces i32, cam 5-tuple, (H, W))"""
    build, cam, size = MESH_SCENES[name]
    if isinstance(cam, str):
        cam = tuple(float(c) for c in _body_cams()[cam])
    v, f = build()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, cam, size


@functools.lru_cache(maxsize=None)
def mesh_reference(name):
    """-> (allowed, decided, bary64, bound) of tests/_raster_ref.classify_mesh, computed once and shared"""
    v, f, cam, (H, W) = mesh_scene(name)
    R, T = camera(cam)
    out = ref.classify_mesh(v, f, R, T, H, W)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def point_scene(name):
    """-> (pts f32, cam 5-tuple, radius, (H, W))"""
    build, cam, radius, size = POINT_SCENES[name]
    p = build()
    p.setflags(write=False)
    return p, cam, radius, size


@functools.lru_cache(maxsize=None)
def point_reference(name):
    p, cam, radius, (H, W) = point_scene(name)
    R, T = camera(cam, points=True)
    return ref.classify_points(p, R, T, radius, H, W)
