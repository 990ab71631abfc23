"""Any-hit (occlusion) queries on the CPU: the new entry points are declared, exported and bound in every layer, and the
definition the GPU tests pin is checked against hand-written answers on a scene where the first candidate in traversal
order is not the nearest one.

Definition (include/bvh_mi355x.h, bvhgpu_traverse_any_*): ray i's answer is the first shape s of FlatBvh::traverse's list,
in its order, with Ray::intersects_triangle(s).distance < tmax[i] (strict), together with that Intersection; else NONE and
(+inf, 0, 0)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_traverse_any_f32", "bvhgpu_traverse_any_f64", "bvhgpu_hits_fetch_any"]
NONE = 0xFFFFFFFF


def first_match(off, isect, tmax):
    """the definition, restated in numpy: per row of the CSR the first j with isect[j, 0] < tmax (strict, in the isect dtype)"""
    n = len(off) - 1
    out = np.zeros((n, 3), dtype=isect.dtype)
    out[:, 0] = np.inf
    shape_pos = np.full(n, -1, dtype=np.int64)
    t = np.broadcast_to(np.asarray(tmax, dtype=isect.dtype), (n,))
    for r in range(n):
        row = isect[off[r]:off[r + 1], 0]
        with np.errstate(invalid="ignore"):
            hit = np.nonzero(row < t[r])[0]
        if len(hit):
            j = int(off[r]) + int(hit[0])
            shape_pos[r] = j
            out[r] = isect[j]
    return out, shape_pos


def test_new_functions_in_every_layer():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), f"{name} is not declared in the header"
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in bound, f"{name} missing from _lib.SYMBOLS"
        assert hasattr(lib, name) and re.search(r" T %s\b" % name, nm), f"{name} not exported"
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} missing from ffi.rs"
    assert "pub fn traverse_any(" in lib_rs and "pub fn occluded(" in lib_rs
    assert "bvhgpu_traverse_any_f32" in lib_rs and "bvhgpu_traverse_any_f64" in lib_rs   # impl_gpu_scalar! entries
    from bvh_amd.api import _TreeBase
    assert callable(getattr(_TreeBase, "any_hits", None)) and callable(getattr(_TreeBase, "occluded", None))


def _scene(dtype):
    """three triangles a ray along +z from the origin crosses at z = 3, 2 and 1.  Their centroids are spread along x (-13, 0, +13), so the
    builder splits on x and the walk meets them in x order: the farthest first, the nearest last.  Vertices run clockwise seen from
    +z (Ray::intersects_triangle culls back faces)."""
    tris = np.array([
        [[-30, -10, 3], [-30, 40, 3], [20, -10, 3]],     # shape 0: z = 3, centroid x = -13.3
        [[30, -10, 1], [-20, -10, 1], [30, 40, 1]],      # shape 1: z = 1, centroid x = +13.3
        [[-10, -10, 2], [0, 20, 2], [10, -10, 2]],       # shape 2: z = 2, centroid x = 0
    ], dtype=dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    return tris, aabbs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_answers_first_in_order_not_nearest(dtype):
    tris, aabbs = _scene(dtype)
    flat = orc.flatten(orc.build(aabbs).nodes)
    tmaxs = [0.5, 1.5, 2.5, math.inf, math.nan, 3.0, 2.0, 0.0, -1.0]
    n = len(tmaxs)
    rays = orc.make_rays(np.zeros((n, 3)), np.tile([[0.0, 0.0, 1.0]], (n, 1)), dtype)
    off, idx, _, _ = orc.traverse_flat(flat, aabbs, rays)
    isect, closest, prim = orc.triangle_stage(tris, rays, off, idx)
    # the premise: every ray's list is shapes 0, 2, 1 (x order) with distances 3, 2, 1 — the first candidate is the farthest
    for r in range(n):
        assert idx[off[r]:off[r + 1]].tolist() == [0, 2, 1]
        assert isect[off[r]:off[r + 1], 0].tolist() == [3.0, 2.0, 1.0]
    assert prim.tolist() == [1] * n                                      # the closest hit is shape 1 for every ray
    got, pos = first_match(off, isect, np.asarray(tmaxs, dtype=dtype))
    shapes = [int(idx[p]) if p >= 0 else NONE for p in pos]
    #                 0.5    1.5  2.5  +inf  NaN   3.0 (= shape 0's distance: strict <)  2.0 (= shape 2's)  0      -1
    assert shapes == [NONE, 1, 2, 0, NONE, 2, 1, NONE, NONE]
    for r, s in enumerate(shapes):
        if s == NONE:
            assert got[r].tolist() == [math.inf, 0.0, 0.0]
        else:
            assert got[r].tobytes() == isect[pos[r]].tobytes()
            assert got[r, 0] == {0: 3.0, 1: 1.0, 2: 2.0}[s]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_answers_misses_never_occlude(dtype):
    """a candidate whose triangle the ray misses (distance +inf) never occludes, not even with tmax = +inf; a back face neither"""
    tris, aabbs = _scene(dtype)
    flat = orc.flatten(orc.build(aabbs).nodes)
    o = np.array([[0.0, 0.0, 0.0], [-15.0, 30.0, 0.0], [0.0, 0.0, 10.0]])  # the origin; inside the boxes of shapes 0 and 1, outside both triangles; above all
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])      # ... the last one looking down: every triangle is a back face
    rays = orc.make_rays(o, d, dtype)
    off, idx, _, _ = orc.traverse_flat(flat, aabbs, rays)
    isect, _, _ = orc.triangle_stage(tris, rays, off, idx)
    got, pos = first_match(off, isect, np.asarray([math.inf] * 3, dtype=dtype))
    assert int(idx[pos[0]]) == 0
    assert off[2] > off[1] and np.isinf(isect[off[1]:off[2], 0]).all() and pos[1] == -1   # a candidate (box hit), not a triangle hit
    assert off[3] - off[2] == 3 and np.isinf(isect[off[2]:off[3], 0]).all() and pos[2] == -1
