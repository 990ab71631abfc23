"""Nearest-first k-nearest point queries (bvhgpu_knearest_tree_*) on the CPU: the entry points are declared, exported and bound in every
layer, and the definition the GPU tests pin (tests/knn_tree_ref.py; include/bvh_mi355x.h) is checked against the oracle's Bvh::nearest_to
(k = 1), against brute force where the arithmetic is exact, against hand-written rows and on the special values of max_dist."""
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref as kr
import knn_tree_ref as ktr
from oracle import orc
from test_knn_cpu import cube_scene, extreme_points, half_grid_queries, integer_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_knearest_tree_f32", "bvhgpu_knearest_tree_f64"]
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]


# ---- 1. every layer --------------------------------------------------------------------------------------------------------
def test_new_functions_in_every_layer():
    raw = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    h = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), f"{name} is not declared in the header"
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int bvhgpu_knearest_tree_f32", raw, flags=re.S)
    assert m, "bvhgpu_knearest_tree_* has no comment in front of it"
    text = " ".join(m.group(1).split())
    assert "BVHGPU_NONE" in text and "+inf" in text and "PADDING" in text.upper()                  # the padding
    assert "BVHGPU_KNN_MAX_K" in text
    assert "max_dist" in text and "negative or NaN" in text and "m * m" in text                    # the max_dist rule
    assert re.search(r"order THIS walk meets them", text) and "not leaf pre-order" in text         # ties follow the walk
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
        assert name in lib_rs, f"{name} is no impl_gpu_scalar! entry"
    assert "pub fn nearest_k_tree(" in lib_rs
    from bvh_amd.api import Bvh, _TreeBase
    assert callable(getattr(_TreeBase, "knearest_tree_batch", None))
    assert "knearest_tree_batch" not in vars(Bvh)                                                  # no flatten needed: no override


# ---- 2. the anchor: k = 1 without max_dist is Bvh::nearest_to ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_k1_equals_oracle_tree_nearest(dtype):
    tris, aabbs = cube_scene(100, dtype)                                  # 1 200 triangles
    nodes = orc.build(aabbs).nodes
    rng = np.random.default_rng(5)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    pts = np.concatenate([rng.uniform(lo * 2, hi * 2, size=(141, 3)).astype(dtype), extreme_points(dtype, (lo + hi) / 2)])
    assert len(pts) == 171
    for t in (None, tris):
        got = ktr.knearest_tree(nodes, aabbs, pts, [1], t)[1]
        ws, wd = orc.nearest(nodes, aabbs, pts, t)
        assert np.array_equal(got[0][:, 0], ws) and kr.same(got[1][:, 0], wd), (dtype, t is not None)


# ---- 3. brute force where arithmetic is exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_definition_equals_brute_force_on_integer_cloud(dtype):
    """1 024 zero-size boxes at integer coordinates in [0, 15]^3, queries at multiples of 0.5: every operation of both distances is
    exact, so the row's squared distances must be the k smallest of all shapes — and with max_dist = 1.5 exactly those of them that are
    <= 2.25.  Shapes are not compared with brute force: ties at equal distance follow the walk."""
    aabbs, tris = integer_cloud(dtype, 15, n=1024)
    nodes = orc.build(aabbs).nodes
    flat = orc.flatten(nodes)
    tl = ktr.tree_lists(nodes)
    qs = half_grid_queries(dtype, 15, 100)
    r2 = ktr.limits(1.5, 1, dtype)[0]
    assert r2 == 2.25
    cut = 0
    for kind_tris in (None, tris):
        for p in qs:
            dl, dr, d = ktr.dists_vector(nodes, aabbs, p, dtype, kind_tris)
            dll, drl, dsl = dl.tolist(), dr.tolist(), d.tolist()
            for k in (1, 3, 8, 33, 64):
                bd, _ = kr.brute_force(flat, d, k)
                ld, ls = ktr.walk(tl, dll, drl, dsl, k)
                assert ld == bd and len(set(ls)) == len(ls) == k and [dsl[s] for s in ls] == ld
                ld, ls = ktr.walk(tl, dll, drl, dsl, k, r2)
                want = [x for x in bd if x <= 2.25]
                assert ld == want and len(set(ls)) == len(ls) and [dsl[s] for s in ls] == ld
                cut += len(want) < k
    assert cut > 0, "the limit never shortened a row"


# ---- 4. hand-written rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answers_on_aligned_boxes(dtype):
    """unit boxes centred at x = -10..10, shape = x + 10, neighbours touch at +-0.5, +-1.5, ...: arithmetic on quarters"""
    boxes = orc.aligned_boxes().astype(dtype)
    nodes = orc.build(boxes).nodes
    pts = np.array([[0.25, 0, 0], [0.75, 0, 0], [-3.25, 0.5, -0.5], [20, 0, 0]], dtype=dtype)
    shape, dist = ktr.knearest_tree(nodes, boxes, pts, [3])[3]
    assert shape.tolist() == [[10, 11, 9], [11, 10, 12], [7, 6, 8], [20, 19, 18]]
    assert dist.tolist() == [[0, 0.25, 0.75], [0, 0.25, 0.75], [0, 0.25, 0.75], [9.5, 10.5, 11.5]]
    shape, dist = ktr.knearest_tree(nodes, boxes, pts, [3], max_dist=0.25)[3]                 # the limit itself is inside
    assert shape.tolist() == [[10, 11, NONE], [11, 10, NONE], [7, 6, NONE], [NONE] * 3]
    assert dist.tolist() == [[0, 0.25, np.inf], [0, 0.25, np.inf], [0, 0.25, np.inf], [np.inf] * 3]
    shape, dist = ktr.knearest_tree(nodes, boxes, pts, [33], max_dist=[1.0, 0.5, 0.2, 10.0])[33]
    assert [sorted(r[r != NONE].tolist()) for r in shape] == [[9, 10, 11], [10, 11], [7], [20]]
    assert (shape[:, 3:] == NONE).all() and np.isposinf(dist[shape == NONE]).all()
    # the tie at x = 0.5: shapes 10 and 11 both at distance 0, 9 and 12 both at 1 — the row holds the two at 0 and one of the two at 1
    shape, dist = ktr.knearest_tree(nodes, boxes, np.array([[0.5, 0, 0]], dtype=dtype), [3])[3]
    assert sorted(shape[0, :2].tolist()) == [10, 11] and shape[0, 2] in (9, 12) and dist.tolist() == [[0, 0, 1]]


# ---- 5. max_dist special values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_max_dist_special_values(dtype):
    tris, aabbs = cube_scene(20, dtype)
    nodes = orc.build(aabbs).nodes
    rng = np.random.default_rng(6)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    inside = (aabbs[::40, :3] + aabbs[::40, 3:]) / 2                                          # centres of shape boxes: distance 0 to them
    pts = np.concatenate([rng.uniform(lo, hi, size=(6, 3)), inside]).astype(dtype)
    free = ktr.knearest_tree(nodes, aabbs, pts, [8])[8]
    assert not np.isnan(free[1]).any()
    zero = ktr.knearest_tree(nodes, aabbs, pts, [8], max_dist=0.0)[8]
    for r in range(len(pts)):                                                                 # 0 keeps exactly the distance-0 shapes
        keep = free[1][r] == 0
        assert zero[0][r][: keep.sum()].tolist() == free[0][r][keep].tolist() and (zero[0][r][keep.sum():] == NONE).all()
        assert (zero[1][r][: keep.sum()] == 0).all() and np.isposinf(zero[1][r][keep.sum():]).all()
    assert (zero[0][6:, 0] != NONE).all()
    for bad in (-1.0, -0.0 - 1e-30, np.nan, -np.inf):                                         # negative and NaN: padding
        s, d = ktr.knearest_tree(nodes, aabbs, pts, [8], max_dist=bad)[8]
        assert (s == NONE).all() and np.isposinf(d).all()
    s, d = ktr.knearest_tree(nodes, aabbs, pts, [8], max_dist=np.inf)[8]                      # +inf = no limit when no distance is NaN
    assert np.array_equal(s, free[0]) and kr.same(d, free[1])
    s, d = ktr.knearest_tree(nodes, aabbs, pts, [8], max_dist=-0.0)[8]                        # -0 >= 0 holds: the same as 0
    assert np.array_equal(s, zero[0]) and kr.same(d, zero[1])
    mixed = np.array([np.inf, -1, np.nan, 0] * 3, dtype=dtype)[: len(pts)]                    # per point
    s, d = ktr.knearest_tree(nodes, aabbs, pts, [8], max_dist=mixed)[8]
    for r, m in enumerate(mixed):
        want = free if m == np.inf else zero if m == 0 else None
        if want is None:
            assert (s[r] == NONE).all() and np.isposinf(d[r]).all()
        else:
            assert np.array_equal(s[r], want[0][r]) and kr.same(d[r], want[1][r])
