"""k-nearest point queries on the CPU: the new entry points are declared, exported and bound in every layer, and the definition the
GPU tests pin (tests/knn_ref.py; include/bvh_mi355x.h, bvhgpu_knearest_*) is checked against itself: k = 1 is the oracle's nearest_to,
hand-written answers on the 21 aligned boxes, brute force where the arithmetic is exact, and the vectorised distances of knn_ref are
bit-equal to the oracle's scalar ones."""
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref as kr
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_knearest_f32", "bvhgpu_knearest_f64"]
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]


def extreme_points(dtype, centre):
    """query points with NaN / infinite / max-finite / subnormal coordinates (the values of tests/test_gpu_fp_extremes.py)"""
    fi = np.finfo(dtype)
    c = np.asarray(centre, dtype=np.float64)
    vals = [np.nan, np.inf, -np.inf, float(fi.max), -float(fi.max), float(fi.smallest_subnormal), -float(fi.smallest_subnormal)]
    pts = []
    for v in vals:
        for axis in range(3):
            p = c.copy(); p[axis] = v
            pts.append(p)
        pts.append(np.full(3, v))
    pts.append(np.array([np.inf, -np.inf, np.nan]))
    pts.append(np.array([float(fi.max), float(fi.smallest_subnormal), 0.0]))
    with np.errstate(over="ignore"):
        return np.asarray(pts).astype(dtype)


def cube_scene(n_cubes, dtype):
    tris32, aabbs32 = orc.create_n_cubes(n_cubes)
    return tris32.astype(dtype), aabbs32.astype(dtype)


def integer_cloud(dtype, hi, n=4096, seed=7):
    """n points at integer coordinates in [0, hi]^3 (duplicates allowed) as zero-size boxes and as point triangles (a = b = c)"""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, hi + 1, size=(n, 3)).astype(dtype)
    return np.concatenate([pts, pts], axis=1), np.repeat(pts[:, None, :], 3, axis=1)


def half_grid_queries(dtype, hi, n, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2 * hi + 2, size=(n, 3)) * 0.5).astype(dtype)


# ---- 1. every layer --------------------------------------------------------------------------------------------------------
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
        assert name in lib_rs, f"{name} is no impl_gpu_scalar! entry"
    assert "pub fn nearest_k(" in lib_rs
    from bvh_amd.api import Bvh, _TreeBase
    assert callable(getattr(_TreeBase, "knearest_batch", None)) and callable(getattr(Bvh, "knearest_batch", None))
    assert _lib.KNN_MAX_K == 64


# ---- 5. header text ----------------------------------------------------------------------------------------------------------
def test_header_names_padding_and_limit():
    h = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert re.search(r"#define BVHGPU_KNN_MAX_K 64u?\b", h)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define BVHGPU_KNN_MAX_K[^\n]*\n\s*int bvhgpu_knearest_f32", h, flags=re.S)
    assert m, "bvhgpu_knearest_* has no comment in front of it"
    text = " ".join(m.group(1).split())
    assert "BVHGPU_NONE" in text and "+inf" in text and "PADDING" in text.upper()
    assert "BVHGPU_KNN_MAX_K" in text and "strict <" in text


# ---- the vectorised distances are the oracle's ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_vector_distances_equal_the_oracles_scalar_ones(dtype):
    """knn_ref.dists_vector against one oracle call per distance, bit for bit (two NaNs equal): cube scene, degenerate triangles,
    ordinary points, points on vertices and the extremes"""
    from test_fp_extremes_cpu import degenerate_triangles
    tris, aabbs = cube_scene(20, dtype)                                   # 240 triangles
    deg = np.asarray(degenerate_triangles(dtype), dtype=dtype).reshape(-1, 3, 3)
    tris = np.concatenate([tris, deg])
    aabbs = np.concatenate([aabbs, np.concatenate([deg.min(axis=1), deg.max(axis=1)], axis=1)])
    flat = orc.flatten(orc.build(aabbs).nodes)
    rng = np.random.default_rng(3)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    pts = np.concatenate([rng.uniform(lo - (hi - lo) / 2, hi + (hi - lo) / 2, size=(8, 3)).astype(dtype), tris[::40, 1],
                          tris[::50].mean(axis=1).astype(dtype), deg[:, 0], extreme_points(dtype, (lo + hi) / 2)[::3]])
    for p in pts:
        for t in (None, tris):
            md_s, d_s = kr.dists_scalar(flat, aabbs, p, dtype, t)
            md_v, d_v = kr.dists_vector(flat, aabbs, p, dtype, t)
            nav = flat["entry"] != NONE
            assert kr.same(md_s[nav], md_v[nav]) and kr.same(d_s, d_v), (p, t is not None)


# ---- 2. k = 1 is nearest_to ---------------------------------------------------------------------------------------------------
def _k1_equals_nearest(flat, aabbs, pts, tris):
    got = kr.knearest(flat, aabbs, pts, [1], tris)[1]
    ws, wd = orc.nearest(flat, aabbs, pts, tris)
    assert np.array_equal(got[0][:, 0], ws) and kr.same(got[1][:, 0], wd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_k1_equals_oracle_nearest(dtype):
    boxes = orc.aligned_boxes().astype(dtype)
    flat = orc.flatten(orc.build(boxes).nodes)
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-12, 12, size=(200, 3)), np.stack([np.arange(-11, 11.5, 0.5)] + [np.zeros(45)] * 2, axis=1)]).astype(dtype)
    _k1_equals_nearest(flat, boxes, pts, None)
    _k1_equals_nearest(flat, boxes, extreme_points(dtype, [0.25, 0, 0]), None)
    tris, aabbs = cube_scene(100, dtype)                                  # 1 200 triangles
    flat = orc.flatten(orc.build(aabbs).nodes)
    lo, hi = aabbs[:, :3].min(axis=0), aabbs[:, 3:].max(axis=0)
    pts = np.concatenate([rng.uniform(lo * 2, hi * 2, size=(150, 3)).astype(dtype), tris[::30].mean(axis=1).astype(dtype), tris[::60, 2],
                          extreme_points(dtype, (lo + hi) / 2)])
    for t in (None, tris):
        _k1_equals_nearest(flat, aabbs, pts, t)


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answers_on_aligned_boxes(dtype):
    """unit boxes centred at x = -10..10, shape = x + 10, neighbours touch at +-0.5, +-1.5, ...: arithmetic on quarters"""
    boxes = orc.aligned_boxes().astype(dtype)
    flat = orc.flatten(orc.build(boxes).nodes)
    pts = np.array([[0.25, 0, 0], [0.75, 0, 0], [0.5, 0, 0]], dtype=dtype)
    for dists in (kr.dists_vector, kr.dists_scalar):
        shape, dist = kr.knearest(flat, boxes, pts, [3], None, dists)[3]
        assert shape.tolist() == [[10, 11, 9], [11, 10, 12], [10, 11, 9]]       # the tie: both at 0, the earlier in leaf pre-order first
        assert dist.tolist() == [[0, 0.25, 0.75], [0, 0.25, 0.75], [0, 0, 1]]
    order = kr.leaf_preorder(flat)
    assert order.index(10) < order.index(11)


# ---- 4. brute force where arithmetic is exact ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hi", [255, 63])
@pytest.mark.parametrize("dtype", DTYPES)
def test_definition_equals_brute_force_on_integer_cloud(dtype, hi):
    """4 096 zero-size boxes at integer coordinates, queries at multiples of 0.5: every operation of both distances is exact, so the
    loop must give the first k of the stable sort in leaf pre-order for EVERY query; ties at the k-th place must occur (counted)"""
    aabbs, tris = integer_cloud(dtype, hi)
    flat = orc.flatten(orc.build(aabbs).nodes)
    n_q = 256 if hi == 255 else 64
    qs = half_grid_queries(dtype, hi, n_q)
    ks = [1, 2, 7, 64]
    fl = kr.flat_lists(flat)
    ties = 0
    for kind_tris in (None, tris):
        for qi, p in enumerate(qs):
            md, d = kr.dists_vector(flat, aabbs, p, dtype, kind_tris)
            if qi % 16 == 0:                                                      # the oracle's own floats on a sample, the same values
                _, d_s = kr.dists_scalar(flat[:0], aabbs[::64], p, dtype, None if kind_tris is None else kind_tris[::64])
                assert kr.same(d_s, d[::64])
            mdl, dl = md.tolist(), d.tolist()
            srt = np.sort(d, kind="stable")
            for k in ks:
                ld, ls = kr.walk(fl, mdl, dl, k)
                bd, bs = kr.brute_force(flat, d, k)
                assert ls == bs and ld == bd, (hi, qi, k, kind_tris is not None)
                ties += int(srt[k - 1] == srt[k])
    print(f"ties at the k-th place: {ties} of {2 * n_q * len(ks)} (query, k, kind) cases")
    assert ties > 0, "no tie at the k-th place: the tie rule was not exercised"
