"""The sphere distance of the point families (bvhgpu_knearest_sphere_* / _knearest_tree_sphere_* / _within_sphere_*) on the
reference alone (tests/sphere_dist_ref.py): hand anchors that are exact in f32 and f64, the scalar form against the vector form, and
what the scenes of tests/test_gpu_sphere_dist.py contain — shown here so that the GPU test's byte comparison is known to exercise them.
Needs no GPU."""
import os
import re

import numpy as np
import pytest

import knn_ref as kr
import sphere_dist_ref as sr
import within_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
KS = [1, 10, 11, 16, 17, 21, 22, 32, 33, 64]     # both sides of every topk_block boundary (f32: 16 | 17, 32 | 33; f64: 10 | 11, 21 | 22)
ENTRIES = [f"bvhgpu_{stem}_{sfx}" for stem in ("knearest_sphere", "knearest_tree_sphere", "within_sphere") for sfx in ("f32", "f64")]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


# ---------------------------------------------------------------------------------------------------------------- the distance
@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_anchors(dtype):
    unit = np.array([[0, 0, 0, 1]], dtype=dtype)

    def d(spheres, p):
        v = sr.sphere_dist2_v(np.asarray(spheres, dtype=dtype), np.asarray(p, dtype=dtype))
        assert v.dtype == dtype
        return v[0]

    assert d(unit, [3, 0, 0]) == 4 and np.sqrt(d(unit, [3, 0, 0])) == 2
    assert d(unit, [0, 4, 3]) == 16 and np.sqrt(d(unit, [0, 4, 3])) == 4
    assert d(unit, [0.5, 0, 0]) == 0 and d(unit, [1, 0, 0]) == 0                       # inside, and on the surface
    assert d([[1, 2, 2, 0]], [0, 0, 0]) == 9 and np.sqrt(d([[1, 2, 2, 0]], [0, 0, 0])) == 3
    assert d([[0, 0, 0, -1]], [3, 0, 0]) == 16 and d([[1, 2, 2, -1]], [0, 0, 0]) == 16   # r = -1: (len + 1)^2
    assert np.isnan(d([[np.nan, 0, 0, 1]], [3, 0, 0])) and np.isnan(d([[0, 0, 0, np.nan]], [3, 0, 0])) and np.isnan(d(unit, [0, np.nan, 0]))
    assert d([[0, 0, 0, np.inf]], [3, 0, 0]) == 0
    assert np.isnan(d([[0, 0, 0, np.inf]], [np.inf, 0, 0]))                              # len = +inf too: inf - inf
    big = 1e19 if dtype == np.float32 else 1e154
    assert np.isposinf(d([[big, big, big, 1]], [-big, -big, -big]))                      # s2 overflows: len = +inf, d = +inf
    assert d([[0, 0, 0, -0.0]], [0, 0, 0]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_form_equals_vector_form(dtype):
    rng = np.random.default_rng(3)
    s = np.empty((4000, 4), dtype=dtype)
    s[:, :3] = rng.uniform(-10, 10, size=(4000, 3))
    s[:, 3] = rng.uniform(0, 3, size=4000)
    fi = np.finfo(dtype)
    odd = [0, -1, np.inf, np.nan, float(fi.smallest_subnormal), float(fi.max), -0.0]
    s[np.arange(len(odd)) * 3, 3] = odd
    s[100:140, 0] = np.resize([np.nan, np.inf, -np.inf, float(fi.max)], 40)
    s[200:220, :3] = 1e19 if dtype == np.float32 else 1e154
    pts = np.concatenate([rng.uniform(-12, 12, size=(6, 3)), [[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [float(fi.max)] * 3, [0, 0, 0]]]).astype(dtype)
    for p in pts:
        v = sr.sphere_dist2_v(s, p)
        w = np.array([sr.sphere_dist2_s(row, p, dtype) for row in s], dtype=dtype)
        assert v.dtype == w.dtype == dtype and kr.same(v, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inscribed_box_distance_never_exceeds_ball_distance(dtype):
    """the premise of "rows are the k nearest where every sphere lies inside its box": on the committed scenes no pair (sphere, point) has
    the box distance above the ball distance, so no walk prunes a sphere that brute force would keep"""
    for n in (12, 700, 2300):
        spheres, aabbs = sr.ball_scene(n, dtype)
        for p in sr.query_points(spheres, dtype):
            with np.errstate(all="ignore"):
                box = kr.aabb_min_dist2_v(aabbs[:, :3], aabbs[:, 3:], p)
                ball = sr.sphere_dist2_v(spheres, p)
            assert not (box > ball).any()


# ---------------------------------------------------------------------------------------------------------------- what the scenes contain
def _scene(orc, n, dtype):
    spheres, aabbs = sr.ball_scene(n, dtype)
    nodes = orc.build(aabbs).nodes
    return spheres, aabbs, nodes, orc.flatten(nodes), sr.query_points(spheres, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_knearest_scene_contents(orc, dtype):
    spheres, aabbs, nodes, oflat, pts = _scene(orc, 700, dtype)
    ks = [1, 10, 33]
    flat_rows = sr.knearest(oflat, aabbs, spheres, pts, ks)
    tree_rows = sr.knearest_tree(nodes, aabbs, spheres, pts, ks)
    d10 = flat_rows[10][1]
    assert (d10[:, 0] == 0).sum() >= 40 and (d10[:, 0] > 100).sum() >= 10              # points inside a ball; points far outside
    for k in ks:
        assert kr.same(flat_rows[k][1], tree_rows[k][1])                                 # the two forms agree in distances
    # ties straddle the k-th slot: the (k+1)-th of brute force is as far as the k-th
    brute11 = sr.brute_rows(oflat, spheres, pts, 11)
    assert sum(1 for ld, _ in brute11 if ld[9] == ld[10]) >= 5
    # inscribed spheres: every row is the stable brute-force sort over all spheres
    for k in ks:
        for r, (ld, ls) in enumerate(sr.brute_rows(oflat, spheres, pts, k)):
            ws, wd = kr.row(ld, ls, k, dtype)
            assert np.array_equal(flat_rows[k][0][r], ws) and kr.same(flat_rows[k][1][r], wd), (k, r)
    # rows shorter than, equal to and longer than k
    s12, a12, n12, f12, p12 = _scene(orc, 12, dtype)
    few = sr.knearest(f12, a12, s12, p12, [11, 12, 13])
    assert (few[13][0][:, 12] == kr.NONE).all() and (few[12][0] != kr.NONE).all() and (few[11][0] != kr.NONE).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_enlarged_spheres_show_that_the_definition_is_the_walk(orc, dtype):
    """radii six times as large over the SAME boxes: spheres reach outside their boxes, the box pruning drops some that brute force
    keeps, and the comparison can tell — at least one row differs from the brute-force sort"""
    spheres, aabbs, nodes, oflat, pts = _scene(orc, 700, dtype)
    big = sr.enlarged(spheres)
    rows = sr.knearest(oflat, aabbs, big, pts, [10])[10]
    differ = 0
    for r, b in enumerate(sr.brute_rows(oflat, big, pts, 10)):
        ws, wd = kr.row(*b, 10, dtype)
        differ += not (np.array_equal(rows[0][r], ws) and kr.same(rows[1][r], wd))
    assert differ >= 1
    lists = sr.within_rows(oflat, aabbs, big, pts, 1.0)
    full = [int((sr.sphere_dist2_v(big, p) <= 1).sum()) for p in pts]
    assert any(len(ls) < f for (_, ls), f in zip(lists, full))                           # within misses some, too


@pytest.mark.parametrize("dtype", DTYPES)
def test_within_scene_contents(orc, dtype):
    spheres, aabbs, nodes, oflat, pts = _scene(orc, 2300, dtype)
    lim = within_limits(len(pts), dtype)
    rows = sr.within_rows(oflat, aabbs, spheres, pts, lim)
    lens = np.array([len(ls) for _, ls in rows])
    assert (lens == 0).any() and ((lens > 0) & (lens <= wr.LANE_MAX)).any() and ((lens > wr.LANE_MAX) & (lens <= wr.LDS_MAX)).any()
    assert (lens > wr.LDS_MAX).any() and lens.max() == 2300
    for i, (ld, ls) in enumerate(rows):                                                  # inscribed: the geometric answer
        if lim[i] >= 0:
            d = sr.sphere_dist2_v(spheres, pts[i])
            assert sorted(ls) == np.nonzero(d <= lim[i] * lim[i])[0].tolist()
    # a row no longer than k holds the same pairs as the tree form with that limit
    tree = sr.knearest_tree(nodes, aabbs, spheres, pts, [64], lim)[64]
    for i, (ld, ls) in enumerate(rows):
        if len(ls) <= 64:
            sd, ss = wr.sort_row(ld, ls)
            m = len(ss)
            assert sorted(ss) == sorted(tree[0][i, :m].tolist()) and (tree[0][i, m:] == kr.NONE).all()
            assert kr.same(np.sqrt(np.asarray(sd, dtype=dtype)), tree[1][i, :m])            # bit-equal distances; only ties may be ordered differently


def within_limits(n, dtype):
    """per-point limits of the GPU test's within scene: rows of every tier, and 0, a negative value, NaN and +inf"""
    m = np.resize(np.array([0.5, 3.0, 8.0, 1.5, 0.0, -1.0, np.nan, 5.0], dtype=dtype), n).copy()
    m[:4] = np.inf
    return m


# ---------------------------------------------------------------------------------------------------------------- the six entries
def test_the_six_entries_are_declared_bound_and_in_the_rust_source():
    from bvh_amd import _lib
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    capi = open(os.path.join(ROOT, "bvh_amd", "csrc", "capi.hip")).read()
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read()
    bound = {name: args for name, _res, args in _lib.SYMBOLS}
    for e in ENTRIES:
        assert re.search(r"^int %s\(bvhgpu_tree \*tree, " % e, header, re.M), e
        assert re.search(r"^int %s\(bvhgpu_tree\* t, " % e, capi, re.M), e
        assert e in bound and f"pub fn {e}(t: *mut bvhgpu_tree, " in ffi and f"ffi::{e}(" in rust, e
    assert len(bound["bvhgpu_knearest_sphere_f32"]) == len(bound["bvhgpu_knearest_f32"]) - 1      # the unsuffixed entry without `kind`
    assert len(bound["bvhgpu_knearest_tree_sphere_f64"]) == len(bound["bvhgpu_knearest_tree_f64"]) - 1
    assert len(bound["bvhgpu_within_sphere_f32"]) == len(bound["bvhgpu_within_f32"]) - 1
    assert "sphere distance needs bvhgpu_tree_set_spheres first" in capi
    assert "#define BVHGPU_ABI_VERSION 7" in header.replace("  ", " ") or re.search(r"BVHGPU_ABI_VERSION\s+7\b", header)
