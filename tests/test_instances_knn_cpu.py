"""k-nearest over instanced scenes, CPU side: the reference walk (tests/instances_knn_ref.py `rows`, the definition with its prunes) against
the same insertion over ALL pairs with no tree (`brute`) — row for row, order included, no exception; that the prune prunes; the ties of
the line of instances; hand cases; and the wiring of the new HIP file into the build.  tests/test_gpu_instances_knn.py holds the engine
to `rows` on these scenes."""
import os

import numpy as np
import pytest

import instances_knn_ref as ikr
import instances_ref as ir
import instances_within_ref as iwr
from test_instances_cpu import SIZES, case, member_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
N_POINTS = 600          # what the GPU test runs
N_CPU = 200             # what the brute force is run on
KS = (1, 5, 64)
LINE_KS = (1, 2, 3, 4, 7, 64)
NONE = ikr.NONE


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the cluster scenes --------------------------------------------------------------------------------------------------------------------
_CLUSTER = {}


def cluster(orc, dtype, n):
    """case(orc, dtype, n)'s scene with instances_within_ref.cluster_points (limits ignored) and the distance cache every k shares
    → (scene case, points[600], cache)"""
    key = (np.dtype(dtype).name, n)
    if key not in _CLUSTER:
        pts, _ = iwr.cluster_points(n, dtype, N_POINTS)
        _CLUSTER[key] = (pts, {})
    return (case(orc, dtype, n),) + _CLUSTER[key]


_ROWS = {}


def cluster_rows(orc, dtype, n, k, count=N_POINTS):
    """the reference rows of the first `count` points (computed once per (scene, k, count), never modified) → (rows, stats)"""
    key = (np.dtype(dtype).name, n, k, count)
    if key not in _ROWS:
        c, pts, cache = cluster(orc, dtype, n)
        stats = {}
        _ROWS[key] = (ikr.rows(c["scene"], pts[:count], k, stats, cache), stats)
    return _ROWS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", KS)
def test_rows_equal_brute_force(orc, dtype, n, k):
    """a condition, not a tolerance: the walk with its prunes gives, row for row and in order, the list built from all pairs"""
    c, pts, cache = cluster(orc, dtype, n)
    rows, _ = cluster_rows(orc, dtype, n, k, N_CPU)
    want = ikr.brute(c["scene"], pts[:N_CPU], k, cache)
    bad = [j for j in range(N_CPU) if rows[j] != want[j]]
    assert not bad, (bad[:5], rows[bad[0]][:3], want[bad[0]][:3])
    total = sum(len(c["scene"].trees[int(t)][1]) for t in c["scene"].tree_of)             # (instance, triangle) pairs in the scene
    assert all(len(r) == min(k, total) for r in rows)
    for r in rows:                                            # ascending, no pair twice
        assert all(r[m][0] <= r[m + 1][0] for m in range(len(r) - 1)) and len(set((i, s) for _, i, s in r)) == len(r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_prune_prunes(orc, dtype):
    """37 instances, 3 743 triangles, k = 1: the mean number of member leaves offered per point is below half the triangle count, and
    instances are skipped as well"""
    c, pts, cache = cluster(orc, dtype, 37)
    sc = c["scene"]
    n_tris = sum(len(sc.trees[int(t)][1]) for t in sc.tree_of)
    assert n_tris == 3743
    _, stats = cluster_rows(orc, dtype, 37, 1, N_CPU)
    leaves, entered = stats["leaves"] / N_CPU, stats["instances"] / N_CPU
    print("leaves offered per point:", leaves, "instances entered per point:", entered)
    assert leaves < n_tris / 2
    assert entered < 37                                       # whole instances are skipped
    # k = 64 looks at more than k = 1 and still not at everything
    _, s64 = cluster_rows(orc, dtype, 37, 64, N_CPU)
    assert stats["leaves"] < s64["leaves"] < n_tris * N_CPU


# ---- the line of instances: ties ---------------------------------------------------------------------------------------------------------
_LINE = {}
LINE_POINTS = [[100.5, 0, 0], [1, 0, 0], [5000, 0, 0], [32.5, 0, 0]]


def line_case(orc, dtype):
    key = np.dtype(dtype).name
    if key not in _LINE:
        trees, tree_of, x = iwr.line_instances(dtype)
        sc = ir.Scene(trees, tree_of, x, dtype)
        pts = np.array(LINE_POINTS, dtype=dtype)
        cache = {}
        _LINE[key] = dict(trees=trees, tree_of=tree_of, x=x, scene=sc, points=pts, rows={k: ikr.rows(sc, pts, k, None, cache) for k in LINE_KS}, cache=cache)
    return _LINE[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene_ties(orc, dtype):
    s = line_case(orc, dtype)
    sc, pts = s["scene"], s["points"]
    assert len(sc.x) == 66
    order = ikr.kr.leaf_preorder(sc.top)
    rank = {i: r for r, i in enumerate(order)}
    member_rank = {sh: r for r, sh in enumerate(ikr.kr.leaf_preorder(sc.flats[0]))}
    for k in LINE_KS:
        assert s["rows"][k] == ikr.brute(sc, pts, k, s["cache"]), k
    # (100.5, 0, 0): x = 100 and x = 101 are both 0.5 away (d = 0.25), x = 99 and x = 102 both 1.5 away (d = 2.25)
    r1, r2, r3, r4 = (s["rows"][k][0] for k in (1, 2, 3, 4))
    assert [e[0] for e in r2] == [0.25, 0.25] and [e[0] for e in r4] == [0.25, 0.25, 2.25, 2.25]
    first, second = r2
    assert (rank[first[1]], member_rank[first[2]]) < (rank[second[1]], member_rank[second[2]])          # the double order
    assert r1 == [first]                                      # k = 1 keeps the one met first
    assert r3 == r4[:3]                                       # k = 3 cuts the next tie: the one met first stays
    assert (rank[r4[2][1]], member_rank[r4[2][2]]) < (rank[r4[3][1]], member_rank[r4[3][2]])
    # (1, 0, 0) lies on the triangle at x = 1, which instance 0 and its coincident copy 64 both hold: distance 0 twice
    z = s["rows"][2][1]
    assert [e[0] for e in z] == [0.0, 0.0] and sorted(e[1] for e in z) == [0, 64] and z[0][2] == z[1][2]
    assert rank[z[0][1]] < rank[z[1][1]]
    assert s["rows"][1][1] == [z[0]]
    # every row of k = 64 is full and ascending
    for r in s["rows"][64]:
        assert len(r) == 64 and all(r[m][0] <= r[m + 1][0] for m in range(63))


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_pairs_than_k_gives_padding(orc, dtype):
    """one instance of the one-triangle member, k = 5: one entry and four padded slots"""
    tri_member = member_trees(orc, dtype)[2]
    assert len(tri_member[1]) == 1
    x = np.eye(3, 4, dtype=dtype)[None].copy()
    x[0, 0, 3] = 2
    sc = ir.Scene([tri_member], [0], x, dtype)
    pts = np.array([[0, 0, 0], [7, -3, 2]], dtype=dtype)
    rows = ikr.rows(sc, pts, 5)
    assert [len(r) for r in rows] == [1, 1] and rows == ikr.brute(sc, pts, 5)
    inst, shape, dist = ikr.padded(rows, 5, dtype)
    assert inst.tolist() == [[0] + [NONE] * 4] * 2 and shape.tolist() == [[0] + [NONE] * 4] * 2
    assert np.isfinite(dist[:, 0]).all() and np.isposinf(dist[:, 1:]).all() and dist.dtype == dtype
    empty = ir.Scene([tri_member], [], np.zeros((0, 3, 4), dtype=dtype), dtype)
    assert ikr.rows(empty, pts, 3) == [[], []] and ikr.brute(empty, pts, 3) == [[], []]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", (1, 3, 64))
def test_nan_coordinate_against_brute(orc, dtype, k):
    """a NaN coordinate makes every distance NaN: accepted only while the list is not full, never replaced, no box test passes"""
    c = case(orc, dtype, 37)
    pts = np.array([[np.nan, 0, 0], [0, np.nan, 1], [np.nan] * 3, [0.5, 0.5, 0.5]], dtype=dtype)
    rows = ikr.rows(c["scene"], pts, k)
    assert ikr.same_rows(rows, ikr.brute(c["scene"], pts, k))
    for r in rows[:3]:
        assert len(r) == k and all(e[0] != e[0] for e in r)
    assert all(e[0] == e[0] for e in rows[3])


def test_the_reference_stands_alone():
    src = open(os.path.join(ROOT, "tests", "instances_knn_ref.py")).read()
    assert "import bvh_amd" not in src and "from bvh_amd" not in src


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_are_built_and_bound():
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances_knn.hip" in build_ext.SOURCES and "instances_arrays.hpp" in build_ext.HEADERS
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_instances_knearest", b"k_instances_knn_fill"):
        assert kern in blob, kern
    names = {s[0] for s in _lib.SYMBOLS}
    for sym in ("bvhgpu_instances_knearest_f32", "bvhgpu_instances_knearest_f64"):
        assert sym in names
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert "#define BVHGPU_INSTANCES_KNN_MAX_K %du" % _lib.INSTANCES_KNN_MAX_K in header
    import bvh_amd
    assert hasattr(bvh_amd.Instances, "knearest_batch") and hasattr(bvh_amd.Instances, "nearest_batch")
    assert not hasattr(bvh_amd, "instances_knearest_batch")     # no module-level function
