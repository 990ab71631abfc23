"""Nearest-first k-nearest over instanced scenes, CPU side: the reference descent with its prunes (tests/instances_knn_tree_ref.py `rows`)
against the same insertion over ALL pairs in the nearest-first order with no box test (`ordered_brute`) — row for row, order included, no
exception; its distances against the flat form's and the radius search's references; that the prune prunes; the row kinds under limits;
the ties of the line of instances; splits without SAH winner, single leaves and NaN coordinates; and the wiring of the new HIP file.
tests/test_gpu_instances_knn_tree.py holds the engine to `rows` on these scenes."""
import os

import numpy as np
import pytest

import instances_knn_ref as ikr
import instances_knn_tree_ref as iktr
import instances_ref as ir
import instances_within_ref as iwr
from test_instances_cpu import SIZES, case, member_trees
from test_instances_knn_cpu import LINE_KS, N_CPU, N_POINTS, cluster, cluster_rows as flat_cluster_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
KS = (1, 5, 64)
LIMITS = ("none", "drawn", "special")
NONE = iktr.NONE


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the cluster scenes --------------------------------------------------------------------------------------------------------------------
def limits_of(kind, dtype, n_instances, count=N_POINTS):
    """none: no limit; drawn: instances_within_ref.cluster_points' own limits; special: 0, negative, NaN, +inf and 2.5 in turn"""
    if kind == "none":
        return None
    if kind == "drawn":
        return np.ascontiguousarray(iwr.cluster_points(n_instances, dtype, N_POINTS)[1][:count])
    return iktr.special_limits(count, dtype)


_ROWS = {}


def cluster_rows(orc, dtype, n, k, kind, count=N_POINTS):
    """the reference rows of the first `count` points (computed once per (scene, k, limits, count), never modified) → (rows, stats)"""
    key = (np.dtype(dtype).name, n, k, kind, count)
    if key not in _ROWS:
        c, pts, cache = cluster(orc, dtype, n)
        stats = {}
        _ROWS[key] = (iktr.rows(c["scene"], pts[:count], k, limits_of(kind, dtype, n, count), stats, cache), stats)
    return _ROWS[key]


@pytest.mark.parametrize("kind", LIMITS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", KS)
def test_rows_equal_ordered_brute(orc, dtype, n, k, kind):
    """a condition, not a tolerance: the descent with its prunes gives, row for row and in order, the list built from all pairs offered in
    the nearest-first order"""
    c, pts, cache = cluster(orc, dtype, n)
    rows, _ = cluster_rows(orc, dtype, n, k, kind, N_CPU)
    want = iktr.ordered_brute(c["scene"], pts[:N_CPU], k, limits_of(kind, dtype, n, N_CPU), None, cache)
    bad = [j for j in range(N_CPU) if rows[j] != want[j]]
    assert not bad, (bad[:5], rows[bad[0]][:3], want[bad[0]][:3])
    for r in rows:                                            # ascending, no pair twice
        assert all(r[m][0] <= r[m + 1][0] for m in range(len(r) - 1)) and len(set((i, s) for _, i, s in r)) == len(r)
    if kind == "none":
        total = sum(len(c["scene"].trees[int(t)][1]) for t in c["scene"].tree_of)
        assert all(len(r) == min(k, total) for r in rows)
    if kind == "special":
        m = limits_of(kind, dtype, n, N_CPU)
        for j, r in enumerate(rows):
            if j % 5 in (1, 2):
                assert r == []                                # a negative or NaN limit: padding
            elif j % 5 == 0:
                assert all(e[0] == 0 for e in r)              # a limit of 0 keeps only distance 0
            elif j % 5 == 4:
                assert all(e[0] <= m[j] * m[j] for e in r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", KS)
def test_distances_equal_the_flat_forms(orc, dtype, n, k):
    """without a limit every row's distances equal instances_knn_ref.rows' bit for bit (the pairs may differ at tied distances)"""
    rows, _ = cluster_rows(orc, dtype, n, k, "none", N_CPU)
    flat, _ = flat_cluster_rows(orc, dtype, n, k, N_CPU)
    assert [[e[0] for e in r] for r in rows] == [[e[0] for e in r] for r in flat]
    # +inf as every point's limit is no limit
    c, pts, cache = cluster(orc, dtype, n)
    assert iktr.rows(c["scene"], pts[:50], k, np.inf, None, None) == rows[:50]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,scale", ((1, 0.5), (2, 0.5), (37, 0.25)))
def test_distances_equal_the_radius_searchs(orc, dtype, n, scale):
    """with a limit and k above the longest row, every row's distances are the sorted instances_within_ref row's, and so is its set of
    pairs.  The drawn limits give rows of up to 777 pairs and the largest k is 64, so they are scaled by a power of two (exact in T) until
    the longest row is below 64 — which is asserted, not assumed"""
    c, pts, cache = cluster(orc, dtype, n)
    m = (limits_of("drawn", dtype, n, N_CPU) * dtype(scale)).astype(dtype)
    within = iwr.rows(c["scene"], pts[:N_CPU], m)
    longest = max(len(r) for r in within)
    assert 1 < longest < 64, longest
    rows = iktr.rows(c["scene"], pts[:N_CPU], 64, m, None, cache)
    assert [[e[0] for e in r] for r in rows] == [sorted(e[0] for e in r) for r in within]
    assert [sorted((i, s) for _, i, s in r) for r in rows] == [sorted((i, s) for _, i, s in r) for r in within]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_prune_prunes(orc, dtype):
    """37 instances, k = 1: fewer member leaves are offered per point than by the flat form's reference on the same points"""
    for k in KS:
        _, tree = cluster_rows(orc, dtype, 37, k, "none", N_CPU)
        _, flat = flat_cluster_rows(orc, dtype, 37, k, N_CPU)
        print("k = %d: member leaves offered per point: tree form %.1f, flat form %.1f; instances entered per point: %.1f against %.1f"
              % (k, tree["leaves"] / N_CPU, flat["leaves"] / N_CPU, tree["instances"] / N_CPU, flat["instances"] / N_CPU))
        if k == 1:
            assert tree["leaves"] < flat["leaves"]
            assert tree["instances"] < flat["instances"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_kinds_under_limits(orc, dtype):
    """the drawn limits on the 37-instance scene at k = 64: empty, partly filled and full rows each occur at least 20 times"""
    rows, _ = cluster_rows(orc, dtype, 37, 64, "drawn", N_CPU)
    lens = [len(r) for r in rows]
    empty, full = lens.count(0), lens.count(64)
    assert empty >= 20 and full >= 20 and N_CPU - empty - full >= 20, (empty, N_CPU - empty - full, full)


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
        _LINE[key] = dict(trees=trees, tree_of=tree_of, x=x, scene=sc, points=pts, cache=cache,
                          rows={k: iktr.rows(sc, pts, k, None, None, cache) for k in LINE_KS})
    return _LINE[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene_ties(orc, dtype):
    s = line_case(orc, dtype)
    sc, pts = s["scene"], s["points"]
    assert len(sc.x) == 66
    for k in LINE_KS:
        assert s["rows"][k] == iktr.ordered_brute(sc, pts, k, None, None, s["cache"]), k
    flat2 = ikr.rows(sc, pts, 2, None, s["cache"])
    # (100.5, 0, 0): x = 100 and x = 101 are both 0.5 away (d = 0.25); (1, 0, 0) lies on the triangle instance 0 and its copy 64 both hold
    for j, d in ((0, 0.25), (1, 0.0)):
        r1, r2 = s["rows"][1][j], s["rows"][2][j]
        assert [e[0] for e in r2] == [d, d]
        assert r1 == r2[:1]                                   # k = 1 keeps the one met first
        assert sorted(e[1:] for e in r2) == sorted(e[1:] for e in flat2[j])      # the tied pairs are both present
    assert sorted(e[1] for e in s["rows"][2][1]) == [0, 64]
    assert [e[0] for e in s["rows"][4][0]] == [0.25, 0.25, 2.25, 2.25]
    for r in s["rows"][64]:
        assert len(r) == 64 and all(r[m][0] <= r[m + 1][0] for m in range(63))
    # with a limit of 0.5 the ties at the limit stay (<=) and nothing else; x = 32 and x = 33 belong to instance 0 and to its copy 64
    assert [[e[0] for e in r] for r in iktr.rows(sc, pts, 64, 0.5)] == [[0.25, 0.25], [0.0, 0.0], [], [0.25] * 4]


# ---- a split without SAH winner ------------------------------------------------------------------------------------------------------------
SAH_CASES = (("member", (1, 5, 64)), ("top", (1, 2, 7, 64)))      # tests/test_gpu_instances_knn.py's two scenes with the k each is run at


def _sah_scene(dtype, which):
    """a member whose root split has no SAH winner (both child boxes Aabb::empty()), alone under a mirrored non-uniform scaling; and three
    instances of it, two with coincident world boxes, so that the top level's split has none either"""
    sc, _, _, pts = iktr.far_member_scene(dtype) if which == "member" else iktr.coincident_scene(dtype)
    top, members = iktr.node_arrays(sc)
    assert iktr.has_empty_child(members[0])                   # the scene really contains an Aabb::empty() child box
    if which == "top":
        assert iktr.has_empty_child(top) and sc.w[0].tobytes() == sc.w[1].tobytes() != sc.w[2].tobytes()
    return sc, pts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which,ks", SAH_CASES)
def test_split_without_sah_winner(orc, dtype, which, ks):
    """rows == ordered_brute on the two scenes, every row, without a limit and with a limit of 0.3 of the scene's size.

    A split loses its SAH winner only when the surface areas overflow, so the coordinates reach 1e19 (f32) / 1e154 (f64) and squared
    distances reach T's largest number: once a list's bound lies above max / F, `bound * F` is +inf.  This is the test admit_b's last
    clause exists for.  With the plain `x < bound * F` a member box whose object-frame distance overflowed as well gave inf < inf = false
    and was pruned although a triangle in it had a finite world distance below the bound; rows that then differed, of 250 (f32 / f64):
    member scene k = 5: 0 / 2, k = 64: 43 / 151; top scene k = 7: 0 / 1, k = 64: 20 / 48.  (The special limits are left out here: a
    limit of 0 leaves no room for the rounding of q, and the points on world vertices of a scaled instance at 1e19 need some — DESIGN.md
    §4q.)"""
    sc, pts = _sah_scene(dtype, which)
    limit = dtype(0.3 * float(np.abs(pts[:150]).max()))
    cache = {}
    differ = {}
    for k in ks:
        for m in (None, limit):
            rows = iktr.rows(sc, pts, k, m, None, cache)
            want = iktr.ordered_brute(sc, pts, k, m, None, cache)
            differ[k, m is not None] = sum(1 for j in range(len(pts)) if rows[j] != want[j])
            print(which, np.dtype(dtype).name, "k =", k, "limited" if m is not None else "no limit", "rows that differ:", differ[k, m is not None], "of", len(pts))
            assert sum(1 for r in rows if r) >= 50
    assert not any(differ.values()), differ
    # the scene does reach the overflow: at the largest k some full row's bound * F is +inf
    big_f = max(sc.ft(iwr.stretch(y)) for y in sc.y)
    with np.errstate(over="ignore"):
        assert any(len(r) == ks[-1] and np.isposinf(sc.ft(r[-1][0]) * big_f) for r in iktr.rows(sc, pts, ks[-1], None, None, cache))


# ---- single leaves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_leaves(orc, dtype):
    """record 0 is a leaf: the one-triangle member (member level), a one-instance set (top level), and both at once"""
    trees = member_trees(orc, dtype)
    tri, cubes = trees[2], trees[1]
    assert len(tri[1]) == 1
    pts = np.array([[0, 0, 0], [7, -3, 2], [-9, 1, 1], [2, 0.5, 0.1]], dtype=dtype)
    x1 = np.eye(3, 4, dtype=dtype)[None].copy()
    x1[0, 0, 3] = 2
    x2 = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x2[0, 0, 3], x2[1, 0, 3] = 2, -4
    for name, sc, pairs in (("both", ir.Scene([tri], [0], x1, dtype), 1), ("member", ir.Scene([tri], [0, 0], x2, dtype), 2),
                            ("top", ir.Scene([cubes], [0], x1, dtype), len(cubes[1]))):
        top, members = iktr.node_arrays(sc)
        assert (top["shape"][0] != NONE) == (name != "member") and (members[0]["shape"][0] != NONE) == (name != "top")
        for k in (1, 2, 5):
            for m in (None, 3.0, iktr.special_limits(len(pts), dtype)):
                rows = iktr.rows(sc, pts, k, m)
                assert rows == iktr.ordered_brute(sc, pts, k, m), (name, k)
                if m is None:
                    assert all(len(r) == min(k, pairs) for r in rows)
                    assert [[e[0] for e in r] for r in rows] == [[e[0] for e in r] for r in ikr.rows(sc, pts, k)]
    inst, shape, dist = iktr.knearest_tree(ir.Scene([tri], [0], x1, dtype), pts[:2], 5)
    assert inst.tolist() == [[0] + [NONE] * 4] * 2 and shape.tolist() == [[0] + [NONE] * 4] * 2
    assert np.isfinite(dist[:, 0]).all() and np.isposinf(dist[:, 1:]).all() and dist.dtype == dtype
    empty = ir.Scene([tri], [], np.zeros((0, 3, 4), dtype=dtype), dtype)
    assert iktr.rows(empty, pts, 3) == [[]] * 4 and iktr.ordered_brute(empty, pts, 3, 1.0) == [[]] * 4


# ---- NaN coordinates -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", (1, 3, 64))
def test_nan_coordinate_against_ordered_brute(orc, dtype, k):
    """a NaN coordinate makes every leaf distance NaN: accepted only while the list is not full and only without a limit (NaN <= r2 is
    false), never replaced"""
    c = case(orc, dtype, 37)
    pts = np.array([[np.nan, 0, 0], [0, np.nan, 1], [np.nan] * 3, [0.5, 0.5, 0.5]], dtype=dtype)
    rows = iktr.rows(c["scene"], pts, k)
    assert iktr.same_rows(rows, iktr.ordered_brute(c["scene"], pts, k))
    for r in rows[:3]:
        assert len(r) == k and all(e[0] != e[0] for e in r)
    assert all(e[0] == e[0] for e in rows[3])
    limited = iktr.rows(c["scene"], pts, k, 100.0)
    assert iktr.same_rows(limited, iktr.ordered_brute(c["scene"], pts, k, 100.0))
    assert limited[:3] == [[], [], []] and limited[3] == rows[3]


def test_the_reference_stands_alone():
    src = open(os.path.join(ROOT, "tests", "instances_knn_tree_ref.py")).read()
    assert "import bvh_amd" not in src and "from bvh_amd" not in src


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_is_built_and_bound():
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances_knn_tree.hip" in build_ext.SOURCES and "tree_node.hpp" in build_ext.HEADERS
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"k_instances_knearest_tree" in blob
    sig = {s[0]: s[2] for s in _lib.SYMBOLS}
    for sym in ("bvhgpu_instances_knearest_tree_f32", "bvhgpu_instances_knearest_tree_f64"):
        assert sym in sig and len(sig[sym]) == len(sig["bvhgpu_instances_knearest_f32"]) + 1      # the flat form's arguments and max_dist
    header = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    assert "bvhgpu_instances_knearest_tree_f32(" in header and "bvhgpu_instances_knearest_tree_f64(" in header
    assert "#define BVHGPU_ABI_VERSION 7" in header
    import bvh_amd
    assert hasattr(bvh_amd.Instances, "knearest_tree_batch") and hasattr(bvh_amd.Instances, "nearest_tree_batch")
    assert not hasattr(bvh_amd, "instances_knearest_tree_batch")     # no module-level function
