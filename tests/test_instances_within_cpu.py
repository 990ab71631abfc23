"""Radius search over instanced scenes, CPU side: the definition's pieces by hand, the scenes tests/test_gpu_instances_within.py runs
shown on the reference alone (tests/instances_within_ref.py) to equal a brute force over all pairs, to be worth running and to reach
every tier of the engine; the identity anchor against tests/within_ref.py; and the wiring of the new HIP file into the build."""
import os

import numpy as np
import pytest

import instances_ref as ir
import instances_within_ref as iwr
import within_ref as wr
from test_instances_cpu import SIZES, _tris_aabbs, case, member_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
N_POINTS = 600


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the definition's pieces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stretch_of_a_known_matrix(dtype):
    """F of [[1, 2, 3], [4, 5, 6], [7, 8, 9]] is 285, of the identity 3, of diag(0.5, 2, 4) 20.25: all exact"""
    y = np.zeros((3, 4), dtype=dtype)
    y[:, :3] = np.arange(1, 10).reshape(3, 3)
    y[:, 3] = [100, -7, 0.5]                                  # the translation is no part of it
    assert iwr.stretch(y) == 285 and type(iwr.stretch(y)) is np.dtype(dtype).type
    assert iwr.stretch(np.eye(3, 4, dtype=dtype)) == 3
    assert iwr.stretch(np.concatenate([np.diag([0.5, 2.0, 4.0]), np.zeros((3, 1))], axis=1).astype(dtype)) == 20.25


@pytest.mark.parametrize("dtype", DTYPES)
def test_object_point_of_a_known_pose(dtype):
    """X = a quarter turn about z scaled by 2, then a translation by (8, 0, 0): the world point (8, 6, 1) is the object point (3, 0, 0.5),
    and Y = X^-1 has F = 3 / 4"""
    x = np.array([[[0, -2, 0, 8], [2, 0, 0, 0], [0, 0, 2, 0]]], dtype=dtype)
    y = ir.inverse(x)[0]
    q = ir.forward(y, np.array([8, 6, 1], dtype=dtype))
    assert q.tolist() == [3.0, 0.0, 0.5] and q.dtype == dtype
    assert iwr.stretch(y) == 0.75
    iy = ir.inverse(np.eye(3, 4, dtype=dtype)[None])[0]       # the identity: Y = I and y3 = -0
    assert iy[:, :3].tobytes() == np.eye(3, dtype=dtype).tobytes() and (iy[:, 3] == 0).all() and np.signbit(iy[:, 3]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_copies_along_x(orc, dtype):
    """one triangle in the plane x = 0 around the origin; instance 0 at x = 8, instance 1 at x = 4, instance 2 = instance 1 scaled by
    (1, 3, 3): from the origin the three are at exactly 8, 4 and 4, whatever the scale does to the object frame"""
    tri = np.array([[[0, -1, -1], [0, 0, 1], [0, 1, -1]]], dtype=dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (3, 1, 1))
    x[0, 0, 3], x[1, 0, 3], x[2, 0, 3] = 8, 4, 4
    x[2, 1, 1] = x[2, 2, 2] = 3
    sc = ir.Scene([(_tris_aabbs(tri), tri)], [0, 0, 0], x, dtype)
    p = np.zeros((1, 3), dtype=dtype)
    got = lambda m, sort=True: [a.tolist() for a in iwr.within(sc, p, m, sort)]
    order = [e[1] for e in iwr.rows(sc, p, 8)[0]]             # the double order: the top level's
    assert sorted(order) == [0, 1, 2]
    assert got(8) == [[0, 3], [i for i in order if i != 0] + [0], [0, 0, 0], [4.0, 4.0, 8.0]]      # the tie stays in the double order
    assert got(8, sort=False)[1] == order
    assert got(4)[0] == [0, 2] and got(4)[3] == [4.0, 4.0]    # the limit itself is inside
    assert got(np.nextafter(dtype(4), dtype(0)))[0] == [0, 0]
    for m in (-1.0, np.nan):
        assert got(m)[0] == [0, 0]
    assert got(np.inf)[0] == [0, 3]
    assert got(-0.0)[0] == [0, 0]                             # -0.0 is the limit 0: walked, nothing is at distance 0
    on = np.array([[4, 0, 0]], dtype=dtype)                   # a point ON instances 1 and 2
    assert [a.tolist() for a in iwr.within(sc, on, -0.0)][3] == [0.0, 0.0]
    # off the axis: (4, 1, 0) lies in the plane of both, 1 / sqrt(5) = 0.447 beyond an edge of instance 1's triangle (which spans
    # |y| <= 0.5 at z = 0) and inside instance 2's (|y| <= 1.5): the scale is in the world triangle, not in the distance
    off = np.array([[4, 1, 0]], dtype=dtype)
    o, inst, shape, dist = iwr.within(sc, off, 0.25)
    assert inst.tolist() == [2] and dist[0] < 1e-6
    o, inst, shape, dist = iwr.within(sc, off, 0.5)
    assert inst.tolist() == [2, 1] and abs(dist[1] - 1 / np.sqrt(5)) < 1e-6


# ---- the cluster scenes --------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def cluster_rows(orc, dtype, n):
    """case(orc, dtype, n)'s scene with the issue's points and limits and their reference rows in the double order (computed once, never
    modified) → (scene case, points, limits, rows, stats)"""
    key = (np.dtype(dtype).name, n)
    if key not in _ROWS:
        c = case(orc, dtype, n)
        pts, m = iwr.cluster_points(n, dtype, N_POINTS)
        stats = {}
        _ROWS[key] = (pts, m, iwr.rows(c["scene"], pts, m, stats), stats)
    return (case(orc, dtype, n),) + _ROWS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_rows_equal_brute_force(orc, dtype, n):
    """a condition, not a tolerance: on every point the walk's candidate set is {d <= r2} over all (instance, triangle) pairs"""
    c, pts, m, rows, _ = cluster_rows(orc, dtype, n)
    want = iwr.brute(c["scene"], pts, m)
    bad = [(j, sorted(set((i, s) for _, i, s in rows[j]) ^ want[j])) for j in range(N_POINTS) if set((i, s) for _, i, s in rows[j]) != want[j]]
    assert not bad, bad[:5]
    assert all(len(r) == len(set((i, s) for _, i, s in r)) for r in rows)      # no pair twice


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_is_worth_running(orc, dtype):
    c, pts, m, rows, stats = cluster_rows(orc, dtype, 37)
    lens = np.array([len(r) for r in rows])
    unordered = sum(1 for r in rows if any(r[k + 1][0] < r[k][0] for k in range(len(r) - 1)))
    multi = sum(1 for r in rows if len(set(i for _, i, _ in r)) >= 2)
    assert (lens == 0).sum() >= 20 and (lens >= 2).sum() >= 20 and unordered >= 20 and multi >= 20
    # what the reference gives for this scene, in f32 and f64
    assert ((lens == 0).sum(), (lens >= 2).sum(), unordered, multi, lens.max(), lens.sum()) == (333, 260, 245, 167, 777, 23654)
    assert stats["instances"] == 3270                         # 5.45 instances entered per point
    off, inst, shape, dist = iwr.csr(rows, dtype, sort=True)
    for j in range(N_POINTS):
        assert (np.diff(dist[off[j]:off[j + 1]]) >= 0).all()


# ---- the identity anchor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_instance_is_the_single_tree(orc, dtype):
    """one identity instance of B: q = p and w = tri bit for bit, so a list-order row holds within_ref's distances and shapes — identical
    on every point of this draw (the wider object-frame prune, md <= 3 r2, keeps no leaf here that md <= r2 drops with d <= r2)"""
    aabbs, tris = member_trees(orc, dtype)[1]
    sc = ir.Scene([(aabbs, tris)], [0], np.eye(3, 4, dtype=dtype)[None], dtype)
    rng = np.random.default_rng(77)
    pts = rng.uniform(-5, 5, size=(400, 3)).astype(dtype)
    m = rng.uniform(0.1, 4.0, size=400).astype(dtype)
    rows = iwr.rows(sc, pts, m)
    want = wr.rows(sc.flats[0], aabbs, pts, m, tris)
    assert sum(1 for r in want if r[0]) >= 200
    for j in range(400):
        assert [e[0] for e in rows[j]] == want[j][0] and [e[2] for e in rows[j]] == want[j][1], j
        assert all(e[1] == 0 for e in rows[j])


# ---- the line of instances: every tier -----------------------------------------------------------------------------------------------------
_LINE = {}


def line_case(orc, dtype):
    """iwr.line_instances with one batch of queries at x = 0 and x = 4097 whose integer limits give a row of every length at which the
    engine takes another path (computed once, never modified)"""
    key = np.dtype(dtype).name
    if key in _LINE:
        return _LINE[key]
    lane_max, lds_max = iwr.engine_thresholds(ROOT)
    trees, tree_of, x = iwr.line_instances(dtype)
    sc = ir.Scene(trees, tree_of, x, dtype)
    # from x = 4097 a limit m below 1409 gives exactly m entries (no coincident copy in reach), from 1472 to 4032 m + 64 (the copy of
    # instance 41), 4096 and +inf all 4224; from x = 0 a limit m gives m + min(m, 64) (the copy of instance 0), more from 2625 on
    far = [0, 1, lane_max - 1, lane_max, lane_max + 1, 100, lds_max - 65, lds_max - 64, lds_max - 63, lds_max - 1, lds_max, lds_max + 1, 4096, np.inf,
           -1.0, np.nan]
    near = [0, 1, 2, lane_max // 2 - 1, lane_max // 2, lane_max // 2 + 1, lane_max + 1, lds_max - 65, lds_max - 64, lds_max - 63, 4096, np.inf, -0.0, 0.5]
    pts = np.zeros((len(far) + len(near), 3), dtype=dtype)
    pts[:len(far), 0] = 4097
    lim = np.array(far + near, dtype=dtype)
    rows = iwr.rows(sc, pts, lim)
    _LINE[key] = dict(trees=trees, tree_of=tree_of, x=x, scene=sc, points=pts, limits=lim, rows=rows, n_far=len(far), lane_max=lane_max, lds_max=lds_max)
    return _LINE[key]


def _tie(row):
    d = sorted(e[0] for e in row)
    return any(a == b for a, b in zip(d, d[1:]))


def _unordered(row):
    return any(row[k + 1][0] < row[k][0] for k in range(len(row) - 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_line_scene_reaches_every_tier(orc, dtype):
    s = line_case(orc, dtype)
    lane_max, lds_max, nf = s["lane_max"], s["lds_max"], s["n_far"]
    assert (lane_max, lds_max) == (32, 2048)                   # the figures below are for these
    lens = [len(r) for r in s["rows"]]
    assert lens[:nf] == [0, 1, 31, 32, 33, 100, 2047, 2048, 2049, 2111, 2112, 2113, 4224, 4224, 0, 0]
    assert lens[nf:] == [0, 2, 4, 30, 32, 34, 66, 2047, 2048, 2049, 4224, 4224, 0, 0]
    for L in (0, 1, lane_max - 1, lane_max, lane_max + 1, lds_max - 1, lds_max, lds_max + 1, 4224):
        assert L in lens, L
    # every row is the brute force over all 66 x 64 pairs
    want = iwr.brute(s["scene"], s["points"], s["limits"])
    for j, r in enumerate(s["rows"]):
        assert set((i, k) for _, i, k in r) == want[j] and len(r) == len(want[j]), j
    # a tie and a list order that is not ascending in a row of each tier — and in rows of exactly both thresholds
    tiers = {"lane": lambda m: 2 <= m <= lane_max, "lds": lambda m: lane_max < m <= lds_max, "global": lambda m: m > lds_max}
    for name, inside in tiers.items():
        assert any(inside(len(r)) and _tie(r) and _unordered(r) for r in s["rows"]), name
    for L in (lane_max, lds_max):
        assert any(len(r) == L and _tie(r) and _unordered(r) for r in s["rows"]), L
    # the whole scene: every distance 1 .. 4096 once, 128 of them twice
    full = sorted(e[0] for e in s["rows"][nf - 4])
    assert len(full) == 4224 and len(set(full)) == 4096 and full[0] == 1.0 and full[-1] == 4096.0 ** 2


def test_the_reference_stands_alone():
    src = open(os.path.join(ROOT, "tests", "instances_within_ref.py")).read()
    assert "import bvh_amd" not in src and "from bvh_amd" not in src


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_are_built_and_bound():
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances_within.hip" in build_ext.SOURCES
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_instances_within_count", b"k_instances_within_fill", b"k_instances_within_sort_row"):
        assert kern in blob, kern
    names = {s[0] for s in _lib.SYMBOLS}
    for sym in ("bvhgpu_instances_within_f32", "bvhgpu_instances_within_f64", "bvhgpu_hits_fetch_instances_within"):
        assert sym in names
    assert _lib.INSTANCES_WITHIN_LIST_ORDER == 1 and _lib.INSTANCES_WITHIN_COUNT_ONLY == 2
    import bvh_amd
    assert hasattr(bvh_amd.Instances, "within_batch")
