"""All-hits over instanced scenes, CPU side: the scenes tests/test_gpu_instances_allhits.py runs, shown on the reference alone
(tests/instances_allhits_ref.py: a filter and a stable sort over tests/instances_ref.py's candidate table) to satisfy the consequences
the header states and to reach every tier of the engine; and the wiring of the new HIP file into the build."""
import os

import numpy as np
import pytest

import instances_allhits_ref as iar
import instances_ref as ir
from test_instances_cpu import N_RAYS, SIZES, _tris_aabbs, case, member_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build_library()
    return o


# ---- the cluster scene ---------------------------------------------------------------------------------------------------------------------
_ROWS = {}


def cluster_rows(orc, dtype, n):
    """case(orc, dtype, n) with its reference rows: rows[(cut, sort)] = (offsets, instance, shape, vals) (computed once, never modified)"""
    key = (np.dtype(dtype).name, n)
    if key not in _ROWS:
        c = case(orc, dtype, n)
        table = c["free"]["table"]
        _ROWS[key] = {(cut, sort): iar.rows(table, N_RAYS, c["tmax"] if cut else None, dtype, sort) for cut in (False, True) for sort in (True, False)}
    return case(orc, dtype, n), _ROWS[key]


def _heads(rows_, n, dtype):
    """the first entry of every row as (vals[n,3], instance[n], shape[n]), a miss where the row is empty"""
    off, inst, shape, vals = rows_
    lo = off[:-1].astype(np.int64)
    full = np.diff(off.astype(np.int64)) > 0
    hv = np.zeros((n, 3), dtype=dtype); hv[:, 0] = np.inf
    hi, hs = np.full(n, NONE, dtype=np.uint32), np.full(n, NONE, dtype=np.uint32)
    hv[full], hi[full], hs[full] = vals[lo[full]], inst[lo[full]], shape[lo[full]]
    return hv, hi, hs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_consequences_hold_on_the_reference(orc, dtype, n):
    """on every ray, free and cut: the sorted row's head is `closest`, the list-order row's head is `first`, a row is empty iff the ray misses"""
    c, rows_ = cluster_rows(orc, dtype, n)
    for cut in (False, True):
        want = c["cut"] if cut else c["free"]
        for sort, name in ((True, "closest"), (False, "first")):
            r = rows_[(cut, sort)]
            assert r[0][-1] == len(r[1]) == len(r[2]) == len(r[3]) and r[0][0] == 0
            hv, hi, hs = _heads(r, N_RAYS, dtype)
            assert hv.tobytes() == want[name][0].tobytes(), (cut, name)
            assert hi.tobytes() == want[name][1].tobytes() and hs.tobytes() == want[name][2].tobytes(), (cut, name)
            assert np.array_equal(np.diff(r[0].astype(np.int64)) == 0, want["first"][1] == NONE)
        # both orders hold the same candidates
        assert rows_[(cut, True)][0].tobytes() == rows_[(cut, False)][0].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_is_worth_running(orc, dtype):
    c, rows_ = cluster_rows(orc, dtype, 37)
    free, cut = rows_[(False, False)], rows_[(True, False)]
    lens, cut_lens = np.diff(free[0].astype(np.int64)), np.diff(cut[0].astype(np.int64))
    assert (lens >= 2).sum() >= 20
    unordered = sum(1 for j in range(N_RAYS) if (np.diff(free[3][free[0][j]:free[0][j + 1], 0]) < 0).any())
    assert unordered >= 20, unordered
    shorter = ((cut_lens < lens) & (cut_lens > 0)).sum()
    assert shorter >= 20, shorter
    srt = rows_[(False, True)]
    for j in range(N_RAYS):
        assert (np.diff(srt[3][srt[0][j]:srt[0][j + 1], 0]) >= 0).all()


# ---- the stack scene: every tier -------------------------------------------------------------------------------------------------------------
N_STACK, N_STACK_RAYS, N_PAIR_RAYS = 40, 64, 8


def stack_scene(orc, dtype):
    """Member S: 128 triangles (-4,-4,z) (4,-4,z) (0,6,z) at z = k/16, every odd one with reversed winding (it misses from one side: misses
    are interleaved in the list).  Member C: test_instances_cpu's single triangle.  40 instances at z = 10 j: j % 3 == 0 a pure translation,
    the others a rotation about z times xy scales; 4, 13, 22, 31 take the transform of 3, 12, 21, 30 (coincident copies: every distance
    there appears twice and the top level has coincident world boxes); 37 and 38 use member C.
    64 rays from z = -5 along +z with x, y in U(-0.3, 0.3), those with index 1 mod 4 from z = 405 along -z, those with index 2 mod 8
    tilted by U(-0.02, 0.02).  A row of these rays that is short enough for the lane tier ends inside the first instance it meets, which
    is no coincident copy, so it holds no tie: 8 more rays (64 .. 71) start at z = 295 along +z, in front of the coincident pair 30 / 31,
    whose distances are exact.  → (trees, tree_of, x[40,3,4], rays[72])"""
    rng = np.random.default_rng(7)
    z = np.arange(128) / 16.0
    s = np.zeros((128, 3, 3))
    s[:, 0] = np.stack([np.full(128, -4.0), np.full(128, -4.0), z], axis=1)
    s[:, 1] = np.stack([np.full(128, 4.0), np.full(128, -4.0), z], axis=1)
    s[:, 2] = np.stack([np.zeros(128), np.full(128, 6.0), z], axis=1)
    s[1::2] = s[1::2, ::-1].copy()
    s = np.ascontiguousarray(s.astype(dtype))
    trees = [(_tris_aabbs(s), s), member_trees(orc, dtype)[2]]
    x = np.zeros((N_STACK, 3, 4))
    for j in range(N_STACK):
        ang, sc = rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 2.0, size=2)
        x[j, :, :3] = np.eye(3)
        if j % 3 != 0:
            x[j, :2, :2] = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) @ np.diag(sc)
        x[j, 2, 3] = 10.0 * j
    for j in (4, 13, 22, 31):
        x[j] = x[j - 1]
    tree_of = np.zeros(N_STACK, dtype=np.uint32)
    tree_of[[37, 38]] = 1
    n = N_STACK_RAYS + N_PAIR_RAYS
    o = np.zeros((n, 3)); d = np.zeros((n, 3))
    o[:, :2] = rng.uniform(-0.3, 0.3, size=(n, 2))
    o[:, 2], d[:, 2] = -5.0, 1.0
    back = np.arange(N_STACK_RAYS) % 4 == 1
    o[:N_STACK_RAYS][back, 2], d[:N_STACK_RAYS][back, 2] = 405.0, -1.0
    tilt = np.nonzero(np.arange(N_STACK_RAYS) % 8 == 2)[0]
    d[tilt, :2] = rng.uniform(-0.02, 0.02, size=(len(tilt), 2))
    o[N_STACK_RAYS:, 2] = 295.0
    rays = orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)
    return trees, tree_of, np.ascontiguousarray(x.astype(dtype)), rays


def reachable(s, j, L):
    """is there a tmax that gives ray j a row of exactly L entries: its uncut row is longer and no tie pair straddles the cut"""
    off, _, _, vals = s["uncut"]
    d = vals[off[j]:off[j + 1], 0]
    return len(d) > L and (L == 0 or d[L] != d[L - 1])


_STACK = {}


def stack_case(orc, dtype):
    """the stack scene with the reference rows of its uncut batch and of its cut batch: tmax[j] = the L-th smallest distance of ray j's
    uncut row, L walking through every length at which the engine takes another path (computed once, never modified)"""
    key = np.dtype(dtype).name
    if key in _STACK:
        return _STACK[key]
    lane_max, lds_max = iar.engine_thresholds(ROOT)
    trees, tree_of, x, rays = stack_scene(orc, dtype)
    sc = ir.Scene(trees, tree_of, x, dtype)
    n = len(rays)
    table = sc.trace(rays)["table"]
    s = dict(trees=trees, tree_of=tree_of, x=x, rays=rays, scene=sc, table=table, uncut=iar.rows(table, n, None, dtype, True),
             uncut_list=iar.rows(table, n, None, dtype, False), lane_max=lane_max, lds_max=lds_max)
    targets = [0, 1, lane_max - 1, lane_max, lane_max + 1, lds_max - 1, lds_max, lds_max + 1, None]
    short = [lane_max, lane_max - 1, 2, lane_max + 1]             # the rays in front of the coincident pair
    off, _, _, vals = s["uncut"]
    tmax = np.full(n, np.inf, dtype=dtype)
    plan = [None] * n
    for j in range(n):
        for k in range(len(targets)):
            L = targets[(j + k) % len(targets)] if j < N_STACK_RAYS else short[(j + k) % len(short)]
            if L is None:
                break
            if reachable(s, j, L):
                tmax[j], plan[j] = vals[off[j] + L, 0], L
                break
    s.update(tmax=tmax, plan=plan, cut=iar.rows(table, n, tmax, dtype, True), cut_list=iar.rows(table, n, tmax, dtype, False))
    _STACK[key] = s
    return s


def _has_tie(rows_, j):
    off, _, _, vals = rows_
    return bool((np.diff(vals[off[j]:off[j + 1], 0]) == 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_stack_scene_reaches_every_tier(orc, dtype):
    s = stack_case(orc, dtype)
    lane_max, lds_max = s["lane_max"], s["lds_max"]
    assert 2 < lane_max < lds_max
    n = N_STACK_RAYS
    lens = np.diff(s["uncut"][0].astype(np.int64))
    # the uncut batch of the 64 rays: rows of 1 152 to 2 434 candidates, 57 beyond the LDS tier, no list in ascending order, 15 621 tied
    # neighbours from the coincident copies, 304 602 list members with the misses (what the reference gives for this scene, in f32 and f64)
    assert lens[:n].min() > lane_max and (lens[:n].min(), lens[:n].max()) == (1152, 2434) and (lens[:n] > lds_max).sum() >= 57
    lo = s["uncut_list"]
    assert all((np.diff(lo[3][lo[0][j]:lo[0][j + 1], 0]) < 0).any() for j in range(n))
    so = s["uncut"]
    ties = sum(int((np.diff(so[3][so[0][j]:so[0][j + 1], 0]) == 0).sum()) for j in range(n))
    assert ties >= 15_000, ties
    assert (s["table"]["ray"] < n).sum() >= 300_000 and len(s["table"]["ray"]) > 2 * len(so[1])     # misses are interleaved in the list
    for j in range(len(lens)):
        assert (np.diff(so[3][so[0][j]:so[0][j + 1], 0]) >= 0).all()
    # every length at which the engine takes another path is reachable on most rays, lds_max - 1 on 17
    for L in (1, lane_max - 1, lane_max, lane_max + 1, lds_max, lds_max + 1):
        assert sum(reachable(s, j, L) for j in range(n)) >= 57, L
    assert sum(reachable(s, j, lds_max - 1) for j in range(n)) >= 17
    # the cut batch: the planned lengths came out, and all of them are there
    cut_lens = np.diff(s["cut"][0].astype(np.int64))
    assert s["cut"][0].tobytes() == s["cut_list"][0].tobytes()
    for j, L in enumerate(s["plan"]):
        assert cut_lens[j] == (lens[j] if L is None else L), (j, L)
    have = set(cut_lens.tolist())
    for L in (0, 1, lane_max - 1, lane_max, lane_max + 1, lds_max - 1, lds_max, lds_max + 1):
        assert L in have, L
    assert any(L is None for L in s["plan"]) and cut_lens.max() > lds_max + 1      # an uncut row
    # a tie in a row of each tier
    tiers = {"lane": lambda m: 2 <= m <= lane_max, "lds": lambda m: lane_max < m <= lds_max, "global": lambda m: m > lds_max}
    for name, inside in tiers.items():
        assert any(inside(cut_lens[j]) and _has_tie(s["cut"], j) for j in range(len(cut_lens))), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_copies_along_x(orc, dtype):
    """test_instances_cpu's hand case: a ray from the origin along +x meets instance 1 at exactly 4 and instance 0 at exactly 8"""
    tri = np.array([[[0, -1, -1], [0, 0, 1], [0, 1, -1]]], dtype=dtype)
    x = np.tile(np.eye(3, 4, dtype=dtype), (2, 1, 1))
    x[0, 0, 3], x[1, 0, 3] = 8, 4
    sc = ir.Scene([(_tris_aabbs(tri), tri)], [0, 0], x, dtype)
    rays = orc.make_rays([[0, 0, 0]], [[1, 0, 0]], dtype)
    table = sc.trace(rays)["table"]
    off, inst, shape, vals = iar.rows(table, 1, None, dtype)
    assert off.tolist() == [0, 2] and inst.tolist() == [1, 0] and shape.tolist() == [0, 0] and vals[:, 0].tolist() == [4.0, 8.0]
    off, inst, shape, vals = iar.rows(table, 1, None, dtype, sort=False)
    assert inst.tolist() == table["instance"].tolist()
    off, inst, shape, vals = iar.rows(table, 1, np.array([8], dtype=dtype), dtype)        # strict: the hit at exactly tmax is outside
    assert off.tolist() == [0, 1] and inst.tolist() == [1]
    for tm in (0.0, -1.0, np.nan):
        assert iar.rows(table, 1, np.array([tm], dtype=dtype), dtype)[0].tolist() == [0, 0]


def test_the_reference_stands_alone():
    src = open(os.path.join(ROOT, "tests", "instances_allhits_ref.py")).read()
    assert "import bvh_amd" not in src and "from bvh_amd" not in src


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_are_built_and_bound():
    import __graft_entry__ as g
    from bvh_amd import build_ext
    assert "instances_allhits.hip" in build_ext.SOURCES
    g.build()
    from bvh_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_instances_allhits_count", b"k_instances_allhits_fill", b"k_instances_allhits_sort_row"):
        assert kern in blob, kern
    names = {s[0] for s in _lib.SYMBOLS}
    for sym in ("bvhgpu_instances_allhits_f32", "bvhgpu_instances_allhits_f64", "bvhgpu_hits_fetch_instances_allhits"):
        assert sym in names
    assert _lib.INSTANCES_ALLHITS_LIST_ORDER == 1 and _lib.INSTANCES_ALLHITS_COUNT_ONLY == 2
    import bvh_amd
    assert hasattr(bvh_amd.Instances, "allhits_batch")
