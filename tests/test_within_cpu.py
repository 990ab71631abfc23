"""Radius-search point queries on the CPU: bvhgpu_within_* is declared, exported and bound in every layer, and the definition the GPU
tests pin (tests/within_ref.py; include/bvh_mi355x.h) is checked against itself — hand-written rows with the special
limits and points, brute force where the arithmetic is exact, heads of rows against knn_ref.knearest cut at the limit, the flat loop
against the recursive form (walk-independence) — and the scenes of tests/test_gpu_within.py are shown, on the oracle alone, to contain
what that file says they contain."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref as kr
import within_ref as wr
from oracle import orc
from test_knn_cpu import cube_scene, extreme_points, half_grid_queries, integer_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bvhgpu_within_f32", "bvhgpu_within_f64", "bvhgpu_hits_fetch_within"]
NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
CUBE_RADIUS = 40000.0        # the cube scene: 100 unit cubes in a cube of 2e5, so a ball of this radius holds about 3 cubes = 40 triangles
CLOUD_RADII = (0.0, 0.5, 1.5, 2.5, 5.0)   # the integer cloud: every r and r * r is exact


# ---- the scenes of tests/test_gpu_within.py (computed once per dtype, shared) ----------------------------------------------------------
def cube_points(tris, aabbs, dtype, seed=41):
    """about 2 000 points: uniform in the scene's bounds, on triangles, on box corners (twice), and the NaN / infinite / max-finite /
    subnormal points of test_knn_cpu.extreme_points"""
    rng = np.random.default_rng(seed)
    lo, hi = aabbs[:, :3].min(axis=0).astype(np.float64), aabbs[:, 3:].max(axis=0).astype(np.float64)
    uni = rng.uniform(lo, hi, size=(1200, 3)).astype(dtype)
    w = rng.dirichlet([1, 1, 1], size=500)
    on = np.einsum("nk,nkd->nd", w, tris[rng.integers(0, len(tris), 500)].astype(np.float64)).astype(dtype)
    corner = aabbs[rng.integers(0, len(aabbs), 120)][:, :3].astype(dtype)
    return np.concatenate([uni, on, corner, corner[:60], extreme_points(dtype, (lo + hi) / 2)])


def mixed_limits(n, dtype, seed=42):
    """per point: 0, -1, NaN, 1, CUBE_RADIUS / 2, 1.5 x CUBE_RADIUS in turn, a random radius for every seventh, +inf for every 40th"""
    rng = np.random.default_rng(seed)
    m = np.asarray([0.0, -1.0, np.nan, 1.0, CUBE_RADIUS / 2, 1.5 * CUBE_RADIUS], dtype=dtype)[np.arange(n) % 6]
    m[6::7] = rng.uniform(0, 2 * CUBE_RADIUS, size=len(m[6::7])).astype(dtype)
    m[::40] = np.inf
    return m


@functools.lru_cache(maxsize=None)
def cube_case(dtype):
    """dict(tris, aabbs, nodes, oflat, pts, limits {"scalar" | "mixed": max_dist}, rows {(kind, limit name): list rows})"""
    tris, aabbs = cube_scene(100, dtype)
    nodes = orc.build(aabbs).nodes
    oflat = orc.flatten(nodes)
    pts = cube_points(tris, aabbs, dtype)
    lim = dict(scalar=dtype(CUBE_RADIUS), mixed=mixed_limits(len(pts), dtype))
    rows = {}
    for kind in (0, 1):
        got = wr.rows_multi(oflat, aabbs, pts, [lim["scalar"], lim["mixed"]], tris if kind else None)
        rows[kind, "scalar"], rows[kind, "mixed"] = got
    return dict(tris=tris, aabbs=aabbs, nodes=nodes, oflat=oflat, pts=pts, limits=lim, rows=rows)


@functools.lru_cache(maxsize=None)
def line_case(dtype, reverse):
    """the row-length scene: dict(aabbs, tris, nodes, oflat, pts, limits, lengths, rows {kind: list rows})"""
    aabbs, tris = wr.line_scene(dtype)
    nodes = orc.build(aabbs).nodes
    oflat = orc.flatten(nodes)
    pts, m, lens = wr.row_length_case(dtype, reverse)
    rows = {kind: wr.rows(oflat, aabbs, pts, m, tris if kind else None) for kind in (0, 1)}
    return dict(aabbs=aabbs, tris=tris, nodes=nodes, oflat=oflat, pts=pts, limits=m, lengths=lens, rows=rows)


TIE_COPIES, TIE_POSITIONS = 3, 1024
TIE_LIMITS = (0, 1, 5, 10, 11, 100, 400, 682, 683, 1024)      # x 3 copies: rows of 3 .. 30 (lane), 33 .. 2046 (LDS), 2049 and 3072 (global)


@functools.lru_cache(maxsize=None)
def ties_case(dtype):
    """the same line with TIE_COPIES shapes per position, queried from both ends: dict(aabbs, tris, nodes, oflat, pts, limits, rows)"""
    aabbs, tris = wr.line_scene(dtype, TIE_COPIES, TIE_POSITIONS)
    nodes = orc.build(aabbs).nodes
    oflat = orc.flatten(nodes)
    m = np.asarray(TIE_LIMITS * 2, dtype=dtype)
    pts = np.zeros((len(m), 3), dtype=dtype)
    pts[len(TIE_LIMITS):, 0] = TIE_POSITIONS + 1
    rows = {kind: wr.rows(oflat, aabbs, pts, m, tris if kind else None) for kind in (0, 1)}
    return dict(aabbs=aabbs, tris=tris, nodes=nodes, oflat=oflat, pts=pts, limits=m, rows=rows)


@functools.lru_cache(maxsize=None)
def cloud_case(dtype):
    """test_knn_cpu's kind of integer cloud (4 096 points in [0, 15]^3: one per cell on average, duplicates allowed) with queries on the
    half grid and the exact radii CLOUD_RADII in turn"""
    aabbs, tris = integer_cloud(dtype, 15)
    nodes = orc.build(aabbs).nodes
    oflat = orc.flatten(nodes)
    pts = half_grid_queries(dtype, 15, 160)
    m = np.asarray(CLOUD_RADII, dtype=dtype)[np.arange(len(pts)) % len(CLOUD_RADII)]
    rows = {kind: wr.rows(oflat, aabbs, pts, m, tris if kind else None) for kind in (0, 1)}
    return dict(aabbs=aabbs, tris=tris, nodes=nodes, oflat=oflat, pts=pts, limits=m, rows=rows)


def far_scene(dtype, seed=35):
    """test_gpu_knn's scene of boxes so far apart that no bucket wins a split: both children get EMPTY bounds; a triangle per box whose
    first vertex is the box's min corner (the first 50 of them are query points) → (aabbs, tris, pts, limits)"""
    rng = np.random.default_rng(seed)
    big = dtype(1e19 if dtype == np.float32 else 1e154)
    lo = (rng.uniform(-1, 1, size=(500, 3)) * big).astype(dtype)
    e = big * dtype(0.01)
    far = np.concatenate([lo, lo + e], axis=1)
    tris = np.stack([lo, far[:, [3, 1, 5]], far[:, [0, 4, 5]]], axis=1).astype(dtype)
    assert np.array_equal(np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1), far)
    pts = np.concatenate([(rng.uniform(-1, 1, size=(300, 3)) * big).astype(dtype), lo[:50], tris[50:200, 1], extreme_points(dtype, [0, 0, 0])])
    m = (np.asarray([0.0, 0.05, 0.3, 0.6, np.inf, -1.0, np.nan])[np.arange(len(pts)) % 7] * float(big)).astype(dtype)
    m[300:500] = 0                                           # the 200 points on triangle vertices: only distance 0 is inside
    m[300:500:5] = big * dtype(0.001)
    return far, tris, pts, m


def lengths(list_rows):
    return np.asarray([len(r[0]) for r in list_rows])


# ---- 1. every layer --------------------------------------------------------------------------------------------------------------------
def test_new_functions_in_every_layer():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), f"{name} is not declared in the header"
    assert re.search(r"#define BVHGPU_WITHIN_LIST_ORDER 1u\b", h) and re.search(r"#define BVHGPU_WITHIN_COUNT_ONLY 2u\b", h)
    import __graft_entry__ as g
    g.build()
    from bvh_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in bound, f"{name} missing from _lib.SYMBOLS"
        assert hasattr(lib, name) and re.search(r" T %s\b" % name, nm), f"{name} not exported"
    assert _lib.WITHIN_LIST_ORDER == 1 and _lib.WITHIN_COUNT_ONLY == 2 and lib.bvhgpu_abi_version() == 7
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_within_count", b"k_within_fill", b"k_within_sort_row", b"k_rows_block_sums", b"k_rows_scan_sums", b"k_rows_scan_final"):
        assert kern in blob, kern
    ffi = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "ffi.rs")).read()
    lib_rs = open(os.path.join(ROOT, "rust", "bvh-mi355x", "src", "lib.rs")).read()
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} missing from ffi.rs"
        assert name in lib_rs, f"{name} is not used by lib.rs"
    assert "pub fn within_distance(" in lib_rs
    from bvh_amd.api import Bvh, _Hits, _TreeBase
    assert callable(getattr(_TreeBase, "within_batch", None)) and callable(getattr(_Hits, "fetch_within", None))
    assert Bvh.within_batch is not _TreeBase.within_batch                       # the flatten_in_place wrapper
    build_py = open(os.path.join(ROOT, "bvh_amd", "build_ext.py")).read()
    assert "within.hip" in build_py and "rows.hip" in build_py


def test_header_states_the_definition():
    h = open(os.path.join(ROOT, "include", "bvh_mi355x.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define BVHGPU_WITHIN_LIST_ORDER", h, flags=re.S)
    assert m, "bvhgpu_within_* has no comment in front of it"
    text = " ".join(m.group(1).replace("\n *", " ").split())
    for word in ("md <= r2", "d <= r2", "one multiplication", "negative or NaN", "leaf pre-order", "sqrt(d)", "BVHGPU_WITHIN_COUNT_ONLY",
                 "BVHGPU_OVERFLOW", "max(0)", "Walk-independence", "bvhgpu_hits_fetch_within"):
        assert word in text, word


# ---- 2. hand-written rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_written_rows_and_special_limits(dtype):
    """unit boxes centred at x = -10 .. 10 (shape = x + 10): arithmetic on quarters"""
    boxes = orc.aligned_boxes().astype(dtype)
    flat = orc.flatten(orc.build(boxes).nodes)
    order = kr.leaf_preorder(flat)
    fi = np.finfo(dtype)
    p = [0.25, 0, 0]
    pts = np.array([p] * 8 + [[np.nan, 0, 0], [np.nan] * 3, [np.inf, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0], [-np.inf, np.nan, 0]], dtype=dtype)
    m = np.array([0, 0.25, 0.5, 0.75, -1, np.nan, -0.0, np.inf, 0, 0, 1e10, fi.max, np.inf, np.inf], dtype=dtype)
    off, shape, dist = wr.within(flat, boxes, pts, m)
    row = lambda i: (shape[off[i]:off[i + 1]].tolist(), dist[off[i]:off[i + 1]].tolist())
    assert row(0) == ([10], [0.0])                                              # m = 0 keeps the shapes at distance 0
    assert row(1) == ([10, 11], [0.0, 0.25])                                    # the limit itself is inside
    assert row(2) == ([10, 11], [0.0, 0.25])
    assert row(3) == ([10, 11, 9], [0.0, 0.25, 0.75])
    assert row(4) == ([], []) and row(5) == ([], [])                            # a negative and a NaN limit
    assert row(6) == ([10], [0.0])                                              # -0.0 >= 0: it is the limit 0
    s7, d7 = row(7)                                                             # +inf: every shape, ascending
    assert sorted(s7) == list(range(21)) and d7 == sorted(d7) and s7[:3] == [10, 11, 9] and d7[-1] == 9.75
    everything = ([s for s in order], [0.0] * 21)
    assert row(8) == everything and row(9) == everything                        # a NaN coordinate adds 0 on its axis: all 21 at 0, leaf pre-order
    assert row(10) == ([], [])                                                  # an infinite coordinate: +inf from every finite box
    assert row(11)[0] == order and np.isposinf(row(11)[1]).all()                # ... which max-finite admits: r2 = max * max = +inf
    assert row(12)[0] == order and row(13)[0] == order                          # ... and +inf
    lo, ls, ld = wr.within(flat, boxes, pts, m, sort=False)
    assert np.array_equal(lo, off)
    assert ls[lo[3]:lo[4]].tolist() == [s for s in order if s in (9, 10, 11)]   # list order is leaf pre-order
    # triangles: a NaN or infinite point gives the triangle distance NaN (never a candidate) or +inf
    tris, aabbs = cube_scene(1, dtype)
    tflat = orc.flatten(orc.build(aabbs).nodes)
    tp = np.array([[np.nan, 0, 0], [np.inf, 0, 0]], dtype=dtype)
    with np.errstate(all="ignore"):
        d_nan = kr.dists_vector(tflat, aabbs, tp[0], dtype, tris)[1]
        d_inf = kr.dists_vector(tflat, aabbs, tp[1], dtype, tris)[1]
    assert np.isnan(d_nan).all() and (np.isnan(d_inf) | np.isposinf(d_inf)).all()
    to, _, _ = wr.within(tflat, aabbs, tp, dtype(np.inf), tris)
    assert to[1] == 0 and to[2] == np.isposinf(d_inf).sum()


# ---- 3. brute force and the k-nearest rows where the arithmetic is exact -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_definition_equals_brute_force_and_knearest_heads_on_integer_cloud(dtype):
    """every operation of both distances and r * r is exact here: a row is every shape with d <= r2 in a stable sort over leaf pre-order;
    its head is knn_ref's k-nearest row cut at the limit"""
    c = cloud_case(dtype)
    flat, aabbs, tris, pts, m = c["oflat"], c["aabbs"], c["tris"], c["pts"], c["limits"]
    order = np.asarray(kr.leaf_preorder(flat))
    fl = kr.flat_lists(flat)
    ties = cut = 0
    for kind in (0, 1):
        for i, p in enumerate(pts):
            md, d = kr.dists_vector(flat, aabbs, p, dtype, tris if kind else None)
            r2 = (m[i] * m[i]).item()
            ld, ls = wr.sort_row(*c["rows"][kind][i])
            dd = d[order]
            idx = np.argsort(dd, kind="stable")
            idx = idx[dd[idx] <= r2]
            assert ls == order[idx].tolist() and ld == dd[idx].tolist(), (kind, i)
            ties += int(len(ld) > 1 and any(a == b for a, b in zip(ld, ld[1:])))
            lo, so = c["rows"][kind][i]
            assert so == [s for s in order.tolist() if d[s] <= r2] and lo == [d[s].item() for s in so]   # list order: leaf pre-order, filtered
            for k in (1, 7, 64):
                kd, ks = kr.walk(fl, md.tolist(), d.tolist(), k)
                head = [(x, s) for x, s in zip(kd, ks) if x <= r2]
                assert head == list(zip(ld, ls))[:k] and len(head) == min(k, len(ld)), (kind, i, k)
                cut += int(len(head) < len(kd))
    n = lengths(c["rows"][0])
    print(f"rows: mean {n.mean():.1f}, max {n.max()}; rows with ties {ties}; k-nearest rows the limit cuts {cut}")
    assert ties > 50 and cut > 50 and n.max() > 64 and (n == 0).any()


# ---- 4. walk-independence -----------------------------------------------------------------------------------------------------------
def _same_candidates(nodes, aabbs, pts, m, list_rows, tris=None):
    tree = wr.tree_candidates(nodes, aabbs, pts, m, tris)
    for i, (ld, ls) in enumerate(list_rows):
        assert sorted(zip(ld, ls)) == tree[i], i


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_loop_and_recursive_form_give_the_same_candidates(dtype):
    """the threshold never moves, so the candidate set is "every box on the shape's path passes md <= r2 and the shape passes d <= r2"
    whatever order a walk visits nodes in: the flat loop (left to right over the FlatNode array) and the recursion over the BvhNode array
    (right child first) agree on every scene of tests/test_gpu_within.py"""
    c = cube_case(dtype)
    for kind in (0, 1):
        for name in ("scalar", "mixed"):
            m = c["limits"][name] if name == "scalar" else c["limits"][name][::4]          # (every fourth point: the recursion is slow)
            _same_candidates(c["nodes"], c["aabbs"], c["pts"][::4], m, c["rows"][kind, name][::4], c["tris"] if kind else None)
    for c in (line_case(dtype, False), line_case(dtype, True), ties_case(dtype), cloud_case(dtype)):
        for kind in (0, 1):
            _same_candidates(c["nodes"], c["aabbs"], c["pts"], c["limits"], c["rows"][kind], c["tris"] if kind else None)
    far, ftris, pts, m = far_scene(dtype)
    nodes = orc.build(far).nodes
    for t in (None, ftris):
        _same_candidates(nodes, far, pts, m, wr.rows(orc.flatten(nodes), far, pts, m, t), t)
    one = c["aabbs"][:1]
    nodes = orc.build(one).nodes
    _same_candidates(nodes, one, c["pts"][:20], dtype(3), wr.rows(orc.flatten(nodes), one, c["pts"][:20], dtype(3)))


# ---- 5. what the GPU scenes contain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cube_scene_batch_is_not_vacuous(dtype):
    c = cube_case(dtype)
    assert 1900 <= len(c["pts"]) <= 2100 and len(c["aabbs"]) == 1200
    m = c["limits"]["mixed"]
    assert (m == 0).any() and (m < 0).any() and np.isnan(m).any() and np.isposinf(m).any()
    p = c["pts"]
    fi = np.finfo(dtype)
    assert np.isnan(p).any() and np.isinf(p).any() and (np.abs(p) == fi.max).any() and (np.abs(p) == fi.smallest_subnormal).any()
    for kind in (0, 1):
        for name in ("scalar", "mixed"):
            n = lengths(c["rows"][kind, name])
            print(f"kind {kind}, {name}: non-empty {np.mean(n > 0):.2f}, mean {n.mean():.1f}, max {n.max()}")
            assert n.max() > wr.LANE_MAX and (n == 0).any(), (kind, name)
        assert np.mean(lengths(c["rows"][kind, "scalar"]) > 0) >= 0.5, kind
        n = lengths(c["rows"][kind, "mixed"])
        assert n[np.isnan(m) | (m < 0)].max() == 0 and n[(m == 0)].max() > 0     # points on shapes have neighbours at distance 0
    assert lengths(c["rows"][0, "mixed"]).max() == 1200                          # a finite point with m = +inf: every box


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_length_scene_reaches_every_length(dtype, reverse):
    c = line_case(dtype, reverse)
    assert kr.leaf_preorder(c["oflat"]) == list(range(4096))                     # leaf pre-order is ascending x in the oracle's tree
    want = set(range(301)) | {wr.LANE_MAX + d for d in (-1, 0, 1)} | {wr.LDS_MAX + d for d in (-1, 0, 1)}
    want |= {v for j in range(13) for v in (2 ** j - 1, 2 ** j, 2 ** j + 1) if v <= 4096}
    assert set(c["lengths"].tolist()) == want and c["lengths"].max() == 4096
    for kind in (0, 1):
        assert np.array_equal(lengths(c["rows"][kind]), c["lengths"])             # row length equals the limit
        for (ld, ls), n in zip(c["rows"][kind], c["lengths"]):
            x = [s + 1 for s in ls]
            if reverse:                                                           # list order is descending distance: a full permutation
                assert x == list(range(4097 - n, 4097)) and ld == [float((4097 - v) ** 2) for v in x]
            else:
                assert x == list(range(1, n + 1)) and ld == [float(v * v) for v in x]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_scene_has_ties_in_every_tier(dtype):
    c = ties_case(dtype)
    order = {s: i for i, s in enumerate(kr.leaf_preorder(c["oflat"]))}
    assert kr.leaf_preorder(c["oflat"]) != sorted(order)                          # leaf pre-order is not index order here
    for kind in (0, 1):
        n = lengths(c["rows"][kind])
        assert np.array_equal(n, np.asarray(TIE_LIMITS * 2) * TIE_COPIES)
        assert (n[n > 0] <= wr.LANE_MAX).any() and ((n > wr.LANE_MAX) & (n <= wr.LDS_MAX)).any() and (n > wr.LDS_MAX).any()
        for ld, ls in c["rows"][kind]:
            sd, ss = wr.sort_row(ld, ls)
            for j in range(0, len(sd), TIE_COPIES):                                # groups of equal distance, each in leaf pre-order
                assert len(set(sd[j:j + TIE_COPIES])) == 1 and [order[s] for s in ss[j:j + TIE_COPIES]] == sorted(order[s] for s in ss[j:j + TIE_COPIES])


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_child_bounds_scene_separates_the_navigator_from_the_shape_box(dtype):
    """below a split without SAH winner a leaf's navigator box is Aabb::empty(), whose min_distance_squared is 0 for every point: the loop
    reaches the leaf whatever the shape's own box says.  The scene has triangle candidates whose own box is farther than the limit in
    floating point (a query on a vertex with m = 0: the box distance rounds above 0) — rows a walk that tests the shape's box in place
    of the navigator box would lose"""
    far, tris, pts, m = far_scene(dtype)
    oflat = orc.flatten(orc.build(far).nodes)
    nav = oflat["entry"] != NONE
    assert np.isposinf(oflat["min"][nav]).all(axis=1).any()
    rows = wr.rows(oflat, far, pts, m, tris)
    lim = wr.limits(m, len(pts), dtype)
    lost = 0
    for i, (ld, ls) in enumerate(rows):
        if ls:
            box_d = kr.dists_vector(oflat[:0], far[ls], pts[i], dtype)[1]
            lost += int((box_d > lim[i]).sum())
    n = lengths(rows)
    print(f"non-empty rows {np.sum(n > 0)}, longest {n.max()}, candidates whose own box is beyond the limit {lost}")
    assert lost > 0 and (n > 0).sum() > 50 and n.max() > wr.LANE_MAX
