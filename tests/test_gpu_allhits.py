"""All-hits ray queries on the GPU (bvhgpu_traverse_allhits_*): row i is ALL candidates of FlatBvh::traverse's list — the members whose
leaf-stage distance is < tmax[i], strict — in a stable ascending sort by distance, or in list order with BVHGPU_ALLHITS_LIST_ORDER, as a CSR
without padding.  Every check compares offsets, shapes and values byte for byte against the oracle's CSR pushed through the definition
(allhits_ref.allhits_match); tests/test_allhits_cpu.py shows on the oracle alone that the scenes used here have the row lengths, the ties
and the reversed lists that cross every tier of bvh_amd/csrc/allhits.hip."""
import ctypes as C

import numpy as np
import pytest

import allhits_ref as ar
import khits_ref as kr
import test_fp_extremes_queries_cpu as q
from sphere_ref import cluster_rays, cluster_scene, list_hits, tmax_draw
from test_allhits_cpu import ROOT, long_pair_case, single_row_case
from test_gpu_any_hit import _rb
from test_khits_cpu import cluster_case, cube_case, pair_row_case, triangle_row_case

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
DTYPES = [np.float32, np.float64]
LEAF_ID = {"box": 0, "triangle": 1, "sphere": 2}


@pytest.fixture(scope="module")
def eng():
    import bvh_amd
    if bvh_amd.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    return bvh_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.Context(0)


def _dev_rays(eng, rays):
    import torch
    dt = np.float32 if rays.dtype.itemsize == 36 else np.float64
    dev = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    return eng.RayBatch.from_device(dev, len(rays), dt)


def _to_host(offsets, shape, vals):
    if isinstance(offsets, np.ndarray):
        assert offsets.dtype == np.uint32 and shape.dtype == np.uint32
        return offsets, shape, vals
    import torch
    assert offsets.dtype == torch.int64 and shape.dtype == torch.int32 and offsets.is_cuda and shape.is_cuda and vals.is_cuda
    o = offsets.cpu().numpy()
    assert o.min(initial=0) >= 0
    return o.astype(np.uint32), shape.cpu().numpy().view(np.uint32), vals.cpu().numpy()


def _check(tree, rb, leaf, tmax, sort, want, label=None):
    """allhits_batch against (offsets, shape, vals) of allhits_match, byte for byte"""
    o, s, v = _to_host(*tree.allhits_batch(rb, leaf, tmax, sort))
    assert v.dtype == want[2].dtype and o.shape == want[0].shape, label
    assert o.tobytes() == want[0].tobytes(), (label, "offsets", np.nonzero(o != want[0])[0][:5])
    assert s.shape == want[1].shape and v.shape == want[2].shape, label
    bad = np.nonzero(s != want[1])[0]
    assert len(bad) == 0, (label, "shapes differ at", bad[:5], "row", np.searchsorted(o, bad[:5], side="right") - 1, s[bad[:5]], want[1][bad[:5]])
    assert v.tobytes() == want[2].tobytes(), (label, "values")
    return o, s, v


def _sphere_tree(eng, spheres, aabbs, ctx):
    flat = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    flat.set_spheres(spheres)
    return flat


def _drawn_tmax(case, dtype, seed=31):
    """test_gpu_khits' segment ends: around each ray's nearest sphere distance, with pinned rows NaN, 0, -1, +inf and exactly the nearest"""
    nearest = kr.khits_match(case["off"], case["idx"], case["sphere"], None, 1)[0][:, 0, 0]
    tmax = tmax_draw(np.random.default_rng(seed), nearest, dtype)
    hit = np.nonzero(np.isfinite(nearest))[0][:50]
    assert len(hit) == 50
    tmax[hit[0:10]] = np.nan
    tmax[hit[10:20]] = 0
    tmax[hit[20:30]] = -1
    tmax[hit[30:40]] = np.inf
    tmax[hit[40:50]] = nearest[hit[40:50]]
    return tmax


# ---- 1. the cluster scene: both leaf kinds, both orders, host and device memory --------------------------------------------------------
@pytest.mark.parametrize("leaf", ["box", "sphere"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_cluster_scene(eng, orc, ctx, dtype, leaf):
    import torch
    case = cluster_case(orc, dtype)
    off, idx, rays, rec = case["off"], case["idx"], case["rays"], case[leaf]
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    tmax = _drawn_tmax(case, dtype)
    rb_host, rb_dev = _rb(eng, rays), _dev_rays(eng, rays)
    tdev = torch.from_numpy(tmax.copy()).cuda()
    for sort in (True, False):
        for tm_host, tm_dev in ((None, None), (tmax, tdev)):
            want = ar.allhits_match(off, idx, rec, tm_host, sort)
            _check(flat, rb_host, leaf, tm_host, sort, want, (sort, "host"))
            _check(flat, rb_dev, leaf, tm_dev, sort, want, (sort, "device"))
    info = flat._hits.info()
    assert info["total"] == info["hits"] == len(want[1]) and info["visited"] == info["leaf_visits"] == info["device_steps"] == info["wave_steps"] == 0
    assert flat._hits.walk_flags() == 0
    t = "float" if dtype == np.float32 else "double"
    assert flat._hits.walk_kernel() == f"bvhgpu::k_allhits_fill<{t}, {LEAF_ID[leaf]}, false>"


# ---- 2. triangles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_triangle_parity(eng, orc, ctx, dtype):
    """12 000 triangles; 20 000 rays of the bench stream (they pass boxes and hit no triangle: rows that are empty after a full walk) and
    20 000 rays aimed at the cubes"""
    for name in ("stream", "aimed"):
        case = cube_case(orc, dtype, name)
        off, idx, rays, rec = case["off"], case["idx"], case["rays"], case["triangle"]
        flat = eng.Bvh.from_aabbs(case["aabbs"], ctx).flatten()
        flat.set_triangles(case["tris"])
        c = case["closest"][:, 0].astype(np.float64)
        tmax = np.where(np.isfinite(c), c * np.random.default_rng(4).uniform(0.3, 1.7, size=len(c)), 4e5).astype(dtype)
        for sort in (True, False):
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), "triangle", tm, sort, ar.allhits_match(off, idx, rec, tm, sort), (name, sort))
        _check(flat, _dev_rays(eng, rays), "triangle", None, True, ar.allhits_match(off, idx, rec, None, True), (name, "device"))


# ---- 3. row lengths across every tier ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_row_lengths(eng, orc, ctx, dtype, reverse):
    """one batch whose rows have every length 0..300, 2^j - 1 / 2^j / 2^j + 1 up to 4096 and both thresholds +-1: the lane tier, the LDS tier
    and the global tier of the sort in one launch; the reverse rows come in descending distance, a full permutation in every tier"""
    case = single_row_case(orc, dtype, reverse)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    flat.set_triangles(case["tris"])
    rb = _rb(eng, case["rays"])
    for leaf in ("box", "sphere", "triangle"):
        want = ar.allhits_match(case["off"], case["idx"], case[leaf], case["tmax"], True)
        assert np.array_equal(np.diff(want[0].astype(np.int64)), case["lengths"])
        _check(flat, rb, leaf, case["tmax"], True, want, (leaf, "sorted"))
    _check(flat, rb, "box", case["tmax"], False, ar.allhits_match(case["off"], case["idx"], case["box"], case["tmax"], False), "list order")
    _check(flat, _dev_rays(eng, case["rays"]), "sphere", None, True, ar.allhits_match(case["off"], case["idx"], case["sphere"], None, True), "whole rows")


# ---- 4. ties at length ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_ties_in_every_tier(eng, orc, ctx, dtype):
    """the pair row at 4096 positions: 8192 candidates per ray with 4096 tie pairs on the +x rays (the global tier); cut by tmax to rows in
    the LDS tier and the lane tier; then the 200-candidate rows of test_khits_cpu (the LDS tier)"""
    case = long_pair_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rb = _rb(eng, case["rays"])
    i = np.arange(64)
    cut = np.where(i < 32, 10.0 + (i % 32) + 8 * np.array([0, 1, 3, 16, 17, 100, 1024, 1025] * 4)[i % 32] + 1,
                   102.0 + (i % 32) + 8 * np.array([0, 1, 3, 16, 17, 100, 1024, 1025] * 4)[i % 32] + 1).astype(dtype)
    for leaf in ("box", "sphere"):
        for tm in (None, cut):
            want = ar.allhits_match(case["off"], case["idx"], case[leaf], tm, True)
            o, s, v = _check(flat, rb, leaf, tm, True, want, (leaf, tm is None))
        lens = np.diff(o.astype(np.int64))                                    # (of the cut batch)
        assert lens.min() <= 4 and ((lens > 32) & (lens <= 2048)).any() and (lens > 2048).any()
        _check(flat, rb, leaf, None, False, ar.allhits_match(case["off"], case["idx"], case[leaf], None, False), (leaf, "list order"))
    case = pair_row_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    for leaf in ("box", "sphere"):
        for sort in (True, False):
            _check(flat, _rb(eng, case["rays"]), leaf, None, sort, ar.allhits_match(case["off"], case["idx"], case[leaf], None, sort), (leaf, sort))
    for alternate in (False, True):
        case = triangle_row_case(orc, dtype, alternate)
        flat = eng.Bvh.from_aabbs(case["aabbs"], ctx).flatten()
        flat.set_triangles(case["tris"])
        for sort in (True, False):
            _check(flat, _rb(eng, case["rays"]), "triangle", None, sort, ar.allhits_match(case["off"], case["idx"], case["triangle"], None, sort),
                   (alternate, sort))


# ---- 5. ray counts and tree kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_ray_counts(eng, orc, ctx, dtype):
    import torch
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    tmax = _drawn_tmax(case, dtype)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20000):
        cut = case["off"][n]
        sub = (case["off"][:n + 1], case["idx"][:cut])
        for leaf in ("box", "sphere"):
            want = ar.allhits_match(*sub, case[leaf][:cut], tmax[:n], True)
            _check(flat, _rb(eng, case["rays"][:n]), leaf, tmax[:n], True, want, (n, leaf, "host"))
            if n:
                _check(flat, _dev_rays(eng, case["rays"][:n]), leaf, torch.from_numpy(tmax[:n].copy()).cuda(), True, want, (n, leaf, "device"))
    o, s, v = flat.allhits_batch(_rb(eng, case["rays"][:0]), "sphere")
    assert o.tolist() == [0] and s.shape == (0,) and v.shape == (0, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_scan_second_round(eng, orc, ctx, dtype):
    """256 * 1024 + 1 rays: 257 scan blocks, so the one-workgroup scan of the block sums runs a second round.  A small tree with short
    rows; the batch repeats 64 distinct rays, so the definition is computed for 64 rows"""
    import torch
    boxes = orc.aligned_boxes().astype(dtype)
    oflat = orc.flatten(orc.build(boxes).nodes)
    rng = np.random.default_rng(45)
    o = np.concatenate([rng.uniform(-12, 12, size=(64, 1)), rng.uniform(-0.45, 0.45, size=(64, 2))], axis=1)   # inside the row's cross-section
    o[0, 0] = -12                                                                           # (ray 0, whose row is repeated at the end: all 21 boxes)
    d = rng.normal(size=(64, 3))
    d[::2] = np.array([1.0, 0, 0]) * np.where(np.arange(32) % 2, -1.0, 1.0)[:, None]      # every other ray along the row of boxes
    base = orc.make_rays(o.astype(dtype), d.astype(dtype), dtype)
    bt = np.asarray([np.inf, 0.5, 3, 10, -1, np.nan, 25, 1.5], dtype=dtype)[np.arange(64) % 8]
    off, idx, ts, _ = orc.traverse_flat(oflat, boxes, base, want_t=True)
    reps, n = 4096, 64 * 4096 + 1
    assert n == 256 * 1024 + 1
    rays, tmax = np.concatenate([np.tile(base, reps), base[:1]]), np.concatenate([np.tile(bt, reps), bt[:1]])
    flat = eng.Bvh.from_aabbs(boxes, ctx).flatten()
    lane_max = ar.engine_thresholds(ROOT)[0]
    for sort in (True, False):
        bo, bs, bv = ar.allhits_match(off, idx, ts, bt, sort)
        first = int(bo[1])
        lens = np.concatenate([np.tile(np.diff(bo.astype(np.int64)), reps), [first]])
        want_o = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        want = (want_o, np.concatenate([np.tile(bs, reps), bs[:first]]), np.concatenate([np.tile(bv, (reps, 1)), bv[:first]]))
        assert 0 < first and 3 < lens.max() <= lane_max and (lens == 0).any() and len(want_o) == n + 1
        if sort:                                                                            # rays and segment ends in HBM, then in host memory
            _check(flat, _dev_rays(eng, rays), "box", torch.from_numpy(tmax.copy()).cuda(), sort, want, ("second round", sort))
        else:
            _check(flat, _rb(eng, rays), "box", tmax, sort, want, ("second round", sort))


@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_tree_kinds(eng, orc, ctx, dtype):
    from bvh_amd import FlatBvh, spheres_aabbs
    centres, spheres = cluster_scene(dtype, 1000)
    rng = np.random.default_rng(6)
    moved = spheres.astype(np.float64)
    moved[:, :3] += rng.uniform(-0.4, 0.4, size=(len(spheres), 3))
    moved = moved.astype(dtype)
    aabbs, aabbs_moved = spheres_aabbs(spheres), spheres_aabbs(moved)
    rays, _ = cluster_rays(orc, centres, 8000, dtype, seed=12)
    built = orc.build(aabbs).nodes
    oflat = orc.flatten(built)

    def csr(flat_nodes, boxes):
        off, idx, ts, _ = orc.traverse_flat(flat_nodes, boxes, rays, want_t=True, threads=orc.max_threads())
        return off, idx, ts

    cases = []
    tree = _sphere_tree(eng, spheres, aabbs, ctx)                         # built here
    cases.append(("built", tree, csr(oflat, aabbs), spheres))
    up = FlatBvh.from_flat_nodes(oflat, aabbs_moved, ctx)                 # an uploaded FlatBvh: the old tree over the moved shapes
    up.set_spheres(moved)
    cases.append(("uploaded", up, csr(oflat, aabbs_moved), moved))
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)                                  # refitted: boxes moved, then refit
    bvh.refit(aabbs_moved)
    refitted = bvh.flatten()
    refitted.set_spheres(moved)
    cases.append(("refitted", refitted, csr(orc.flatten(orc.refit(built, aabbs_moved)), aabbs_moved), moved))
    blob = np.zeros(tree.scene_nbytes(), dtype=np.uint8)                  # scene-imported (carries no spheres)
    tree.scene_export(blob)
    imported = FlatBvh.scene_import(blob, len(blob), ctx)
    imported.set_spheres(spheres)
    cases.append(("imported", imported, csr(oflat, aabbs), spheres))
    for name, t, (off, idx, ts), sph in cases:
        recs = {"box": ts, "sphere": list_hits(off, idx, rays, sph)}
        tmax = tmax_draw(np.random.default_rng(13), kr.khits_match(off, idx, recs["sphere"], None, 1)[0][:, 0, 0], dtype)
        for leaf in ("box", "sphere"):
            assert kr.candidate_counts(off, recs[leaf]).max() > 3
            for sort in (True, False):
                for tm in (None, tmax):
                    _check(t, _rb(eng, rays), leaf, tm, sort, ar.allhits_match(off, idx, recs[leaf], tm, sort), (name, leaf, sort))
    # a Bvh flattens in place first
    _check(eng.Bvh.from_aabbs(aabbs, ctx), _rb(eng, rays), "box", None, True, ar.allhits_match(*cases[0][2][:2], cases[0][2][2], None, True), "Bvh")
    # one shape: a single (leaf) entry
    one = np.array([[0.5, 0.5, 1.5, 0.5]], dtype=dtype)
    o = np.array([[0.5, 0.5, 0], [0.5, 0.5, 0], [2, 2, 0], [0.5, 0.5, 3], [0.0625, 0.0625, 0]], dtype=dtype)
    r1 = orc.make_rays(o, np.tile(np.array([[0, 0, 1]], dtype=dtype), (len(o), 1)), dtype)
    t1 = np.array([np.inf, 1, np.inf, np.inf, np.inf], dtype=dtype)
    ab1 = spheres_aabbs(one)
    off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(ab1).nodes), ab1, r1, want_t=True)
    single = _sphere_tree(eng, one, ab1, ctx)
    for leaf, rec in (("box", ts), ("sphere", list_hits(off, idx, r1, one))):
        for sort in (True, False):
            _check(single, _rb(eng, r1), leaf, t1, sort, ar.allhits_match(off, idx, rec, t1, sort), ("one", leaf, sort))
    assert ar.allhits_match(off, idx, ts, t1, True)[0].tolist() == [0, 1, 1, 1, 1, 2]
    # no shapes: all offsets 0, for every leaf kind
    empty = eng.Bvh.from_aabbs(np.zeros((0, 6), dtype), ctx).flatten()
    empty.set_spheres(np.zeros((0, 4), dtype))
    empty.set_triangles(np.zeros((0, 9), dtype))
    for leaf, w in (("box", 2), ("sphere", 2), ("triangle", 3)):
        for rb in (_rb(eng, r1), _dev_rays(eng, r1)):
            for sort in (True, False):
                _check(empty, rb, leaf, None, sort, (np.zeros(len(r1) + 1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, w), dtype)), ("empty", leaf))


@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_tree_with_empty_child_bounds(eng, orc, ctx, dtype):
    """the scene of test_khits_tree_with_empty_child_bounds, built the same way: splits without SAH winner leave empty child bounds"""
    rng = np.random.default_rng(9)
    big = 1e19 if dtype == np.float32 else 1e154
    g, t = 2.0 ** 41, 2.0 ** 42
    lo = (np.round(rng.uniform(-1, 1, size=(500, 3)) * big / g) * g).astype(dtype)
    tris = np.stack([lo, lo + np.array([0, 0, t], dtype), lo + np.array([t, 0, 0], dtype)], axis=1).astype(dtype)
    aabbs = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1).astype(dtype)
    spheres = np.concatenate([lo + np.array([t / 2, 0, t / 2], dtype), np.full((500, 1), t / 2, dtype)], axis=1).astype(dtype)
    n = 5000
    o = (lo[rng.integers(0, 500, size=n)] + np.array([t / 4, t, t / 4], dtype)).astype(dtype)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], dtype), (n, 1))
    d[::3] = rng.normal(size=(len(d[::3]), 3))
    d[1::3, 0] = 1e-3
    rays = orc.make_rays(o, d, dtype)
    oflat = orc.flatten(orc.build(aabbs).nodes)
    assert np.isposinf(oflat[oflat["entry"] != NONE]["min"]).all(axis=1).any()   # the tree does have empty child bounds
    off, idx, ts, _ = orc.traverse_flat(oflat, aabbs, rays, want_t=True, threads=orc.max_threads())
    isect, _, _ = orc.triangle_stage(tris, rays, off, idx)
    flat = _sphere_tree(eng, spheres, aabbs, ctx)
    flat.set_triangles(tris)
    tmax = np.where(np.arange(n) % 2 == 0, t / 2, 2 * t).astype(dtype)
    for leaf, rec in (("box", ts), ("sphere", list_hits(off, idx, rays, spheres)), ("triangle", isect)):
        assert leaf == "triangle" or kr.candidate_counts(off, rec).sum() > 500, leaf   # (in f64 no ray of this scene hits a triangle)
        for sort in (True, False):
            for tm in (None, tmax):
                _check(flat, _rb(eng, rays), leaf, tm, sort, ar.allhits_match(off, idx, rec, tm, sort), (leaf, sort))


# ---- 6. floating-point extremes ------------------------------------------------------------------------------------------------------
def _fp_case(eng, case, leaves, label):
    from bvh_amd import Context
    flat = eng.Bvh.from_aabbs(case["aabbs"], Context(0)).flatten()
    assert flat.nodes.tobytes() == case["oflat"].tobytes()
    rb = _rb(eng, case["rays"])
    for leaf, rec in leaves:
        if leaf == "triangle":
            flat.set_triangles(case["tris"])
        if leaf == "sphere":
            flat.set_spheres(case["spheres"])
        for tm in (None, case["tmax"]):
            _check(flat, rb, leaf, tm, True, ar.allhits_match(case["off"], case["idx"], rec, tm, True), (label, leaf, tm is None))


@pytest.mark.parametrize("dtype,k", q.sweep_params(q.QUERY_SCALES))
def test_allhits_scale_sweep(eng, dtype, k):
    case = q.ray_case(dtype, k)
    _fp_case(eng, case, (("box", case["ts"]), ("triangle", case["isect"])), f"{q.tname(dtype)} 2^{k}")


@pytest.mark.parametrize("dtype,k", q.sweep_params(q.SPHERE_SCALES))
def test_allhits_sphere_sweep(eng, dtype, k):
    case = q.sphere_case(dtype, k)
    _fp_case(eng, case, (("sphere", case["members"]),), f"{q.tname(dtype)} spheres 2^{k}")


@pytest.mark.parametrize("dtype", q.DTYPES)
def test_allhits_pathological_spheres_and_mixed_magnitudes(eng, dtype):
    case = q.pathological_case(dtype)
    _fp_case(eng, case, (("sphere", case["members"]),), f"{q.tname(dtype)} pathological")
    for n in q.MIXED_N:
        case = q.mixed_case(dtype, n)
        _fp_case(eng, case, (("box", case["ts"]),), f"{q.tname(dtype)} mixed {n}")


# ---- 7. cross-checks on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_allhits_against_khits_and_the_csr_walk(eng, orc, ctx, dtype):
    """GPU against GPU: khits_batch's rows are the heads of the sorted rows; the LIST_ORDER box rows without tmax are traverse_batch's CSR
    with its t-slices (every enter of this scene is finite: tests/test_allhits_cpu.py)"""
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rb = _rb(eng, case["rays"])
    tmax = _drawn_tmax(case, dtype)
    for leaf in ("box", "sphere"):
        for tm in (None, tmax):
            o, s, v = flat.allhits_batch(rb, leaf, tm)
            for k in (1, 16, 64):
                hv, hs = ar.head_rows(o, s, v, k)
                kv, ks = flat.khits_batch(rb, k, leaf, tm)
                assert hs.tobytes() == ks.tobytes() and hv.tobytes() == kv.tobytes(), (leaf, k)
    o, s, v = flat.allhits_batch(rb, "box", None, sort=False)
    off, idx, ts, _ = flat.traverse_batch(rb, want_t=True)
    assert o.tobytes() == off.tobytes() and s.tobytes() == idx.tobytes() and v.tobytes() == ts.tobytes()


# ---- 8. one result object through every kind of batch ----------------------------------------------------------------------------------
def test_allhits_result_object_reuse(eng, orc, ctx):
    from bvh_amd import _lib
    from bvh_amd._lib import HOST, INVALID_ARG, OK, ptr
    lib = _lib.load()
    dtype = np.float32
    case = cluster_case(orc, dtype)
    flat = _sphere_tree(eng, case["spheres"], case["aabbs"], ctx)
    rays = np.ascontiguousarray(case["rays"])
    n, n2 = len(rays), 3000
    off, idx, box = case["off"], case["idx"], case["box"]
    h = C.c_void_p()
    total, nr = C.c_uint64(), C.c_size_t()
    scratch_o, scratch_s = np.zeros(n + 1, np.uint32), np.zeros(len(idx), np.uint32)
    scratch_v = np.zeros((len(idx), 3), dtype)

    def info():
        assert lib.bvhgpu_hits_info(h, C.byref(nr), C.byref(total), None) == OK
        return nr.value, total.value

    def wrong_kind_fetches_refused(allhits):
        fetches = [lambda: lib.bvhgpu_hits_fetch(h, ptr(scratch_o), ptr(scratch_s), None, HOST),
                   lambda: lib.bvhgpu_hits_fetch_triangles(h, ptr(scratch_v), HOST),
                   lambda: lib.bvhgpu_hits_fetch_closest(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_any(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_box(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_fetch_sphere(h, ptr(scratch_v), ptr(scratch_s), HOST),
                   lambda: lib.bvhgpu_hits_device(h, None, None, None)]
        if allhits:
            for f in fetches:
                assert f() == INVALID_ARG
                assert "allhits" in lib.bvhgpu_last_error(ctx._h).decode()
        else:
            assert lib.bvhgpu_hits_fetch_allhits(h, ptr(scratch_o), ptr(scratch_s), ptr(scratch_v), HOST) == INVALID_ARG
            assert "bvhgpu_traverse_allhits" in lib.bvhgpu_last_error(ctx._h).decode()

    def fetch_allhits(nrays, want):
        assert info() == (nrays, len(want[1]))
        o, s, v = np.zeros(nrays + 1, np.uint32), np.zeros(len(want[1]), np.uint32), np.zeros(want[2].shape, dtype)
        assert lib.bvhgpu_hits_fetch_allhits(h, ptr(o), ptr(s), ptr(v), HOST) == OK
        assert o.tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes() and v.tobytes() == want[2].tobytes()
        assert lib.bvhgpu_hits_fetch_allhits(h, None, None, None, HOST) == OK        # each may be NULL
        assert lib.bvhgpu_hits_wait(h) == OK
        wrong_kind_fetches_refused(True)

    def fetch_csr():
        assert info() == (n, len(idx))
        o, s, t = np.zeros(n + 1, np.uint32), np.zeros(len(idx), np.uint32), np.zeros((len(idx), 2), dtype)
        assert lib.bvhgpu_hits_fetch(h, ptr(o), ptr(s), ptr(t), HOST) == OK
        assert o.tobytes() == off.tobytes() and s.tobytes() == idx.tobytes() and t.tobytes() == box.tobytes()
        wrong_kind_fetches_refused(False)

    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), n, HOST, 1, C.byref(h)) == OK                       # traverse (T_SLICE)
    fetch_csr()
    first = h.value
    assert lib.bvhgpu_traverse_allhits_f32(flat._t, ptr(rays), None, n, HOST, 2, 0, C.byref(h)) == OK      # all hits, spheres
    assert h.value == first
    fetch_allhits(n, ar.allhits_match(off, idx, case["sphere"], None, True))
    assert lib.bvhgpu_traverse_box_f32(flat._t, ptr(rays), None, n, HOST, 0, C.byref(h)) == OK             # box
    sl, shape = np.zeros((n, 2), dtype), np.zeros(n, np.uint32)
    assert lib.bvhgpu_hits_fetch_box(h, ptr(sl), ptr(shape), HOST) == OK
    want = kr.khits_match(off, idx, box, None, 1)
    assert sl.tobytes() == want[0][:, 0].tobytes() and shape.tobytes() == want[1][:, 0].tobytes()
    wrong_kind_fetches_refused(False)
    tmax = _drawn_tmax(case, dtype)[:n2].copy()                                                          # all hits, a shorter batch, list order
    assert lib.bvhgpu_traverse_allhits_f32(flat._t, ptr(rays[:n2]), ptr(tmax), n2, HOST, 0, 1, C.byref(h)) == OK
    cut = off[n2]
    fetch_allhits(n2, ar.allhits_match(off[:n2 + 1], idx[:cut], box[:cut], tmax, False))
    assert lib.bvhgpu_traverse_f32(flat._t, ptr(rays), n, HOST, 1, C.byref(h)) == OK                       # traverse again
    fetch_csr()
    assert h.value == first
    lib.bvhgpu_hits_destroy(h)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_allhits_refusals(eng, orc):
    from bvh_amd import BvhGpuError, Context, _lib, spheres_aabbs
    from bvh_amd._lib import DTYPE_MISMATCH, HOST, INVALID_ARG, NOT_FLATTENED, OK, OVERFLOW, ptr
    lib = _lib.load()
    ctx = Context(0)
    spheres = np.array([[0.5, 0.5, 1.25, 0.25], [0.5, 0.5, 2.25, 0.25]], dtype=np.float32)
    aabbs = spheres_aabbs(spheres)
    o, d = np.array([[0.5, 0.5, 0]] * 4), np.array([[0, 0, 1]] * 4)
    rays = np.ascontiguousarray(orc.make_rays(o, d, np.float32))
    rays64 = np.ascontiguousarray(orc.make_rays(o, d, np.float64))
    tmax = np.full(4, 2.25, np.float32)
    f32, f64 = lib.bvhgpu_traverse_allhits_f32, lib.bvhgpu_traverse_allhits_f64
    bvh = eng.Bvh.from_aabbs(aabbs, ctx)
    # the result object holds a box batch: a refused call leaves it, and what it answers, as they were
    other = eng.Bvh.from_aabbs(aabbs, ctx).flatten()
    h = C.c_void_p()
    assert lib.bvhgpu_traverse_box_f32(other._t, ptr(rays), None, 4, HOST, 0, C.byref(h)) == OK
    held = h.value
    sl0, sh0 = np.zeros((4, 2), np.float32), np.zeros(4, np.uint32)
    assert lib.bvhgpu_hits_fetch_box(h, ptr(sl0), ptr(sh0), HOST) == OK
    SENT = 0xABCD1234
    out_o, out_s, out_v = np.full(5, SENT, np.uint32), np.full(8, SENT, np.uint32), np.full((8, 3), -77.5, np.float32)

    def refused(rc, status, word, handle=ctx._h, hp=None):
        assert rc == status, (rc, status, word)
        msg = lib.bvhgpu_last_error(handle).decode()
        assert word in msg, (word, msg)
        assert h.value == held                                                     # *hits as it was
        sl, sh = np.zeros((4, 2), np.float32), np.zeros(4, np.uint32)
        assert lib.bvhgpu_hits_fetch_box(h, ptr(sl), ptr(sh), HOST) == OK and sl.tobytes() == sl0.tobytes() and sh.tobytes() == sh0.tobytes()
        assert lib.bvhgpu_hits_fetch_allhits(h, ptr(out_o), ptr(out_s), ptr(out_v), HOST) == INVALID_ARG
        assert np.all(out_o == SENT) and np.all(out_s == SENT) and np.all(out_v == -77.5), word

    refused(f32(None, ptr(rays), ptr(tmax), 4, HOST, 0, 0, C.byref(h)), INVALID_ARG, "NULL tree", None)
    refused(f64(bvh._t, ptr(rays64), None, 4, HOST, 0, 0, C.byref(h)), DTYPE_MISMATCH, "dtype")
    refused(f32(bvh._t, ptr(rays), ptr(tmax), 4, HOST, 0, 0, C.byref(h)), NOT_FLATTENED, "bvhgpu_flatten")
    flat = bvh.flatten()
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, 0, None), INVALID_ARG, "hits is NULL")
    refused(f32(flat._t, None, ptr(tmax), 4, HOST, 0, 0, C.byref(h)), INVALID_ARG, "rays is NULL")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, 7, 0, 0, C.byref(h)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    for leaf in (3, -1, 1 << 20):
        refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, leaf, 0, C.byref(h)), INVALID_ARG, "BVHGPU_LEAF_BOX")
    for flags in (2, 3, 16, 1 << 28, 1 << 31):
        refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 0, flags, C.byref(h)), INVALID_ARG, "BVHGPU_ALLHITS_LIST_ORDER")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 1, 0, C.byref(h)), INVALID_ARG, "bvhgpu_tree_set_triangles")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 4, HOST, 2, 0, C.byref(h)), INVALID_ARG, "bvhgpu_tree_set_spheres")
    refused(f32(flat._t, ptr(rays), ptr(tmax), 0xFFFFFFFF, HOST, 0, 0, C.byref(h)), OVERFLOW, "rays")
    # the order of the checks: the first broken rule names itself
    refused(f32(flat._t, None, None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "rays is NULL")
    refused(f32(flat._t, ptr(rays), None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "BVHGPU_HOST or BVHGPU_DEVICE")
    refused(f32(flat._t, ptr(rays), None, 0xFFFFFFFF, HOST, 9, 8, C.byref(h)), INVALID_ARG, "BVHGPU_LEAF_BOX")
    refused(f32(flat._t, ptr(rays), None, 0xFFFFFFFF, HOST, 2, 8, C.byref(h)), INVALID_ARG, "BVHGPU_ALLHITS_LIST_ORDER")
    refused(f32(flat._t, ptr(rays), None, 0xFFFFFFFF, HOST, 2, 1, C.byref(h)), INVALID_ARG, "bvhgpu_tree_set_spheres")
    # a tree whose asynchronous build failed: the settle's answer comes before everything else
    import torch
    j = np.arange(1000, dtype=np.float32)
    chain = np.stack([j, 0 * j, 0 * j, j + 0.5, 0 * j + 1, 0 * j + 1], axis=1).astype(np.float32)
    nan_tree = eng.Bvh.from_aabbs(chain, ctx)
    chain[77, 3] = np.nan
    bad = torch.from_numpy(chain).cuda()
    nan_tree.rebuild_async(bad)
    refused(f64(nan_tree._t, None, None, 4, 7, 9, 8, C.byref(h)), INVALID_ARG, "NaN")
    # the Python surface
    rb = _rb(eng, rays)
    with pytest.raises(BvhGpuError, match="leaf"):
        flat.allhits_batch(rb, "cone")
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_spheres"):
        flat.allhits_batch(rb, "sphere")
    with pytest.raises(BvhGpuError, match="bvhgpu_tree_set_triangles"):
        flat.allhits_batch(rb, "triangle")
    with pytest.raises(BvhGpuError):
        flat.allhits_batch(_rb(eng, rays64))                                   # a ray dtype that differs
    with pytest.raises(BvhGpuError):
        flat.allhits_batch(rb, "box", tmax[:-1])
    with pytest.raises(BvhGpuError):
        flat.allhits_batch(rb, "box", tmax.astype(np.float64))
    # ... and a valid call after all that works: an empty batch with NULL pointers on a fresh result object, then rows
    h2 = C.c_void_p()
    assert f32(flat._t, None, None, 0, HOST, 0, 0, C.byref(h2)) == OK and h2.value
    one = np.full(1, SENT, np.uint32)
    assert lib.bvhgpu_hits_fetch_allhits(h2, ptr(one), None, None, HOST) == OK and one.tolist() == [0]
    lib.bvhgpu_hits_destroy(h2)
    flat.set_spheres(spheres)
    off, idx, ts, _ = orc.traverse_flat(orc.flatten(orc.build(aabbs).nodes), aabbs, rays, want_t=True)
    for leaf, rec in (("box", ts), ("sphere", list_hits(off, idx, rays, spheres))):
        want = ar.allhits_match(off, idx, rec, tmax, True)
        _check(flat, rb, leaf, tmax, True, want, leaf)
    assert want[0].tolist() == [0, 2, 4, 6, 8] and want[1].tolist() == [0, 1] * 4 and want[2][:2].tolist() == [[1.0, 1.5], [2.0, 2.5]]
    lib.bvhgpu_hits_destroy(h)
